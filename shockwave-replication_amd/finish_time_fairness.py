"""Host mirror of the Gavel FinishTimeFairness (Themis) policies
(scheduler/policies/finish_time_fairness.py:14-140, isolated.py:13-52,
policy.py:14-63) over the native allocation kernel.

Same names, ``_name`` strings and call signature as the reference:
``policy.get_allocation(unflattened_throughputs, scale_factors,
priority_weights, times_since_start, num_steps_remaining, cluster_spec)`` →
``{job_id: {worker_type: share}}`` (or None when there are no jobs).  The ECOS
solve (finish_time_fairness.py:106-126) is replaced by ``sw_ftf_allocate``:
the program's optimal ratio ρ*, and the unique optimum when capacity binds or
the analytic centre of the optimal face when it does not.

State kept between calls, as in the reference (:61-63, :98-104, :128-133):
``_cumulative_isolated_time`` (never deleted), and the previous call's
remaining steps and isolated throughputs (reset when there are no jobs).
Priority weights are ignored, as in the reference (:86-89).

The kernel solves one worker type.  Several worker types whose per-job
throughputs are identical — what ``FinishTimeFairnessPolicy`` produces by
copying the v100 throughput to every type (:35-43) — reduce to one type with
Σ workers: the program sees only Σ_k x[j][k], and the split
x[j][k] = x_j · workers_k / Σ workers satisfies every type's capacity.
Throughputs that differ by type need a different solver:
``NotImplementedError`` by default, and with
``FinishTimeFairnessPolicyWithPerf(worker_types=True)`` they go to
``sw_ftf_allocate_types``: the same program over the types as
they are, ρ* the root of the max-min level t*(ρ) = 1 and the analytic centre of
the feasible set at ρ*; ``last_level`` is then (ρ*, level solves).  There a zero
throughput raises only for a job with steps left and no positive throughput on
a type that has workers.  (A finished job whose throughputs are all zero has no
isolated throughput either: its expected isolated time is 0/0, and the check
of that time raises ``ValueError`` naming it, as on the default path.)  A zero throughput, or a job whose expected isolated
time is not positive (remaining steps that grew since the previous call make
the reference's cumulative term negative), raises ``ValueError`` naming the
job: the reference divides by zero or builds a non-convex program there, and
the mirror does not paper over it.  The result is clipped to [0, 1]
(:140).  A native error raises; there is no CPU fallback.
"""
import copy

import numpy as np

import sw_native


def _flatten(d, cluster_spec):
    """policy.py:28-44: jobs sorted by id, worker types sorted by name (from
    the first job), the throughput matrix."""
    job_ids = sorted(d.keys())
    if len(job_ids) == 0:
        return None, None
    worker_types = sorted(d[job_ids[0]].keys())
    if len(worker_types) == 0:
        return None, None
    m = np.array([[d[j][wt] for wt in worker_types] for j in job_ids], dtype=np.float64)
    return m, (job_ids, worker_types)


def _isolated_throughputs(throughputs, index, scale_factors, cluster_spec):
    """IsolatedPolicy.get_throughputs (isolated.py:15-52): the cluster split
    evenly over the jobs, divided by the scale factor, each row scaled to sum
    to at most 1."""
    job_ids, worker_types = index
    m, n = throughputs.shape
    sfa = np.array([[scale_factors[j]] * n for j in job_ids], dtype=np.float64)
    x = np.array([[cluster_spec[wt] / m for wt in worker_types] for _ in range(m)])
    x = x / sfa
    per_row_sum = np.maximum(np.sum(x, axis=1), np.ones(m))
    x = x / per_row_sum[:, None]
    return np.sum(np.multiply(throughputs, x), axis=1)


class FinishTimeFairnessPolicyWithPerf:
    """finish_time_fairness.py:55-140."""

    def __init__(self, solver="ECOS", native=None, worker_types=False):
        self._name = "FinishTimeFairness_Perf"
        self._solver = solver  # kept for the signature; the program runs on the GPU
        self._native = native
        self._worker_types = worker_types  # throughputs that differ by type: sw_ftf_allocate_types
        self._cumulative_isolated_time = {}
        self._isolated_throughputs_prev_iteration = {}
        self._num_steps_remaining_prev_iteration = {}
        self.last_level = None  # (ρ*, μ) of the last solve; (ρ*, level solves) of one over differing types

    @property
    def name(self):
        return self._name

    def _engine(self):
        if self._native is None:
            self._native = sw_native.Solver(device=0)
        return self._native

    def get_allocation(self, unflattened_throughputs, scale_factors, unflattened_priority_weights,
                       times_since_start, num_steps_remaining, cluster_spec):
        throughputs, index = _flatten(unflattened_throughputs, cluster_spec)
        if throughputs is None:
            self._isolated_throughputs_prev_iteration = {}
            self._num_steps_remaining_prev_iteration = {}
            return None
        m, n = throughputs.shape
        job_ids, worker_types = index
        workers = [int(cluster_spec[wt]) for wt in worker_types]
        over_types = not (throughputs == throughputs[:, :1]).all()
        if over_types and not self._worker_types:
            raise NotImplementedError(
                "FinishTimeFairness with throughputs that differ by worker type is not supported: "
                "the native kernel solves one worker type (or several identical ones); "
                "worker_types=True selects the kernel over differing types")
        for i in range(m):
            if over_types:
                live = num_steps_remaining[job_ids[i]] > 0
                if live and not any(throughputs[i, k] > 0 for k in range(n) if workers[k] > 0):
                    raise ValueError(f"job {job_ids[i]} has zero throughput on every worker type that has workers: "
                                     "its finish time is undefined")
            elif throughputs[i, 0] == 0:
                raise ValueError(f"job {job_ids[i]} has zero throughput: its finish time is undefined")
        isolated = _isolated_throughputs(throughputs, index, scale_factors, cluster_spec)
        full_time, elapsed, expected = np.zeros(m), np.zeros(m), np.zeros(m)
        for i in range(m):
            j = job_ids[i]
            if j not in self._cumulative_isolated_time:
                self._cumulative_isolated_time[j] = 0
            if j in self._num_steps_remaining_prev_iteration:
                self._cumulative_isolated_time[j] += (
                    self._num_steps_remaining_prev_iteration[j] - num_steps_remaining[j]
                ) / self._isolated_throughputs_prev_iteration[j]
            expected[i] = self._cumulative_isolated_time[j] + num_steps_remaining[j] / isolated[i]
            elapsed[i] = times_since_start[j]
            if not over_types:
                full_time[i] = num_steps_remaining[j] / throughputs[i, 0]
        # the state is updated before the solve can raise, in the reference's order (:128-133)
        self._num_steps_remaining_prev_iteration = copy.copy(num_steps_remaining)
        self._isolated_throughputs_prev_iteration = {job_ids[i]: isolated[i] for i in range(m)}
        for i in range(m):
            if not expected[i] > 0:
                raise ValueError(f"job {job_ids[i]} has expected isolated time {expected[i]!r} <= 0")
        total = sum(workers)
        sf = np.array([scale_factors[j] for j in job_ids], dtype=np.int32)
        if over_types:
            steps = np.array([num_steps_remaining[j] for j in job_ids], dtype=np.float64)
            x, rho, _, _, solves, _ = self._engine().ftf_allocate_types(
                np.array(workers, dtype=np.int32), sf, throughputs, steps, elapsed, expected)
            self.last_level = (rho, solves)
            xs = np.asarray(x, dtype=np.float64).reshape(m, n).clip(min=0.0).clip(max=1.0)
            return {job_ids[i]: {worker_types[k]: xs[i, k] for k in range(n)} for i in range(m)}
        x, rho, mu = self._engine().ftf_allocate(sf, full_time, elapsed, expected, total)
        self.last_level = (rho, mu)
        x = np.asarray(x, dtype=np.float64)
        if n == 1:
            xs = x.reshape(m, 1)
        else:
            xs = np.array([[x[i] * workers[k] / total for k in range(n)] for i in range(m)])
        xs = xs.clip(min=0.0).clip(max=1.0)
        return {job_ids[i]: {worker_types[k]: xs[i, k] for k in range(n)} for i in range(m)}


class FinishTimeFairnessPolicy:
    """finish_time_fairness.py:14-52: the WithPerf policy with every worker
    type's throughput replaced by the job's v100 throughput."""

    def __init__(self, solver="ECOS", native=None):
        self._name = "FinishTimeFairness"
        self._finish_time_fairness_perf_policy = FinishTimeFairnessPolicyWithPerf(solver, native)

    @property
    def name(self):
        return self._name

    def get_allocation(self, unflattened_throughputs, scale_factors, unflattened_priority_weights,
                       times_since_start, num_steps_remaining, cluster_spec):
        throughputs, _ = _flatten(unflattened_throughputs, cluster_spec)
        if throughputs is None:
            return None
        new_unflattened_throughputs = {}
        for job_id in unflattened_throughputs:
            new_unflattened_throughputs[job_id] = {}
            for worker_type in unflattened_throughputs[job_id]:
                new_unflattened_throughputs[job_id][worker_type] = unflattened_throughputs[job_id]["v100"]
        return self._finish_time_fairness_perf_policy.get_allocation(
            new_unflattened_throughputs, scale_factors, unflattened_priority_weights, times_since_start,
            num_steps_remaining, cluster_spec)
