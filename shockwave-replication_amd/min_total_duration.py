"""Host mirror of the Gavel MinTotalDuration (makespan) policies
(scheduler/policies/min_total_duration.py:11-106, policy.py:14-63) over the
native allocation kernel.

Same names, ``_name`` strings and call signature as the reference:
``policy.get_allocation(unflattened_throughputs, scale_factors,
num_steps_remaining, cluster_spec)`` → ``{job_id: {worker_type: share}}`` (or
None when there are no jobs).  The reference's bisection over T, one ECOS
feasibility solve per probe (:82-101), is replaced by ``sw_mtd_allocate``: the
same probe sequence on the closed-form feasibility test, and the analytic
centre of the feasible face at the found T.

``sw_mtd_allocate`` solves one worker type.  Several worker types whose per-job
throughputs are identical — what ``MinTotalDurationPolicy`` produces by copying
the v100 throughput to every type (:25-31) — reduce to one type with Σ workers:
the LP sees only Σ_k x[j][k], and the split x[j][k] = x_j · workers_k / Σ workers
satisfies every type's capacity.  Throughputs that differ by type are a
genuine LP per probe: ``NotImplementedError`` unless the policy was built with
``worker_types=True``.  Then they go to ``sw_mtd_allocate_types``
(csrc/sw_mtd_types.h): the max-min level t* of throughput / steps over the
types answers every probe (the LP is feasible at T exactly when T·t* ≥ 1), and
the allocation is the analytic centre of the reference's LP at the found T;
``last_level`` is then (T, t*, flags).  Identical throughputs still take the
one-type path.  A zero throughput raises
``ValueError`` naming the job: the reference's LP is infeasible at every T
there and its search never ends.  Remaining steps below zero are taken as
zero: with x ≥ 0 the LP's row is the same.  The result is clipped to [0, 1]
(:105).  A native error raises; there is no CPU fallback.
``MinTotalDurationPolicyWithPacking`` is not built.
"""
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


class MinTotalDurationPolicyWithPerf:
    """min_total_duration.py:41-106."""

    def __init__(self, solver=None, native=None, worker_types=False):
        self._name = "MinTotalDuration_Perf"
        self._solver = solver  # kept for the signature; the search runs on the GPU
        self._native = native
        self._worker_types = worker_types  # throughputs that differ by type: sw_mtd_allocate_types
        self.last_level = None  # (T, μ) of the last solve; (T, t*, flags) of one over differing types

    @property
    def name(self):
        return self._name

    def _engine(self):
        if self._native is None:
            self._native = sw_native.Solver(device=0)
        return self._native

    def get_allocation(self, unflattened_throughputs, scale_factors, num_steps_remaining, cluster_spec):
        throughputs, index = _flatten(unflattened_throughputs, cluster_spec)
        if throughputs is None:
            return None
        m, n = throughputs.shape
        job_ids, worker_types = index
        if not (throughputs == throughputs[:, :1]).all():
            if not self._worker_types:
                raise NotImplementedError(
                    "MinTotalDuration with throughputs that differ by worker type needs worker_types=True: "
                    "the default kernel solves one worker type (or several identical ones)")
            return self._allocation_over_types(throughputs, index, scale_factors, num_steps_remaining, cluster_spec)
        for i in range(m):
            if throughputs[i, 0] == 0:
                raise ValueError(f"job {job_ids[i]} has zero throughput: no T lets it finish")
        # a remainder below zero asks for nothing: tp·x ≥ steps/T with x ≥ 0 is then the row of steps = 0
        full_time = np.array([max(num_steps_remaining[job_ids[i]], 0) / throughputs[i, 0] for i in range(m)],
                             dtype=np.float64)
        workers = [int(cluster_spec[wt]) for wt in worker_types]
        total = sum(workers)
        sf = np.array([scale_factors[j] for j in job_ids], dtype=np.int32)
        x, T, mu = self._engine().mtd_allocate(sf, full_time, total)
        self.last_level = (T, mu)
        x = np.asarray(x, dtype=np.float64)
        if n == 1:
            xs = x.reshape(m, 1)
        else:
            xs = np.array([[x[i] * workers[k] / total for k in range(n)] for i in range(m)])
        xs = xs.clip(min=0.0).clip(max=1.0)
        return {job_ids[i]: {worker_types[k]: xs[i, k] for k in range(n)} for i in range(m)}


    def _allocation_over_types(self, throughputs, index, scale_factors, num_steps_remaining, cluster_spec):
        m, n = throughputs.shape
        job_ids, worker_types = index
        workers = np.array([int(cluster_spec[wt]) for wt in worker_types], dtype=np.int32)
        steps = np.array([max(num_steps_remaining[j], 0) for j in job_ids], dtype=np.float64)
        for i in range(m):
            if steps[i] > 0 and not (throughputs[i, workers > 0] > 0).any():
                raise ValueError(f"job {job_ids[i]} has zero throughput on every worker type that has workers: "
                                 "no T lets it finish")
        sf = np.array([scale_factors[j] for j in job_ids], dtype=np.int32)
        x, T, t, _, flags = self._engine().mtd_allocate_types(workers, sf, throughputs, steps)
        self.last_level = (T, t, flags)
        xs = np.asarray(x, dtype=np.float64).reshape(m, n).clip(min=0.0).clip(max=1.0)
        return {job_ids[i]: {worker_types[k]: xs[i, k] for k in range(n)} for i in range(m)}


class MinTotalDurationPolicy:
    """min_total_duration.py:11-38: the WithPerf policy with every worker
    type's throughput replaced by the job's v100 throughput."""

    def __init__(self, solver=None, native=None):
        self._name = "MinTotalDuration"
        self._min_total_duration_perf_policy = MinTotalDurationPolicyWithPerf(solver, native)

    @property
    def name(self):
        return self._name

    @property
    def last_level(self):
        return self._min_total_duration_perf_policy.last_level

    def get_allocation(self, unflattened_throughputs, scale_factors, num_steps_remaining, cluster_spec):
        throughputs, _ = _flatten(unflattened_throughputs, cluster_spec)
        if throughputs is None:
            return None
        new_unflattened_throughputs = {}
        for job_id in unflattened_throughputs:
            new_unflattened_throughputs[job_id] = {}
            for worker_type in unflattened_throughputs[job_id]:
                new_unflattened_throughputs[job_id][worker_type] = unflattened_throughputs[job_id]["v100"]
        return self._min_total_duration_perf_policy.get_allocation(
            new_unflattened_throughputs, scale_factors, num_steps_remaining, cluster_spec)
