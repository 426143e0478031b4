"""Host mirror of the Gavel max-sum-throughput policies
(scheduler/policies/max_sum_throughput.py:11-96, policy.py:14-63) over the
native allocation kernel.

Same names, ``_name`` strings and call signatures as the reference:
``ThroughputSumWithPerf.get_allocation(unflattened_throughputs, scale_factors,
cluster_spec)``, ``ThroughputNormalizedByCostSumWithPerf.get_allocation(…,
instance_costs)`` and ``ThroughputNormalizedByCostSumWithPerfSLOs
.get_allocation(…, instance_costs=None, SLOs={}, num_steps_remaining={})`` →
``{job_id: {worker_type: share}}`` (or None when there are no jobs).  The
reference's ECOS solve, and its second solve without the SLO rows when they are
infeasible (:85-94), are replaced by ``sw_mst_allocate``: the density threshold
of the fractional knapsack and, on the jobs tied at it, the analytic centre of
the optimal face.

The kernel solves one worker type.  Several worker types reduce to one type on
Σ workers when each job's throughput and the instance costs are identical
across the types: the LP then sees only Σ_k x[j][k], and the split
x[j][k] = x_j · workers_k / Σ workers satisfies every type's capacity.
Throughputs or costs that differ by type are a genuine LP:
``NotImplementedError``.  As in the reference, a job in ``SLOs`` that is
missing from ``num_steps_remaining`` is an ``AssertionError`` and ``SLO == 0``
a ``ZeroDivisionError``; a row with steps/SLO ≤ 0 holds for every x ≥ 0 and is
dropped.  When the SLO rows are infeasible the reference's warning is printed
and the allocation is the one without them.  The result is clipped to [0, 1]
(:96).  A native error raises; there is no CPU fallback.
``ThroughputNormalizedByCostSumWithPackingSLOs`` is not built.
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


class ThroughputNormalizedByCostSumWithPerfSLOs:
    """max_sum_throughput.py:39-96."""

    def __init__(self, solver=None, native=None):
        self._name = "ThroughputNormalizedByCostSum_PerfSLOs"
        self._solver = solver  # kept for the signature; the solve runs on the GPU
        self._native = native
        self.last_level = None  # (λ, m, objective, slo_dropped) of the last solve

    @property
    def name(self):
        return self._name

    def _engine(self):
        if self._native is None:
            self._native = sw_native.Solver(device=0)
        return self._native

    def get_allocation(self, unflattened_throughputs, scale_factors, cluster_spec, instance_costs=None,
                       SLOs={}, num_steps_remaining={}):
        throughputs, index = _flatten(unflattened_throughputs, cluster_spec)
        if throughputs is None:
            return None
        m, n = throughputs.shape
        job_ids, worker_types = index
        costs = [1.0 if instance_costs is None else float(instance_costs[wt]) for wt in worker_types]
        if not (throughputs == throughputs[:, :1]).all() or any(c != costs[0] for c in costs):
            raise NotImplementedError(
                "max sum throughput with throughputs or instance costs that differ by worker type is "
                "not supported: the native kernel solves one worker type (or several identical ones)")
        tp = throughputs[:, 0]
        weights = tp / costs[0]
        floors = None
        for job_id in SLOs:
            i = job_ids.index(job_id)
            assert job_id in num_steps_remaining
            r = num_steps_remaining[job_id] / SLOs[job_id]
            if floors is None:
                floors = np.zeros(m, dtype=np.float64)
            if r > 0:
                floors[i] = r / tp[i] if tp[i] > 0 else np.inf
        workers = [int(cluster_spec[wt]) for wt in worker_types]
        total = sum(workers)
        sf = np.array([scale_factors[j] for j in job_ids], dtype=np.int32)
        x, lam, mult, objective, slo_dropped = self._engine().mst_allocate(sf, weights, floors, total)
        self.last_level = (lam, mult, objective, slo_dropped)
        if slo_dropped:
            print("WARNING: No allocation possible with provided SLOs!")
        x = np.asarray(x, dtype=np.float64)
        if n == 1:
            xs = x.reshape(m, 1)
        else:
            xs = np.array([[x[i] * workers[k] / total for k in range(n)] for i in range(m)])
        xs = xs.clip(min=0.0).clip(max=1.0)
        return {job_ids[i]: {worker_types[k]: xs[i, k] for k in range(n)} for i in range(m)}


class ThroughputNormalizedByCostSumWithPerf:
    """max_sum_throughput.py:23-36."""

    def __init__(self, solver=None, native=None):
        self._name = "ThroughputNormalizedByCostSum_Perf"
        self._policy = ThroughputNormalizedByCostSumWithPerfSLOs(solver, native)

    @property
    def name(self):
        return self._name

    @property
    def last_level(self):
        return self._policy.last_level

    def get_allocation(self, unflattened_throughputs, scale_factors, cluster_spec, instance_costs):
        return self._policy.get_allocation(unflattened_throughputs, scale_factors, cluster_spec,
                                           instance_costs=instance_costs)


class ThroughputSumWithPerf:
    """max_sum_throughput.py:11-20."""

    def __init__(self, solver=None, native=None):
        self._name = "ThroughputSumWithPerf"
        self._policy = ThroughputNormalizedByCostSumWithPerfSLOs(solver, native)

    @property
    def name(self):
        return self._name

    @property
    def last_level(self):
        return self._policy.last_level

    def get_allocation(self, unflattened_throughputs, scale_factors, cluster_spec):
        return self._policy.get_allocation(unflattened_throughputs, scale_factors, cluster_spec)
