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
``NotImplementedError`` unless the policy was built with ``worker_types=True``.
Then they go to ``sw_mst_allocate_types`` (csrc/sw_mst_types.h): with
y = scale_factor·x the LP is a transportation problem with integer supplies
and capacities, solved exactly by successive best paths, and the allocation is
a vertex of the LP; ``last_level`` is then (prices, augmentations, objective,
flags).  Generic inputs have one optimum.  With ties among differing types
ECOS returns a point inside the optimal face and the kernel the vertex of its
tie rule (lowest job, then lowest type); the objective is the same.  Identical
types still take the one-type path.  SLOs together with differing types still
raise ``NotImplementedError`` (a floor on Σ_k throughput·x breaks the
transportation structure), and an instance cost ≤ 0 raises ``ValueError``
naming the type.  As in the reference, a job in ``SLOs`` that is
missing from ``num_steps_remaining`` is an ``AssertionError`` and ``SLO == 0``
a ``ZeroDivisionError``; a row with steps/SLO ≤ 0 holds for every x ≥ 0 and is
dropped.  When the SLO rows are infeasible the reference's warning is printed
and the allocation is the one without them.  The result is clipped to [0, 1]
(:96).  A native error raises; there is no CPU fallback.
``ThroughputNormalizedByCostSumWithPackingSLOs`` is not built.
"""
import numpy as np

from sw_policy import Policy, clipped, identical_types, int_workers, split_over_types
from sw_policy import flatten as _flatten, unflatten as _unflatten


class ThroughputNormalizedByCostSumWithPerfSLOs(Policy):
    """max_sum_throughput.py:39-96."""

    def __init__(self, solver=None, native=None, worker_types=False):
        self._name = "ThroughputNormalizedByCostSum_PerfSLOs"
        self._solver = solver  # kept for the signature; the solve runs on the GPU
        self._native = native
        self._worker_types = worker_types  # throughputs or costs that differ by type: sw_mst_allocate_types
        # (λ, m, objective, slo_dropped) of the last solve; (prices, augmentations, objective, flags) of one
        # over differing types
        self.last_level = None

    def get_allocation(self, unflattened_throughputs, scale_factors, cluster_spec, instance_costs=None,
                       SLOs={}, num_steps_remaining={}):
        throughputs, index = _flatten(unflattened_throughputs)
        if throughputs is None:
            return None
        m = len(throughputs)
        job_ids, worker_types = index
        costs = [1.0 if instance_costs is None else float(instance_costs[wt]) for wt in worker_types]
        if not identical_types(throughputs) or any(c != costs[0] for c in costs):
            if self._worker_types:
                return self._allocation_over_types(throughputs, index, costs, scale_factors, cluster_spec, SLOs)
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
        workers = int_workers(worker_types, cluster_spec)
        total = sum(workers)
        sf = np.array([scale_factors[j] for j in job_ids], dtype=np.int32)
        x, lam, mult, objective, slo_dropped = self._engine().mst_allocate(sf, weights, floors, total)
        self.last_level = (lam, mult, objective, slo_dropped)
        if slo_dropped:
            print("WARNING: No allocation possible with provided SLOs!")
        x = np.asarray(x, dtype=np.float64)
        xs = split_over_types(x, workers, total)
        return _unflatten(clipped(xs), index)

    def _allocation_over_types(self, throughputs, index, costs, scale_factors, cluster_spec, SLOs):
        m, n = throughputs.shape
        job_ids, worker_types = index
        if SLOs:
            raise NotImplementedError(
                "max sum throughput with SLOs and throughputs or instance costs that differ by worker type is "
                "not supported: a floor on Σ_k throughput·x breaks the transportation structure that "
                "sw_mst_allocate_types solves")
        for k, c in enumerate(costs):
            if not c > 0:
                raise ValueError(f"worker type {worker_types[k]} has instance cost {c}: costs must be > 0")
        weights = throughputs / np.array(costs, dtype=np.float64)[None, :]
        workers = np.array(int_workers(worker_types, cluster_spec), dtype=np.int32)
        sf = np.array([scale_factors[j] for j in job_ids], dtype=np.int32)
        x, prices, objective, augmentations, _, flags = self._engine().mst_allocate_types(workers, sf, weights)
        self.last_level = (prices, augmentations, objective, flags)
        return _unflatten(clipped(np.asarray(x, dtype=np.float64).reshape(m, n)), index)


class ThroughputNormalizedByCostSumWithPerf(Policy):
    """max_sum_throughput.py:23-36."""

    def __init__(self, solver=None, native=None, worker_types=False):
        self._name = "ThroughputNormalizedByCostSum_Perf"
        self._policy = ThroughputNormalizedByCostSumWithPerfSLOs(solver, native, worker_types)

    @property
    def last_level(self):
        return self._policy.last_level

    def get_allocation(self, unflattened_throughputs, scale_factors, cluster_spec, instance_costs):
        return self._policy.get_allocation(unflattened_throughputs, scale_factors, cluster_spec,
                                           instance_costs=instance_costs)


class ThroughputSumWithPerf(Policy):
    """max_sum_throughput.py:11-20."""

    def __init__(self, solver=None, native=None, worker_types=False):
        self._name = "ThroughputSumWithPerf"
        self._policy = ThroughputNormalizedByCostSumWithPerfSLOs(solver, native, worker_types)

    @property
    def last_level(self):
        return self._policy.last_level

    def get_allocation(self, unflattened_throughputs, scale_factors, cluster_spec):
        return self._policy.get_allocation(unflattened_throughputs, scale_factors, cluster_spec)
