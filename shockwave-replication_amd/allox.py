"""Host mirror of the AlloX policy (scheduler/policies/allox.py:13-141,
policy.py:14-44) over the native assignment kernel.

Same name (``AlloX_Perf``), constructor argument and call signature as the
reference: ``policy.get_allocation(unflattened_throughputs, scale_factors,
times_since_start, num_steps_remaining, cluster_spec)`` →
``{job_id: {worker_type: 0.0 or 1.0}}`` (or None when there are no jobs).  The
dense cost matrix and scipy's ``linear_sum_assignment`` (:71-103) are replaced
by ``sw_allox_assign``: an assignment of the same minimal total cost, with the
tie rule of csrc/sw_allox.h instead of scipy's (DESIGN.md §17 — the optimum
is not unique: workers of one type are identical columns).

What is kept from the reference, in its order:
  * jobs sorted by id, worker types sorted by name (policy.py:28-44); no jobs
    or no worker types → None, the state untouched (:27-29);
  * every scale factor must be 1: ``AssertionError`` (:35-36);
  * a job holds a worker when its previous row sums to exactly 1.0 over the
    worker types, added in their order from 0.0 (:42-52); each such job takes
    one worker off every type where its row is 1.0 (:57-64);
  * the other jobs, in the iteration order of ``unflattened_throughputs``, are
    stably sorted by ``-times_since_start`` and cut to the first
    ``max(int(alpha·m), n)``, m their number and n the free workers (:67-69);
  * processing time = steps remaining / throughput on the type, a throughput
    of 0.0 replaced by 1e-10 (:77-82); delay = time since start (:93);
  * on every free worker the job that runs first gets 1.0 on the worker's
    type (:130-134); every job with a previous row starts from a copy of it,
    the others from zeros over ``cluster_spec`` (:124-129); the result becomes
    the previous allocation (:139).
Several worker types with different throughputs are the policy's point and
are supported.  With no free worker, or no job without one, nothing is
launched.  A processing time or delay that is negative or not finite raises
``ValueError`` naming the job before any launch (the reference hands NaN or
inf to scipy, which raises or returns an arbitrary matching).  A native error
raises; there is no CPU fallback.
"""
import copy
import math

import numpy as np

import sw_native


class AlloXPolicy:
    """allox.py:13-141."""

    def __init__(self, alpha=1.0, native=None):
        self._name = "AlloX_Perf"
        self._alpha = alpha
        self._prev_allocation = {}
        self._native = native
        self.last_cost = None  # total cost of the last assignment

    @property
    def name(self):
        return self._name

    def _engine(self):
        if self._native is None:
            self._native = sw_native.Solver(device=0)
        return self._native

    def get_allocation(self, unflattened_throughputs, scale_factors, times_since_start,
                       num_steps_remaining, cluster_spec):
        job_ids = sorted(unflattened_throughputs.keys())
        if len(job_ids) == 0:
            return None
        worker_types = sorted(unflattened_throughputs[job_ids[0]].keys())
        if len(worker_types) == 0:
            return None
        for j in scale_factors:
            assert scale_factors[j] == 1

        prev = self._prev_allocation
        waiting, holding = [], []
        for j in unflattened_throughputs:
            held = False
            if j in prev:
                total = 0.0
                for wt in worker_types:
                    total += prev[j][wt]
                held = total == 1.0
            (holding if held else waiting).append(j)

        # a type with more holders than workers (a cluster that shrank) has none free (:62)
        free = [max(0, cluster_spec[wt] - sum(1 for j in holding if prev[j][wt] == 1.0))
                for wt in worker_types]
        n = sum(free)
        waiting.sort(key=lambda j: -times_since_start[j])
        waiting = waiting[:max(int(self._alpha * len(waiting)), n)]
        m = len(waiting)

        allocation = {j: {wt: 0.0 for wt in cluster_spec} for j in job_ids}
        for j in job_ids:
            if j in prev:
                allocation[j] = copy.copy(prev[j])
        if m > 0 and n > 0:
            p = np.zeros((m, len(worker_types)))
            d = np.zeros(m)
            for i, j in enumerate(waiting):
                d[i] = times_since_start[j]
                if not (math.isfinite(d[i]) and d[i] >= 0):
                    raise ValueError(f"job {j} has delay {d[i]!r}: it must be finite and >= 0")
                for k, wt in enumerate(worker_types):
                    throughput = unflattened_throughputs[j][wt]
                    if throughput == 0.0:
                        throughput = 1e-10
                    p[i, k] = num_steps_remaining[j] / throughput
                    if not (math.isfinite(p[i, k]) and p[i, k] >= 0):
                        raise ValueError(f"job {j} has processing time {p[i, k]!r} on {wt}: "
                                         "it must be finite and >= 0")
            _, _, worker_first, cost = self._engine().allox_assign(free, p, d)
            self.last_cost = cost
            type_of = [k for k, f in enumerate(free) for _ in range(f)]
            for w in range(n):
                if worker_first[w] >= 0:
                    allocation[waiting[int(worker_first[w])]][worker_types[type_of[w]]] = 1.0
        self._prev_allocation = copy.copy(allocation)
        return allocation
