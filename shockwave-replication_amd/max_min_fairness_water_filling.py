"""Host mirror of the Gavel water-filling MaxMinFairness policies
(scheduler/policies/max_min_fairness_water_filling.py:412-556, policy.py:14-63,
proportional.py:10-44) over the native allocation kernel.

Same names, ``_name`` strings, constructor argument and call signature as the
reference: ``policy.get_allocation(unflattened_throughputs, scale_factors,
priority_weights, cluster_spec, entity_weights=None,
entity_to_job_mapping=None, verbose=False,
return_effective_throughputs=False)`` → ``{job_id: {worker_type: share}}`` (or
None when there are no jobs).  The stage loop (:303-409: one ECOS LP and one
GLPK MILP per stage) is replaced by ``sw_wf_allocate``, which returns the
loop's fixed point x_j = min(1, L*/c_j), c_j = scale factor / priority weight,
in one kernel.

``sw_wf_allocate`` solves one worker type.  Several worker types whose per-job
throughputs are identical — always the case for
``MaxMinFairnessWaterFillingPolicy``, which replaces every throughput by 1.0
(:437-441) — reduce to one type with Σ workers: the proportional throughput of
a job is then its own throughput (proportional.py:15-44), the program sees
only Σ_k x[j][k], and the split x[j][k] = x_j · workers_k / Σ workers satisfies
every type's capacity.  ``return_effective_throughputs=True`` returns the
normalised effective throughputs and the job ids (:550-551): Σ_k x[j][k] for
the WithPerf policy.  The result is clipped to [0, 1] (:556).  A native error
raises; there is no CPU fallback.

Not built here:
  * the entity hierarchy (``priority_reweighting_policies`` "fairness" and
    "fifo", :21-77) is built by the classes of
    ``max_min_fairness_water_filling_hierarchical``; in these two classes a
    constructor argument other than None still raises ``NotImplementedError``
    (naming those classes); ``entity_weights`` and ``entity_to_job_mapping``
    are accepted and, as in the reference without reweighting (:30-32), unused.
    The reference scheduler never passes entities (scheduler.py:2433-2436);
  * throughputs that differ by worker type raise ``NotImplementedError`` unless
    the WithPerf policy is built with ``worker_types=True``.  Then they go to
    ``sw_wf_allocate_types``: the stage loop in one kernel on the
    coefficients c_jk = thr_jk / prop_j · (1/w_j)·sf_j, every stage a level solve
    of the interior-point engine, the bottlenecks read off its end point
    instead of the MILP; the shares are the centre of the last stage's optimal
    face, as the reference's last ECOS point is.  ``last_level`` is then (last
    level, stages), ``last_flags`` the call's flags, and a flagged result
    (SW_WFT_NEAR, SW_WFT_COARSE) raises ``WaterFillingStageWarning``.  Identical throughputs still go to ``sw_wf_allocate``;
  * entities over worker types that differ, warm starts between the stages;
  * ``MaxMinFairnessWaterFillingPolicyWithPacking`` (:559-691).
A priority weight ≤ 0 (the reference never raises such a job, :336-345) or a
zero throughput (its proportional throughput divides by zero, :127-129) raises
``ValueError`` naming the job.
"""
import warnings

import numpy as np

import sw_native


class WaterFillingStageWarning(UserWarning):
    """sw_wf_allocate_types flagged its own result: a bottleneck statistic near
    its threshold (a job may have frozen a stage late or early) or a stage solved
    again at a coarser path point (levels eased by more than a part in 2^30)."""


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


def _proportional_throughputs(throughputs, worker_types, cluster_spec):
    """ProportionalPolicy.get_throughputs (proportional.py:15-44)."""
    m, _ = throughputs.shape
    x = np.array([[cluster_spec[wt] / m for wt in worker_types] for _ in range(m)])
    x = x / np.sum(x, axis=1).max()
    return np.sum(np.multiply(throughputs, x), axis=1)


def _check_reweighting(priority_reweighting_policies):
    if priority_reweighting_policies is not None:
        raise NotImplementedError(
            "the entity hierarchy (priority_reweighting_policies 'fairness' / 'fifo') is built by "
            "MaxMinFairnessWaterFillingHierarchicalPolicy and ...PolicyWithPerf in "
            "max_min_fairness_water_filling_hierarchical, not by this class")


class MaxMinFairnessWaterFillingPolicyWithPerf:
    """max_min_fairness_water_filling.py:471-556."""

    def __init__(self, priority_reweighting_policies=None, native=None, worker_types=False):
        _check_reweighting(priority_reweighting_policies)
        self._name = "MaxMinFairnessWaterFilling_Perf"
        self._priority_reweighting_policies = priority_reweighting_policies
        self._native = native
        self._worker_types = worker_types  # throughputs that differ by type: sw_wf_allocate_types
        self.last_level = None  # (L*, Σ sf_j·x_j) of the last solve; (last level, stages) over differing types
        self.last_flags = 0  # the flags of the last sw_wf_allocate_types call (SW_WFT_NEAR, SW_WFT_COARSE)

    @property
    def name(self):
        return self._name

    def _engine(self):
        if self._native is None:
            self._native = sw_native.Solver(device=0)
        return self._native

    def get_allocation(self, unflattened_throughputs, scale_factors, unflattened_priority_weights,
                       cluster_spec, entity_weights=None, entity_to_job_mapping=None, verbose=False,
                       return_effective_throughputs=False):
        throughputs, index = _flatten(unflattened_throughputs, cluster_spec)
        if throughputs is None:
            return None
        m, n = throughputs.shape
        job_ids, worker_types = index
        if not (throughputs == throughputs[:, :1]).all():
            if not self._worker_types:
                raise NotImplementedError(
                    "water filling with throughputs that differ by worker type is not supported: "
                    "the native kernel solves one worker type (or several identical ones)")
            return self._allocate_types(throughputs, job_ids, worker_types, scale_factors,
                                        unflattened_priority_weights, cluster_spec, verbose,
                                        return_effective_throughputs)
        for i, j in enumerate(job_ids):
            if throughputs[i, 0] == 0:
                raise ValueError(f"job {j} has zero throughput: its normalised throughput is undefined")
            if not unflattened_priority_weights[j] > 0:
                raise ValueError(f"job {j} has priority weight {unflattened_priority_weights[j]!r} <= 0")
        workers = [int(cluster_spec[wt]) for wt in worker_types]
        total = sum(workers)
        sf = np.array([scale_factors[j] for j in job_ids], dtype=np.int32)
        # mult_j = (1 / w_j) · sf_j in the reference's float operations (:336-345, :146-148)
        coef = np.array([(1.0 / unflattened_priority_weights[j]) * scale_factors[j] for j in job_ids],
                        dtype=np.float64)
        x, level, used = self._engine().wf_allocate(sf, coef, total)
        self.last_level = (level, used)
        x = np.asarray(x, dtype=np.float64)
        if verbose:
            print("Normalized effective throughputs:", x)
            print("Water level:", level, "allocated workers:", used)
        if n == 1:
            xs = x.reshape(m, 1)
        else:
            xs = np.array([[x[i] * workers[k] / total for k in range(n)] for i in range(m)])
        if return_effective_throughputs:
            return np.sum(xs, axis=1), job_ids
        xs = xs.clip(min=0.0).clip(max=1.0)
        return {job_ids[i]: {worker_types[k]: xs[i, k] for k in range(n)} for i in range(m)}


    def _allocate_types(self, throughputs, job_ids, worker_types, scale_factors, priority_weights, cluster_spec,
                        verbose, return_effective_throughputs):
        """:303-409 over throughputs that differ by worker type."""
        m, n = throughputs.shape
        workers = np.array([int(cluster_spec[wt]) for wt in worker_types], dtype=np.int32)
        for i, j in enumerate(job_ids):
            if not (throughputs[i, workers > 0] > 0).any():
                raise ValueError(f"job {j} has no throughput on a worker type that has workers: "
                                 "its normalised throughput is undefined")
            if not priority_weights[j] > 0:
                raise ValueError(f"job {j} has priority weight {priority_weights[j]!r} <= 0")
        prop = _proportional_throughputs(throughputs, worker_types, cluster_spec)
        sf = np.array([scale_factors[j] for j in job_ids], dtype=np.int32)
        # mult_j = (1 / w_j) · sf_j in the reference's float operations (:336-345, :146-148)
        mult = np.array([(1.0 / priority_weights[j]) * scale_factors[j] for j in job_ids], dtype=np.float64)
        coef = throughputs / prop[:, None] * mult[:, None]
        x, levels, level, steps, stages, flags = self._engine().wf_allocate_types(workers, sf, coef)
        self.last_level = (level, stages)
        self.last_flags = flags
        if flags & (sw_native.Solver.WFT_NEAR | sw_native.Solver.WFT_COARSE):
            warnings.warn("sw_wf_allocate_types: " + " and ".join(
                t for b, t in ((sw_native.Solver.WFT_NEAR, "a job's bottleneck statistic came within a factor 10 "
                                "of its threshold (validated up to 24 jobs; a stage may be spurious)"),
                               (sw_native.Solver.WFT_COARSE, "a stage's solve broke down and was done again at a "
                                "coarser path point and ease")) if flags & b), WaterFillingStageWarning, stacklevel=3)
        x = np.asarray(x, dtype=np.float64)
        if verbose:
            print("Normalized effective throughputs:", np.sum(throughputs * x, axis=1) / prop)
            print("Last water level:", level, "stages:", stages)
        if return_effective_throughputs:
            return np.sum(np.multiply(throughputs, x), axis=1) / prop, job_ids
        x = x.clip(min=0.0).clip(max=1.0)
        return {job_ids[i]: {worker_types[k]: x[i, k] for k in range(n)} for i in range(m)}


class MaxMinFairnessWaterFillingPolicy:
    """max_min_fairness_water_filling.py:412-468: the WithPerf policy with every
    throughput replaced by 1.0."""

    def __init__(self, priority_reweighting_policies=None, native=None):
        _check_reweighting(priority_reweighting_policies)
        self._name = "MaxMinFairnessWaterFilling"
        self._max_min_fairness_perf_policy = MaxMinFairnessWaterFillingPolicyWithPerf(
            priority_reweighting_policies, native)

    @property
    def name(self):
        return self._name

    @property
    def last_level(self):
        return self._max_min_fairness_perf_policy.last_level

    def get_allocation(self, unflattened_throughputs, scale_factors, unflattened_priority_weights,
                       cluster_spec, entity_weights=None, entity_to_job_mapping=None, verbose=False,
                       return_effective_throughputs=False):
        throughputs, index = _flatten(unflattened_throughputs, cluster_spec)
        if throughputs is None:
            return None
        job_ids, worker_types = index
        ones = {j: {wt: 1.0 for wt in unflattened_throughputs[j]} for j in unflattened_throughputs}
        unflattened_x = self._max_min_fairness_perf_policy.get_allocation(
            ones, scale_factors, unflattened_priority_weights, cluster_spec,
            entity_weights=entity_weights, entity_to_job_mapping=entity_to_job_mapping, verbose=verbose,
            return_effective_throughputs=False)
        if return_effective_throughputs:
            # :457-467: the real throughputs over the allocation, normalised by the
            # proportional ones; Σ_k x[j][k] when a job's throughputs are identical
            x = np.array([[unflattened_x[j][wt] for wt in worker_types] for j in job_ids])
            if (throughputs == throughputs[:, :1]).all():
                return np.sum(x, axis=1), job_ids
            prop = _proportional_throughputs(throughputs, worker_types, cluster_spec)
            for i, j in enumerate(job_ids):
                if prop[i] == 0:
                    raise ValueError(f"job {j} has zero throughput: its normalised throughput is undefined")
            return np.sum(np.multiply(throughputs, x), axis=1) / prop, job_ids
        return unflattened_x
