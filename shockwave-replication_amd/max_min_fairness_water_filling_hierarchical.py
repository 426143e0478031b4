"""Host mirror of the Gavel water-filling MaxMinFairness policies with the
entity hierarchy (scheduler/policies/max_min_fairness_water_filling.py:21-77,
:412-556: ``priority_reweighting_policies`` "fairness" or "fifo" per entity)
over the native kernel ``sw_wfh_allocate``.

The reference's constructor argument and call signature:
``Policy(priority_reweighting_policies)`` with a dict entity → "fairness" |
"fifo", and ``policy.get_allocation(unflattened_throughputs, scale_factors,
priority_weights, cluster_spec, entity_weights=None,
entity_to_job_mapping=None, verbose=False,
return_effective_throughputs=False)`` → ``{job_id: {worker_type: share}}`` (or
None when there are no jobs).  ``entity_weights`` maps an entity to its weight
and ``entity_to_job_mapping`` to the list of its job ids.  The stage loop with
its per-stage reweighting is replaced by the fixed point of the process that
the reference's comments state (:41-45, :61-62), two nested water fillings in
one kernel: the entities share the cluster in proportion to
their weights, a "fairness" entity shares its capacity among its jobs in
proportion to their priority weights, a "fifo" entity fills its jobs in
ascending job id.

As in the flat mirror (max_min_fairness_water_filling.py): several worker types
with identical per-job throughputs reduce to one type with Σ workers;
throughputs that differ by worker type raise ``NotImplementedError``;
``return_effective_throughputs=True`` returns the normalised effective
throughputs and the job ids; the result is clipped to [0, 1]; a native error
raises, there is no CPU fallback.

``ValueError``: ``entity_to_job_mapping`` is None (:33-37); a mode other than
"fairness" or "fifo" (:75-76); an entity without a mode or a weight; a job in
no entity or in two (the reference would leave it without a weight, or give it
the later entity's); an entity weight that is not finite and > 0; a priority
weight ≤ 0 or a zero throughput, naming the job.  A job id in the mapping that
is not among the jobs is ignored, as in the reference (:48-50 only skip it).
"""
import math

import numpy as np

import sw_native
from max_min_fairness_water_filling import _flatten, _proportional_throughputs

_MODES = {"fairness": 0, "fifo": 1}


class MaxMinFairnessWaterFillingHierarchicalPolicyWithPerf:
    """max_min_fairness_water_filling.py:471-556 with a reweighting policy per entity."""

    def __init__(self, priority_reweighting_policies, native=None):
        if priority_reweighting_policies is None:
            raise ValueError("priority_reweighting_policies is None: use MaxMinFairnessWaterFillingPolicyWithPerf")
        for entity, mode in priority_reweighting_policies.items():
            if mode not in _MODES:
                raise ValueError(f"Unknown priority reweighting policy {mode!r} for entity {entity!r}")
        self._name = "MaxMinFairnessWaterFilling_Perf"
        self._priority_reweighting_policies = dict(priority_reweighting_policies)
        self._native = native
        self.last_level = None  # (C*, Σ sf_j·x_j) of the last solve
        self.last_entity_capacity = None  # {entity: g_e} of the last solve

    @property
    def name(self):
        return self._name

    def _engine(self):
        if self._native is None:
            self._native = sw_native.Solver(device=0)
        return self._native

    def _entities(self, job_ids, entity_weights, entity_to_job_mapping):
        """The entity index of every job, and the entities' ids, weights and modes."""
        if entity_to_job_mapping is None:
            raise ValueError("entity_to_job_mapping cannot be None when priority_reweighting_policies is not None!")
        if entity_weights is None:
            raise ValueError("entity_weights cannot be None when priority_reweighting_policies is not None!")
        entities = list(entity_to_job_mapping)
        row = {j: i for i, j in enumerate(job_ids)}
        ent = np.full(len(job_ids), -1, dtype=np.int32)
        weights, modes = [], []
        for e, entity in enumerate(entities):
            if entity not in self._priority_reweighting_policies:
                raise ValueError(f"entity {entity!r} has no priority reweighting policy")
            if entity not in entity_weights:
                raise ValueError(f"entity {entity!r} has no weight")
            wgt = float(entity_weights[entity])
            if not (wgt > 0 and math.isfinite(wgt)):
                raise ValueError(f"entity {entity!r} has weight {entity_weights[entity]!r}: not finite and > 0")
            weights.append(wgt)
            modes.append(_MODES[self._priority_reweighting_policies[entity]])
            for j in entity_to_job_mapping[entity]:
                if j not in row:
                    continue
                if ent[row[j]] >= 0:
                    raise ValueError(f"job {j} is in two entities: {entities[ent[row[j]]]!r} and {entity!r}")
                ent[row[j]] = e
        for i, j in enumerate(job_ids):
            if ent[i] < 0:
                raise ValueError(f"job {j} is in no entity")
        return ent, entities, np.array(weights, dtype=np.float64), np.array(modes, dtype=np.int32)

    def get_allocation(self, unflattened_throughputs, scale_factors, unflattened_priority_weights,
                       cluster_spec, entity_weights=None, entity_to_job_mapping=None, verbose=False,
                       return_effective_throughputs=False):
        throughputs, index = _flatten(unflattened_throughputs, cluster_spec)
        if throughputs is None:
            return None
        m, n = throughputs.shape
        job_ids, worker_types = index
        ent, entities, weights, modes = self._entities(job_ids, entity_weights, entity_to_job_mapping)
        if not (throughputs == throughputs[:, :1]).all():
            raise NotImplementedError(
                "water filling with throughputs that differ by worker type is not supported: "
                "the native kernel solves one worker type (or several identical ones)")
        for i, j in enumerate(job_ids):
            if throughputs[i, 0] == 0:
                raise ValueError(f"job {j} has zero throughput: its normalised throughput is undefined")
            if not unflattened_priority_weights[j] > 0:
                raise ValueError(f"job {j} has priority weight {unflattened_priority_weights[j]!r} <= 0")
        workers = [int(cluster_spec[wt]) for wt in worker_types]
        total = sum(workers)
        sf = np.array([scale_factors[j] for j in job_ids], dtype=np.int32)
        coef = np.array([(1.0 / unflattened_priority_weights[j]) * scale_factors[j] for j in job_ids],
                        dtype=np.float64)
        x, g, level, used = self._engine().wfh_allocate(sf, coef, ent, weights, modes, total)
        self.last_level = (level, used)
        self.last_entity_capacity = {entity: float(g[e]) for e, entity in enumerate(entities)}
        x = np.asarray(x, dtype=np.float64)
        if verbose:
            print("Normalized effective throughputs:", x)
            print("Entity level:", level, "allocated workers:", used)
        if n == 1:
            xs = x.reshape(m, 1)
        else:
            xs = np.array([[x[i] * workers[k] / total for k in range(n)] for i in range(m)])
        if return_effective_throughputs:
            return np.sum(xs, axis=1), job_ids
        xs = xs.clip(min=0.0).clip(max=1.0)
        return {job_ids[i]: {worker_types[k]: xs[i, k] for k in range(n)} for i in range(m)}


class MaxMinFairnessWaterFillingHierarchicalPolicy:
    """max_min_fairness_water_filling.py:412-468 with a reweighting policy per
    entity: the WithPerf policy with every throughput replaced by 1.0."""

    def __init__(self, priority_reweighting_policies, native=None):
        self._name = "MaxMinFairnessWaterFilling"
        self._max_min_fairness_perf_policy = MaxMinFairnessWaterFillingHierarchicalPolicyWithPerf(
            priority_reweighting_policies, native)

    @property
    def name(self):
        return self._name

    @property
    def last_level(self):
        return self._max_min_fairness_perf_policy.last_level

    @property
    def last_entity_capacity(self):
        return self._max_min_fairness_perf_policy.last_entity_capacity

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
            # :457-467: the real throughputs over the allocation, normalised by the proportional ones
            x = np.array([[unflattened_x[j][wt] for wt in worker_types] for j in job_ids])
            if (throughputs == throughputs[:, :1]).all():
                return np.sum(x, axis=1), job_ids
            prop = _proportional_throughputs(throughputs, worker_types, cluster_spec)
            for i, j in enumerate(job_ids):
                if prop[i] == 0:
                    raise ValueError(f"job {j} has zero throughput: its normalised throughput is undefined")
            return np.sum(np.multiply(throughputs, x), axis=1) / prop, job_ids
        return unflattened_x
