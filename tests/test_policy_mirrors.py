"""The seven host mirrors of the Gavel policies, replayed on the CPU twins
against tests/golden/policy_mirrors.json (written by
tests/golden/make_policy_mirrors.py from ``record()`` below, at the commit
before the mirrors were moved onto sw_policy.py).

For every public policy class: the allocation, the ``last_*`` attributes, the
warnings and, where the call raises, the exception's type and full text, on

  * one worker type with 5 jobs;
  * three identical types with 2, 3 and 5 workers and 5 jobs (and, where the
    class has it, ``return_effective_throughputs=True`` there);
  * 3 types that differ, one without workers, and 6 jobs: with
    ``worker_types=True`` / ``centred=True`` where the class takes it, and
    without (the exception, or the default path's result);
  * no jobs, and jobs without types;
  * three calls in a row on one object (the state FinishTimeFairness and AlloX
    keep between calls), remaining steps that grew between two calls, and a job
    with no steps left (its expected isolated time is not positive);
  * a zero throughput, and a priority weight that is not positive.

Every float is compared through ``float.hex``: the comparison is exact.
"""
import functools
import json
import os
import warnings

import numpy as np
import pytest

import allox
import allox_ref
import finish_time_fairness as ftf
import ftftcases
import max_min_fairness as mmf
import max_min_fairness_water_filling as wf
import max_min_fairness_water_filling_hierarchical as wfh
import max_sum_throughput as mst
import min_total_duration as mtd
import mmfccases
import mst_ref
import mtdtcases
import wfh_ref
import wftcases

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "policy_mirrors.json")
REWEIGHTING = {"a": "fairness", "b": "fifo"}


class TwinEngines:
    """Every engine call of the mirrors, backed by the CPU twins."""

    def __init__(self):
        self._engines = [e.TwinEngine() for e in (mmfccases, wftcases, wfh_ref, ftftcases, mtdtcases, mst_ref,
                                                  allox_ref)]

    def __getattr__(self, name):
        for e in self._engines:
            if hasattr(e, name):
                return getattr(e, name)
        raise AttributeError(name)


def _inputs(types, workers, m, differ):
    """m jobs over the types: throughputs (one value per job unless differ),
    scale factors, priority weights, times since start, steps, cluster, entities."""
    rng = np.random.default_rng(20261126 + 100 * len(types) + m + int(differ))
    jobs = [int(j) for j in rng.permutation(m)]
    if differ:
        thr = {j: {wt: float(rng.uniform(0.5, 4.0)) for wt in types} for j in jobs}
    else:
        thr = {j: dict.fromkeys(types, float(rng.uniform(0.5, 4.0))) for j in jobs}
    return {"thr": thr,
            "sf": {j: int(rng.choice([1, 2, 4])) for j in jobs},
            "pw": {j: float(rng.choice([1.0, 2.0, 0.5])) for j in jobs},
            "times": {j: float(rng.uniform(0.0, 5000.0)) for j in jobs},
            "steps": {j: int(rng.integers(1000, 200000)) for j in jobs},
            "spec": dict(zip(types, workers)),
            "weights": {"a": 1.0, "b": 2.0},
            "entities": {"a": [j for j in jobs if j < m // 2], "b": [j for j in jobs if j >= m // 2]}}


def _later(s, k):
    """The inputs k rounds on: less to do, more time gone."""
    t = dict(s)
    t["steps"] = {j: v - 400 * k * (j + 1) for j, v in s["steps"].items()}
    t["times"] = {j: v + 360.0 * k for j, v in s["times"].items()}
    return t


def _with(s, key, job, value):
    t = dict(s)
    t[key] = {j: (dict.fromkeys(v, value) if isinstance(v, dict) else value) if j == job else v
              for j, v in s[key].items()}
    return t


ONE = _inputs(["v100"], [4], 5, False)
SAME = _inputs(["k80", "p100", "v100"], [2, 3, 5], 5, False)
DIFFER = _inputs(["k80", "p100", "v100"], [3, 0, 4], 6, True)

# name → (constructor of the plain object, constructor with the worker-type flag or None, the call)
_PW = lambda p, s, **kw: p.get_allocation(s["thr"], s["sf"], s["pw"], s["spec"], **kw)  # noqa: E731
_WF = lambda p, s, **kw: p.get_allocation(s["thr"], s["sf"], s["pw"], s["spec"], entity_weights=s["weights"],  # noqa: E731
                                          entity_to_job_mapping=s["entities"], **kw)
_FTF = lambda p, s: p.get_allocation(s["thr"], s["sf"], s["pw"], s["times"], s["steps"], s["spec"])  # noqa: E731
_MTD = lambda p, s: p.get_allocation(s["thr"], s["sf"], s["steps"], s["spec"])  # noqa: E731
_ONES = lambda s: dict.fromkeys(s["sf"], 1)  # AlloX takes single-GPU jobs only  # noqa: E731
CLASSES = {
    "MaxMinFairnessPolicyWithPerf": (lambda e: mmf.MaxMinFairnessPolicyWithPerf(native=e),
                                     lambda e: mmf.MaxMinFairnessPolicyWithPerf(native=e, centred=True), _PW),
    "MaxMinFairnessPolicy": (lambda e: mmf.MaxMinFairnessPolicy(native=e),
                             lambda e: mmf.MaxMinFairnessPolicy(native=e, centred=True), _PW),
    "MaxMinFairnessWaterFillingPolicyWithPerf": (
        lambda e: wf.MaxMinFairnessWaterFillingPolicyWithPerf(native=e),
        lambda e: wf.MaxMinFairnessWaterFillingPolicyWithPerf(native=e, worker_types=True), _WF),
    "MaxMinFairnessWaterFillingPolicy": (lambda e: wf.MaxMinFairnessWaterFillingPolicy(native=e), None, _WF),
    "MaxMinFairnessWaterFillingHierarchicalPolicyWithPerf": (
        lambda e: wfh.MaxMinFairnessWaterFillingHierarchicalPolicyWithPerf(REWEIGHTING, native=e), None, _WF),
    "MaxMinFairnessWaterFillingHierarchicalPolicy": (
        lambda e: wfh.MaxMinFairnessWaterFillingHierarchicalPolicy(REWEIGHTING, native=e), None, _WF),
    "FinishTimeFairnessPolicyWithPerf": (
        lambda e: ftf.FinishTimeFairnessPolicyWithPerf(native=e),
        lambda e: ftf.FinishTimeFairnessPolicyWithPerf(native=e, worker_types=True), _FTF),
    "FinishTimeFairnessPolicy": (lambda e: ftf.FinishTimeFairnessPolicy(native=e), None, _FTF),
    "MinTotalDurationPolicyWithPerf": (
        lambda e: mtd.MinTotalDurationPolicyWithPerf(native=e),
        lambda e: mtd.MinTotalDurationPolicyWithPerf(native=e, worker_types=True), _MTD),
    "MinTotalDurationPolicy": (lambda e: mtd.MinTotalDurationPolicy(native=e), None, _MTD),
    "ThroughputNormalizedByCostSumWithPerfSLOs": (
        lambda e: mst.ThroughputNormalizedByCostSumWithPerfSLOs(native=e), None,
        lambda p, s: p.get_allocation(s["thr"], s["sf"], s["spec"], instance_costs=dict.fromkeys(s["spec"], 2.0),
                                      SLOs={min(s["steps"]): 1.0e5}, num_steps_remaining=s["steps"])),
    "ThroughputNormalizedByCostSumWithPerf": (
        lambda e: mst.ThroughputNormalizedByCostSumWithPerf(native=e), None,
        lambda p, s: p.get_allocation(s["thr"], s["sf"], s["spec"], dict.fromkeys(s["spec"], 2.0))),
    "ThroughputSumWithPerf": (lambda e: mst.ThroughputSumWithPerf(native=e), None,
                              lambda p, s: p.get_allocation(s["thr"], s["sf"], s["spec"])),
    "AlloXPolicy": (lambda e: allox.AlloXPolicy(native=e), None,
                    lambda p, s: p.get_allocation(s["thr"], _ONES(s), s["times"], s["steps"], s["spec"])),
}


def _enc(v):
    """The value as JSON: floats as float.hex, dictionary keys as strings."""
    if v is None or isinstance(v, (bool, np.bool_)):
        return None if v is None else bool(v)
    if isinstance(v, (int, np.integer)):
        return int(v)
    if isinstance(v, (float, np.floating)):
        return float(v).hex()
    if isinstance(v, dict):
        return {str(k): _enc(x) for k, x in v.items()}
    if isinstance(v, (list, tuple, np.ndarray)):
        return [_enc(x) for x in v]
    raise TypeError(type(v))


def _calls(make, call, states, **kw):
    """The outcome of every call of the sequence on one object."""
    mmf._WARNED = False  # the once-per-process warning: every sequence starts unwarned
    policy = make(TwinEngines())
    out = []
    for s in states:
        with warnings.catch_warnings(record=True) as caught:
            warnings.simplefilter("always")
            try:
                r = {"returns": _enc(call(policy, s, **kw))}
            except Exception as exc:  # the type and the text are what is compared
                r = {"raises": [type(exc).__name__, str(exc)]}
        r["warnings"] = [[w.category.__name__, str(w.message)] for w in caught]
        r["last"] = {a: _enc(getattr(policy, a)) for a in ("last_level", "last_flags", "last_entity_capacity",
                                                          "last_cost") if hasattr(policy, a)}
        out.append(r)
    return out


def record_class(name):
    plain, flagged, call = CLASSES[name]
    job = min(ONE["sf"])
    out = {"one_type": _calls(plain, call, [ONE]),
           "identical_types": _calls(plain, call, [SAME]),
           "differing_types_unflagged": _calls(plain, call, [DIFFER]),
           "no_jobs": _calls(plain, call, [dict(ONE, thr={})]),
           "no_types": _calls(plain, call, [dict(ONE, thr=dict.fromkeys(ONE["thr"], {}))]),
           "three_calls": _calls(plain, call, [SAME, _later(SAME, 1), _later(SAME, 2)]),
           "three_calls_then_none": _calls(plain, call, [ONE, dict(ONE, thr={}), _later(ONE, 1)]),
           "steps_that_grew": _calls(plain, call, [_later(ONE, 2), ONE]),
           "no_steps_left": _calls(plain, call, [_with(ONE, "steps", job, 0)]),
           "zero_throughput": _calls(plain, call, [_with(ONE, "thr", job, 0.0)]),
           "zero_throughput_identical_types": _calls(plain, call, [_with(SAME, "thr", job, 0.0)]),
           "zero_priority_weight": _calls(plain, call, [_with(ONE, "pw", job, 0.0)]),
           "negative_priority_weight": _calls(plain, call, [_with(SAME, "pw", job, -1.0)])}
    if flagged is not None:
        dead = min(DIFFER["sf"])
        out["differing_types"] = _calls(flagged, call, [DIFFER])
        out["differing_types_three_calls"] = _calls(flagged, call, [DIFFER, _later(DIFFER, 1), _later(DIFFER, 2)])
        out["differing_types_identical_input"] = _calls(flagged, call, [SAME])
        out["differing_types_zero_throughput"] = _calls(flagged, call, [_with(DIFFER, "thr", dead, 0.0)])
        out["differing_types_zero_priority_weight"] = _calls(flagged, call, [_with(DIFFER, "pw", dead, 0.0)])
        out["differing_types_steps_that_grew"] = _calls(flagged, call, [_later(DIFFER, 2), DIFFER])
        out["differing_types_no_steps_left"] = _calls(flagged, call, [_with(DIFFER, "steps", dead, 0)])
    if call is _WF:
        out["effective_throughputs"] = _calls(plain, call, [SAME], return_effective_throughputs=True)
        out["effective_throughputs_one_type"] = _calls(plain, call, [ONE], return_effective_throughputs=True)
        if flagged is not None:
            out["differing_types_effective_throughputs"] = _calls(flagged, call, [DIFFER],
                                                                  return_effective_throughputs=True)
    return out


def record():
    return {name: record_class(name) for name in CLASSES}


@functools.lru_cache(maxsize=None)
def _golden():
    with open(GOLDEN) as f:
        return json.load(f)["classes"]


def test_every_public_policy_class_is_recorded():
    public = {n for mod in (mmf, wf, wfh, ftf, mtd, mst, allox) for n, c in vars(mod).items()
              if isinstance(c, type) and c.__module__ == mod.__name__ and not issubclass(c, Warning)}
    assert public == set(CLASSES) == set(_golden())


@pytest.mark.parametrize("name", sorted(CLASSES))
def test_mirror_matches_recorded_behaviour(name):
    got, want = record_class(name), _golden()[name]
    assert sorted(got) == sorted(want)
    for scenario in want:
        assert got[scenario] == want[scenario], (name, scenario)
    # what the recording is worth: allocations on every path, and the exceptions
    assert all("returns" in r for r in want["one_type"] + want["identical_types"] + want["three_calls"])
    assert want["one_type"][0]["returns"] is not None and want["no_jobs"][0]["returns"] is None


def test_the_recorded_exceptions_cover_every_kind():
    """Throughputs that differ without the flag, a zero throughput, a priority
    weight ≤ 0 and an expected isolated time ≤ 0 each raise in some class."""
    raised = {}
    for name, scenarios in _golden().items():
        for scenario, calls in scenarios.items():
            for r in calls:
                if "raises" in r:
                    raised.setdefault(scenario, set()).add(r["raises"][0])
    assert "NotImplementedError" in raised["differing_types_unflagged"]
    assert "ValueError" in raised["zero_throughput"] and "ValueError" in raised["differing_types_zero_throughput"]
    assert "ValueError" in raised["zero_priority_weight"] and "ValueError" in raised["negative_priority_weight"]
    assert "ValueError" in raised["no_steps_left"] and "ValueError" in raised["differing_types_no_steps_left"]
