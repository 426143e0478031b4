"""The water-filling policy mirror (max_min_fairness_water_filling.py) and the
simulator's max_min_fairness_water_filling policy, without a GPU: the CPU twin
of the kernel is injected as the engine (tests/test_gpu_wf.py repeats both on
the HIP engine and compares exactly)."""
import json
import os

import numpy as np
import pytest

import ftf_ref
import max_min_fairness_water_filling as wf
import mmf_ref
import sw_sim
import wf_ref
import wfcases as wc

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "sim30_gavel_policies.json")


def test_allocation_over_three_calls_restated_elementwise():
    """Jobs leave and arrive between the calls; the policy keeps no state.  Each
    call's engine arguments and shares are restated per job: c_j = (1/w_j)·sf_j,
    x_j = min(1, L/c_j) with the exact level, clipped to [0, 1]."""
    eng = wf_ref.TwinEngine()
    calls, out, pol = wc.policy_sequence(eng)
    G = 6
    saturated = []
    for call, got, rec in zip(calls, out, eng.calls):
        ids = sorted(call["tp"])
        sf = [call["sf"][j] for j in ids]
        coef = [(1.0 / call["w"][j]) * call["sf"][j] for j in ids]
        rsf, rc, rG, (x, level, used) = rec
        assert list(rsf) == sf and list(rc) == coef and rG == G
        assert sorted(got) == ids
        exact = wf_ref.closed_form_level(sf, coef, G)
        for i, j in enumerate(ids):
            assert got[j] == {"v100": min(1.0, max(0.0, x[i]))}
            assert abs(got[j]["v100"] - min(1.0, float(exact) / coef[i])) <= 1e-15
        assert abs(sum(s * got[j]["v100"] for s, j in zip(sf, ids)) - min(G, sum(sf))) <= 1e-12
        saturated.append(sorted(j for j in ids if got[j]["v100"] == 1.0))
    # L = 3 (shares 1, 1, 3/4), L = 5/4 (1, 5/16, 15/32), then the cluster holds both jobs whole
    assert saturated == [[0, 1], [0], [2, 3]]
    assert pol.last_level == (level, used) and used == 6.0
    assert pol._name == "MaxMinFairnessWaterFilling_Perf"


def args(tp, sf, w, spec):
    ids = sorted(tp)
    return tp, {j: s for j, s in zip(ids, sf)}, {j: v for j, v in zip(ids, w)}, spec


def test_empty_input_returns_none():
    inner = wf.MaxMinFairnessWaterFillingPolicyWithPerf(native=wf_ref.TwinEngine())
    outer = wf.MaxMinFairnessWaterFillingPolicy(native=wf_ref.TwinEngine())
    assert outer._name == "MaxMinFairnessWaterFilling" and outer.name == outer._name
    for pol in (inner, outer):
        assert pol.get_allocation({}, {}, {}, {"v100": 4}) is None
        assert pol.get_allocation({}, {}, {}, {"v100": 4}, return_effective_throughputs=True) is None
        assert pol.get_allocation({0: {}}, {0: 1}, {0: 1.0}, {}) is None  # no worker types


def test_unit_throughput_copy_ignores_the_real_throughputs():
    """max_min_fairness_water_filling.py:437-441: every throughput becomes 1.0,
    so types that differ, and a zero, do not matter."""
    sf, w = [1, 2, 4], [1.0, 2.0, 0.5]
    tp = {j: {"k80": 0.1 * (j + 1), "p100": 0.0, "v100": 5.0 + j} for j in range(3)}
    one = {j: {"v100": 1.0} for j in range(3)}
    e3, e1 = wf_ref.TwinEngine(), wf_ref.TwinEngine()
    a3 = wf.MaxMinFairnessWaterFillingPolicy(native=e3).get_allocation(*args(tp, sf, w, {"k80": 1, "p100": 1, "v100": 2}))
    a1 = wf.MaxMinFairnessWaterFillingPolicyWithPerf(native=e1).get_allocation(*args(one, sf, w, {"v100": 4}))
    assert e3.calls[0][2] == 4 and wc.same_bits(e3.calls[0][3], e1.calls[0][3])
    assert np.array_equal(e3.calls[0][1], e1.calls[0][1])
    assert sorted(a3[0]) == ["k80", "p100", "v100"] and sorted(a1[0]) == ["v100"]
    for j in range(3):
        assert abs(sum(a3[j].values()) - a1[j]["v100"]) <= 1e-15


def test_identical_types_reduce_to_one_type_and_split_by_workers():
    sf, w = [1, 2, 4, 1, 2], [1.0, 0.5, 2.0, 3.0, 1.0]
    spec = {"a": 1, "b": 2, "c": 3}
    tp3 = {j: {t: 3.0 + j for t in spec} for j in range(5)}
    tp1 = {j: {"v100": 3.0 + j} for j in range(5)}
    p3 = wf.MaxMinFairnessWaterFillingPolicyWithPerf(native=wf_ref.TwinEngine())
    p1 = wf.MaxMinFairnessWaterFillingPolicyWithPerf(native=wf_ref.TwinEngine())
    a3 = p3.get_allocation(*args(tp3, sf, w, spec))
    a1 = p1.get_allocation(*args(tp1, sf, w, {"v100": 6}))
    assert p3.last_level == p1.last_level
    for j in range(5):
        for t, k in spec.items():
            assert a3[j][t] == a1[j]["v100"] * k / 6
        assert sum(a3[j].values()) <= 1.0 + 1e-15
    for t, k in spec.items():  # every type's capacity holds
        assert sum(sf[j] * a3[j][t] for j in range(5)) <= k * (1 + 1e-12)


def test_return_effective_throughputs():
    sf, w = [1, 2, 4, 1, 2], [1.0, 0.5, 2.0, 3.0, 1.0]
    spec = {"a": 1, "b": 2, "c": 3}
    tp3 = {j: {t: 3.0 + j for t in spec} for j in range(5)}
    for cls in (wf.MaxMinFairnessWaterFillingPolicyWithPerf, wf.MaxMinFairnessWaterFillingPolicy):
        alloc = cls(native=wf_ref.TwinEngine()).get_allocation(*args(tp3, sf, w, spec))
        eff, ids = cls(native=wf_ref.TwinEngine()).get_allocation(*args(tp3, sf, w, spec),
                                                                  return_effective_throughputs=True)
        assert ids == [0, 1, 2, 3, 4] and len(eff) == 5
        for i, j in enumerate(ids):
            assert abs(eff[i] - sum(alloc[j].values())) <= 1e-15
    # verbose prints and changes nothing; the entity arguments are accepted and unused
    pol = wf.MaxMinFairnessWaterFillingPolicy(native=wf_ref.TwinEngine())
    assert pol.get_allocation(*args(tp3, sf, w, spec), entity_weights=None, entity_to_job_mapping=None) == alloc


def test_errors():
    eng = wf_ref.TwinEngine()
    for cls in (wf.MaxMinFairnessWaterFillingPolicyWithPerf, wf.MaxMinFairnessWaterFillingPolicy):
        with pytest.raises(NotImplementedError):
            cls(priority_reweighting_policies={0: "fairness"}, native=eng)
        with pytest.raises(NotImplementedError):
            cls({0: "fifo"})
    pol = wf.MaxMinFairnessWaterFillingPolicyWithPerf(native=eng)
    differ = {0: {"p100": 1.0, "v100": 2.0}, 1: {"p100": 1.0, "v100": 1.0}}
    with pytest.raises(NotImplementedError):
        pol.get_allocation(*args(differ, [1, 1], [1.0, 1.0], {"p100": 2, "v100": 2}))
    with pytest.raises(ValueError, match="job 7"):
        pol.get_allocation(*args({0: {"v100": 2.0}, 7: {"v100": 0.0}}, [1, 1], [1.0, 1.0], {"v100": 2}))
    for bad in (0.0, -1.0):
        for p in (pol, wf.MaxMinFairnessWaterFillingPolicy(native=eng)):
            with pytest.raises(ValueError, match="job 5"):
                p.get_allocation(*args({2: {"v100": 2.0}, 5: {"v100": 1.0}}, [1, 1], [1.0, bad], {"v100": 1}))
    assert eng.calls == []


@pytest.fixture(scope="module")
def sim30():
    rec = {"workers": [], "allocations": []}
    return wc.simulate_30("max_min_fairness_water_filling", rec, wf_allocator=wf_ref.twin_allocator), rec


def test_simulation_completes_within_capacity(sim30):
    s, rec = sim30
    assert s["policy"] == "MaxMinFairnessWaterFilling"
    assert s["jobs_completed"] == 30 and all(v is not None for v in s["jcts"].values())
    assert s["makespan"] > 0 and s["solves"] >= 1 and 0 < s["utilization"] <= 1.0
    assert rec["workers"] and rec["allocations"]
    for used in rec["workers"]:
        assert len(used) == len(set(used)) <= 8
    for alloc in rec["allocations"]:
        assert all(0.0 <= v <= 1.0 for v in alloc.values())


def test_simulation_is_deterministic(sim30):
    again = wc.simulate_30("max_min_fairness_water_filling", wf_allocator=wf_ref.twin_allocator)
    first = dict(sim30[0])
    for s in (first, again):
        s.pop("solve_seconds")
    assert first == again


def test_existing_policies_are_unchanged_on_the_same_prefix():
    """tests/golden/sim30_gavel_policies.json: the summaries of the two Gavel
    baselines on the 30-job prefix, recorded with the twin engines on the
    commit before the water-filling policy was added.  Neither touches the new
    allocator."""
    def untouched(*_):
        raise AssertionError("the water-filling allocator was called")

    want = json.load(open(GOLDEN))
    got = {
        "max_min_fairness": wc.simulate_30("max_min_fairness", mmf_allocator=mmf_ref.twin_allocator,
                                           wf_allocator=untouched),
        "finish_time_fairness": wc.simulate_30("finish_time_fairness", ftf_allocator=ftf_ref.TwinEngine(),
                                               wf_allocator=untouched),
    }
    for s in got.values():
        s.pop("solve_seconds")
    assert json.loads(json.dumps(got)) == want


def test_policy_name_is_listed():
    assert sw_sim.POLICY_NAMES["max_min_fairness_water_filling"] == "MaxMinFairnessWaterFilling"
    assert sw_sim.POLICY_NAMES["max_min_fairness"] == "MaxMinFairness"
    with pytest.raises(ValueError):
        sw_sim.Simulator("max_min_fairness_water_filling_packing", {}, {})
