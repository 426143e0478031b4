"""The MinTotalDuration policy mirror (min_total_duration.py) and the
simulator's min_total_duration policy, without a GPU: the CPU twin of the
kernel is injected as the engine (tests/test_gpu_mtd.py repeats both on the
HIP engine and compares exactly)."""
import json
import os

import numpy as np
import pytest

import min_total_duration as mtd
import mtd_ref
import mtdcases as mc
import sw_sim

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "sim30_min_total_duration.json")


def test_engine_arguments_and_shares_over_three_calls():
    """min_total_duration.py:62-106 over three calls, restated per job: the
    policy keeps no state, p_j = steps_j / tp_j in sorted id order, and the
    shares are the engine's, clipped."""
    eng = mtd_ref.TwinEngine()
    calls, out, pol = mc.policy_sequence(eng)
    for c, got, rec in zip(calls, out, eng.calls):
        ids = sorted(c["tp"])
        sf = [c["sf"][j] for j in ids]
        p = [c["rem"][j] / c["tp"][j] for j in ids]
        rsf, rp, rG, (x, T, mu) = rec
        assert list(rsf) == sf and list(rp) == p and rG == 4
        assert sorted(got) == ids
        for i, j in enumerate(ids):
            assert got[j] == {"v100": min(1.0, max(0.0, x[i]))}
        mc.check_allocation((np.array(sf, dtype=np.int32), np.array(p), 4), x, T, mu)
    assert pol.last_level == (T, mu)
    assert pol._name == "MinTotalDuration_Perf" and pol.name == pol._name


def test_empty_input_returns_none():
    pol = mtd.MinTotalDurationPolicyWithPerf(native=mtd_ref.TwinEngine())
    assert pol.get_allocation({}, {}, {}, {"v100": 4}) is None
    outer = mtd.MinTotalDurationPolicy(native=mtd_ref.TwinEngine())
    assert outer._name == "MinTotalDuration" and outer.name == "MinTotalDuration"
    assert outer.get_allocation({}, {}, {}, {"v100": 4}) is None
    assert mtd.MinTotalDurationPolicy()._min_total_duration_perf_policy._native is None  # (solver=None, native=None)


def args(tp, sf, G):
    ids = sorted(tp)
    return tp, {j: s for j, s in zip(ids, sf)}, {j: 20000 + 1000 * j for j in ids}, G


def test_v100_throughput_is_copied_to_every_type():
    """min_total_duration.py:25-31: the other types' throughputs are not read."""
    sf = [1, 2, 1]
    tp = {j: {"k80": 0.1 * (j + 1), "p100": 0.0, "v100": 5.0 + j} for j in range(3)}
    one = {j: {"v100": 5.0 + j} for j in range(3)}
    e3, e1 = mtd_ref.TwinEngine(), mtd_ref.TwinEngine()
    a3 = mtd.MinTotalDurationPolicy(native=e3).get_allocation(*args(tp, sf, {"k80": 1, "p100": 2, "v100": 3}))
    a1 = mtd.MinTotalDurationPolicy(native=e1).get_allocation(*args(one, sf, {"v100": 6}))
    # the kernel saw the v100 throughputs on the summed workers
    assert e3.calls[0][2] == 6
    assert np.array_equal(e3.calls[0][1], e1.calls[0][1])
    assert sorted(a3[0]) == ["k80", "p100", "v100"] and sorted(a1[0]) == ["v100"]


def test_identical_types_reduce_to_one_type_on_the_summed_workers():
    sf = [1, 2, 4, 1, 2]
    spec = {"a": 2, "b": 3, "c": 5}
    tp3 = {j: {t: 3.0 + j for t in spec} for j in range(5)}
    tp1 = {j: {"v100": 3.0 + j} for j in range(5)}
    p3 = mtd.MinTotalDurationPolicyWithPerf(native=mtd_ref.TwinEngine())
    p1 = mtd.MinTotalDurationPolicyWithPerf(native=mtd_ref.TwinEngine())
    a3 = p3.get_allocation(*args(tp3, sf, spec))
    a1 = p1.get_allocation(*args(tp1, sf, {"v100": 10}))
    assert p3.last_level == p1.last_level  # the same engine call
    for j in range(5):
        assert abs(sum(a3[j].values()) - a1[j]["v100"]) <= 1e-15
        assert sum(a3[j].values()) <= 1.0 + 1e-12
        for t, w in spec.items():
            assert a3[j][t] == a1[j]["v100"] * w / 10
    for t, w in spec.items():  # every type's capacity holds
        assert sum(sf[j] * a3[j][t] for j in range(5)) <= w * (1 + 1e-12)


def test_types_that_differ_are_not_implemented():
    tp = {0: {"p100": 1.0, "v100": 2.0}, 1: {"p100": 1.0, "v100": 1.0}}
    pol = mtd.MinTotalDurationPolicyWithPerf(native=mtd_ref.TwinEngine())
    with pytest.raises(NotImplementedError):
        pol.get_allocation(*args(tp, [1, 1], {"p100": 2, "v100": 2}))


def test_zero_throughput_names_the_job():
    tp = {0: {"v100": 2.0}, 7: {"v100": 0.0}}
    pol = mtd.MinTotalDurationPolicy(native=mtd_ref.TwinEngine())
    with pytest.raises(ValueError, match="job 7"):
        pol.get_allocation(*args(tp, [1, 1], {"v100": 2}))


def test_a_negative_remainder_is_the_row_of_zero_steps():
    """tp·x ≥ steps/T with x ≥ 0 is the same row for steps = −40 and steps = 0."""
    tp = {0: {"v100": 2.0}, 1: {"v100": 5.0}}
    e_neg, e_zero = mtd_ref.TwinEngine(), mtd_ref.TwinEngine()
    a_neg = mtd.MinTotalDurationPolicy(native=e_neg).get_allocation(tp, {0: 1, 1: 2}, {0: 9000, 1: -40}, {"v100": 2})
    a_zero = mtd.MinTotalDurationPolicy(native=e_zero).get_allocation(tp, {0: 1, 1: 2}, {0: 9000, 1: 0}, {"v100": 2})
    assert list(e_neg.calls[0][1]) == [4500.0, 0.0]
    assert a_neg == a_zero


@pytest.fixture(scope="module")
def sim30():
    rec = {"workers": [], "allocations": []}
    return mc.simulate_30(mtd_ref.TwinEngine(), rec), rec


def test_simulation_completes_within_capacity(sim30):
    s, rec = sim30
    assert s["policy"] == "MinTotalDuration"
    assert s["jobs_completed"] == 30 and all(v is not None for v in s["jcts"].values())
    assert s["makespan"] > 0 and s["solves"] >= 1 and 0 < s["utilization"] <= 1.0
    assert rec["workers"] and rec["allocations"]
    for used in rec["workers"]:
        assert len(used) == len(set(used)) <= 8
    for alloc in rec["allocations"]:
        assert all(0.0 <= v <= 1.0 for v in alloc.values())


def test_simulation_is_deterministic_and_matches_the_record(sim30):
    """tests/golden/sim30_min_total_duration.json: the summary of the 30-job,
    8-GPU simulation on the twin engine."""
    again = mc.simulate_30(mtd_ref.TwinEngine())
    first = dict(sim30[0])
    for s in (first, again):
        s.pop("solve_seconds")
    assert first == again
    assert json.loads(json.dumps(first)) == json.load(open(GOLDEN))


def test_policy_name_is_listed():
    assert sw_sim.POLICY_NAMES["min_total_duration"] == "MinTotalDuration"
    with pytest.raises(ValueError):
        sw_sim.Simulator("min_total_duration_packing", {}, {})
