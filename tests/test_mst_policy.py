"""The max-sum-throughput policy mirror (max_sum_throughput.py) and the
simulator's max_sum_throughput_perf policy, without a GPU: the CPU twin of the
kernel is injected as the engine (tests/test_gpu_mst.py repeats both on the
HIP engine and compares exactly)."""
import json
import os

import numpy as np
import pytest

import max_sum_throughput as mst
import mst_ref
import mstcases as mc
import sw_sim

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "sim30_max_sum_throughput.json")
WARNING = "WARNING: No allocation possible with provided SLOs!"


def v100(tp):
    return {j: {"v100": v} for j, v in tp.items()}


def test_engine_arguments_and_shares_over_three_calls():
    """max_sum_throughput.py:45-96 over three calls, restated per job: the
    policy keeps no state, jobs in sorted id order, w_j = tp_j / cost,
    l_j = (steps_j / SLO_j) / tp_j, and the shares are the engine's, clipped."""
    eng = mst_ref.TwinEngine()
    calls, out, pol = mc.policy_sequence(eng)
    for c, got, rec in zip(calls, out, eng.calls):
        ids = sorted(c["tp"])
        cost = c["kw"].get("instance_costs", {"v100": 1.0})["v100"]
        sf = [c["sf"][j] for j in ids]
        w = [c["tp"][j] / cost for j in ids]
        rsf, rw, rl, rG, (x, lam, m, obj, dropped) = rec
        assert list(rsf) == sf and list(rw) == w and rG == 2
        slos = c["kw"].get("SLOs", {})
        if slos:
            steps = c["kw"]["num_steps_remaining"]
            assert list(rl) == [steps[j] / slos[j] / c["tp"][j] if j in slos else 0.0 for j in ids]
        else:
            assert rl is None
        assert sorted(got) == ids
        for i, j in enumerate(ids):
            assert got[j] == {"v100": min(1.0, max(0.0, x[i]))}
        mst_ref.check_allocation((np.array(sf, dtype=np.int32), np.array(w), rl, 2), x, lam, m, obj, dropped,
                                 cap_excess=mc.CAP_BAR)
    assert pol.last_level == (lam, m, obj, dropped)
    # first call: the two dense jobs fill the cluster; second: three tied jobs share it equally
    assert out[0] == {0: {"v100": 1.0}, 1: {"v100": 0.0}, 2: {"v100": 1.0}}
    assert out[1][0] == out[1][2] == out[1][4] and abs(out[1][0]["v100"] - 2 / 3) < 1e-15
    assert out[2][3] == {"v100": 0.25}  # the SLO's floor


def test_names_and_signatures_are_the_references():
    eng = mst_ref.TwinEngine()
    a = mst.ThroughputSumWithPerf(native=eng)
    b = mst.ThroughputNormalizedByCostSumWithPerf(native=eng)
    c = mst.ThroughputNormalizedByCostSumWithPerfSLOs(native=eng)
    assert (a._name, b._name, c._name) == ("ThroughputSumWithPerf", "ThroughputNormalizedByCostSum_Perf",
                                          "ThroughputNormalizedByCostSum_PerfSLOs")
    assert (a.name, b.name, c.name) == (a._name, b._name, c._name)
    tp, sf, spec = v100({0: 3.0, 1: 5.0}), {0: 1, 1: 1}, {"v100": 1}
    want = {0: {"v100": 0.0}, 1: {"v100": 1.0}}
    assert a.get_allocation(tp, sf, spec) == want
    assert b.get_allocation(tp, sf, spec, {"v100": 3.0}) == want
    assert c.get_allocation(tp, sf, spec) == want
    # the threshold is the starved job's density: at it the dense job fits exactly
    assert a.last_level == c.last_level == (3.0, 0.0, 5.0, False)
    assert b.last_level == (1.0, 0.0, 5.0 / 3.0, False)
    assert mst.ThroughputSumWithPerf()._policy._native is None  # (solver=None, native=None)


def test_empty_input_returns_none():
    for pol in (mst.ThroughputSumWithPerf(native=mst_ref.TwinEngine()),
                mst.ThroughputNormalizedByCostSumWithPerfSLOs(native=mst_ref.TwinEngine())):
        assert pol.get_allocation({}, {}, {"v100": 4}) is None
    pol = mst.ThroughputNormalizedByCostSumWithPerf(native=mst_ref.TwinEngine())
    assert pol.get_allocation({}, {}, {"v100": 4}, {"v100": 1.0}) is None


def test_identical_types_reduce_to_one_type_on_the_summed_workers():
    sf = {j: s for j, s in enumerate([1, 2, 4, 1, 2])}
    spec = {"a": 2, "b": 1, "c": 1}
    tp3 = {j: {t: 3.0 + j for t in spec} for j in range(5)}
    tp1 = {j: {"v100": 3.0 + j} for j in range(5)}
    p3 = mst.ThroughputSumWithPerf(native=mst_ref.TwinEngine())
    p1 = mst.ThroughputSumWithPerf(native=mst_ref.TwinEngine())
    a3 = p3.get_allocation(tp3, sf, spec)
    a1 = p1.get_allocation(tp1, sf, {"v100": 4})
    assert p3.last_level == p1.last_level  # the same engine call
    for j in range(5):
        assert abs(sum(a3[j].values()) - a1[j]["v100"]) <= 1e-15
        for t, w in spec.items():
            assert a3[j][t] == a1[j]["v100"] * w / 4
    for t, w in spec.items():  # every type's capacity holds
        assert sum(sf[j] * a3[j][t] for j in range(5)) <= w * (1 + 1e-12)
    # identical costs across the types are the one-type case too
    pc = mst.ThroughputNormalizedByCostSumWithPerf(native=mst_ref.TwinEngine())
    assert pc.get_allocation(tp3, sf, spec, {t: 2.0 for t in spec}) == a3


def test_types_or_costs_that_differ_are_not_implemented():
    sf, spec = {0: 1, 1: 1}, {"p100": 2, "v100": 2}
    differ = {0: {"p100": 1.0, "v100": 2.0}, 1: {"p100": 1.0, "v100": 1.0}}
    same = {0: {"p100": 2.0, "v100": 2.0}, 1: {"p100": 1.0, "v100": 1.0}}
    with pytest.raises(NotImplementedError):
        mst.ThroughputSumWithPerf(native=mst_ref.TwinEngine()).get_allocation(differ, sf, spec)
    pol = mst.ThroughputNormalizedByCostSumWithPerf(native=mst_ref.TwinEngine())
    with pytest.raises(NotImplementedError):
        pol.get_allocation(same, sf, spec, {"p100": 1.0, "v100": 3.0})
    assert pol.get_allocation(same, sf, spec, {"p100": 3.0, "v100": 3.0}) is not None


def slo_policy():
    eng = mst_ref.TwinEngine()
    return mst.ThroughputNormalizedByCostSumWithPerfSLOs(native=eng), eng


TP, SF, SPEC = v100({0: 10.0, 1: 4.0, 2: 2.0}), {0: 1, 1: 1, 2: 1}, {"v100": 2}


def test_slo_feasible_sets_the_floor(capsys):
    pol, eng = slo_policy()
    a = pol.get_allocation(TP, SF, SPEC, SLOs={2: 1000.0}, num_steps_remaining={2: 1200, 0: 5})
    assert list(eng.calls[0][2]) == [0.0, 0.0, 1200 / 1000.0 / 2.0]
    assert a[0] == {"v100": 1.0} and a[2] == {"v100": 0.6} and abs(a[1]["v100"] - 0.4) < 1e-15
    assert pol.last_level[3] is False and WARNING not in capsys.readouterr().out


def test_slo_infeasible_is_dropped_with_the_references_warning(capsys):
    pol, _ = slo_policy()
    a = pol.get_allocation(TP, SF, SPEC, SLOs={2: 100.0}, num_steps_remaining={2: 1200})  # floor 6 > 1
    assert capsys.readouterr().out.strip() == WARNING
    assert pol.last_level[3] is True
    assert a == pol.get_allocation(TP, SF, SPEC)  # the solve without the SLO rows
    # a zero throughput with steps to run cannot meet any SLO
    pol.get_allocation(v100({0: 10.0, 1: 0.0}), {0: 1, 1: 1}, SPEC, SLOs={1: 50.0}, num_steps_remaining={1: 10})
    assert capsys.readouterr().out.strip() == WARNING


def test_slo_rows_with_nothing_left_to_ask_are_vacuous(capsys):
    """steps/SLO ≤ 0 (no steps left, or a deadline that has passed) holds for
    every x ≥ 0: the allocation is the one without the row."""
    pol, eng = slo_policy()
    plain = pol.get_allocation(TP, SF, SPEC)
    for slo, steps in [(1000.0, 0), (-5.0, 1200), (1000.0, -3)]:
        assert pol.get_allocation(TP, SF, SPEC, SLOs={2: slo}, num_steps_remaining={2: steps}) == plain
        assert list(eng.calls[-1][2]) == [0.0, 0.0, 0.0]
    assert WARNING not in capsys.readouterr().out


def test_slo_job_without_steps_asserts_and_zero_slo_divides_by_zero():
    pol, _ = slo_policy()
    with pytest.raises(AssertionError):
        pol.get_allocation(TP, SF, SPEC, SLOs={2: 1000.0}, num_steps_remaining={0: 5})
    with pytest.raises(ZeroDivisionError):
        pol.get_allocation(TP, SF, SPEC, SLOs={2: 0}, num_steps_remaining={2: 1200})


def test_scaling_all_costs_leaves_the_allocation_unchanged():
    rng = np.random.default_rng(9)
    sf, tp, _, G = mc.draw(rng, 40, fill=0.4)
    tpd, sfd = v100(dict(enumerate(tp))), dict(enumerate(int(s) for s in sf))
    pol = mst.ThroughputNormalizedByCostSumWithPerf(native=mst_ref.TwinEngine())
    a1 = pol.get_allocation(tpd, sfd, {"v100": G}, {"v100": 1.0})
    l1 = pol.last_level
    a4 = pol.get_allocation(tpd, sfd, {"v100": G}, {"v100": 4.0})  # a power of two: every density scales exactly
    assert a1 == a4
    assert pol.last_level[0] == l1[0] / 4.0 and pol.last_level[2] == l1[2] / 4.0
    a3 = pol.get_allocation(tpd, sfd, {"v100": G}, {"v100": 3.0})
    for j in a1:
        assert abs(a1[j]["v100"] - a3[j]["v100"]) <= 1e-12


@pytest.fixture(scope="module")
def sim30():
    rec = {"workers": [], "allocations": []}
    return mc.simulate_30(mst_ref.TwinEngine(), rec), rec


def test_simulation_completes_within_capacity(sim30):
    s, rec = sim30
    assert s["policy"] == "ThroughputSumWithPerf"
    assert s["jobs_completed"] == 30 and all(v is not None for v in s["jcts"].values())
    assert s["makespan"] > 0 and s["solves"] >= 1 and 0 < s["utilization"] <= 1.0
    assert rec["workers"] and rec["allocations"]
    for used in rec["workers"]:
        assert len(used) == len(set(used)) <= 8
    for alloc in rec["allocations"]:
        assert all(0.0 <= v <= 1.0 for v in alloc.values())


def test_simulation_is_deterministic_and_matches_the_record(sim30):
    """tests/golden/sim30_max_sum_throughput.json: the summary of the 30-job,
    8-GPU simulation on the twin engine."""
    again = mc.simulate_30(mst_ref.TwinEngine())
    first = dict(sim30[0])
    for s in (first, again):
        s.pop("solve_seconds")
    assert first == again
    assert json.loads(json.dumps(first)) == json.load(open(GOLDEN))


def test_policy_name_is_listed():
    assert sw_sim.POLICY_NAMES["max_sum_throughput_perf"] == "ThroughputSumWithPerf"
    with pytest.raises(ValueError):
        sw_sim.Simulator("max_sum_throughput_packing", {}, {})
