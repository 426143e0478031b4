"""The FinishTimeFairness policy mirror (finish_time_fairness.py) and the
simulator's finish_time_fairness policy, without a GPU: the CPU twin of the
kernel is injected as the engine (tests/test_gpu_ftf.py repeats both on the
HIP engine and compares exactly)."""
import numpy as np
import pytest

import finish_time_fairness as ftf
import ftf_ref
import ftfcases as fc
import sw_sim


def isolated_throughput(tp, sf, m, G):
    """isolated.py:34-52 for one worker type, elementwise."""
    x = (G / m) / sf
    return tp * (x / max(x, 1.0))


def test_state_evolves_as_in_the_reference():
    """finish_time_fairness.py:94-133 over three calls, restated per job: the
    cumulative isolated time grows by (previous remaining − remaining) /
    previous isolated throughput, a finished job keeps its entry, a new job
    starts at 0."""
    eng = ftf_ref.TwinEngine()
    calls, out, pol = fc.policy_sequence(eng)
    G = 4
    cum, prev_rem, prev_iso = {}, {}, {}
    for c, got, rec in zip(calls, out, eng.calls):
        ids = sorted(c["tp"])
        m = len(ids)
        E, p, a, sf = [], [], [], []
        iso = {}
        for j in ids:
            cum.setdefault(j, 0)
            if j in prev_rem:
                cum[j] += (prev_rem[j] - c["rem"][j]) / prev_iso[j]
            iso[j] = isolated_throughput(c["tp"][j], c["sf"][j], m, G)
            E.append(cum[j] + c["rem"][j] / iso[j])
            p.append(c["rem"][j] / c["tp"][j])
            a.append(c["t"][j])
            sf.append(c["sf"][j])
        prev_rem, prev_iso = dict(c["rem"]), iso
        rsf, rp, ra, rE, rG, (x, rho, mu) = rec
        assert list(rsf) == sf and rG == G
        assert list(rp) == p and list(ra) == a and list(rE) == E
        assert sorted(got) == ids
        for i, j in enumerate(ids):
            assert got[j] == {"v100": min(1.0, max(0.0, x[i]))}
        fc.check_allocation((np.array(sf), np.array(p), np.array(a), np.array(E), G), x, rho, mu)
    assert pol.last_level == (rho, mu)
    assert pol._cumulative_isolated_time == cum and set(cum) == {0, 1, 2, 3}  # job 1 is never deleted
    assert pol._num_steps_remaining_prev_iteration == calls[-1]["rem"]
    assert pol._isolated_throughputs_prev_iteration == prev_iso
    assert pol._name == "FinishTimeFairness_Perf"


def test_empty_input_returns_none_and_resets_the_previous_iteration():
    _, _, pol = fc.policy_sequence(ftf_ref.TwinEngine())
    cum = dict(pol._cumulative_isolated_time)
    assert pol.get_allocation({}, {}, {}, {}, {}, {"v100": 4}) is None
    assert pol._isolated_throughputs_prev_iteration == {}
    assert pol._num_steps_remaining_prev_iteration == {}
    assert pol._cumulative_isolated_time == cum
    outer = ftf.FinishTimeFairnessPolicy(native=ftf_ref.TwinEngine())
    assert outer._name == "FinishTimeFairness"
    assert outer.get_allocation({}, {}, {}, {}, {}, {"v100": 4}) is None


def args(tp, sf, G):
    ids = sorted(tp)
    return (tp, {j: s for j, s in zip(ids, sf)}, {j: 1.0 for j in ids}, {j: 100.0 * j for j in ids},
            {j: 20000 + 1000 * j for j in ids}, G)


def test_v100_throughput_is_copied_to_every_type():
    """finish_time_fairness.py:35-43: the other types' throughputs are not read."""
    sf = [1, 2, 1]
    tp = {j: {"k80": 0.1 * (j + 1), "p100": 0.0, "v100": 5.0 + j} for j in range(3)}
    one = {j: {"v100": 5.0 + j} for j in range(3)}
    e3, e1 = ftf_ref.TwinEngine(), ftf_ref.TwinEngine()
    a3 = ftf.FinishTimeFairnessPolicy(native=e3).get_allocation(*args(tp, sf, {"k80": 1, "p100": 2, "v100": 3}))
    a1 = ftf.FinishTimeFairnessPolicy(native=e1).get_allocation(*args(one, sf, {"v100": 6}))
    # the kernel saw the v100 throughputs on the summed workers
    assert e3.calls[0][4] == 6
    assert np.array_equal(e3.calls[0][1], e1.calls[0][1])
    assert sorted(a3[0]) == ["k80", "p100", "v100"] and sorted(a1[0]) == ["v100"]


def test_identical_types_reduce_to_one_type_on_the_summed_workers():
    sf = [1, 2, 4, 1, 2]
    spec = {"a": 2, "b": 3, "c": 5}
    tp3 = {j: {t: 3.0 + j for t in spec} for j in range(5)}
    tp1 = {j: {"v100": 3.0 + j} for j in range(5)}
    p3 = ftf.FinishTimeFairnessPolicyWithPerf(native=ftf_ref.TwinEngine())
    p1 = ftf.FinishTimeFairnessPolicyWithPerf(native=ftf_ref.TwinEngine())
    a3 = p3.get_allocation(*args(tp3, sf, spec))
    a1 = p1.get_allocation(*args(tp1, sf, {"v100": 10}))
    # the isolated split over three types sums to the one-type split only up to
    # rounding, so the level agrees to rounding, not bit for bit
    assert abs(p3.last_level[0] - p1.last_level[0]) <= 1e-12 * p1.last_level[0]
    for j in range(5):
        assert abs(sum(a3[j].values()) - a1[j]["v100"]) <= 1e-9
        assert sum(a3[j].values()) <= 1.0 + 1e-12
    for t, w in spec.items():  # every type's capacity holds
        assert sum(sf[j] * a3[j][t] for j in range(5)) <= w * (1 + 1e-12)


def test_types_that_differ_are_not_implemented():
    tp = {0: {"p100": 1.0, "v100": 2.0}, 1: {"p100": 1.0, "v100": 1.0}}
    pol = ftf.FinishTimeFairnessPolicyWithPerf(native=ftf_ref.TwinEngine())
    with pytest.raises(NotImplementedError):
        pol.get_allocation(*args(tp, [1, 1], {"p100": 2, "v100": 2}))


def test_zero_throughput_names_the_job():
    tp = {0: {"v100": 2.0}, 7: {"v100": 0.0}}
    pol = ftf.FinishTimeFairnessPolicy(native=ftf_ref.TwinEngine())
    with pytest.raises(ValueError, match="job 7"):
        pol.get_allocation(*args(tp, [1, 1], {"v100": 2}))


def test_nonpositive_isolated_time_names_the_job():
    """Remaining steps that grew while the job shared the cluster (a small
    isolated throughput) drive the reference's cumulative term, and with it
    E_j once the job is alone, below zero."""
    pol = ftf.FinishTimeFairnessPolicyWithPerf(native=ftf_ref.TwinEngine())
    four = {j: {"v100": 2.0} for j in range(4)}
    ones = {j: 1 for j in range(4)}
    pol.get_allocation(four, ones, {j: 1.0 for j in range(4)}, {j: 0.0 for j in range(4)},
                       {j: 100 for j in range(4)}, {"v100": 1})
    with pytest.raises(ValueError, match="job 3"):
        pol.get_allocation({3: {"v100": 2.0}}, {3: 1}, {3: 1.0}, {3: 10.0}, {3: 5000}, {"v100": 1})


@pytest.fixture(scope="module")
def sim30():
    rec = {"workers": [], "allocations": []}
    return fc.simulate_30(ftf_ref.TwinEngine(), rec), rec


def test_simulation_completes_within_capacity(sim30):
    s, rec = sim30
    assert s["policy"] == "FinishTimeFairness"
    assert s["jobs_completed"] == 30 and all(v is not None for v in s["jcts"].values())
    assert s["makespan"] > 0 and s["solves"] >= 1 and 0 < s["utilization"] <= 1.0
    assert rec["workers"] and rec["allocations"]
    for used in rec["workers"]:
        assert len(used) == len(set(used)) <= 8
    for alloc in rec["allocations"]:
        assert all(0.0 <= v <= 1.0 for v in alloc.values())


def test_simulation_is_deterministic(sim30):
    again = fc.simulate_30(ftf_ref.TwinEngine())
    first = dict(sim30[0])
    for s in (first, again):
        s.pop("solve_seconds")
    assert first == again


def test_policy_name_is_listed():
    assert sw_sim.POLICY_NAMES["finish_time_fairness"] == "FinishTimeFairness"
