"""The AlloX policy mirror (allox.py) and the simulator's allox policy,
without a GPU: a recording fake engine and the CPU twin of the kernel are
injected as the engine (tests/test_gpu_allox.py repeats the sequence and the
simulation on the HIP engine and compares exactly)."""
import json
import os

import numpy as np
import pytest

import allox
import allox_ref
import alloxcases as ac
import sw_sim

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "sim30_allox.json")


class FakeEngine:
    """Records its arguments and deals the jobs round-robin: job i on worker
    i mod n at position i // n + 1 (a valid structure, not an optimum)."""

    def __init__(self):
        self.calls = []

    def allox_assign(self, free_workers, proc_time, delay):
        m, n = len(delay), int(np.sum(free_workers))
        jw = np.array([i % n for i in range(m)], dtype=np.int32)
        jp = np.array([i // n + 1 for i in range(m)], dtype=np.int32)
        wf = np.full(n, -1, dtype=np.int32)
        for i in range(m):
            wf[jw[i]] = i  # the last job dealt to a worker has its highest position
        r = (jw, jp, wf, 0.0)
        self.calls.append((np.array(free_workers), np.array(proc_time), np.array(delay), r))
        return r


def check_allocation(a, spec):
    """At most cluster_spec[type] ones per type, and every job sums to 0 or 1."""
    for t, workers in spec.items():
        assert sum(1 for r in a.values() if r[t] == 1.0) <= workers
    for r in a.values():
        assert all(v in (0.0, 1.0) for v in r.values()) and sum(r.values()) in (0.0, 1.0)


@pytest.mark.parametrize("engine_cls", [FakeEngine, allox_ref.TwinEngine])
def test_three_calls_restated_element_by_element(engine_cls):
    """allox.py:27-139 over three calls: a job finishes and one arrives between
    them; a job that holds a worker keeps its row, takes one worker off its
    type and never reaches the engine."""
    eng = engine_cls()
    calls, out, pol = ac.policy_sequence(eng)
    assert len(eng.calls) == 3
    prev = {}
    seen_holder = False
    for c, got, (rfree, rp, rd, (_, _, wfirst, _)) in zip(calls, out, eng.calls):
        holding = [j for j in c["tp"] if j in prev and sum(prev[j][t] for t in ac.TYPES) == 1.0]
        waiting = [j for j in c["tp"] if j not in holding]
        free = [c["spec"][t] - sum(1 for j in holding if prev[j][t] == 1.0) for t in ac.TYPES]
        waiting.sort(key=lambda j: -c["tss"][j])  # stable
        waiting = waiting[:max(int(1.0 * len(waiting)), sum(free))]
        assert list(rfree) == free
        assert rd.tolist() == [c["tss"][j] for j in waiting]
        assert rp.tolist() == [[c["steps"][j] / c["tp"][j][t] for t in ac.TYPES] for j in waiting]
        want = {j: dict(prev[j]) if j in prev else {t: 0.0 for t in c["spec"]} for j in sorted(c["tp"])}
        type_of = [t for t, f in zip(ac.TYPES, free) for _ in range(f)]
        assert len(wfirst) == len(type_of)
        for w, i in enumerate(wfirst):
            if i >= 0:
                want[waiting[i]][type_of[w]] = 1.0
        assert got == want and list(got) == sorted(c["tp"])
        for j in holding:  # the row is kept and the job is not in the engine's instance
            assert got[j] == prev[j] and j not in waiting
            seen_holder = True
        check_allocation(got, c["spec"])
        prev = got
    assert seen_holder
    assert pol._prev_allocation == out[-1]
    # first call: four new jobs, three free workers (k80: 1, v100: 2), oldest first
    assert list(eng.calls[0][0]) == [1, 2] and eng.calls[0][2].tolist() == [120.0, 60.0, 60.0, 20.0]
    # later calls: two holders stay, so one worker is free and two jobs wait
    assert [int(c[0].sum()) for c in eng.calls] == [3, 1, 1]
    assert [len(c[2]) for c in eng.calls] == [4, 2, 2]


def test_first_call_on_the_twin_by_hand():
    """Call 1 of the sequence: p = steps / throughput on (k80, v100) is job 0
    (2000, 500), job 2 (500, 428.6), job 1 (9000, 1000), job 3 (14000, 1166.7).
    Job 2 takes the k80 (500) and the other three share the two v100s with
    the shortest, job 0, at position 2: cost 500 + 2·500 + 1000 + 1166.7 plus
    the delays.  Job 0 runs first on its v100; whether job 1 or job 3 queues
    behind it costs the same, so which of them gets the other v100 is the tie
    rule's choice, not the optimum's."""
    eng = allox_ref.TwinEngine()
    _, out, pol = ac.policy_sequence(eng)
    assert out[0][0] == {"k80": 0.0, "v100": 1.0} and out[0][2] == {"k80": 1.0, "v100": 0.0}
    assert sorted([out[0][1]["v100"], out[0][3]["v100"]]) == [0.0, 1.0]
    assert out[0][1]["k80"] == out[0][3]["k80"] == 0.0
    assert abs(eng.calls[0][3][3] - (500 + 2 * 500 + 1000 + 7000 / 6.0 + 260.0)) < 1e-9


def args(tp, tss, steps, sf=None):
    ids = list(tp)
    return ({j: {"v100": tp[j]} for j in ids}, {j: 1 for j in ids} if sf is None else sf,
            dict(zip(ids, tss)), dict(zip(ids, steps)))


def test_alpha_cut_uses_max_of_int_alpha_m_and_n():
    eng = FakeEngine()
    pol = allox.AlloXPolicy(alpha=0.5, native=eng)
    tp = {j: 1.0 for j in range(7)}
    a = pol.get_allocation(*args(tp, [70, 60, 50, 40, 30, 20, 10], [100] * 7), {"v100": 2})
    assert len(eng.calls[0][2]) == 3 == max(int(0.5 * 7), 2)  # the three oldest jobs
    assert eng.calls[0][2].tolist() == [70.0, 60.0, 50.0]
    check_allocation(a, {"v100": 2})
    eng2 = FakeEngine()
    pol2 = allox.AlloXPolicy(alpha=0.1, native=eng2)
    pol2.get_allocation(*args(tp, [70, 60, 50, 40, 30, 20, 10], [100] * 7), {"v100": 4})
    assert len(eng2.calls[0][2]) == 4  # n = 4 > int(0.1·7) = 0


def test_sort_is_stable_over_the_iteration_order():
    eng = FakeEngine()
    pol = allox.AlloXPolicy(native=eng)
    tp = {5: 1.0, 2: 2.0, 9: 4.0, 1: 8.0}  # iteration order 5, 2, 9, 1
    pol.get_allocation(*args(tp, [10.0, 30.0, 10.0, 30.0], [80, 80, 80, 80]), {"v100": 1})
    # equal start times keep the iteration order: (2, 1) then (5, 9)
    assert eng.calls[0][1].reshape(-1).tolist() == [40.0, 10.0, 80.0, 20.0]


def test_zero_throughput_becomes_1e_minus_10():
    eng = FakeEngine()
    pol = allox.AlloXPolicy(native=eng)
    pol.get_allocation(*args({0: 0.0, 1: 2.0}, [5.0, 4.0], [3, 8]), {"v100": 1})
    assert eng.calls[0][1].reshape(-1).tolist() == [3 / 1e-10, 4.0]


def test_scale_factor_other_than_one_asserts_and_empty_input_is_none():
    eng = FakeEngine()
    pol = allox.AlloXPolicy(native=eng)
    with pytest.raises(AssertionError):
        pol.get_allocation(*args({0: 1.0, 1: 2.0}, [5.0, 4.0], [3, 8], sf={0: 1, 1: 2}), {"v100": 1})
    assert pol.get_allocation({}, {}, {}, {}, {"v100": 4}) is None
    assert eng.calls == [] and pol._prev_allocation == {}


def test_no_free_workers_copies_the_previous_rows():
    eng = FakeEngine()
    pol = allox.AlloXPolicy(native=eng)
    first = pol.get_allocation(*args({0: 1.0, 1: 2.0}, [5.0, 4.0], [30, 80]), {"v100": 2})
    assert first == {0: {"v100": 1.0}, 1: {"v100": 1.0}} and len(eng.calls) == 1
    # both hold a worker; job 2 arrives and finds none free: nothing is launched
    second = pol.get_allocation(*args({0: 1.0, 1: 2.0, 2: 9.0}, [125.0, 124.0, 1.0], [20, 70, 50]), {"v100": 2})
    assert second == {0: {"v100": 1.0}, 1: {"v100": 1.0}, 2: {"v100": 0.0}} and len(eng.calls) == 1
    # job 0 finishes: its worker goes to job 2
    third = pol.get_allocation(*args({1: 2.0, 2: 9.0}, [244.0, 121.0], [60, 50]), {"v100": 2})
    assert third == {1: {"v100": 1.0}, 2: {"v100": 1.0}} and len(eng.calls) == 2
    assert list(eng.calls[1][0]) == [1] and eng.calls[1][2].tolist() == [121.0]


def test_bad_times_raise_naming_the_job_before_any_launch():
    eng = FakeEngine()
    pol = allox.AlloXPolicy(native=eng)
    for tss, steps in (([5.0, -1.0], [3, 8]), ([5.0, float("nan")], [3, 8]), ([5.0, 4.0], [3, -8]),
                       ([5.0, 4.0], [3, float("inf")])):
        with pytest.raises(ValueError, match="job 7"):
            pol.get_allocation(*args({0: 1.0, 7: 2.0}, tss, steps), {"v100": 1})
    assert eng.calls == [] and pol._prev_allocation == {}


def test_names_are_the_references():
    pol = allox.AlloXPolicy(native=FakeEngine())
    assert pol.name == pol._name == "AlloX_Perf" and pol._alpha == 1.0
    assert sw_sim.POLICY_NAMES["allox"] == "AlloX_Perf"
    assert sw_sim.Simulator("allox", {}, {}).policy_name == "AlloX_Perf"
    sim = sw_sim.Simulator("allox_alpha=0.25", {}, {})
    assert sim.policy_name == "AlloX_Perf" and sim._allox_alpha == 0.25
    with pytest.raises(ValueError):
        sw_sim.Simulator("allox_packing", {}, {})
    with pytest.raises(ValueError):
        sw_sim.Simulator("fifo", {}, {})


# ---- the simulator ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def sim30():
    rec = {"workers": [], "allocations": []}
    return ac.simulate_30(allox_ref.TwinEngine(), rec), rec


def test_simulation_completes_and_uses_no_worker_twice(sim30):
    """All 30 jobs leave the simulator.  Job 29 leaves by the reference's
    failed-attempt rule (scheduler.py:49, :627-705: jct None) after a
    batch-size rescale puts its steps run above its total — MaxMinFairness and
    FinishTimeFairness on the same 30 jobs retire it the same way; the other
    29 finish."""
    s, rec = sim30
    assert s["policy"] == "AlloX_Perf"
    assert s["jobs_completed"] == 30 and len(s["jcts"]) == 30
    assert [j for j, v in s["jcts"].items() if v is None] == ["29"]
    assert s["makespan"] > 0 and s["solves"] >= 1 and 0 < s["utilization"] <= 1.0
    assert rec["workers"] and rec["allocations"]
    for used in rec["workers"]:
        assert len(used) == len(set(used)) <= 8
    for alloc in rec["allocations"]:
        assert all(v in (0.0, 1.0) for v in alloc.values()) and sum(alloc.values()) <= 8


def test_simulation_is_deterministic_and_matches_the_record(sim30):
    """tests/golden/sim30_allox.json: the summary of the 30-job, 8-GPU
    simulation on the twin engine, recorded from this build's twin."""
    again = ac.simulate_30(allox_ref.TwinEngine())
    first = dict(sim30[0])
    for s in (first, again):
        s.pop("solve_seconds")
    assert first == again
    assert json.loads(json.dumps(first)) == json.load(open(GOLDEN))


def test_alpha_policy_name_runs_in_the_simulator():
    s = ac.simulate_30(allox_ref.TwinEngine(), policy="allox_alpha=0.5")
    assert s["policy"] == "AlloX_Perf" and s["jobs_completed"] == 30


def test_multi_gpu_job_raises_the_references_assertion():
    """allox.py:35-36: the unfiltered trace prefix holds jobs of scale factor 2."""
    import wfcases as wc

    with pytest.raises(AssertionError):
        wc.simulate_30("allox", allox_allocator=allox_ref.TwinEngine())


def test_existing_policies_are_unchanged_and_never_call_the_new_engine():
    """The five baselines on their own 30-job prefix against their recorded
    summaries: sim30_gavel_policies.json, sim30_min_total_duration.json and
    sim30_max_sum_throughput.json as committed, and sim30_water_filling.json,
    recorded with the simulator of the commit before AlloX was added (it had
    no record).  None touches the AlloX engine."""
    import ftf_ref
    import mmf_ref
    import mst_ref
    import mtd_ref
    import wf_ref
    import wfcases as wc

    class Untouched:
        def allox_assign(self, *_):
            raise AssertionError("the AlloX engine was called")

    gold = lambda name: json.load(open(os.path.join(HERE, "golden", name)))
    runs = {
        "max_min_fairness": dict(mmf_allocator=mmf_ref.twin_allocator),
        "finish_time_fairness": dict(ftf_allocator=ftf_ref.TwinEngine()),
        "max_min_fairness_water_filling": dict(wf_allocator=wf_ref.twin_allocator),
        "min_total_duration": dict(mtd_allocator=mtd_ref.TwinEngine()),
        "max_sum_throughput_perf": dict(mst_allocator=mst_ref.TwinEngine()),
    }
    got = {}
    for policy, engines in runs.items():
        s = wc.simulate_30(policy, allox_allocator=Untouched(), **engines)
        s.pop("solve_seconds")
        got[policy] = json.loads(json.dumps(s))
    gavel = gold("sim30_gavel_policies.json")
    assert got["max_min_fairness"] == gavel["max_min_fairness"]
    assert got["finish_time_fairness"] == gavel["finish_time_fairness"]
    assert got["max_min_fairness_water_filling"] == gold("sim30_water_filling.json")
    assert got["min_total_duration"] == gold("sim30_min_total_duration.json")
    assert got["max_sum_throughput_perf"] == gold("sim30_max_sum_throughput.json")
