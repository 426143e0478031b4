"""The FinishTimeFairness policy mirror over worker types that differ
(FinishTimeFairnessPolicyWithPerf(worker_types=True), finish_time_fairness.py)
without a GPU, over the CPU twins (tests/ftftcases.py TwinEngine)."""
import numpy as np
import pytest

import finish_time_fairness as ftf
import ftftcases as tc

TYPES = ["k80", "p100", "v100"]


def policy_args(thr, sf, steps, elapsed, W, types=TYPES, first=0):
    """The policy's arguments for jobs first, first + 1, …"""
    m = len(sf)
    ids = [first + j for j in range(m)]
    tp = {i: {t: float(thr[j, k]) for k, t in enumerate(types)} for j, i in enumerate(ids)}
    return (tp, {i: int(sf[j]) for j, i in enumerate(ids)}, {i: 1.0 for i in ids},
            {i: float(elapsed[j]) for j, i in enumerate(ids)}, {i: float(steps[j]) for j, i in enumerate(ids)},
            {t: int(W[k]) for k, t in enumerate(types)})


def _instance():
    """Seven live jobs on three types; capacity binds."""
    W, sf, thr, left, a, E = tc.dead_among_live_case()
    return W, sf, thr, np.where(left > 0.0, left, 2e4)


def test_default_still_raises_and_names_the_flag():
    W, sf, thr, left = _instance()
    eng = tc.TwinEngine()
    pol = ftf.FinishTimeFairnessPolicyWithPerf(native=eng)
    with pytest.raises(NotImplementedError, match="worker_types=True"):
        pol.get_allocation(*policy_args(thr, sf, left, np.zeros(len(sf)), W))
    assert eng.calls == [] and pol._num_steps_remaining_prev_iteration == {}


def test_identical_types_give_the_default_result():
    sf = np.array([1, 2, 4, 1, 2], dtype=np.int32)
    thr = np.repeat(np.array([3.0, 4.0, 5.0, 6.0, 7.0])[:, None], 3, axis=1)
    args = policy_args(thr, sf, np.full(5, 3e5), [0.0, 100.0, 50.0, 0.0, 10.0], [1, 1, 1])
    e0, e1 = tc.TwinEngine(), tc.TwinEngine()
    a0 = ftf.FinishTimeFairnessPolicyWithPerf(native=e0).get_allocation(*args)
    p1 = ftf.FinishTimeFairnessPolicyWithPerf(native=e1, worker_types=True)
    a1 = p1.get_allocation(*args)
    assert a0 == a1 and e0.calls == e1.calls == ["ftf_allocate"]
    # the kernel over types on the same program: the same ρ and the same job totals within 1e-6
    W = np.array([1, 1, 1], dtype=np.int32)
    E = np.array([p1._cumulative_isolated_time[j] for j in range(5)]) + 3e5 / np.array(
        [p1._isolated_throughputs_prev_iteration[j] for j in range(5)])
    x, rho, t, _, solves, _ = tc.twin_allocate(W, sf, thr, np.full(5, 3e5), [0.0, 100.0, 50.0, 0.0, 10.0], E)
    assert abs(rho - p1.last_level[0]) <= 1e-6 * rho and solves == 1
    tot = np.array([sum(a0[j].values()) for j in range(5)])
    assert np.abs(x.sum(axis=1) - tot).max() <= 1e-6


def test_several_calls_carry_the_state_in_the_reference_order():
    W, sf, thr, left = _instance()
    m = len(sf)
    eng = tc.TwinEngine()
    pol = ftf.FinishTimeFairnessPolicyWithPerf(native=eng, worker_types=True)
    cum = np.zeros(m)
    prev_left = prev_iso = None
    elapsed = np.zeros(m)
    for call in range(3):
        args = policy_args(thr, sf, left, elapsed, W)
        alloc = pol.get_allocation(*args)
        iso = ftf._isolated_throughputs(thr, (list(range(m)), TYPES), args[1], args[5])
        if prev_left is not None:
            cum += (prev_left - left) / prev_iso
        E = cum + left / iso
        x = np.array([[alloc[j][t] for t in TYPES] for j in range(m)])
        xt, rho, t, _, solves, flags = tc.twin_allocate(W, sf, thr, left, elapsed, E)
        assert pol.last_level == (rho, solves)
        assert np.array_equal(x, xt.clip(min=0.0).clip(max=1.0))
        tc.check_rows(W, sf, thr, left, elapsed, E, x, rho)
        assert pol._num_steps_remaining_prev_iteration == args[4]
        assert [pol._cumulative_isolated_time[j] for j in range(m)] == list(cum)
        # a round at the allocation, long enough for the first job to finish: a dead row from then on
        rate = (thr * x).sum(axis=1)
        dt = 1.5 * float((left[left > 0.0] / rate[left > 0.0]).min())
        prev_left, prev_iso = left, iso
        left = np.maximum(left - dt * rate, 0.0)
        elapsed = elapsed + dt
    assert eng.calls == ["ftf_allocate_types"] * 3 and (left == 0.0).any()


def test_refusals_each_followed_by_a_good_call():
    W, sf, thr, left = _instance()
    m = len(sf)
    good = policy_args(thr, sf, left, np.zeros(m), W)

    def fresh():
        return ftf.FinishTimeFairnessPolicyWithPerf(native=tc.TwinEngine(), worker_types=True)

    want = fresh().get_allocation(*good)

    def later_jobs(pol):
        """These two refusals come after the state update, as in the reference, and leave the
        refused jobs' isolated times spoilt; the same policy goes on with the jobs that come next."""
        alloc = pol.get_allocation(*policy_args(thr, sf, left, np.zeros(m), W, first=100))
        return [alloc[100 + j] for j in range(m)]

    # a live job without throughput anywhere, then only on a type without workers
    bad = thr.copy()
    bad[3, :] = 0.0
    pol = fresh()
    with pytest.raises(ValueError, match="job 3"):
        pol.get_allocation(*policy_args(bad, sf, left, np.zeros(m), W))
    assert pol.get_allocation(*good) == want
    bad[3, 1] = 2.0
    pol = fresh()
    with pytest.raises(ValueError, match="job 3"):
        pol.get_allocation(*policy_args(bad, sf, left, np.zeros(m), [W[0], 0, W[2]]))
    assert pol.get_allocation(*good) == want
    # a job with nothing left on its first call: its expected isolated time is 0
    none_left = left.copy()
    none_left[2] = 0.0
    pol = fresh()
    with pytest.raises(ValueError, match="job 2"):
        pol.get_allocation(*policy_args(thr, sf, none_left, np.zeros(m), W))
    assert later_jobs(pol) == list(want.values())
    # remaining steps that grew while the cluster did: the expected isolated time is not positive
    pol = fresh()
    pol.get_allocation(*good)
    grown = left.copy()
    grown[0] = 1e3 * left[0] + 1e9
    with pytest.raises(ValueError, match="job 0"):
        pol.get_allocation(*policy_args(thr, sf, grown, np.zeros(m), 2 * W))
    assert later_jobs(pol) == list(want.values())
    # no jobs: None, and the state of the previous call is dropped
    assert pol.get_allocation({}, {}, {}, {}, {}, {t: 1 for t in TYPES}) is None
    assert pol._num_steps_remaining_prev_iteration == {}
