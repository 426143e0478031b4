"""FinishTimeFairness over worker types that differ on the GPU
(sw_ftf_allocate_types / _batch, csrc/sw_ftf_types.hip): the kernel against the
CPU twin bit for bit — allocation and all five results — at the smallest shapes
at which each part can go wrong, and the GPU's own results against the
reference that shares no code with it.

  1 × 1, 1 × 3, 2 × 2, 5 × 3   fewer jobs than a wave, than types
  33 × 8, 40 × 16              the widest reductions and reduced system
  513 × 2, 1100 × 3            more jobs than threads: chunks of 2 and of 3, a ragged end
  zero_worker                  the compaction of the types
  dead_among_live, all_dead    rows that do not hold the level; no level at all
  box                          ρ* = ρ_box, one solve
  tight                        ρ* far above ρ_box: the start's bisection, several solves
  no_elapsed                   t* linear in ρ: two solves
  most_solves                  the fuzz instance with the most level solves
  dead_sets_level              t*(ρ_box) > 1: the centring run after the last probe
"""
import functools

import numpy as np
import pytest

import ftftcases as tc

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1), (1, 3), (2, 2), (5, 3), (33, 8), (40, 16), (513, 2), (1100, 3)]
RHO_BAR = 1e-6  # tests/test_ftf_types.py
SHARE_BAR = 1e-6


def _dead_sets_level():
    W, sf, thr, left, a, E = tc.dead_among_live_case()
    a = a.copy()
    a[2] = 3.0 * E[2]
    return W, sf, thr, left, a, E


@functools.lru_cache(maxsize=None)
def _case(name):
    """The inputs and the twin's answer, computed once and left unchanged."""
    if name == "dead_sets_level":
        inst = _dead_sets_level()
    else:
        inst = tc.NAMED[name]() if isinstance(name, str) else tc.shaped(*name)
    out = tc.twin_allocate(*inst)
    for a in inst + (out[0],):
        a.setflags(write=False)
    return inst, out


def _same(got, want):
    assert got[1:] == want[1:], (got[1:], want[1:])
    assert float(got[1]).hex() == float(want[1]).hex() and float(got[2]).hex() == float(want[2]).hex()
    assert np.array_equal(np.ascontiguousarray(got[0]).view(np.uint64), np.ascontiguousarray(want[0]).view(np.uint64))


@pytest.mark.parametrize("name", SHAPES + list(tc.NAMED) + ["dead_sets_level"], ids=str)
def test_gpu_bit_exact_vs_twin(gpu_solver, name):
    inst, want = _case(name)
    got = gpu_solver.ftf_allocate_types(*inst)
    print(f"{name}: gpu rho {got[1]!r} t {got[2]!r} steps {got[3]} solves {got[4]} flags {got[5]}; twin {want[1:]}")
    _same(got, want)
    flags = got[5]
    if name == "all_dead":
        assert flags == gpu_solver.FTFT_IDLE and got[2] == 0.0
    if name == "box":
        assert flags == gpu_solver.FTFT_BOX and got[4] == 1
    if name == "tight":
        assert flags == 0 and got[4] >= 2
    if name == "no_elapsed":
        assert flags == 0 and got[4] == 2
    if name == "most_solves":
        assert got[4] >= 4
    if name == "dead_sets_level":
        assert flags == gpu_solver.FTFT_BOX and got[1] == 3.0 and got[2] > 1.001
    if name == "zero_worker":
        assert (got[0][:, 1] == 0.0).all()
    tc.check_rows(*inst, got[0], got[1])


def test_gpu_batch_equals_single_calls_and_twin(gpu_solver):
    import sw_native as sn

    names = [(5, 3), (513, 3), None, (1, 3), "zero_worker", "all_dead", "dead_among_live", "tight", "no_elapsed",
             "dead_sets_level", (33, 3)]
    insts = []
    for nm in names:
        if nm is None:
            insts.append((np.array([2, 0, 1], dtype=np.int32), np.zeros(0, dtype=np.int32), np.zeros((0, 3)),
                          np.zeros(0), np.zeros(0), np.zeros(0)))
        else:
            insts.append(_case(nm)[0])
    out = gpu_solver.ftf_allocate_types_batch(insts)
    assert len(out) == len(insts)
    for nm, inst, got in zip(names, insts, out):
        if nm is None:
            assert got[0].shape == (0, 3) and got[1:] == (0.0, 0.0, 0, 0, 0)
            continue
        _same(got, gpu_solver.ftf_allocate_types(*inst))
        _same(got, _case(nm)[1])
    good = np.cumsum([0] + [len(i[1]) for i in insts])
    for bad in (good + 1, np.r_[good[:2], good[1] - 1, good[3:]]):
        with pytest.raises(sn.NativeError) as e:
            gpu_solver.ftf_allocate_types_batch(insts, offsets=bad)
        assert e.value.code == sn.SW_ERR_INVALID
    assert gpu_solver.ftf_allocate_types_batch([]) == []


def test_gpu_within_the_bars_of_the_reference(gpu_solver):
    """The GPU's own shares and ρ against the independent reference: 10 tiny
    instances of the centre fuzz, five of each family."""
    cases = tc.centre_fuzz()
    picked = list(range(10))  # alternating families: five of each
    assert [cases[i][0] for i in picked].count("narrow") == 5
    worst = gap = 0.0
    for i in picked:
        inst, (xr, rho_ref, box) = cases[i][1], tc.centre_ref(i)
        x, rho, t, _, solves, flags = gpu_solver.ftf_allocate_types(*inst)
        tc.check_rows(*inst, x, rho)
        gap = max(gap, abs(rho - rho_ref) / rho_ref)
        worst = max(worst, float(np.abs(x - xr).max()))
    print(f"gpu centre: worst rho gap {gap:.3e}, worst max|x - x_ref| = {worst:.3e}")
    assert len(picked) == 10 and gap <= RHO_BAR and worst <= SHARE_BAR


def test_gpu_rejects_bad_input_and_goes_on(gpu_solver):
    import sw_native as sn

    ok = dict(W=np.array([4, 2], dtype=np.int32), sf=np.array([1, 1], dtype=np.int32), thr=np.ones((2, 2)),
              steps=np.array([1e5, 2e5]), a=np.array([10.0, 0.0]), E=np.array([2e5, 3e5]))

    def refused(match=None, **kw):
        v = dict(ok, **kw)
        with pytest.raises(sn.NativeError, match=match) as e:
            gpu_solver.ftf_allocate_types(v["W"], v["sf"], v["thr"], v["steps"], v["a"], v["E"])
        assert e.value.code == sn.SW_ERR_INVALID
        x, rho, t, _, solves, flags = gpu_solver.ftf_allocate_types(*ok.values())  # and a good call after it
        assert solves >= 1 and rho > 0.0

    refused(sf=[1, 0], match="job 1")
    refused(sf=[256, 1], match="job 0")
    refused(W=[4, -1])
    refused(thr=np.array([[1.0, np.nan], [1.0, 1.0]]), match="job 0")
    refused(thr=np.array([[1.0, -1.0], [1.0, 1.0]]))
    refused(thr=np.array([[1.0, np.inf], [1.0, 1.0]]))
    refused(steps=[1e5, -1.0], match="job 1")
    refused(steps=[1e5, np.inf])
    refused(a=[-1.0, 0.0], match="job 0")
    refused(a=[0.0, np.nan], match="job 1")
    refused(E=[0.0, 1e5], match="job 0")
    refused(E=[1e5, np.inf], match="job 1")
    refused(E=[1e5, -3.0])
    refused(thr=np.array([[0.0, 0.0], [1.0, 1.0]]), match="job 0")  # a live job without throughput
    refused(W=[4, 0], thr=np.array([[0.0, 2.0], [1.0, 1.0]]), match="job 0")  # … on a type with workers
    refused(thr=np.array([[1e-3, 1e-4], [1.0, 1.0]]), steps=[1.1e12, 1e5], match="job 0")  # best full time above 1e15
    refused(a=[1e308, 0.0], E=[1e-300, 1e5], match="job 0")  # ρ_box not finite
    # a dead job may have no throughput
    x, rho, t, _, solves, flags = gpu_solver.ftf_allocate_types(ok["W"], ok["sf"], np.array([[0.0, 0.0], [1.0, 1.0]]),
                                                                [0.0, 1e5], ok["a"], ok["E"])
    assert (x[0] >= 0.0).all() and solves >= 1
    got = gpu_solver.ftf_allocate_types([4, 2], [], np.zeros((0, 2)), [], [], [])
    assert got[0].shape == (0, 2) and got[1:] == (0.0, 0.0, 0, 0, 0)
    with pytest.raises(sn.NativeError) as e:
        gpu_solver.ftf_allocate_types(np.full(17, 8), [1, 1], np.ones((2, 17)), [1e5, 1e5], [0.0, 0.0], [1e5, 1e5])
    assert e.value.code == sn.SW_ERR_INVALID
    n = tc.const("max_jobs") + 1
    assert n == 16385
    with pytest.raises(sn.NativeError) as e:
        gpu_solver.ftf_allocate_types([4], np.ones(n, dtype=np.int32), np.ones((n, 1)), np.full(n, 1e5), np.zeros(n),
                                      np.full(n, 1e5))
    assert e.value.code == sn.SW_ERR_INVALID
    inst, want = _case((5, 3))
    _same(gpu_solver.ftf_allocate_types(*inst), want)


def test_gpu_policy_mirror_equals_the_twin_backed_one(gpu_solver):
    import finish_time_fairness as ftf
    from test_ftf_types_policy import _instance, policy_args

    W, sf, thr, left = _instance()
    pg = ftf.FinishTimeFairnessPolicyWithPerf(native=gpu_solver, worker_types=True)
    pt = ftf.FinishTimeFairnessPolicyWithPerf(native=tc.TwinEngine(), worker_types=True)
    elapsed = np.zeros(len(sf))
    for _ in range(2):
        args = policy_args(thr, sf, left, elapsed, W)
        ag, at = pg.get_allocation(*args), pt.get_allocation(*args)
        assert ag == at and pg.last_level == pt.last_level
        left, elapsed = left * 0.7, elapsed + 500.0
