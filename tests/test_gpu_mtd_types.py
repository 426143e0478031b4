"""MinTotalDuration over worker types that differ on the GPU
(sw_mtd_allocate_types / _batch, csrc/sw_mtd_types.hip): the kernel against the
CPU twin bit for bit — allocation and all four results — at the smallest shapes
at which each part can go wrong, and the GPU's own results against the
reference that shares no code with it.

  1 × 1, 1 × 3, 2 × 2, 5 × 3   fewer jobs than a wave, than types
  33 × 8, 40 × 16              the widest reductions and reduced system
  513 × 2, 1100 × 3            more jobs than threads: chunks of 2 and of 3, a ragged end
  zero_worker                  the compaction of the types
  dead_among_live, all_dead    rows that do not hold the level; no level at all
  thin                         phase 2 skipped
  short, long                  1/t* < 100 and 1/t* > 1e6 (the decade rounds)
"""
import functools

import numpy as np
import pytest

import mtd_types_ref as ref
import mtdtcases as tc

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1), (1, 3), (2, 2), (5, 3), (33, 8), (40, 16), (513, 2), (1100, 3)]


@functools.lru_cache(maxsize=None)
def _case(name):
    """The inputs and the twin's answer, computed once and left unchanged."""
    inst = tc.NAMED[name]() if isinstance(name, str) else tc.shaped(*name)
    out = tc.twin_allocate(*inst)
    for a in inst + (out[0],):
        a.setflags(write=False)
    return inst, out


def _same(got, want):
    assert got[1:] == want[1:], (got[1:], want[1:])
    assert float(got[1]).hex() == float(want[1]).hex() and float(got[2]).hex() == float(want[2]).hex()
    assert np.array_equal(np.ascontiguousarray(got[0]).view(np.uint64), np.ascontiguousarray(want[0]).view(np.uint64))


@pytest.mark.parametrize("name", SHAPES + list(tc.NAMED), ids=str)
def test_gpu_bit_exact_vs_twin(gpu_solver, name):
    inst, want = _case(name)
    got = gpu_solver.mtd_allocate_types(*inst)
    print(f"{name}: gpu T {got[1]!r} t* {got[2]!r} steps {got[3]} flags {got[4]}; twin {want[1:]}")
    _same(got, want)
    flags = got[4]
    if isinstance(name, tuple) or name in ("zero_worker", "dead_among_live"):
        assert flags == 0 and got[2] > 0.0
    if name == "all_dead":
        assert flags == gpu_solver.MTDT_IDLE and got[2] == 0.0
    if name == "thin":
        assert flags == gpu_solver.MTDT_THIN and got[1] == tc.FIRST_PROBE
    if name == "short":
        assert 1.0 / got[2] < 100.0 and got[1] < 105.0
    if name == "long":
        assert 1.0 / got[2] > 1e6 and got[1] > 1e6
    if name == "zero_worker":
        assert (got[0][:, 1] == 0.0).all()
    tc.check_rows(*inst, got[0], got[1])


def test_gpu_batch_equals_single_calls_and_twin(gpu_solver):
    import sw_native as sn

    def three(name):  # the named cases as 3-type instances where they are not
        inst, want = _case(name)
        return inst, want

    names = [(5, 3), (513, 3), None, (1, 3), "zero_worker", "all_dead", "dead_among_live", "long", (33, 3)]
    insts = []
    for nm in names:
        if nm is None:
            insts.append((np.array([2, 0, 1], dtype=np.int32), np.zeros(0, dtype=np.int32), np.zeros((0, 3)),
                          np.zeros(0)))
        else:
            insts.append(three(nm)[0])
    out = gpu_solver.mtd_allocate_types_batch(insts)
    assert len(out) == len(insts)
    for nm, inst, got in zip(names, insts, out):
        if nm is None:
            assert got[0].shape == (0, 3) and got[1:] == (0.0, 0.0, 0, 0)
            continue
        _same(got, gpu_solver.mtd_allocate_types(*inst))
        _same(got, _case(nm)[1])
    good = np.cumsum([0] + [len(i[1]) for i in insts])
    for bad in (good + 1, np.r_[good[:2], good[1] - 1, good[3:]]):
        with pytest.raises(sn.NativeError) as e:
            gpu_solver.mtd_allocate_types_batch(insts, offsets=bad)
        assert e.value.code == sn.SW_ERR_INVALID
    assert gpu_solver.mtd_allocate_types_batch([]) == []


def test_gpu_within_1e_6_of_the_reference(gpu_solver):
    """The GPU's own shares and T against the independent reference: 10 tiny
    instances of the centre fuzz, five of each family."""
    cases = tc.centre_fuzz()
    picked = [c for c in cases if c[0] == "narrow"][:5] + [c for c in cases if c[0] == "wide"][:5]
    worst = 0.0
    for fam, inst, (xr, T_ref, t_ref, margin, near) in picked:
        assert near >= 1e-5 and margin >= 1e-3
        x, T, t, _, flags = gpu_solver.mtd_allocate_types(*inst)
        assert T == T_ref
        assert abs(t - t_ref) <= 1e-5 * t_ref
        worst = max(worst, float(np.abs(x - xr).max()))
    print(f"gpu centre: worst max|x - x_ref| = {worst:.3e}")
    assert len(picked) == 10 and worst <= 1e-6


def test_gpu_rejects_bad_input_and_goes_on(gpu_solver):
    import sw_native as sn

    ok = (np.array([4, 2], dtype=np.int32), np.array([1, 1], dtype=np.int32), np.ones((2, 2)), np.array([1e5, 2e5]))

    def refused(W=ok[0], sf=ok[1], thr=ok[2], steps=ok[3]):
        with pytest.raises(sn.NativeError) as e:
            gpu_solver.mtd_allocate_types(W, sf, thr, steps)
        assert e.value.code == sn.SW_ERR_INVALID

    refused(sf=[1, 0])
    refused(sf=[1, 256])
    refused(W=[4, -1])
    refused(thr=np.array([[1.0, np.nan], [1.0, 1.0]]))
    refused(thr=np.array([[1.0, -1.0], [1.0, 1.0]]))
    refused(thr=np.array([[1.0, np.inf], [1.0, 1.0]]))
    refused(steps=[1e5, -1.0])
    refused(steps=[1e5, np.inf])
    refused(thr=np.array([[0.0, 0.0], [1.0, 1.0]]))  # a live job without throughput
    refused(W=[4, 0], thr=np.array([[0.0, 2.0], [1.0, 1.0]]))  # … on a type with workers
    refused(thr=np.array([[1e-3, 1e-4], [1.0, 1.0]]), steps=[1.1e12, 1e5])  # best full time above 1e15
    # a dead job may have no throughput
    x, T, t, _, flags = gpu_solver.mtd_allocate_types(ok[0], ok[1], np.array([[0.0, 0.0], [1.0, 1.0]]), [0.0, 1e5])
    assert (x[0] >= 0.0).all() and flags == 0
    x, T, t, its, flags = gpu_solver.mtd_allocate_types([4, 2], [], np.zeros((0, 2)), [])
    assert x.shape == (0, 2) and (T, t, its, flags) == (0.0, 0.0, 0, 0)
    with pytest.raises(sn.NativeError) as e:
        gpu_solver.mtd_allocate_types(np.full(17, 8), [1, 1], np.ones((2, 17)), [1e5, 1e5])
    assert e.value.code == sn.SW_ERR_INVALID
    n = tc.const("max_jobs") + 1
    assert n == 16385
    with pytest.raises(sn.NativeError) as e:
        gpu_solver.mtd_allocate_types([4], np.ones(n, dtype=np.int32), np.ones((n, 1)), np.full(n, 1e5))
    assert e.value.code == sn.SW_ERR_INVALID
    inst, want = _case((5, 3))
    _same(gpu_solver.mtd_allocate_types(*inst), want)


def test_gpu_policy_mirror_equals_the_twin_backed_one(gpu_solver):
    import min_total_duration as mtd
    from test_mtd_types import _policy_args

    W, sf, thr, steps = tc.dead_among_live_case()
    args = _policy_args(thr, sf, steps, W, ["k80", "p100", "v100"])
    pg = mtd.MinTotalDurationPolicyWithPerf(native=gpu_solver, worker_types=True)
    pt = mtd.MinTotalDurationPolicyWithPerf(native=tc.TwinEngine(), worker_types=True)
    assert pg.get_allocation(*args) == pt.get_allocation(*args)
    assert pg.last_level == pt.last_level
