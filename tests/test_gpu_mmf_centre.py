"""The centred MaxMinFairness allocation over worker types on the GPU
(sw_mmf_allocate_types_centred / _batch, csrc/sw_mmf_ipm.hip): the kernel
against the CPU twin bit for bit — allocation, level and Newton steps — at the
smallest shapes at which each part can go wrong, and the GPU's own results
against the references that share no code with it.

  1 × 1, 1 × 3, 2 × 2, 5 × 3   fewer jobs than a wave, than types
  33 × 8, 40 × 16              rows of 12 and of 20 sums; the widest reduced system
  513 × 2, 1100 × 3            more jobs than threads: chunks of 2 and of 3, a ragged end
  a type without workers       the compaction of the types
  level zero                   no t column, jobs without a value row
"""
import functools

import numpy as np
import pytest

import mmf_ref
import mmfccases as mc
from test_mmf_types import _policy_inputs

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1), (1, 3), (2, 2), (5, 3), (33, 8), (40, 16), (513, 2), (1100, 3)]


@functools.lru_cache(maxsize=None)
def _case(name):
    """The inputs and the twin's answer, computed once and left unchanged."""
    W, sf, c = (mc.zero_worker_case() if name == "zero_worker" else mc.level_zero_case() if name == "level_zero"
                else mc.shaped(*name))
    x, t, its = mc.twin_allocate(W, sf, c)
    for a in (W, sf, c, x):
        a.setflags(write=False)
    return W, sf, c, x, t, its


def _same(got, want):
    xg, tg, ig = got
    xt, tt, it = want
    assert ig == it, (ig, it)
    assert float(tg).hex() == float(tt).hex()
    assert np.array_equal(np.ascontiguousarray(xg).view(np.uint64), np.ascontiguousarray(xt).view(np.uint64))


@pytest.mark.parametrize("name", SHAPES + ["zero_worker", "level_zero"], ids=str)
def test_gpu_centred_bit_exact_vs_twin(gpu_solver, name):
    W, sf, c, xt, tt, it = _case(name)
    got = gpu_solver.mmf_allocate_types_centred(W, sf, c)
    print(f"{name}: steps gpu {got[2]} twin {it}, t gpu {got[1]!r} twin {tt!r}")
    _same(got, (xt, tt, it))
    if isinstance(name, tuple):
        assert got[1] > 0.0  # the path with t: none of these is a level-zero instance
    if name == "level_zero":
        assert got[1] == 0.0
    if name in ("zero_worker", "level_zero"):
        assert (got[0][:, 1] == 0.0).all()


def test_gpu_centred_batch_equals_single_calls_and_twin(gpu_solver):
    import sw_native as sn

    names = [(5, 3), (513, 3), None, (1, 3), "zero_worker", (33, 3)]
    insts = []
    for nm in names:
        if nm is None:
            insts.append((np.array([2, 0, 1], dtype=np.int32), np.zeros(0, dtype=np.int32), np.zeros((0, 3))))
        else:
            insts.append(_case(nm)[:3])
    out = gpu_solver.mmf_allocate_types_centred_batch(insts)
    assert len(out) == len(insts)
    for nm, inst, got in zip(names, insts, out):
        if nm is None:
            assert got[0].shape == (0, 3) and got[1] == 0.0 and got[2] == 0
            continue
        _same(got, gpu_solver.mmf_allocate_types_centred(*inst))
        _same(got, _case(nm)[3:])
    # malformed offsets are refused
    good = np.cumsum([0] + [len(i[1]) for i in insts])
    for bad in (good + 1, np.r_[good[:2], good[1] - 1, good[3:]]):
        with pytest.raises(sn.NativeError) as e:
            gpu_solver.mmf_allocate_types_centred_batch(insts, offsets=bad)
        assert e.value.code == sn.SW_ERR_INVALID
    assert gpu_solver.mmf_allocate_types_centred_batch([]) == []


def test_gpu_centre_within_1e_6_of_the_reference(gpu_solver):
    """The GPU's own shares against the independent centre: 10 tiny instances
    (the first of each family first, so that all three are in)."""
    cases = mc.centre_fuzz()
    picked = [next(c for c in cases if c[0] == f) for f in mc.FAMILIES]
    picked += [c for c in cases if all(c is not p for p in picked)][:10 - len(picked)]
    worst = 0.0
    for fam, W, sf, c, xr, tr in picked:
        x, t, _ = gpu_solver.mmf_allocate_types_centred(W, sf, c)
        worst = max(worst, float(np.abs(x - xr).max()))
        assert abs(t - tr) <= 1e-6 * max(1.0, tr)
    print(f"gpu centre: worst max|x - x_ref| = {worst:.3e}")
    assert len(picked) == 10 and worst <= 1e-6


def test_gpu_one_type_within_1e_6_of_the_closed_form(gpu_solver):
    for G, sf, c, x1, t1, _ in mc.one_type_fuzz()[:5]:
        x, t, _ = gpu_solver.mmf_allocate_types_centred([G], sf, c[:, None])
        assert np.abs(x[:, 0] - x1).max() <= 1e-6
        assert abs(t - t1) <= 1e-6 * t1


def test_gpu_centred_rejects_bad_input(gpu_solver):
    import sw_native as sn

    with pytest.raises(sn.NativeError):
        gpu_solver.mmf_allocate_types_centred([4, 2], [1, 0], np.ones((2, 2)))
    with pytest.raises(sn.NativeError):
        gpu_solver.mmf_allocate_types_centred([4, -1], [1, 1], np.ones((2, 2)))
    with pytest.raises(sn.NativeError):
        gpu_solver.mmf_allocate_types_centred([4, 2], [1, 1], np.array([[1.0, np.nan], [1.0, 1.0]]))
    with pytest.raises(sn.NativeError):
        gpu_solver.mmf_allocate_types_centred([4, 2], [1, 1], np.array([[1.0, -1.0], [1.0, 1.0]]))
    x, t, its = gpu_solver.mmf_allocate_types_centred([4, 2], [], np.zeros((0, 2)))
    assert x.shape == (0, 2) and t == 0.0 and its == 0
    # above the limits: too many types, too many jobs; the handle still works afterwards
    with pytest.raises(sn.NativeError) as e:
        gpu_solver.mmf_allocate_types_centred(np.full(17, 8), [1, 1], np.ones((2, 17)))
    assert e.value.code == sn.SW_ERR_INVALID
    n = mc.max_jobs() + 1
    assert n == 16385
    with pytest.raises(sn.NativeError) as e:
        gpu_solver.mmf_allocate_types_centred([4], np.ones(n, dtype=np.int32), np.ones((n, 1)))
    assert e.value.code == sn.SW_ERR_INVALID
    W, sf, c, xt, tt, it = _case((5, 3))
    _same(gpu_solver.mmf_allocate_types_centred(W, sf, c), (xt, tt, it))


def test_gpu_policy_mirror_centred(gpu_solver):
    import warnings

    import max_min_fairness as mmfp

    types = ["k80", "p100", "v100"]
    thr, sf, pw, spec = _policy_inputs(4, types)
    pol = mmfp.MaxMinFairnessPolicyWithPerf(native=gpu_solver, centred=True)
    with warnings.catch_warnings():
        warnings.simplefilter("error", mmfp.SimplexVertexWarning)
        alloc = pol.get_allocation(thr, sf, pw, spec)
    coef, sfa, (job_ids, wts), W = pol.coefficients(thr, sf, pw, spec)
    x = np.array([[alloc[j][w] for w in wts] for j in job_ids])
    assert ((x >= 0.0) & (x <= 1.0)).all()
    t_lp, _ = mmf_ref.lp_level_types(W, sfa, coef)
    assert (coef * x).sum(axis=1).min() == pytest.approx(t_lp, rel=1e-6)
    xt, _, _ = mc.twin_allocate(W, sfa, coef)
    assert np.array_equal(x, xt.clip(min=0.0).clip(max=1.0))
