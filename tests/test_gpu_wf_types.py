"""Water-filling MaxMinFairness over worker types that differ on the GPU
(sw_wf_allocate_types / _batch, csrc/sw_wf_types.hip): the kernel against the
CPU twin bit for bit — allocation, levels and all four results — at the
smallest shapes at which each part can go wrong, and the GPU's own results
against the reference that shares no code with it.

  1 × 1, 1 × 3, 2 × 2, 5 × 3   fewer jobs than a wave, than types
  33 × 8, 40 × 16              the widest reductions and reduced system
  513 × 2, 1100 × 3            more jobs than threads: chunks of 2 and of 3, a ragged end
                               (jobs in a few classes of identical rows, so a few stages)
  zero_worker                  the compaction of the types
  one_stage                    capacity fills at the first level: no repeat
  all_capped                   every job ends at its time row, a stage per job
  many_stages                  the fuzz instance with the most stages
  last_job_alone               a final stage with one unfrozen row among m − 1 β-rows
"""
import functools

import numpy as np
import pytest

import wftcases as tc

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1), (1, 3), (2, 2), (5, 3), (33, 8), (40, 16), (513, 2), (1100, 3)]
LEVEL_BAR = 1e-6  # tests/test_wf_types.py
SHARE_BAR = 1e-6


@functools.lru_cache(maxsize=None)
def _case(name):
    """The inputs and the twin's answer, computed once and left unchanged."""
    if isinstance(name, str):
        inst = tc.NAMED[name]()
    elif name[0] > 100:
        inst = tc.classes(*name, groups=3)
    else:
        inst = tc.shaped(*name)
    out = tc.twin_allocate(*inst)[:6]
    for a in inst + out[:2]:
        a.setflags(write=False)
    return inst, out


def _same(got, want):
    assert got[2:] == want[2:], (got[2:], want[2:])
    assert float(got[2]).hex() == float(want[2]).hex()
    for a, b in zip(got[:2], want[:2]):
        assert np.array_equal(np.ascontiguousarray(a).view(np.uint64), np.ascontiguousarray(b).view(np.uint64))


@pytest.mark.parametrize("name", SHAPES + list(tc.NAMED), ids=str)
def test_gpu_bit_exact_vs_twin(gpu_solver, name):
    inst, want = _case(name)
    got = gpu_solver.wf_allocate_types(*inst)
    print(f"{name}: gpu level {got[2]!r} steps {got[3]} stages {got[4]} flags {got[5]}; twin {want[2:]}")
    _same(got, want)
    x, F, level, steps, stages, flags = got
    if name == "one_stage":
        assert stages == 1 and flags & gpu_solver.WFT_ONE
    if name == "all_capped":
        assert np.abs(x.sum(axis=1) - 1.0).max() <= SHARE_BAR and stages >= 2
    if name == "many_stages":
        assert stages >= 8
    if name == "last_job_alone":
        assert stages == 2 and F[5] > F[0]
    if name == "zero_worker":
        assert (x[:, [1, 3]] == 0.0).all()
    tc.check_rows(*inst, x, F)


def test_gpu_batch_equals_single_calls_and_twin(gpu_solver):
    import sw_native as sn

    names = [(5, 3), (513, 3), None, (1, 3), "last_job_alone", "one_stage", "all_capped", (33, 3)]
    insts = []
    for nm in names:
        if nm is None:
            insts.append((np.array([2, 0, 1], dtype=np.int32), np.zeros(0, dtype=np.int32), np.zeros((0, 3))))
        else:
            insts.append(_case(nm)[0])
    out = gpu_solver.wf_allocate_types_batch(insts)
    assert len(out) == len(insts)
    for nm, inst, got in zip(names, insts, out):
        if nm is None:
            assert got[0].shape == (0, 3) and got[1].shape == (0,) and got[2:] == (0.0, 0, 0, 0)
            continue
        _same(got, gpu_solver.wf_allocate_types(*inst))
        _same(got, _case(nm)[1])
    good = np.cumsum([0] + [len(i[1]) for i in insts])
    for bad in (good + 1, np.r_[good[:2], good[1] - 1, good[3:]]):
        with pytest.raises(sn.NativeError) as e:
            gpu_solver.wf_allocate_types_batch(insts, offsets=bad)
        assert e.value.code == sn.SW_ERR_INVALID
    assert gpu_solver.wf_allocate_types_batch([]) == []


def test_gpu_within_the_bars_of_the_reference(gpu_solver):
    """The GPU's own levels, frozen sets and shares against the independent
    reference: the first 8 fuzz instances with m·n ≤ 40."""
    import wf_types_ref as ref

    picked = [i for i, inst in enumerate(tc.fuzz()) if inst[2].size <= 40][:8]
    worst = gap = 0.0
    for i in picked:
        inst = tc.fuzz()[i]
        F_ref, froze_ref, stages_ref, *_ = ref.allocate(*inst)
        assert F_ref is not None
        x, F, level, _, stages, flags = gpu_solver.wf_allocate_types(*inst)
        tc.check_rows(*inst, x, F)
        assert stages == stages_ref
        for s in range(1, stages + 1):  # the jobs of a stage share its level, bit for bit
            assert len(set(F[froze_ref == s])) == 1
        gap = max(gap, float((np.abs(F - F_ref) / F_ref).max()))
        worst = max(worst, float(np.abs(x - ref.centre(*inst, F_ref, froze_ref)).max()))
    print(f"gpu: worst level gap {gap:.3e}, worst max|x - x_ref| = {worst:.3e}")
    assert len(picked) == 8 and gap <= LEVEL_BAR and worst <= SHARE_BAR


def test_gpu_rejects_bad_input_and_goes_on(gpu_solver):
    import sw_native as sn

    ok = dict(W=np.array([4, 2], dtype=np.int32), sf=np.array([1, 1], dtype=np.int32),
              c=np.array([[1.0, 2.0], [3.0, 1.0]]))

    def refused(match=None, **kw):
        v = dict(ok, **kw)
        with pytest.raises(sn.NativeError, match=match) as e:
            gpu_solver.wf_allocate_types(v["W"], v["sf"], v["c"])
        assert e.value.code == sn.SW_ERR_INVALID
        x, F, level, _, stages, flags = gpu_solver.wf_allocate_types(*ok.values())  # and a good call after it
        assert stages >= 1 and level > 0.0

    refused(sf=[1, 0], match="job 1")
    refused(sf=[256, 1], match="job 0")
    refused(W=[4, -1])
    refused(c=np.array([[1.0, np.nan], [1.0, 1.0]]), match="job 0")
    refused(c=np.array([[1.0, -1.0], [1.0, 1.0]]))
    refused(c=np.array([[1.0, np.inf], [1.0, 1.0]]))
    refused(c=np.array([[0.0, 0.0], [1.0, 1.0]]), match="job 0")  # no positive coefficient
    refused(W=[4, 0], c=np.array([[0.0, 2.0], [1.0, 1.0]]), match="job 0")  # … on a type with workers
    got = gpu_solver.wf_allocate_types([4, 2], [], np.zeros((0, 2)))
    assert got[0].shape == (0, 2) and got[2:] == (0.0, 0, 0, 0)
    got = gpu_solver.wf_allocate_types([0, 0], [1, 1], np.ones((2, 2)))  # no type has workers
    assert (got[0] == 0.0).all() and got[2:] == (0.0, 0, 0, 0)
    with pytest.raises(sn.NativeError) as e:
        gpu_solver.wf_allocate_types(np.full(17, 8), [1, 1], np.ones((2, 17)))
    assert e.value.code == sn.SW_ERR_INVALID
    n = tc.const("max_jobs") + 1
    assert n == 16385
    with pytest.raises(sn.NativeError) as e:
        gpu_solver.wf_allocate_types([4], np.ones(n, dtype=np.int32), np.ones((n, 1)))
    assert e.value.code == sn.SW_ERR_INVALID
    inst, want = _case((5, 3))
    _same(gpu_solver.wf_allocate_types(*inst), want)


def test_gpu_policy_mirror_equals_the_twin_backed_one(gpu_solver):
    import max_min_fairness_water_filling as wf
    from test_wf_types_policy import _instance, policy_args

    W, sf, w, thr = _instance()
    pg = wf.MaxMinFairnessWaterFillingPolicyWithPerf(native=gpu_solver, worker_types=True)
    pt = wf.MaxMinFairnessWaterFillingPolicyWithPerf(native=tc.TwinEngine(), worker_types=True)
    args = policy_args(thr, sf, w, W)
    assert pg.get_allocation(*args) == pt.get_allocation(*args) and pg.last_level == pt.last_level
