"""The water-filling policy mirror over worker types that differ
(MaxMinFairnessWaterFillingPolicyWithPerf(worker_types=True),
max_min_fairness_water_filling.py) without a GPU, over the CPU twins
(tests/wftcases.py TwinEngine)."""
import numpy as np
import pytest

import max_min_fairness_water_filling as wf
import wf_types_ref as ref
import wftcases as tc

TYPES = ["k80", "p100", "v100"]


def _instance():
    """Seven jobs on three types; capacity binds, three stages."""
    rng = np.random.default_rng(6184)
    W = np.array([2, 1, 1], dtype=np.int32)
    sf = np.array([1, 2, 1, 4, 1, 2, 1], dtype=np.int32)
    w = np.array([1.0, 2.0, 0.5, 1.0, 4.0, 1.0, 2.0])
    thr = rng.uniform(0.2, 5.0, size=(7, 3)) * np.array([0.6, 1.0, 1.8])[None, :]
    return W, sf, w, thr


def policy_args(thr, sf, w, W, types=TYPES, first=0):
    ids = [first + j for j in range(len(sf))]
    tp = {i: {t: float(thr[j, k]) for k, t in enumerate(types)} for j, i in enumerate(ids)}
    return (tp, {i: int(sf[j]) for j, i in enumerate(ids)}, {i: float(w[j]) for j, i in enumerate(ids)},
            {t: int(W[k]) for k, t in enumerate(types)})


def test_default_still_raises():
    W, sf, w, thr = _instance()
    eng = tc.TwinEngine()
    pol = wf.MaxMinFairnessWaterFillingPolicyWithPerf(native=eng)
    with pytest.raises(NotImplementedError, match="differ by worker type"):
        pol.get_allocation(*policy_args(thr, sf, w, W))
    assert eng.calls == []
    with pytest.raises(NotImplementedError):
        wf.MaxMinFairnessWaterFillingPolicyWithPerf(priority_reweighting_policies={}, worker_types=True)


def test_worker_types_returns_the_kernel_s_shares_clipped():
    W, sf, w, thr = _instance()
    eng = tc.TwinEngine()
    pol = wf.MaxMinFairnessWaterFillingPolicyWithPerf(native=eng, worker_types=True)
    args = policy_args(thr, sf, w, W)
    alloc = pol.get_allocation(*args)
    assert eng.calls == ["wf_allocate_types"]
    assert sorted(alloc) == list(range(7)) and all(sorted(alloc[j]) == TYPES for j in alloc)
    x = np.array([[alloc[j][t] for t in TYPES] for j in range(7)])
    assert (x >= 0.0).all() and (x <= 1.0).all()
    # restated: the coefficients in the reference's operations, the twin on them
    prop = tc.proportional(thr, W)
    coef = thr / prop[:, None] * np.array([(1.0 / w[j]) * sf[j] for j in range(7)])[:, None]
    xt, F, level, _, stages, _, _ = tc.twin_allocate(W, sf, coef)
    assert np.array_equal(x, xt.clip(min=0.0).clip(max=1.0))
    assert pol.last_level == (level, stages) and stages >= 2
    tc.check_rows(W, sf, coef, x, F)
    # and the independent stage loop on the same coefficients
    F_ref, froze_ref, stages_ref, *_ = ref.allocate(W, sf, coef)
    assert stages == stages_ref and (np.abs(F - F_ref) <= 1e-6 * F_ref).all()


def test_effective_throughputs_are_the_levels_over_the_multipliers():
    W, sf, w, thr = _instance()
    pol = wf.MaxMinFairnessWaterFillingPolicyWithPerf(native=tc.TwinEngine(), worker_types=True)
    args = policy_args(thr, sf, w, W)
    eff, ids = pol.get_allocation(*args, return_effective_throughputs=True)
    alloc = pol.get_allocation(*args)
    assert ids == list(range(7))
    x = np.array([[alloc[j][t] for t in TYPES] for j in range(7)])
    prop = tc.proportional(thr, W)
    assert np.abs(eff - (thr * x).sum(axis=1) / prop).max() <= 1e-12
    # val_j = eff_j · mult_j is at least the job's level
    mult = np.array([(1.0 / w[j]) * sf[j] for j in range(7)])
    _, F, *_ = tc.twin_allocate(W, sf, thr / prop[:, None] * mult[:, None])
    assert (eff * mult >= F * (1.0 - 1e-9)).all()


def test_a_flagged_result_warns():
    W, sf, w, thr = _instance()

    class Flagged(tc.TwinEngine):
        def wf_allocate_types(self, W, sf, coef):
            return super().wf_allocate_types(W, sf, coef)[:5] + (2,)

    pol = wf.MaxMinFairnessWaterFillingPolicyWithPerf(native=Flagged(), worker_types=True)
    with pytest.warns(wf.WaterFillingStageWarning, match="threshold"):
        pol.get_allocation(*policy_args(thr, sf, w, W))
    assert pol.last_flags == 2
    import warnings
    quiet = wf.MaxMinFairnessWaterFillingPolicyWithPerf(native=tc.TwinEngine(), worker_types=True)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        quiet.get_allocation(*policy_args(thr, sf, w, W))
    assert quiet.last_flags == 0


def test_identical_types_still_go_to_the_one_type_call():
    sf = np.array([1, 2, 4, 1, 2], dtype=np.int32)
    thr = np.repeat(np.array([3.0, 4.0, 5.0, 6.0, 7.0])[:, None], 3, axis=1)
    args = policy_args(thr, sf, [1.0, 2.0, 1.0, 0.5, 1.0], [1, 1, 1])
    e0, e1 = tc.TwinEngine(), tc.TwinEngine()
    a0 = wf.MaxMinFairnessWaterFillingPolicyWithPerf(native=e0).get_allocation(*args)
    a1 = wf.MaxMinFairnessWaterFillingPolicyWithPerf(native=e1, worker_types=True).get_allocation(*args)
    assert a0 == a1 and e0.calls == e1.calls == ["wf_allocate"]


def test_refusals_each_followed_by_a_good_call():
    W, sf, w, thr = _instance()
    pol = wf.MaxMinFairnessWaterFillingPolicyWithPerf(native=tc.TwinEngine(), worker_types=True)
    good = policy_args(thr, sf, w, W)
    want = pol.get_allocation(*good)
    bad = thr.copy()
    bad[3, :] = 0.0
    with pytest.raises(ValueError, match="job 3"):
        pol.get_allocation(*policy_args(bad, sf, w, W))
    assert pol.get_allocation(*good) == want
    bad[3, 1] = 2.0  # only on a type without workers
    with pytest.raises(ValueError, match="job 3"):
        pol.get_allocation(*policy_args(bad, sf, w, [W[0], 0, W[2]]))
    wbad = w.copy()
    wbad[5] = 0.0
    with pytest.raises(ValueError, match="job 5"):
        pol.get_allocation(*policy_args(thr, sf, wbad, W))
    assert pol.get_allocation(*good) == want
    assert pol.get_allocation({}, {}, {}, {t: 1 for t in TYPES}) is None
