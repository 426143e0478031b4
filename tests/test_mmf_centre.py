"""The centred MaxMinFairness allocation over worker types
(sw_mmf_allocate_types_centred, csrc/sw_mmf_ipm.h) on the CPU: the twin of the
interior-point kernel (tests/twins/mmfc_twin.c) against

  * HiGHS for the level (1e-6·max(1, t*)) and the LP's constraints (1e-9);
  * an independent computation of the analytic centre of the optimal face
    (tests/mmf_centre_ref.py) for the shares: max |x − x_ref| ≤ 1e-6, the
    project's own bar, on 105 tiny instances of three families, none skipped;
  * the closed form of the one-type kernel (oracle/mmf_twin.c);
  * symmetry over identical types, the two degenerate inputs, exact scaling
    by powers of two, and the policy mirror's ``centred=True``.

Measured worst distances from the reference's centre per family (printed by
test_centre_matches_the_reference): generic 3.5e-9, identical 1.9e-10,
integer 4.6e-9.  One type: shares 3.8e-10, level 2.3e-13 relative."""
import os
import sys
import warnings

import numpy as np
import pytest

import mmf_centre_ref
import mmf_ref
import mmfccases as mc
from test_mmf_types import _policy_inputs, lp_cases

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                                "shockwave-replication_amd"))
import max_min_fairness as mmfp  # noqa: E402

CENTRE_TOL = 1e-6
LEVEL_TOL = 1e-6
FEAS_TOL = 1e-9


def check_level_and_feasibility(W, sf, c, x, t):
    """check_optimal of tests/test_mmf_types.py with the level's bar at 1e-6
    and every job reaching t·(1 − 1e-6)."""
    t_lp, _ = mmf_ref.lp_level_types(W, sf, c)
    assert abs(t - t_lp) <= LEVEL_TOL * max(1.0, abs(t_lp)), (t, t_lp)
    assert (x >= -FEAS_TOL).all()
    assert (x.sum(axis=1) <= 1.0 + FEAS_TOL).all()
    assert ((sf[:, None] * x).sum(axis=0) <= W + FEAS_TOL * np.maximum(W, 1)).all()
    assert ((c * x).sum(axis=1) >= t * (1.0 - 1e-6)).all()
    return abs(t - t_lp) / max(1.0, abs(t_lp))


@pytest.mark.parametrize("i", range(len(lp_cases())))
def test_level_and_feasibility_on_the_lp_cases(i):
    W, sf, c = lp_cases()[i]
    x, t, its = mc.twin_allocate(W, sf, c)
    check_level_and_feasibility(W, sf, c, x, t)
    assert 0 < its <= mc.max_iters()


def test_level_and_feasibility_fuzz():
    worst = 0.0
    fams = set()
    for fam, W, sf, c in mc.level_fuzz():
        x, t, _ = mc.twin_allocate(W, sf, c)
        worst = max(worst, check_level_and_feasibility(W, sf, c, x, t))
        fams.add(fam)
        assert (x[:, W == 0] == 0.0).all()
    print(f"level: worst |t - t*| / max(1, t*) = {worst:.3e} over {len(mc.level_fuzz())} instances")
    assert fams == set(mc.FAMILIES) and len(mc.level_fuzz()) == 150


def test_centre_matches_the_reference():
    cases = mc.centre_fuzz()
    assert len(cases) >= 100
    worst = {f: 0.0 for f in mc.FAMILIES}
    count = {f: 0 for f in mc.FAMILIES}
    for fam, W, sf, c, xr, tr in cases:
        x, t, _ = mc.twin_allocate(W, sf, c)
        worst[fam] = max(worst[fam], float(np.abs(x - xr).max()))
        count[fam] += 1
        assert abs(t - tr) <= LEVEL_TOL * max(1.0, tr)
    print("centre: worst max|x - x_ref| per family:", {f: f"{worst[f]:.3e} of {count[f]}" for f in worst})
    assert all(count[f] >= 10 for f in count), count
    assert max(worst.values()) <= CENTRE_TOL, worst


def test_reference_is_symmetric_on_symmetric_inputs():
    """The reference itself: identical types with equal worker counts get equal shares to 1e-10."""
    rng = np.random.default_rng(8)
    for _ in range(6):
        m, n = int(rng.integers(2, 10)), int(rng.integers(2, 4))
        sf = rng.choice([1, 2, 4], size=m).astype(np.int32)
        cj = rng.uniform(0.2, 4.0, size=m) * sf
        W = np.full(n, int(rng.integers(1, 2 * m)), dtype=np.int32)
        xr, _ = mmf_centre_ref.face_centre(W, sf, np.repeat(cj[:, None], n, axis=1))
        assert np.abs(xr - xr[:, :1]).max() <= 1e-10


def test_one_type_matches_the_closed_form():
    cases = mc.one_type_fuzz()
    assert len(cases) == 60
    wx = wt = 0.0
    for G, sf, c, x1, t1, _ in cases:
        x, t, _ = mc.twin_allocate([G], sf, c[:, None])
        wx = max(wx, float(np.abs(x[:, 0] - x1).max()))
        wt = max(wt, abs(t - t1) / t1)
    slack = sum(1 for case in cases if case[5])
    print(f"one type: worst |x - x1| = {wx:.3e}, worst |t - t1| / t1 = {wt:.3e}, capacity slack in {slack} of 60")
    assert 3 * slack >= len(cases)
    assert wx <= 1e-6 and wt <= 1e-6


def test_identical_types_get_equal_shares():
    rng = np.random.default_rng(5)
    worst = 0.0
    for i in range(40):
        m, n = int(rng.integers(1, 40)), int(rng.integers(2, 6))
        sf = rng.choice([1, 2, 4, 8], size=m).astype(np.int32)
        cj = sf / rng.choice([1.0, 2.0, 5.0], size=m) if i % 2 else rng.uniform(0.2, 4.0, size=m) * sf
        W = np.full(n, int(rng.integers(1, 2 * m + 2)), dtype=np.int32)
        x, _, _ = mc.twin_allocate(W, sf, np.repeat(cj[:, None], n, axis=1))
        worst = max(worst, float(np.abs(x - x[:, :1]).max()))
    print(f"symmetry: worst spread over identical types = {worst:.3e}")
    assert worst <= 1e-8


def test_a_type_without_workers_gets_exact_zeros():
    W, sf, c = mc.zero_worker_case()
    x, t, _ = mc.twin_allocate(W, sf, c)
    assert (x[:, 1] == 0.0).all()
    check_level_and_feasibility(W, sf, c, x, t)
    xr, _ = mmf_centre_ref.face_centre(W, sf, c)
    assert np.abs(x - xr).max() <= CENTRE_TOL


def test_level_zero_is_exact_and_the_allocation_is_still_the_centre():
    W, sf, c = mc.level_zero_case()
    x, t, _ = mc.twin_allocate(W, sf, c)
    assert t == 0.0
    assert (x[:, 1] == 0.0).all()
    xr, tr = mmf_centre_ref.face_centre(W, sf, c)
    assert tr == 0.0
    assert np.abs(x - xr).max() <= CENTRE_TOL
    # no type has workers: nothing to share out
    x, t, its = mc.twin_allocate([0, 0], [1, 2], np.ones((2, 2)))
    assert (x == 0.0).all() and t == 0.0 and its == 0


@pytest.mark.parametrize("k", [-30, -1, 1, 30])
def test_powers_of_two_scale_the_level_and_leave_the_allocation(k):
    for W, sf, c in (mc.shaped(5, 3), mc.shaped(33, 8), mc.zero_worker_case()):
        x0, t0, i0 = mc.twin_allocate(W, sf, c)
        x, t, i = mc.twin_allocate(W, sf, np.ldexp(c, k))
        assert i == i0 and t == float(np.ldexp(t0, k))
        assert np.array_equal(x.view(np.uint64), x0.view(np.uint64))


# ---- the policy mirror ----

TYPES = ["k80", "p100", "v100"]


def test_policy_centred_does_not_warn_and_reaches_the_level(monkeypatch):
    monkeypatch.setattr(mmfp, "_WARNED", False)
    thr, sf, pw, spec = _policy_inputs(6, TYPES)
    eng = mc.TwinEngine()
    pol = mmfp.MaxMinFairnessPolicyWithPerf(native=eng, centred=True)
    with warnings.catch_warnings(record=True) as seen:
        warnings.simplefilter("always")
        alloc = pol.get_allocation(thr, sf, pw, spec)
    assert not [w for w in seen if issubclass(w.category, mmfp.SimplexVertexWarning)]
    assert mmfp._WARNED is False
    assert eng.calls == ["mmf_allocate_types_centred"]
    coef, sfa, (job_ids, wts), W = pol.coefficients(thr, sf, pw, spec)
    x = np.array([[alloc[j][w] for w in wts] for j in job_ids])
    assert ((x >= 0.0) & (x <= 1.0)).all()
    t_lp, _ = mmf_ref.lp_level_types(W, sfa, coef)
    assert (coef * x).sum(axis=1).min() == pytest.approx(t_lp, rel=1e-6)
    assert pol.get_allocation({}, {}, {}, spec) is None


def test_policy_default_still_calls_the_simplex_and_warns(monkeypatch):
    monkeypatch.setattr(mmfp, "_WARNED", False)
    thr, sf, pw, spec = _policy_inputs(6, TYPES)
    eng = mc.TwinEngine()
    with pytest.warns(mmfp.SimplexVertexWarning):
        mmfp.MaxMinFairnessPolicyWithPerf(native=eng).get_allocation(thr, sf, pw, spec)
    assert eng.calls == ["mmf_allocate_types"]


def test_unit_policy_centred_differs_from_the_vertex(monkeypatch):
    """Unit throughputs over identical-looking types: the optimum is never
    unique, the vertex piles shares up, the centre spreads them."""
    monkeypatch.setattr(mmfp, "_WARNED", True)
    thr, sf, pw, spec = _policy_inputs(2, TYPES)
    eng = mc.TwinEngine()
    centre = mmfp.MaxMinFairnessPolicy(native=eng, centred=True).get_allocation(thr, sf, pw, spec)
    vertex = mmfp.MaxMinFairnessPolicy(native=eng).get_allocation(thr, sf, pw, spec)
    assert eng.calls == ["mmf_allocate_types_centred", "mmf_allocate_types"]
    jobs = sorted(thr)
    xc = np.array([[centre[j][w] for w in sorted(TYPES)] for j in jobs])
    xv = np.array([[vertex[j][w] for w in sorted(TYPES)] for j in jobs])
    assert np.abs(xc - xv).max() > 1e-3
    assert (xc > 0.0).all() and (xv == 0.0).any()
