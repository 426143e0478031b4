"""Water-filling MaxMinFairness allocation (Gavel baseline, sw_wf_allocate):
the CPU twin of the HIP kernel (tests/twins/wf_twin.c) against an exact
rational certificate of its level, the sort-based closed form, the
reference's stage loop restated over HiGHS
(policies/max_min_fairness_water_filling.py:303-409) and the MaxMinFairness
twin.  The HIP kernel against the twin, bit for bit: tests/test_gpu_wf.py."""
import math
from fractions import Fraction

import numpy as np
import pytest

import mmf_ref
import wf_ref
import wfcases as wc


def check(inst):
    r = wf_ref.twin_allocate(*inst)
    wc.check_allocation(inst, *r)
    return r


@pytest.mark.parametrize("name", sorted(wc.FIXED))
def test_twin_level_certified_and_closed_form(name):
    check(wc.FIXED[name])


def test_fixed_list_covers_the_cases_and_their_edges():
    r = {k: wf_ref.twin_allocate(*v) for k, v in wc.FIXED.items()}
    assert r["n1"][0][0] == 1.0 and r["n1"][1] == 2.0 and r["n1"][2] == 2.0
    assert r["n1_binds"][0][0] == 0.5 and r["n1_binds"][2] == 2.0
    x, level, used = r["sum_equals_G"]
    assert np.all(x == 1.0) and level == 4.0 and used == 8.0
    x, level, used = r["sum_is_G_plus_1"]
    # the level reaches c = 2 exactly as capacity fills; L* lies a few ulps past it
    assert abs(x[1] - 0.5) <= 1e-15 and np.all(np.delete(x, 1) == 1.0) and abs(used - 7.0) <= 1e-14
    assert np.all(r["all_saturate"][0] == 1.0) and r["all_saturate"][2] == 16.0
    assert np.all(r["none_saturates"][0] < 1.0) and r["none_saturates"][1] == 0.5
    x, level, _ = r["tie_at_level"]
    assert np.all(x[:2] == 1.0) and np.all(np.abs(x[2:] - 0.5) <= 1e-15) and abs(level - 1.0) <= 1e-15
    x = r["tie_above_level"][0]
    assert x[0] == 1.0 and x[1] == x[2] == x[3] < 1.0
    assert min(wc.FIXED["no_unit_width"][0]) > 1 and max(wc.FIXED["sf255"][0]) == 255
    assert wc.FIXED["G1"][2] == 1 and abs(r["G1"][2] - 1.0) <= 1e-15
    x = r["spread"][0]
    assert x[0] == x[1] == 1.0 and abs(x[2] - 0.375) <= 1e-15 and 0.0 < x[4] < x[3] < 1e-100
    sizes = sorted(len(v[0]) for v in wc.FIXED.values() if len(v[0]) > 500)
    assert sizes == [511, 512, 513, 1025, 2048, 2049, 2500, 2500]
    big = [k for k, v in wc.FIXED.items() if len(v[0]) > 500]
    some = [0.0 < (r[k][0] == 1.0).mean() < 1.0 for k in big]
    assert any(some) and not all(some)  # some saturate a part of the jobs, some none or all


def test_twin_random_instances():
    whole = partly = 0
    for inst in wc.random_instances(200, seed=7, max_n=300):
        x, _, _ = check(inst)
        whole += bool(np.all(x == 1.0))
        partly += bool(0 < (x == 1.0).sum() < len(x))
    assert whole >= 5 and partly >= 40


def test_shares_agree_with_the_reference_stage_loop():
    """|x − x_stage_loop| ≤ 1e-6 absolute (ten times HiGHS's default
    feasibility tolerance) on 60 seeded instances with N ≤ 13; the ones where
    scipy reports failure are left out, at most 5 of them."""
    insts = wc.stage_instances()
    failed, worst, most_stages = 0, 0.0, 0
    for sf, w, G in insts:
        x, _, _ = wf_ref.twin_allocate(sf, sf / w, G)
        ref, stages, ok = wf_ref.stage_loop(sf, w, G)
        if not ok:
            failed += 1
            continue
        most_stages = max(most_stages, stages)
        diff = float(np.max(np.abs(np.clip(ref, 0.0, 1.0) - x)))
        worst = max(worst, diff)
        assert diff <= 1e-6, (diff, list(sf), list(w), G)
    print(f"stage loop: {failed} of {len(insts)} failed, up to {most_stages} stages, "
          f"worst share difference {worst:.3g}")
    assert failed <= 5
    assert most_stages >= 3


def mmf_instances():
    return list(wc.FIXED.values()) + wc.random_instances(100, seed=13, max_n=300)


def test_equals_max_min_fairness_where_capacity_binds_first():
    """Where G/Σ sf/c ≤ min c no job saturates and the allocation is the
    max-min LP's t*/c_j."""
    seen = 0
    for sf, c, G in mmf_instances():
        if not Fraction(G) / sum(Fraction(int(s)) / Fraction(float(v)) for s, v in zip(sf, c)) <= float(c.min()):
            continue
        seen += 1
        x, _, _ = wf_ref.twin_allocate(sf, c, G)
        _, t, _ = mmf_ref.twin_allocate(sf, c, G)
        assert np.all(np.abs(x - t / c) <= 1e-12 * (t / c))
    assert seen >= 20


def test_dominates_max_min_fairness_and_conserves_work():
    """Where capacity does not bind first every share is at least the max-min
    level's t*/c_j and the allocated capacity is min(G, Σ sf)."""
    seen = 0
    for sf, c, G in mmf_instances():
        if Fraction(G) / sum(Fraction(int(s)) / Fraction(float(v)) for s, v in zip(sf, c)) <= float(c.min()):
            continue
        seen += 1
        x, _, used = wf_ref.twin_allocate(sf, c, G)
        _, t, _ = mmf_ref.twin_allocate(sf, c, G)
        assert np.all(x >= np.minimum(1.0, t / c) * (1 - 1e-12))
        want = min(G, int(sf.sum()))
        assert abs(used - want) <= 1e-12 * want
        assert abs(math.fsum(float(s) * float(v) for s, v in zip(sf, x)) - want) <= 1e-12 * want
    assert seen >= 20


def test_twin_empty_and_deterministic():
    x, level, used = wf_ref.twin_allocate([], [], 8)
    assert len(x) == 0 and level == 0.0 and used == 0.0
    for name in [k for k in wc.FIXED if k.startswith(("n513_", "n2049_"))] + ["spread"]:
        inst = wc.FIXED[name]
        assert wc.same_bits(wf_ref.twin_allocate(*inst), wf_ref.twin_allocate(*inst))


def test_certificate_rejects_a_wrong_level():
    sf, c, G = inst = wc.FIXED["no_unit_width"]
    _, level, _ = wf_ref.twin_allocate(*inst)
    assert wf_ref.certified(sf, c, G, level, 1e-9)
    assert not wf_ref.certified(sf, c, G, level * (1 + 1e-6), 1e-9)
    assert not wf_ref.certified(sf, c, G, level * (1 - 1e-6), 1e-9)


def test_level_is_ill_determined_past_a_kink_but_the_shares_are_not():
    """The limit sw_wf.h documents: the exact level sits just under c = 1e-150
    and the only job still rising beyond it has c = 1; cap in doubles is flat
    from 1e-150 to about 2e-16, L* is the far end of that flat, and every
    share is within an ulp of G = 2 of the exact one."""
    sf, c, G = np.array([1, 1, 1], dtype=np.int32), np.array([1e-300, 1e-150, 1.0]), 2
    x, level, used = wf_ref.twin_allocate(sf, c, G)
    exact = wf_ref.closed_form_level(sf, c, G)
    assert exact < Fraction(1e-150) < Fraction(level) < Fraction(1e-15)
    want = [min(Fraction(1), exact / Fraction(float(v))) for v in c]
    assert all(abs(Fraction(float(a)) - b) <= Fraction(2.0 ** -51) for a, b in zip(x, want))
    assert used == 2.0
