"""Max-sum-throughput allocation (Gavel's efficiency baseline, sw_mst_allocate):
the CPU twin of the HIP kernel (tests/twins/mst_twin.c) against the LP's exact
optimum (the fractional knapsack in rational arithmetic) and against the
reference's LP through HiGHS, in tests/mst_ref.py.
The HIP kernel against the twin, bit for bit: tests/test_gpu_mst.py."""
from fractions import Fraction

import numpy as np
import pytest

import mst_ref
import mstcases as mc


def measure(inst, probes=None):
    """(result, relative objective gap to the exact optimum, exact capacity
    excess relative to G), the gap taken on the exact objective of the
    returned x."""
    sf, w, l, G = inst
    r = mst_ref.twin_allocate(*inst, probes)
    opt, dropped = mst_ref.exact_optimum(sf, w, l, G)
    assert r[4] == dropped
    got = mst_ref.exact_objective(w, r[0])
    gap = abs(opt - got) / opt if opt > 0 else abs(opt - got)
    excess = (mst_ref.exact_used(sf, r[0]) - G) / G
    # the reported objective is the detsum of w·x: N roundings of a sum of positives
    assert abs(r[3] - float(got)) <= 4 * len(sf) * mst_ref.EPS * float(got)
    return r, gap, excess


@pytest.fixture(scope="module")
def fixed():
    out = {}
    for name, inst in mc.FIXED.items():
        probes = []
        out[name] = measure(inst, probes) + (probes[0],)
    return out


@pytest.fixture(scope="module")
def fuzz():
    insts = mc.random_instances(300, seed=3, max_n=60)
    return insts, [measure(inst) for inst in insts]


@pytest.mark.parametrize("name", sorted(mc.FIXED))
def test_fixed_list_is_optimal_and_centred(fixed, name):
    r, gap, excess, probes = fixed[name]
    print(name, "gap", float(gap), "excess", float(excess), "probes", probes)
    assert gap <= Fraction(mc.OBJ_BAR)
    assert excess <= Fraction(mc.CAP_BAR)
    assert probes[0] <= 64 and probes[1] <= 64
    mst_ref.check_allocation(mc.FIXED[name], *r, cap_excess=mc.CAP_BAR)


def test_fixed_list_reaches_every_path(fixed):
    seen = set()
    for name, (r, *_) in fixed.items():
        seen |= mc.paths(mc.FIXED[name], r)
    assert seen == mc.ALL_PATHS, (mc.ALL_PATHS - seen, seen - mc.ALL_PATHS)
    assert {len(i[0]) for i in mc.FIXED.values()} >= {1, 2, 511, 512, 513, 1025, 3072, 3073}


def test_fixed_list_by_hand():
    """The cases whose answer is known by hand."""
    f = mc.FIXED
    x, lam, m, obj, dropped = mst_ref.twin_allocate(*f["all_tied"])
    assert lam == 2.5 and np.all(np.abs(x - 0.6) < 1e-15) and x[0] == x[1] == x[2] == x[3] == x[4]
    x, lam, m, obj, dropped = mst_ref.twin_allocate(*f["boundary"])
    assert list(x) == [1.0, 1.0, 0.0, 0.0] and (lam, m, obj, dropped) == (2.0, 0.0, 7.0, False)
    x, lam, m, obj, dropped = mst_ref.twin_allocate(*f["point_at_floors"])
    assert list(x) == [0.5, 0.5, 0.0] and (lam, m, dropped) == (1.0, 0.0, False)
    x, lam, m, obj, dropped = mst_ref.twin_allocate(*f["sf_above_G"])
    assert list(x) == [0.5, 0.0, 0.0] and lam == 10.0 and obj == 40.0
    x, lam, m, obj, dropped = mst_ref.twin_allocate(*f["slack_empty_class"])
    assert list(x) == [1.0, 1.0, 1.0] and (lam, m, obj, dropped) == (0.0, 0.0, 11.0, False)
    x, lam, m, obj, dropped = mst_ref.twin_allocate(*f["slack_point"])
    assert list(x) == [1.0, 0.0] and (lam, m) == (0.0, 0.0)
    for name in ("floor_above_one", "floors_above_G", "floor_inf"):
        assert mst_ref.twin_allocate(*f[name])[4] is True
    x, lam, m, obj, dropped = mst_ref.twin_allocate(*f["floor_is_one"])
    assert x[0] == 1.0 and abs(x[1] - 0.5) < 1e-15 and x[1] == x[2] and not dropped
    # floors of None and floors of zeros are the same instance
    sf, w, l, G = f["floors_all_zero"]
    assert mc.same_bits(mst_ref.twin_allocate(sf, w, l, G), mst_ref.twin_allocate(sf, w, None, G))


def test_random_instances_are_optimal_and_centred(fuzz):
    insts, res = fuzz
    worst_gap = max(g for _, g, _ in res)
    worst_excess = max(e for _, _, e in res)
    print("worst gap", float(worst_gap), "worst excess", float(worst_excess))
    assert worst_gap <= Fraction(mc.OBJ_BAR)
    assert worst_excess <= Fraction(mc.CAP_BAR)
    for inst, (r, _, _) in zip(insts, res):
        mst_ref.check_allocation(inst, *r, cap_excess=mc.CAP_BAR)
    # the set has ties, floors, infeasible floors and zero throughputs
    tags = [mc.paths(inst, r) for inst, (r, _, _) in zip(insts, res)]
    for t in ("tight_nu_neg", "tight_nu_pos", "tight_point", "slack_mu", "slack_empty", "dropped",
              "floor_in_class"):
        assert sum(t in p for p in tags) >= 5, t


def test_recorded_worst_figures_are_the_measured_ones(fixed, fuzz):
    """The bars are 8 × the recorded worst figures: the record must be what
    these sets give."""
    gaps = [g for _, g, _, _ in fixed.values()] + [g for _, g, _ in fuzz[1]]
    excesses = [e for _, _, e, _ in fixed.values()] + [e for _, _, e in fuzz[1]]
    assert float(max(gaps)) == mc.WORST_OBJ_GAP
    assert float(max(excesses)) == mc.WORST_CAP_EXCESS


def test_highs_agrees_with_the_exact_optimum(fuzz):
    """The reference's LP through HiGHS, held to its own tolerance 1e-7."""
    insts = list(mc.FIXED.values()) + fuzz[0]
    for sf, w, l, G in insts:
        if len(sf) > 60:
            continue
        opt, dropped = mst_ref.exact_optimum(sf, w, l, G)
        lp, lp_dropped = mst_ref.lp_optimum(sf, w, l, G)
        assert lp_dropped == dropped
        assert abs(lp - float(opt)) <= 1e-7 * max(1.0, float(opt))
        got = mst_ref.twin_allocate(sf, w, l, G)[3]
        assert abs(lp - got) <= 1e-7 * max(1.0, float(opt))


def test_twin_is_deterministic_and_empty_input_yields_zeros():
    for inst in [mc.FIXED["n513"], mc.FIXED["floors_on_class"], mc.FIXED["slack_zero_tp"]]:
        assert mc.same_bits(mst_ref.twin_allocate(*inst), mst_ref.twin_allocate(*inst))
    x, lam, m, obj, dropped = mst_ref.twin_allocate([], [], None, 8)
    assert len(x) == 0 and (lam, m, obj, dropped) == (0.0, 0.0, 0.0, False)


def test_checker_rejects_a_shifted_x_and_a_wrong_lambda():
    inst = mc.FIXED["floors_on_class"]
    x, lam, m, obj, dropped = mst_ref.twin_allocate(*inst)
    mst_ref.check_allocation(inst, x, lam, m, obj, dropped, cap_excess=mc.CAP_BAR)
    cls = np.flatnonzero(inst[1] / inst[0] == lam)
    y = x.copy()  # capacity kept, stationarity broken
    y[cls[0]] += 1e-6
    y[cls[1]] -= 1e-6
    with pytest.raises(AssertionError):
        mst_ref.check_allocation(inst, y, lam, m, obj, dropped, cap_excess=mc.CAP_BAR)
    y = x.copy()  # capacity exceeded
    y[cls[0]] += 1e-9
    with pytest.raises(AssertionError):
        mst_ref.check_allocation(inst, y, lam, m, obj, dropped, cap_excess=mc.CAP_BAR)
    for wrong in (4.5, 1.0, 0.0):  # another job's density, a value below, slack
        with pytest.raises(AssertionError):
            mst_ref.check_allocation(inst, x, wrong, m, obj, dropped, cap_excess=mc.CAP_BAR)
    with pytest.raises(AssertionError):
        mst_ref.check_allocation(inst, x, lam, m, obj, True, cap_excess=mc.CAP_BAR)
