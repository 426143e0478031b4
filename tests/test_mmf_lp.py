"""The worker-type MaxMinFairness LP (sw_mmf_allocate_types, csrc/sw_mmf_lp.h)
at hard shapes, on the CPU: the twin of the simplex kernel (oracle/mmf_twin.c,
the kernel's pivots and bits) against a plain reference (tests/mmf_lp_ref.py:
the level from HiGHS at tolerances of 1e-10, the constraint residuals in exact
rational arithmetic) on the families of tests/mmflpcases.py.

Bars (check_optimal of tests/test_mmf_types.py): rc = 0, the level within
1e-9·max(1, |t*|), every residual ≤ 1e-9; and the pivots taken within 10 % of
sw_lp_max_pivots.  The GPU side (tests/test_gpu_mmf_lp.py) holds the kernel to
this twin bit for bit.
"""
import functools

import numpy as np
import pytest

import mmf_lp_ref as ref
import mmf_ref
import mmflpcases as mc

TOL = 1e-9
PIVOT_SHARE = 0.10
# decades6 (coefficients over six decades, levels near 1e-3): HiGHS's own
# accuracy there is not known, so the level is held relative to t* itself.  The
# twin's worst |t − t*| / t* against mmf_lp_ref.level over this file's decades6
# cases is 1.68e-11 (80 × 16, seed 1); the bar is ten times that
# (the twin is deterministic; the margin is room for later rule changes).
DECADES6_MEASURED = 1.68e-11
DECADES6_LEVEL_REL = 10 * DECADES6_MEASURED

OTHER_SEEDS = range(2)


def _cases():
    out = []
    for m, n in mc.SHAPES:
        out += [("sparse", m, n, s) for s in mc.SPARSE_SEEDS]
    out += [("sparse", m, n, s) for m, n, s in mc.SPARSE_EXTRA]
    for fam in mc.FAMILIES:
        if fam != "sparse":
            out += [(fam, m, n, s) for m, n in mc.SHAPES for s in OTHER_SEEDS]
    return out


CASES = _cases()


@functools.lru_cache(maxsize=None)
def _solved(fam, m, n, seed):
    W, sf, c = mc.FAMILIES[fam](m, n, seed)
    return (W, sf, c) + mmf_ref.twin_allocate_types_rc(W, sf, c)


def check(W, sf, c, x, t, piv, rc, level_bar=None):
    m, n = c.shape
    cap = mmf_ref.twin_lp_max_pivots(m, n)
    t_lp = ref.level(W, sf, c)
    print(f"rc {rc} pivots {piv} of {cap} t {t!r} t* {t_lp!r}")
    assert rc == 0, f"rc {rc} after {piv} pivots (cap {cap})"
    res = ref.residuals(W, sf, c, x, t)
    print(res)
    assert max(res.values()) <= TOL, res
    if level_bar is None:
        assert abs(t - t_lp) <= TOL * max(1.0, abs(t_lp)), (t, t_lp)
    else:
        assert abs(t - t_lp) <= level_bar * abs(t_lp), (t, t_lp, abs(t - t_lp) / abs(t_lp))
    assert piv <= PIVOT_SHARE * cap, (piv, cap)


@pytest.mark.parametrize("fam,m,n,seed", CASES, ids=[f"{f}-{m}x{n}-{s}" for f, m, n, s in CASES])
def test_twin_vs_reference(fam, m, n, seed):
    W, sf, c, x, t, piv, rc = _solved(fam, m, n, seed)
    check(W, sf, c, x, t, piv, rc, DECADES6_LEVEL_REL if fam == "decades6" else None)
    if fam == "all_zero_job":
        assert t == 0.0


_EDGES = mc.edges()


@pytest.mark.parametrize("i", range(len(_EDGES)), ids=[name for name, _ in _EDGES])
def test_twin_edges_vs_reference(i):
    name, (W, sf, c) = _EDGES[i]
    x, t, piv, rc = mmf_ref.twin_allocate_types_rc(W, sf, c)
    check(W, sf, c, x, t, piv, rc)
    if name.startswith("stranded"):
        assert t == 0.0


@pytest.mark.parametrize("fam", ["decades3", "zero_type", "tight"])
@pytest.mark.parametrize("k", mc.SCALE_EXPONENTS)
def test_scale_invariance_is_exact(fam, k):
    """t*(s·c) = s·t*(c), and the allocation does not depend on s: for s = 2^k
    the coefficients normalise to the same tableau, so x is the unscaled call's
    bit for bit, and so are the pivots, and t is exactly s times its level."""
    m, n = mc.SCALE_SHAPE
    for seed in range(2):
        W, sf, c, x0, t0, p0, rc0 = _solved(fam, m, n, seed)
        assert rc0 == 0 and t0 > 0.0
        x, t, p, rc = mmf_ref.twin_allocate_types_rc(*mc.scaled((W, sf, c), k))
        assert rc == 0 and p == p0
        assert np.array_equal(x.view(np.uint64), x0.view(np.uint64))
        assert t == float(np.ldexp(t0, k)), (t, t0, k)


@pytest.mark.parametrize("fam", ["decades3", "zero_type", "tight"])
def test_scale_base_cases_are_optimal(fam):
    m, n = mc.SCALE_SHAPE
    for seed in range(2):
        check(*_solved(fam, m, n, seed))


def test_entering_rule_by_hand():
    """The steep rule takes the most negative entry, ties to the lowest column;
    Bland's the lowest column below −eps; neither a column at or above −eps."""
    enter = mmf_ref.twin_lp_enter
    obj = [0.0, -1.0, -3.0, 5.0, -3.0, -2.0, -3.0]
    assert enter(obj, False) == 2
    assert enter(obj, True) == 1
    assert enter(obj[::-1], False) == 0
    assert enter(obj[::-1], True) == 0
    assert enter([0.0, -1e-12, 2.0, -1e-11], False) == mmf_ref.LP_NO_COLUMN
    assert enter([0.0, -1e-12, 2.0, -1e-11], True) == mmf_ref.LP_NO_COLUMN
    assert enter([0.0, -1e-12, -2e-11, -1e-9], False) == 3
    assert enter([0.0, -1e-12, -2e-11, -1e-9], True) == 2
    assert enter([], False) == mmf_ref.LP_NO_COLUMN


def test_stall_counter_by_hand():
    """Bland's rule takes over after 8 pivots in a row that did not raise the
    objective above the best value seen, and holds until one does."""
    stall = mmf_ref.twin_lp_stall
    assert stall([0.0] * 7) == [False] * 7           # the slack basis has value 0: no rise
    assert stall([0.0] * 10) == [False] * 7 + [True] * 3
    assert stall([1.0] + [1.0] * 8 + [1.0, 2.0, 2.0]) == [False] * 8 + [True, True, False, False]
    # a dip below the best seen (rounding) is no rise, nor is the way back up to it
    assert stall([1.0, 0.5] + [0.75] * 6 + [1.0, 1.0 + 2.0 ** -52]) == [False] * 8 + [True, False]
    # rises between stalls reset the count
    assert stall(([3.0] * 7 + [4.0]) + [4.0] * 7) == [False] * 15


def test_normalisation_exponent_and_scaling():
    """2^k brings the largest coefficient into [1, 2): normal and subnormal
    doubles, both ends of the range; 0 is left alone; the scaling is exact."""
    shift, scale = mmf_ref.twin_lp_shift, mmf_ref.twin_lp_scale
    assert shift(0.0) == 0
    rng = np.random.default_rng(17)
    vals = [1.0, 1.5, np.nextafter(2.0, 0.0), 2.0, 0.75, np.nextafter(1.0, 0.0), 255.0, 1e-3, 3e-31, 2.0 ** 30,
            2.0 ** -300, 2.0 ** 300, np.finfo(np.float64).max, np.finfo(np.float64).tiny,
            np.nextafter(np.finfo(np.float64).tiny, 0.0), 5e-324, 3 * 5e-324, 2.0 ** -1060 * 1.25]
    vals += list(np.ldexp(rng.uniform(1.0, 2.0, size=200), rng.integers(-1074, 1024, size=200)))
    for v in vals:
        v = float(v)
        if v == 0.0:
            continue
        k = shift(v)
        s = scale(v, k)
        assert 1.0 <= s < 2.0, (v, k, s)
        assert s == float(np.ldexp(v, k))         # exact: ldexp upwards loses nothing
        assert scale(s, -k) == v                  # and back
    assert scale(0.0, 700) == 0.0
