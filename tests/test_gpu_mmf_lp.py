"""The worker-type MaxMinFairness LP on the GPU (sw_mmf_allocate_types:
k_lp_init, k_lp_select, k_lp_update, k_lp_result of csrc/sw_mmf.hip) at the
smallest shapes at which each part can go wrong, against the CPU twin bit for
bit — allocation, level and pivots — and the GPU's own allocation and level
against the exact residuals of tests/mmf_lp_ref.py (≤ 1e-9).  The twin itself is
held to HiGHS on these families by tests/test_mmf_lp.py.

  sparse 80 × 16, 120 × 12   Bland's rule alone took about 20,000 pivots / hit the cap
  sparse, decades3 24 × 16   the entering arg-min over 16 types
  300 × 2                    R = 602 rows: a second trip of k_lp_select's row loop
  3 × 16, 1 × 1, 2 × 1       fewer rows and columns than a wave
  unit, dup 60 × 8           ties in the entering and in the leaving rule
  tight 40 × 4, 100 × 8      W in {0, 1, 2}: degenerate rows, the pivot element's bar
  all_zero_job, stranded     t* = 0
  40 × 4 at 2^-30 and 2^30   the normalisation in k_lp_init and k_lp_result
"""
import functools

import numpy as np
import pytest

import mmf_lp_ref as ref
import mmf_ref
import mmflpcases as mc

pytestmark = pytest.mark.gpu

TOL = 1e-9

CASES = [
    ("sparse", 80, 16, 0, 0), ("sparse", 80, 16, 1, 0), ("sparse", 80, 16, 148, 0),
    ("sparse", 120, 12, 0, 0), ("sparse", 120, 12, 3, 0),
    ("sparse", 24, 16, 0, 0), ("decades3", 24, 16, 0, 0),
    ("decades3", 300, 2, 0, 0), ("zero_type", 300, 2, 0, 0),
    ("decades3", 3, 16, 0, 0), ("sparse", 3, 16, 0, 0), ("decades3", 1, 1, 0, 0), ("decades3", 2, 1, 0, 0),
    ("unit", 60, 8, 0, 0), ("dup", 60, 8, 0, 0),
    ("tight", 40, 4, 0, 0), ("tight", 40, 4, 1, 0), ("tight", 100, 8, 1, 0),
    ("all_zero_job", 60, 8, 0, 0), ("stranded_job", 12, 4, 0, 0),
    ("decades3", 40, 4, 0, -30), ("decades3", 40, 4, 0, 30), ("tight", 40, 4, 1, -30), ("tight", 40, 4, 1, 30),
]
_FAMILIES = dict(mc.FAMILIES, stranded_job=mc.stranded_job)


@functools.lru_cache(maxsize=None)
def _twin(fam, m, n, seed, k):
    """The inputs and the twin's answer, computed once and left unchanged."""
    W, sf, c = mc.scaled(_FAMILIES[fam](m, n, seed), k)
    x, t, piv, rc = mmf_ref.twin_allocate_types_rc(W, sf, c)
    assert rc == 0
    for a in (W, sf, c, x):
        a.setflags(write=False)
    return W, sf, c, x, t, piv


def _check(gpu_solver, case):
    W, sf, c, xt, tt, pt = _twin(*case)
    xg, tg, pg = gpu_solver.mmf_allocate_types(W, sf, c)
    print(f"{case}: pivots gpu {pg} twin {pt}, t gpu {tg!r} twin {tt!r}")
    assert pg == pt
    assert float(tg).hex() == float(tt).hex()
    assert np.array_equal(np.ascontiguousarray(xg).view(np.uint64), xt.view(np.uint64))
    res = ref.residuals(W, sf, c, xg, tg)
    print(res)
    assert max(res.values()) <= TOL, res
    return tg


@pytest.mark.parametrize("case", CASES, ids=[f"{f}-{m}x{n}-{s}" + (f"-2^{k}" if k else "") for f, m, n, s, k in CASES])
def test_gpu_lp_bit_exact_vs_twin(gpu_solver, case):
    t = _check(gpu_solver, case)
    if case[0] in ("all_zero_job", "stranded_job"):
        assert t == 0.0


def test_gpu_lp_level_scales_exactly(gpu_solver):
    """t(2^k·c) = 2^k·t(c) and the same allocation, on the GPU's own results."""
    W, sf, c, _, _, _ = _twin("decades3", 40, 4, 0, 0)
    x0, t0, p0 = gpu_solver.mmf_allocate_types(W, sf, c)
    for k in (-30, 30):
        x, t, p = gpu_solver.mmf_allocate_types(W, sf, np.ldexp(c, k))
        assert p == p0 and t == float(np.ldexp(t0, k))
        assert np.array_equal(np.ascontiguousarray(x).view(np.uint64), np.ascontiguousarray(x0).view(np.uint64))


def test_gpu_lp_one_handle_sizes_interleaved(gpu_solver):
    """Large, small, large on one handle: MmfBufs keeps the tableau, the basis
    and LpState (pivots, stall counter, best objective) between calls, so a
    stale one would change the pivots or the bits of the call after it."""
    order = [("sparse", 120, 12, 0, 0), ("decades3", 2, 1, 0, 0), ("sparse", 80, 16, 1, 0), ("decades3", 3, 16, 0, 0),
             ("decades3", 300, 2, 0, 0), ("all_zero_job", 60, 8, 0, 0), ("tight", 100, 8, 1, 0),
             ("decades3", 1, 1, 0, 0), ("sparse", 120, 12, 0, 0)]
    for case in order:
        _check(gpu_solver, case)
