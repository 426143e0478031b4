"""TEST INFRASTRUCTURE: an independent computation of the FinishTimeFairness
allocation over worker types that differ (sw_ftf_allocate_types,
csrc/sw_ftf_types.h), for tiny instances.  Plain numpy / scipy; it shares no
code with csrc.

  1. The program at a level ρ is feasible exactly when HiGHS's max-min level of
     the rows Σ_k thr_jk·(ρ·E_j − a_j)/s_j·x_jk over the live jobs (s_j > 0) is
     ≥ 1 (mtd_types_ref.level on throughputs scaled by ρ·E_j − a_j).
  2. ρ* = ρ_box = max_j (a_j + p_j)/E_j if that level is feasible (within
     HiGHS's own 1e-9); otherwise a bracket [infeasible, feasible] from doubling
     is narrowed to 1e-13 relative by scipy's brentq, which keeps the bracket
     at every step and bisects whenever its interpolation does not halve it:
     the end of a plain bisection in a fifth of the HiGHS solves.
  3. The analytic centre of the program's feasible set at that ρ: mmf_centre_ref.face_centre on the rows at that ρ (the
     optimal face of the level LP, t* = 1, is that set), or, with dead jobs
     (whose rows bound nothing and have right side 0), mtd_types_ref.centre on
     the same rows, which is the same method with such rows.
"""
import numpy as np
from scipy.optimize import brentq

import mmf_centre_ref
import mtd_types_ref

BOX_SLACK = 1e-9
BRACKET = 1e-13


def _arrays(workers, scale_factors, throughputs, steps, elapsed, expected):
    return (np.asarray(workers, dtype=np.float64), np.asarray(scale_factors, dtype=np.float64),
            np.asarray(throughputs, dtype=np.float64), np.asarray(steps, dtype=np.float64),
            np.asarray(elapsed, dtype=np.float64), np.asarray(expected, dtype=np.float64))


def rho_box(workers, throughputs, steps, elapsed, expected):
    W, _, thr, st, a, E = _arrays(workers, [], throughputs, steps, elapsed, expected)
    if len(st) == 0:
        return 0.0
    best = np.where(W[None, :] > 0, thr, 0.0).max(axis=1) if (W > 0).any() else np.zeros(len(st))
    p = np.where(st > 0.0, st / np.where(best > 0.0, best, 1.0), 0.0)
    return float(((a + p) / E).max())


def scaled(throughputs, steps, elapsed, expected, rho):
    """thr_jk·d_j(ρ) for the live jobs, thr_jk for the dead ones: with the
    steps, the rows of the program at ρ."""
    thr = np.asarray(throughputs, dtype=np.float64)
    d = rho * np.asarray(expected, dtype=np.float64) - np.asarray(elapsed, dtype=np.float64)
    return thr * np.where(np.asarray(steps) > 0.0, np.maximum(d, 0.0), 1.0)[:, None]


def level_at(workers, scale_factors, throughputs, steps, elapsed, expected, rho):
    """HiGHS's t*(ρ); inf without a live job."""
    if not (np.asarray(steps) > 0.0).any():
        return np.inf
    return mtd_types_ref.level(workers, scale_factors, scaled(throughputs, steps, elapsed, expected, rho), steps)


def solve_rho(workers, scale_factors, throughputs, steps, elapsed, expected):
    """(ρ*, whether it is ρ_box, HiGHS solves)."""
    args = (workers, scale_factors, throughputs, steps, elapsed, expected)
    box = rho_box(workers, throughputs, steps, elapsed, expected)
    if not (np.asarray(steps) > 0.0).any():
        return box, True, 0
    f = lambda r: level_at(*args, r) - 1.0
    flo = f(box)
    solves = 1
    if flo >= -BOX_SLACK:
        return box, True, solves
    lo, hi = box, 2.0 * box
    fhi = f(hi)
    solves += 1
    while fhi < 0.0:
        lo, flo = hi, fhi
        hi = 2.0 * hi
        fhi = f(hi)
        solves += 1
    count = [solves]

    def g(r):
        count[0] += 1
        return f(r)

    root = brentq(g, lo, hi, xtol=BRACKET * lo, rtol=BRACKET, maxiter=200)
    return float(root), False, count[0]


def centre(workers, scale_factors, throughputs, steps, elapsed, expected, rho):
    st = np.asarray(steps, dtype=np.float64)
    thr_d = scaled(throughputs, steps, elapsed, expected, rho)
    if (st > 0.0).all():
        x, _ = mmf_centre_ref.face_centre(workers, scale_factors, thr_d / st[:, None])
        return x
    return mtd_types_ref.centre(workers, scale_factors, thr_d, st, 1.0)


def allocate(workers, scale_factors, throughputs, steps, elapsed, expected):
    """(x, ρ*, whether ρ* = ρ_box)."""
    rho, box, _ = solve_rho(workers, scale_factors, throughputs, steps, elapsed, expected)
    return centre(workers, scale_factors, throughputs, steps, elapsed, expected, rho), rho, box
