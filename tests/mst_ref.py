"""tests/mst_ref.py — TEST INFRASTRUCTURE for the max-sum-throughput allocation.

An instance is (sf, w, l, G): scale factors, weights (throughput / cost),
floors (or None: all zero) and workers.

  * ``twin_allocate`` / ``TwinEngine`` — tests/twins/mst_twin.c, the bit-exact
    CPU twin of the HIP kernel (built by csrc/Makefile into
    shockwave-replication_amd/lib/libmst_twin.so), loaded through ctypes.
  * ``exact_optimum`` — the LP's optimum by the greedy fractional knapsack in
    exact rational arithmetic on the values of the doubles (fractions.Fraction),
    with the reference's rule for infeasible SLO rows.
  * ``lp_optimum`` — the reference's LP (max_sum_throughput.py:66-94 with the
    base constraints of policy.py:57-63) through scipy.optimize.linprog
    (HiGHS), solved again without the floors when they are infeasible.  The
    reference used ECOS through CVXPY; both are absent here.
  * ``check_allocation`` — the conditions a returned point must meet.
Only tests/ (and tools/ run by hand) may import this module.
"""
import ctypes as C
import math
import os
import subprocess
from fractions import Fraction

import numpy as np
from scipy.optimize import linprog

_HERE = os.path.dirname(os.path.abspath(__file__))
_CSRC = os.path.join(os.path.dirname(_HERE), "shockwave-replication_amd", "csrc")
_SO = os.path.join(os.path.dirname(_HERE), "shockwave-replication_amd", "lib", "libmst_twin.so")
_LIB = None


def _lib():
    global _LIB
    if _LIB is None:
        if not os.path.exists(_SO):
            subprocess.check_call(["make", "-s", "-C", _CSRC, "../lib/libmst_twin.so"])
        lib = C.CDLL(_SO)
        dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int32)
        lib.mst_twin_allocate.argtypes = [C.c_int32, C.c_int32, ip, dp, dp, dp, dp, dp, ip]
        lib.mst_twin_allocate.restype = C.c_int
        _LIB = lib
    return _LIB


def twin_allocate(scale_factors, weights, floors, num_workers, probes=None):
    """(x, λ, m, objective, slo_dropped) from the CPU twin of the HIP kernel;
    probes (a list) receives (θ-probes, multiplier probes)."""
    sf = np.ascontiguousarray(scale_factors, dtype=np.int32)
    w = np.ascontiguousarray(weights, dtype=np.float64)
    l = None if floors is None else np.ascontiguousarray(floors, dtype=np.float64)
    n = len(sf)
    assert len(w) == n and (l is None or len(l) == n)
    x = np.zeros(n)
    lvl = np.zeros(4)
    scratch = np.zeros(max(n, 1))
    cnt = np.zeros(2, dtype=np.int32)
    dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int32)
    _lib().mst_twin_allocate(n, int(num_workers), sf.ctypes.data_as(ip), w.ctypes.data_as(dp),
                             None if l is None else l.ctypes.data_as(dp), x.ctypes.data_as(dp),
                             lvl.ctypes.data_as(dp), scratch.ctypes.data_as(dp), cnt.ctypes.data_as(ip))
    if probes is not None:
        probes.append((int(cnt[0]), int(cnt[1])))
    return x, float(lvl[0]), float(lvl[1]), float(lvl[2]), bool(lvl[3])


class TwinEngine:
    """The policy mirror's / simulator's engine interface backed by the twin."""

    def __init__(self):
        self.calls = []

    def mst_allocate(self, scale_factors, weights, floors, num_workers):
        r = twin_allocate(scale_factors, weights, floors, num_workers)
        self.calls.append((np.array(scale_factors), np.array(weights),
                           None if floors is None else np.array(floors), int(num_workers), r))
        return r


def _frac(v):
    return Fraction(float(v))


def exact_floors(sf, l, G):
    """(floors as Fractions, slo_dropped): the reference's rule, exact — the
    SLO rows are infeasible when a floor exceeds 1 or Σ sf·l > G."""
    n = len(sf)
    if l is None:
        return [Fraction(0)] * n, False
    if any(math.isinf(float(v)) or float(v) > 1.0 for v in l):
        return [Fraction(0)] * n, True
    lf = [_frac(v) if float(v) > 0.0 else Fraction(0) for v in l]
    if sum((int(s) * v for s, v in zip(sf, lf)), Fraction(0)) > int(G):
        return [Fraction(0)] * n, True
    return lf, False


def exact_optimum(sf, w, l, G):
    """(objective, slo_dropped): every job at its floor, then the remaining
    capacity to the jobs in order of exact density w/sf until it runs out."""
    lf, dropped = exact_floors(sf, l, G)
    wf = [_frac(v) for v in w]
    rest = int(G) - sum((int(s) * v for s, v in zip(sf, lf)), Fraction(0))
    obj = sum((a * b for a, b in zip(wf, lf)), Fraction(0))
    for j in sorted(range(len(sf)), key=lambda j: wf[j] / int(sf[j]), reverse=True):
        if rest <= 0 or wf[j] == 0:
            break
        up = min(1 - lf[j], rest / int(sf[j]))
        obj += wf[j] * up
        rest -= int(sf[j]) * up
    return obj, dropped


def exact_objective(w, x):
    return sum((_frac(a) * _frac(b) for a, b in zip(w, x)), Fraction(0))


def exact_used(sf, x):
    return sum((int(s) * _frac(v) for s, v in zip(sf, x)), Fraction(0))


def lp_optimum(sf, w, l, G):
    """(objective, slo_dropped) of the reference LP through HiGHS."""
    n = len(sf)
    c = -np.asarray(w, dtype=np.float64)
    A = np.asarray(sf, dtype=np.float64).reshape(1, n)
    opts = {"primal_feasibility_tolerance": 1e-9, "dual_feasibility_tolerance": 1e-9}
    lo = np.zeros(n) if l is None else np.where(np.asarray(l, dtype=np.float64) > 0, l, 0.0)
    dropped = False
    if np.any(lo > 1.0):  # linprog refuses lower > upper: the row set is infeasible
        dropped = True
    else:
        r = linprog(c, A_ub=A, b_ub=[float(G)], bounds=list(zip(lo, np.ones(n))), method="highs", options=opts)
        assert r.status in (0, 2), r.message
        dropped = r.status == 2
    if dropped:  # max_sum_throughput.py:91-94
        r = linprog(c, A_ub=A, b_ub=[float(G)], bounds=(0, 1), method="highs", options=opts)
        assert r.status == 0, r.message
    return -float(r.fun), dropped


EPS = 2.0 ** -53


def check_allocation(inst, x, lam, m, objective, dropped, cap_excess):
    """The returned point against the LP: the floors' rule, the bounds,
    capacity in exact arithmetic within cap_excess·G, the knapsack structure
    (1 above λ, the floor below it), and on the tie class the stationarity of
    the analytic centre, h_j(x_j)/sf_j = m for every class job strictly inside
    its interval, with the multiplier's own condition (capacity tight for
    λ > 0, μ·slack = 1 for λ = 0)."""
    sf, w, l, G = inst
    sf = np.asarray(sf)
    w = np.asarray(w, dtype=np.float64)
    x = np.asarray(x, dtype=np.float64)
    lf, want_dropped = exact_floors(sf, l, G)
    assert dropped == want_dropped
    lo = np.array([float(v) for v in lf])
    assert np.all(x >= lo) and np.all(x <= 1.0)
    used = exact_used(sf, x)
    assert used <= int(G) * (1 + Fraction(cap_excess)), float(used - int(G))
    d = np.where(w > 0, w / sf, 0.0)
    assert lam >= 0.0 and (lam == 0.0 or np.any(d == lam)), lam
    assert np.all(x[d > lam] == 1.0)
    assert np.all(x[d < lam] == lo[d < lam])
    # λ is the least threshold at which the jobs above it fit beside the others' floors
    fits = lambda t: sum((int(s) * (1 if dj > t else v) for s, dj, v in zip(sf, d, lf)), Fraction(0)) <= int(G)
    assert fits(lam)
    if lam > 0.0:
        assert not fits(np.nextafter(lam, 0.0))
    cls = d == lam
    # the sum with the class at its floors, exact: at G, or with an empty class, there is nothing to share
    at_floors = sum((int(s) * (1 if dj > lam else v) for s, dj, v in zip(sf, d, lf)), Fraction(0))
    if not np.any(cls) or at_floors >= int(G):
        assert m == 0.0
        assert np.all(x[cls] == lo[cls])
        return
    slack = float(int(G) - used)
    if lam > 0.0:
        assert abs(slack) <= 1e-9 * G, slack
    else:
        assert m > 0.0 and abs(m * slack - 1.0) < 1e-9, (m, slack)
    assert np.all(x[cls & (lo < 1.0)] > lo[cls & (lo < 1.0)])
    inside = cls & (x < 1.0)  # x_j = 1: l_j = 1, or the root lies above the last double below 1
    xi, si, li = x[inside], sf[inside].astype(np.float64), lo[inside]
    has = li > 0
    den = np.where(has, xi - li, 1.0)
    h = 1 / xi - 1 / (1 - xi) + np.where(has, 1 / den, 0.0)
    scale = 1 / xi + 1 / (1 - xi) + np.where(has, 1 / den, 0.0)
    curv = 1 / xi ** 2 + 1 / (1 - xi) ** 2 + np.where(has, 1 / den ** 2, 0.0)
    # x_j is resolved to an ulp or to 2^-64 (the 64 halvings of [l, 1]); h is evaluated to a few ulps
    dx = np.maximum(np.spacing(xi), 2.0 ** -64)
    assert np.all(np.abs(h - si * m) <= 4 * dx * curv + 16 * EPS * (scale + np.abs(si * m))), \
        (h / si, m)
