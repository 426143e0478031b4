"""tests/mtd_ref.py — TEST INFRASTRUCTURE for the MinTotalDuration allocation.

  * ``twin_allocate`` / ``TwinEngine`` — tests/twins/mtd_twin.c, the bit-exact
    CPU twin of the HIP kernel (built by csrc/Makefile into
    shockwave-replication_amd/lib/libmtd_twin.so), loaded through ctypes.
  * ``reference_search`` — the reference's two loops as written
    (policies/min_total_duration.py:82-101) over any feasibility predicate.
  * ``exact_search`` — that search over the closed-form predicate
    (max p ≤ T and Σ sf·p ≤ G·T) in exact rational arithmetic on the values of
    the doubles (fractions.Fraction); the probes T are the reference's doubles.
  * ``lp_search`` — that search over the reference's LP (:47-60 with the base
    constraints of policy.py:57-63) on a (jobs × types) variable, as a
    scipy.optimize.linprog (HiGHS) feasibility problem.  The reference used
    ECOS through CVXPY; both are absent here.
Only tests/ (and tools/ run by hand) may import this module.
"""
import ctypes as C
import os
import subprocess
from fractions import Fraction

import numpy as np
from scipy.optimize import linprog
from scipy.sparse import csr_matrix

_HERE = os.path.dirname(os.path.abspath(__file__))
_CSRC = os.path.join(os.path.dirname(_HERE), "shockwave-replication_amd", "csrc")
_SO = os.path.join(os.path.dirname(_HERE), "shockwave-replication_amd", "lib", "libmtd_twin.so")
_LIB = None


def _lib():
    global _LIB
    if _LIB is None:
        if not os.path.exists(_SO):
            subprocess.check_call(["make", "-s", "-C", _CSRC, "../lib/libmtd_twin.so"])
        lib = C.CDLL(_SO)
        dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int32)
        lib.mtd_twin_allocate.argtypes = [C.c_int32, C.c_int32, ip, dp, dp, dp, dp, ip]
        lib.mtd_twin_allocate.restype = C.c_int
        _LIB = lib
    return _LIB


def twin_allocate(scale_factors, full_time, num_workers, probes=None):
    """(x, T, μ) from the CPU twin of the HIP kernel; probes (a list) receives
    the number of T-probes the search took."""
    sf = np.ascontiguousarray(scale_factors, dtype=np.int32)
    p = np.ascontiguousarray(full_time, dtype=np.float64)
    n = len(sf)
    assert len(p) == n
    x = np.zeros(n)
    lvl = np.zeros(2)
    scratch = np.zeros(max(n, 1))
    cnt = np.zeros(1, dtype=np.int32)
    dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int32)
    _lib().mtd_twin_allocate(n, int(num_workers), sf.ctypes.data_as(ip), p.ctypes.data_as(dp),
                             x.ctypes.data_as(dp), lvl.ctypes.data_as(dp), scratch.ctypes.data_as(dp),
                             cnt.ctypes.data_as(ip))
    if probes is not None:
        probes.append(int(cnt[0]))
    return x, float(lvl[0]), float(lvl[1])


class TwinEngine:
    """The policy mirror's / simulator's engine interface backed by the twin."""

    def __init__(self):
        self.calls = []

    def mtd_allocate(self, scale_factors, full_time, num_workers):
        r = twin_allocate(scale_factors, full_time, num_workers)
        self.calls.append((np.array(scale_factors), np.array(full_time), int(num_workers), r))
        return r


def reference_search(feasible, max_rounds=40):
    """min_total_duration.py:82-101 as written.  Returns (T, probes, min_T):
    the last feasible probe, every probe in order, and the lower end of the
    interval when the inner loop that found T ended.  max_rounds only keeps a
    wrong predicate from looping for ever."""
    max_T = 1000000.0
    min_T = 100.0
    last_max_T = max_T
    found = None
    probes = []
    rounds = 0
    while found is None:
        assert rounds < max_rounds, "no feasible T"
        rounds += 1
        while (1.05 * min_T) < max_T:
            T = (min_T + max_T) / 2.0
            probes.append(T)
            if feasible(T):
                found = T
                max_T = T
            else:
                min_T = T
        end_min = min_T
        max_T = last_max_T * 10.0
        min_T = last_max_T
        last_max_T *= 10
    return found, probes, end_min


def exact_predicate(sf, p, G):
    """feasible(T) of the closed form, exact: max p ≤ T and Σ sf·p ≤ G·T."""
    pf = [Fraction(float(v)) for v in p]
    maxp = max(pf) if pf else Fraction(0)
    S = sum((int(s) * v for s, v in zip(sf, pf)), Fraction(0))
    G = int(G)
    return lambda T: maxp <= Fraction(float(T)) and S <= G * Fraction(float(T))


def exact_search(sf, p, G):
    return reference_search(exact_predicate(sf, p, G))


def least_feasible(sf, p, G):
    """T* = max(max p, Σ sf·p / G), exact."""
    pf = [Fraction(float(v)) for v in p]
    S = sum((int(s) * v for s, v in zip(sf, pf)), Fraction(0))
    return max(max(pf), S / int(G))


def lp_feasible(tp, sf, steps, workers, T):
    """The reference's LP at T over x[j][w] ≥ 0 (row-major):
    Σ_w x_jw ≤ 1, Σ_j sf_j·x_jw ≤ workers_w, Σ_w tp_jw·x_jw ≥ steps_j / T."""
    tp = np.asarray(tp, dtype=np.float64)
    m, n = tp.shape
    var = np.arange(m * n).reshape(m, n)
    job = np.repeat(np.arange(m), n)
    typ = np.tile(np.arange(n), m)
    rows = np.concatenate([job, m + typ, m + n + job])
    cols = np.concatenate([var.ravel()] * 3)
    vals = np.concatenate([np.ones(m * n), np.repeat(np.asarray(sf, dtype=np.float64), n), -tp.ravel()])
    A = csr_matrix((vals, (rows, cols)), shape=(2 * m + n, m * n))
    b = np.concatenate([np.ones(m), np.asarray(workers, dtype=np.float64),
                        -(np.asarray(steps, dtype=np.float64) / T)])
    r = linprog(np.zeros(m * n), A_ub=A, b_ub=b, bounds=(0, None), method="highs",
                options={"primal_feasibility_tolerance": 1e-9, "dual_feasibility_tolerance": 1e-9})
    assert r.status in (0, 2), r.message
    return r.status == 0


def lp_search(tp, sf, steps, workers):
    return reference_search(lambda T: lp_feasible(tp, sf, steps, workers, T))
