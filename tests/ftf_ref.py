"""tests/ftf_ref.py — TEST INFRASTRUCTURE for the FinishTimeFairness allocation.

  * ``twin_allocate`` / ``TwinEngine`` — tests/twins/ftf_twin.c, the bit-exact
    CPU twin of the HIP kernel (built by csrc/Makefile into
    shockwave-replication_amd/lib/libftf_twin.so), loaded through ctypes.
  * ``certified`` — an exact rational certificate of the optimal level: the
    feasibility test of sw_ftf.h (d_j(ρ) ≥ p_j for every job and
    Σ sf_j·p_j/d_j(ρ) ≤ G) evaluated with fractions.Fraction on the exact
    values of the doubles; it must hold just above the level and fail just
    below it.
  * ``slsqp_level`` — the reference's program as written
    (policies/finish_time_fairness.py:55-140: an epigraph variable over
    (a_j + p_j/x_j)/E_j, the capacity row and the bounds) through scipy's
    SLSQP.  The reference used ECOS through CVXPY; both are absent here.
Only tests/ may import this module.
"""
import ctypes as C
import math
import os
import subprocess
from fractions import Fraction

import numpy as np
from scipy.optimize import minimize

_HERE = os.path.dirname(os.path.abspath(__file__))
_CSRC = os.path.join(os.path.dirname(_HERE), "shockwave-replication_amd", "csrc")
_SO = os.path.join(os.path.dirname(_HERE), "shockwave-replication_amd", "lib", "libftf_twin.so")
_LIB = None


def _lib():
    global _LIB
    if _LIB is None:
        if not os.path.exists(_SO):
            subprocess.check_call(["make", "-s", "-C", _CSRC, "../lib/libftf_twin.so"])
        lib = C.CDLL(_SO)
        dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int32)
        lib.ftf_twin_allocate.argtypes = [C.c_int32, C.c_int32, ip, dp, dp, dp, dp, dp, dp]
        lib.ftf_twin_allocate.restype = C.c_int
        _LIB = lib
    return _LIB


def twin_allocate(scale_factors, full_time, elapsed, isolated_time, num_workers):
    """(x, ρ*, μ) from the CPU twin of the HIP kernel."""
    sf = np.ascontiguousarray(scale_factors, dtype=np.int32)
    p = np.ascontiguousarray(full_time, dtype=np.float64)
    a = np.ascontiguousarray(elapsed, dtype=np.float64)
    e = np.ascontiguousarray(isolated_time, dtype=np.float64)
    n = len(sf)
    assert len(p) == len(a) == len(e) == n
    x = np.zeros(n)
    lvl = np.zeros(2)
    scratch = np.zeros(max(n, 1))
    dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int32)
    _lib().ftf_twin_allocate(n, int(num_workers), sf.ctypes.data_as(ip), p.ctypes.data_as(dp),
                             a.ctypes.data_as(dp), e.ctypes.data_as(dp), x.ctypes.data_as(dp),
                             lvl.ctypes.data_as(dp), scratch.ctypes.data_as(dp))
    return x, float(lvl[0]), float(lvl[1])


class TwinEngine:
    """The policy mirror's / simulator's engine interface backed by the twin."""

    def __init__(self):
        self.calls = []

    def ftf_allocate(self, scale_factors, full_time, elapsed, isolated_time, num_workers):
        r = twin_allocate(scale_factors, full_time, elapsed, isolated_time, num_workers)
        self.calls.append((np.array(scale_factors), np.array(full_time), np.array(elapsed),
                           np.array(isolated_time), int(num_workers), r))
        return r


def _feasible(sf, p, a, E, G, rho):
    terms = []
    for s, pj, aj, Ej in zip(sf, p, a, E):
        d = rho * Ej - aj
        if d < pj:
            return False
        if pj > 0:
            terms.append(s * pj / d)
    # Each exact term rounds to a double within 2^-53 relative and fsum adds
    # the doubles exactly, so the rounded sum decides unless it is within
    # 1e-12·G of G; only then is the exact sum formed (its denominators grow
    # with every term).
    approx = math.fsum(float(t) for t in terms)
    if abs(approx - G) > 1e-12 * G:
        return approx <= G
    return sum(terms, Fraction(0)) <= G


def certified(sf, p, a, E, G, rho, rel):
    """True when level ρ·(1+rel) is feasible and ρ·(1−rel) is not, in exact
    rational arithmetic on the values of the doubles."""
    sf = [int(s) for s in sf]
    p, a, E = ([Fraction(float(v)) for v in arr] for arr in (p, a, E))
    r, eps = Fraction(float(rho)), Fraction(rel)
    return _feasible(sf, p, a, E, int(G), r * (1 + eps)) and not _feasible(sf, p, a, E, int(G), r * (1 - eps))


def slsqp_level(sf, p, a, E, G):
    """min ρ s.t. (a_j + p_j/x_j)/E_j ≤ ρ, Σ sf_j x_j ≤ G, 0 ≤ x_j ≤ 1
    (variables [x, ρ]); returns (ρ, success)."""
    sf = np.asarray(sf, dtype=np.float64)
    p, a, E = (np.asarray(v, dtype=np.float64) for v in (p, a, E))
    n = len(sf)
    lo = 1e-9
    x0 = np.minimum(1.0, G / (n * sf))
    rho0 = float(np.max((a + p / x0) / E)) * 1.01
    z0 = np.concatenate([x0, [rho0]])

    def ratio_con(z):
        return z[n] - (a + p / z[:n]) / E

    def ratio_jac(z):
        J = np.zeros((n, n + 1))
        J[np.arange(n), np.arange(n)] = p / (z[:n] ** 2 * E)
        J[:, n] = 1.0
        return J

    cons = [{"type": "ineq", "fun": ratio_con, "jac": ratio_jac},
            {"type": "ineq", "fun": lambda z: G - sf @ z[:n],
             "jac": lambda z: np.concatenate([-sf, [0.0]])}]
    grad = np.concatenate([np.zeros(n), [1.0]])
    r = minimize(lambda z: z[n], z0, jac=lambda z: grad, method="SLSQP",
                 bounds=[(lo, 1.0)] * n + [(None, None)], constraints=cons,
                 options={"ftol": 1e-14, "maxiter": 2000})
    return float(r.x[n]), bool(r.success)
