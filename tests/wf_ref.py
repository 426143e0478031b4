"""tests/wf_ref.py — TEST INFRASTRUCTURE for the water-filling MaxMinFairness
allocation.

  * ``twin_allocate`` / ``twin_allocator`` / ``TwinEngine`` — tests/twins/
    wf_twin.c, the bit-exact CPU twin of the HIP kernel (built by csrc/Makefile
    into shockwave-replication_amd/lib/libwf_twin.so), loaded through ctypes.
  * ``cap_le`` / ``certified`` — an exact rational certificate of the level:
    cap(L) = Σ sf_j·min(1, L/c_j) evaluated with fractions.Fraction on the
    exact values of the doubles; it must be at most G just below the level
    and above G just above it.
  * ``closed_form_level`` — the sort-based closed form in Fractions: saturate
    the jobs in ascending c_j, then L = (G − Σ_sat sf)/Σ_unsat sf/c.
  * ``stage_loop`` — the reference's stage loop
    (policies/max_min_fairness_water_filling.py:303-409) restated for one
    worker type over scipy's HiGHS: the stage LP (:79-189) through linprog, the
    bottleneck MILP (:191-301, slack 1.0001, epsilon 1e-5) through milp.  The
    reference used ECOS and GLPK through CVXPY; all three are absent here.
Only tests/ may import this module.
"""
import ctypes as C
import math
import os
import subprocess
from fractions import Fraction

import numpy as np
from scipy.optimize import Bounds, LinearConstraint, linprog, milp

_HERE = os.path.dirname(os.path.abspath(__file__))
_CSRC = os.path.join(os.path.dirname(_HERE), "shockwave-replication_amd", "csrc")
_SO = os.path.join(os.path.dirname(_HERE), "shockwave-replication_amd", "lib", "libwf_twin.so")
_LIB = None


def _lib():
    global _LIB
    if _LIB is None:
        if not os.path.exists(_SO):
            subprocess.check_call(["make", "-s", "-C", _CSRC, "../lib/libwf_twin.so"])
        lib = C.CDLL(_SO)
        dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int32)
        lib.wf_twin_allocate.argtypes = [C.c_int32, C.c_int32, ip, dp, dp, dp, dp]
        lib.wf_twin_allocate.restype = C.c_int
        _LIB = lib
    return _LIB


def twin_allocate(scale_factors, coefficients, num_workers):
    """(x, L*, Σ sf_j·x_j) from the CPU twin of the HIP kernel."""
    sf = np.ascontiguousarray(scale_factors, dtype=np.int32)
    c = np.ascontiguousarray(coefficients, dtype=np.float64)
    n = len(sf)
    assert len(c) == n
    x = np.zeros(n)
    lvl = np.zeros(2)
    scratch = np.zeros(max(n, 1))
    dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int32)
    _lib().wf_twin_allocate(n, int(num_workers), sf.ctypes.data_as(ip), c.ctypes.data_as(dp),
                            x.ctypes.data_as(dp), lvl.ctypes.data_as(dp), scratch.ctypes.data_as(dp))
    return x, float(lvl[0]), float(lvl[1])


def twin_allocator(scale_factors, coefficients, num_workers):
    """The simulator's wf_allocator interface backed by the twin."""
    return twin_allocate(scale_factors, coefficients, num_workers)[0]


class TwinEngine:
    """The policy mirror's engine interface backed by the twin."""

    def __init__(self):
        self.calls = []

    def wf_allocate(self, scale_factors, coefficients, num_workers):
        r = twin_allocate(scale_factors, coefficients, num_workers)
        self.calls.append((np.array(scale_factors), np.array(coefficients), int(num_workers), r))
        return r


def _exact(sf, c):
    return [int(s) for s in sf], [Fraction(float(v)) for v in c]


def cap_le(sf, c, G, L):
    """cap(L) ≤ G in exact arithmetic (sf ints, c and L Fractions)."""
    terms = [s if L >= cj else s * L / cj for s, cj in zip(sf, c)]
    # Each exact term rounds to a double within 2^-53 relative and fsum adds
    # the doubles exactly, so the rounded sum decides unless it is within
    # 1e-12·G of G; only then is the exact sum formed.
    approx = math.fsum(float(t) for t in terms)
    if abs(approx - G) > 1e-12 * G:
        return approx <= G
    return sum(terms, Fraction(0)) <= G


def certified(sf, c, G, level, rel):
    """True when cap(L·(1−rel)) ≤ G < cap(L·(1+rel)) in exact rational
    arithmetic on the values of the doubles (Σ sf > G is the caller's)."""
    sf, c = _exact(sf, c)
    L, eps = Fraction(float(level)), Fraction(rel)
    return cap_le(sf, c, int(G), L * (1 - eps)) and not cap_le(sf, c, int(G), L * (1 + eps))


def closed_form_level(sf, c, G):
    """The exact level as a Fraction: with the jobs in ascending c_j, the first
    k are saturated when the level (G − Σ_{<k} sf)/Σ_{≥k} sf/c they leave to the
    others is at least c_k; the level is the first one below the next c.
    max_j c_j when Σ sf ≤ G."""
    sf, c = _exact(sf, c)
    G = int(G)
    if sum(sf) <= G:
        return max(c)
    groups = {}
    for s, cj in zip(sf, c):  # jobs that tie in c_j rise and saturate together
        groups[cj] = groups.get(cj, 0) + s
    keys = sorted(groups)
    inv = sum((Fraction(groups[k]) / k for k in keys), Fraction(0))  # Σ_unsat sf/c
    sat = 0
    for k in keys:
        L = (G - sat) / inv
        if L < k:
            return L
        sat += groups[k]
        inv -= Fraction(groups[k]) / k
    raise AssertionError("Σ sf > G: some job stays below 1")


# ---- the reference's stage loop over HiGHS ----
def _stage_lp(sf, mult, so_far, lower, frozen, G, M):
    """_get_allocation (:79-189): maximise min over the unfrozen jobs of
    (x_i − so_far_i)·mult_i (the frozen ones contribute the constant M) under
    the base constraints (policy.py:57-63) and x ≥ lower.  Variables [x, t]."""
    m = len(sf)
    rows, ub = [np.concatenate([sf, [0.0]])], [float(G)]
    for i in range(m):
        r = np.zeros(m + 1)
        r[i] = -1.0  # x_i ≥ lower_i, a constraint row as in the reference (:180-183)
        rows.append(r)
        ub.append(-lower[i])
        if not frozen[i]:
            r = np.zeros(m + 1)
            r[i], r[m] = -mult[i], 1.0  # t ≤ (x_i − so_far_i)·mult_i
            rows.append(r)
            ub.append(-so_far[i] * mult[i])
    cost = np.zeros(m + 1)
    cost[m] = -1.0
    res = linprog(cost, A_ub=np.array(rows), b_ub=np.array(ub),
                  bounds=[(0.0, 1.0)] * m + [(None, M)], method="highs")
    if res.status != 0:
        return None, None
    return res.x[:m], float(res.x[m])


def _bottleneck_milp(sf, so_far, lower, masked, G, M, slack=1.0001, epsilon=1e-5):
    """_get_bottleneck_jobs (:191-301): maximise Σ z, z_i = 1 only where x_i can
    exceed so_far_i·slack.  Variables [x, z].  Once capacity is full the
    program is infeasible for every job below 0.1 (z_i = 0 asks for
    x_i ≤ so_far_i·slack − ε < so_far_i, z_i = 1 for capacity that is gone); the
    reference raises on a status that is not optimal (:296-299), catches it and
    takes z = 0, which freezes every job (:385-386).  An infeasible status is
    therefore an answer here, not a failure; any other status but optimal is."""
    m = len(sf)
    I, Z = np.eye(m), np.zeros((m, m))
    A = np.vstack([np.concatenate([sf, np.zeros(m)])[None, :],
                   np.hstack([I, -M * I]),    # M·z ≥ x − so_far·slack + ε
                   np.hstack([-I, M * I]),    # M·(1 − z) ≥ so_far·slack − x
                   np.hstack([-I, Z])])       # x ≥ lower, a constraint row (:287-290)
    ub = np.concatenate([[float(G)], so_far * slack - epsilon, M - so_far * slack, -lower])
    cost = np.concatenate([np.zeros(m), -np.ones(m)])
    hi = np.concatenate([np.ones(m), np.where(masked, 0.0, 1.0)])  # mask·z == 0
    res = milp(cost, constraints=LinearConstraint(A, -np.inf, ub),
               integrality=np.concatenate([np.zeros(m), np.ones(m)]),
               bounds=Bounds(np.zeros(2 * m), hi))
    if res.status == 2:
        return np.zeros(m, dtype=bool)
    if res.status != 0:
        return None
    return np.round(res.x[m:]).astype(bool)


def stage_loop(scale_factors, priority_weights, num_workers):
    """_run_get_allocation_iterations (:303-409) for one worker type with unit
    throughputs and no entities; returns (x, stages, ok).  ok is False when
    scipy reports a failure in any stage (the reference swallows solver
    exceptions, :364-366, :385-386; here the instance is reported instead)."""
    sf = np.asarray(scale_factors, dtype=np.float64)
    m = len(sf)
    inv_w = np.array([1.0 / w if w > 0 else 0.0 for w in priority_weights])  # :336-345
    M = float(np.max(sf))  # :507-512 with unit throughputs
    final = {}
    so_far = np.zeros(m)
    x, stages = None, 0
    done = False
    while not done:
        frozen = np.array([i in final for i in range(m)])
        mult = np.where(frozen, 0.0, inv_w * sf)  # :143-155
        mask = np.where(frozen, 0.0, 1.0 / np.where(frozen, 1.0, inv_w * sf))
        lower = np.array([final[i] if i in final else so_far[i] for i in range(m)])
        nx, c = _stage_lp(sf, mult, so_far, lower, frozen, num_workers, M)
        if nx is None:
            return x, stages, False
        x = nx
        so_far = so_far + mask * c  # :363
        lower = np.array([final[i] if i in final else so_far[i] for i in range(m)])
        z = _bottleneck_milp(sf, so_far, lower, frozen, num_workers, M)
        if z is None:
            return x, stages, False
        before = len(final)
        for i in range(m):
            if i not in final and not z[i]:
                final[i] = so_far[i]  # :388-398
        stages += 1
        if len(final) == before or len(final) == m:
            done = True
    return x, stages, True
