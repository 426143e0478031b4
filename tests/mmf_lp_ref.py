"""A plain reference for the worker-type MaxMinFairness LP
(sw_mmf_allocate_types): the constraint residuals of an allocation computed
exactly, and the optimal level from HiGHS at tightened tolerances.

    maximise t   s.t.  t ≤ Σ_k c[j][k]·x[j][k],  Σ_j sf_j·x[j][k] ≤ W_k,
                       Σ_k x[j][k] ≤ 1,  x ≥ 0
"""
import sys
from fractions import Fraction

import numpy as np

import mmf_ref

TINY = sys.float_info.min
HIGHS_TOL = 1e-10


def residuals(W, sf, c, x, t):
    """The four constraint violations of (x, t), each the worst over its rows,
    from the inputs in rational arithmetic over the doubles (no solver, no
    tolerance, no rounding before the final conversion):
      neg    max(0, −x)
      time   Σ_k x[j][k] − 1
      cap    (Σ_j sf_j·x[j][k] − W_k) / max(W_k, 1)
      value  (t − min_j Σ_k c[j][k]·x[j][k]) / max(|t|, tiny)
    A value ≤ 0 means the constraint holds with room."""
    c = np.asarray(c, dtype=np.float64)
    x = np.asarray(x, dtype=np.float64)
    m, n = c.shape
    assert x.shape == (m, n)
    X = [[Fraction(float(v)) for v in row] for row in x]
    Cf = [[Fraction(float(v)) for v in row] for row in c]
    S = [int(v) for v in sf]
    Wk = [int(v) for v in W]
    T = Fraction(float(t))
    neg = max([Fraction(0)] + [-v for row in X for v in row])
    time = max(sum(row) - 1 for row in X)
    cap = max((sum(S[j] * X[j][k] for j in range(m)) - Wk[k]) / max(Wk[k], 1) for k in range(n))
    reach = min(sum(Cf[j][k] * X[j][k] for k in range(n)) for j in range(m))
    value = (T - reach) / max(abs(T), Fraction(TINY))
    return {"neg": float(neg), "time": float(time), "cap": float(cap), "value": float(value)}


def level(W, sf, c):
    """t* of the LP: mmf_ref.lp_level_types's model, HiGHS's primal and dual
    feasibility tolerances at 1e-10."""
    opts = {"primal_feasibility_tolerance": HIGHS_TOL, "dual_feasibility_tolerance": HIGHS_TOL}
    return mmf_ref.lp_level_types(W, sf, c, options=opts)[0]
