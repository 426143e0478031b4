"""TEST INFRASTRUCTURE: an independent computation of the analytic centre of the
optimal face of the worker-type MaxMinFairness LP (csrc/sw_mmf_lp.h), for tiny
instances only (m·n up to about 130).  Plain numpy / scipy; it shares no code
with csrc/sw_mmf_ipm.h, whose result it checks (sw_mmf_allocate_types_centred).

  1. t* by HiGHS at feasibility tolerances 1e-10.
  2. For every inequality (rows, x ≥ 0, t ≥ 0) one HiGHS LP maximises its slack
     over {the LP's constraints, t ≥ t* − 1e-10·max(1, t*)}; a slack ≤ 1e-7
     means the inequality is tight on the whole face.
  3. Newton's method with backtracking on Σ log(slack) of the other
     inequalities, in the null space of the tight ones, from the mean of the
     LP solutions of step 2, until the squared Newton decrement is < 1e-24.

Limit: the face bound's 1e-10 is amplified by 1/coefficient, so nonzero
coefficients must not be tiny (≥ 0.2·sf in the tests; exact zeros are fine).
"""
import numpy as np
from scipy.linalg import null_space
from scipy.optimize import linprog

import mmf_ref

_OPTS = {"primal_feasibility_tolerance": 1e-10, "dual_feasibility_tolerance": 1e-10}
TIGHT = 1e-7


def _system(W, sf, c):
    """G z ≤ h over z = [x (job-major), t]: value, capacity, time rows, −x ≤ 0, −t ≤ 0."""
    m, n = c.shape
    nv = m * n + 1
    G, h = [], []
    for j in range(m):
        r = np.zeros(nv)
        r[j * n:(j + 1) * n] = -c[j]
        r[-1] = 1.0
        G.append(r)
        h.append(0.0)
    for k in range(n):
        r = np.zeros(nv)
        r[k:m * n:n] = sf
        G.append(r)
        h.append(float(W[k]))
    for j in range(m):
        r = np.zeros(nv)
        r[j * n:(j + 1) * n] = 1.0
        G.append(r)
        h.append(1.0)
    for i in range(nv):
        r = np.zeros(nv)
        r[i] = -1.0
        G.append(r)
        h.append(0.0)
    return np.array(G), np.array(h)


def face_centre(workers, scale_factors, coefficients):
    """(x[m][n], t*) — the analytic centre of the optimal face."""
    W = np.asarray(workers, dtype=np.float64)
    sf = np.asarray(scale_factors, dtype=np.float64)
    c = np.asarray(coefficients, dtype=np.float64)
    m, n = c.shape
    t_star, _ = mmf_ref.lp_level_types(W, sf, c, options=_OPTS)
    t_star = max(t_star, 0.0)
    G, h = _system(W, sf, c)
    nv = G.shape[1]
    face = np.zeros(nv)
    face[-1] = -1.0
    Gf = np.vstack([G, face])
    hf = np.append(h, -(t_star - 1e-10 * max(1.0, t_star)))
    slack = np.zeros(len(hf))
    pts = []
    for i in range(len(hf)):
        res = linprog(Gf[i], A_ub=Gf, b_ub=hf, bounds=[(None, None)] * nv, method="highs", options=_OPTS)
        assert res.status == 0, res.message
        slack[i] = hf[i] - res.fun
        pts.append(res.x)
    tight = slack <= TIGHT
    z0 = np.mean(pts, axis=0)
    N = null_space(Gf[tight]) if tight.any() else np.eye(nv)
    if N.shape[1] == 0:
        return z0[:-1].reshape(m, n).copy(), t_star
    A = Gf[~tight] @ N
    s0 = hf[~tight] - Gf[~tight] @ z0
    assert (s0 > 0.0).all(), s0.min()
    y = np.zeros(N.shape[1])

    def f(y):
        s = s0 - A @ y
        return np.inf if (s <= 0.0).any() else -np.log(s).sum()

    for _ in range(200):
        # the Newton step H·dy = −g with g = Ãᵀ·1, H = ÃᵀÃ, Ã = A / s: the least-squares
        # solution of Ã·dy = −1, and decrement² = ‖Ã·dy‖² (never the normal equations:
        # their rounding floor lies above 1e-24 where slacks are small)
        s = s0 - A @ y
        As = A / s[:, None]
        dy = np.linalg.lstsq(As, -np.ones(len(s)), rcond=None)[0]
        dec2 = float(np.sum((As @ dy) ** 2))
        if dec2 < 1e-24:
            break
        # Σ log is self-concordant: at a decrement below 1/4 the full step is
        # feasible and converges quadratically, and f can no longer resolve the
        # decrease (decrement² far below f's rounding), so backtrack only above it
        step, f0 = 1.0, f(y)
        while dec2 >= 1.0 / 16.0 and f(y + step * dy) > f0 - 0.25 * step * dec2 and step > 1e-12:
            step *= 0.5
        y = y + step * dy
    else:
        raise AssertionError(f"the reference's Newton iteration did not converge (decrement² {dec2})")
    z = z0 + N @ y
    return z[:-1].reshape(m, n).copy(), t_star
