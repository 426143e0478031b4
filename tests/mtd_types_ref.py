"""TEST INFRASTRUCTURE: an independent computation of the MinTotalDuration
allocation over worker types that differ (sw_mtd_allocate_types,
csrc/sw_mtd_types.h), for tiny instances.  Plain numpy / scipy; it shares no
code with csrc.

  1. t*, the max-min level of Σ_k (thr_jk / steps_j)·x_jk over the live jobs,
     by HiGHS at feasibility tolerances 1e-10.
  2. The reference's search (min_total_duration.py:82-101) with
     feasible(T) = T·t* ≥ 1.
  3. The analytic centre of {value, capacity, time rows, x ≥ 0} at the found T
     as tests/mmf_centre_ref.py does it: one LP per inequality to find those
     tight on the whole set (slack ≤ 1e-7), then Newton in their null space
     until the squared decrement is < 1e-24.  Live value rows are scaled to
     right side 1 (which does not move the centre), so that the tightness
     threshold means the same on every row.
"""
import numpy as np
from scipy.linalg import null_space
from scipy.optimize import linprog

_OPTS = {"primal_feasibility_tolerance": 1e-10, "dual_feasibility_tolerance": 1e-10}
TIGHT = 1e-7


def level(workers, scale_factors, throughputs, steps):
    """t* in 1/seconds; 0.0 without a live job."""
    W = np.asarray(workers, dtype=np.float64)
    sf = np.asarray(scale_factors, dtype=np.float64)
    thr = np.asarray(throughputs, dtype=np.float64)
    st = np.asarray(steps, dtype=np.float64)
    m, n = thr.shape
    live = np.flatnonzero(st > 0.0)
    if len(live) == 0:
        return 0.0
    c = thr[live] / st[live, None]
    s = 1.0 / c.max()  # the LP on coefficients of size 1; t* scaled back
    nv = m * n + 1
    A, b = [], []
    for i, j in enumerate(live):
        r = np.zeros(nv)
        r[j * n:(j + 1) * n] = -c[i] * s
        r[-1] = 1.0
        A.append(r)
        b.append(0.0)
    for k in range(n):
        r = np.zeros(nv)
        r[k:m * n:n] = sf
        A.append(r)
        b.append(W[k])
    for j in range(m):
        r = np.zeros(nv)
        r[j * n:(j + 1) * n] = 1.0
        A.append(r)
        b.append(1.0)
    obj = np.zeros(nv)
    obj[-1] = -1.0
    res = linprog(obj, A_ub=np.array(A), b_ub=np.array(b), bounds=[(0, None)] * nv, method="highs", options=_OPTS)
    assert res.status == 0, res.message
    return float(-res.fun) / s


def search(feasible):
    """min_total_duration.py:82-101; returns (T, the probes taken)."""
    max_T, min_T, last_max_T, found, probes = 1e6, 100.0, 1e6, None, []
    while found is None:
        while 1.05 * min_T < max_T:
            T = (min_T + max_T) / 2.0
            probes.append(T)
            if feasible(T):
                found, max_T = T, T
            else:
                min_T = T
        max_T = last_max_T * 10.0
        min_T = last_max_T
        last_max_T *= 10.0
    return found, probes


def replay(t_star):
    """(T, the least relative distance of a probe from 1/t*)."""
    if t_star <= 0.0:
        T, _ = search(lambda T: True)
        return T, np.inf
    T, probes = search(lambda T: T * t_star >= 1.0)
    return T, min(abs(p * t_star - 1.0) for p in probes)


def centre(workers, scale_factors, throughputs, steps, T):
    """x[m][n]: the analytic centre of the reference's LP at T."""
    W = np.asarray(workers, dtype=np.float64)
    sf = np.asarray(scale_factors, dtype=np.float64)
    thr = np.asarray(throughputs, dtype=np.float64)
    st = np.asarray(steps, dtype=np.float64)
    m, n = thr.shape
    nv = m * n
    G, h = [], []
    for j in range(m):
        r = np.zeros(nv)
        if st[j] > 0.0:
            r[j * n:(j + 1) * n] = -thr[j] / st[j] * T
            h.append(-1.0)
        else:
            r[j * n:(j + 1) * n] = -thr[j] / max(thr[j].max(), 1e-300)
            h.append(0.0)
        G.append(r)
    for k in range(n):
        r = np.zeros(nv)
        r[k::n] = sf
        G.append(r)
        h.append(W[k])
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
    G, h = np.array(G), np.array(h)
    slack = np.zeros(len(h))
    pts = []
    for i in range(len(h)):
        res = linprog(G[i], A_ub=G, b_ub=h, bounds=[(None, None)] * nv, method="highs", options=_OPTS)
        assert res.status == 0, res.message
        slack[i] = h[i] - res.fun
        pts.append(res.x)
    tight = slack <= TIGHT
    z0 = np.mean(pts, axis=0)
    N = null_space(G[tight]) if tight.any() else np.eye(nv)
    if N.shape[1] == 0:
        return z0.reshape(m, n).copy()
    A = G[~tight] @ N
    s0 = h[~tight] - G[~tight] @ z0
    assert (s0 > 0.0).all(), s0.min()
    y = np.zeros(N.shape[1])

    def f(y):
        s = s0 - A @ y
        return np.inf if (s <= 0.0).any() else -np.log(s).sum()

    for _ in range(200):
        s = s0 - A @ y
        As = A / s[:, None]
        dy = np.linalg.lstsq(As, -np.ones(len(s)), rcond=None)[0]
        dec2 = float(np.sum((As @ dy) ** 2))
        if dec2 < 1e-24:
            break
        step, f0 = 1.0, f(y)
        while dec2 >= 1.0 / 16.0 and f(y + step * dy) > f0 - 0.25 * step * dec2 and step > 1e-12:
            step *= 0.5
        y = y + step * dy
    else:
        raise AssertionError(f"the reference's Newton iteration did not converge (decrement² {dec2})")
    return (z0 + N @ y).reshape(m, n).copy()


def allocate(workers, scale_factors, throughputs, steps):
    """(x, T, t*, margin T·t* − 1, least probe distance)."""
    t = level(workers, scale_factors, throughputs, steps)
    T, near = replay(t)
    x = centre(workers, scale_factors, throughputs, steps, T)
    return x, T, t, (T * t - 1.0 if t > 0.0 else np.inf), near
