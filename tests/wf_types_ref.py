"""TEST INFRASTRUCTURE: an independent computation of the water-filling
MaxMinFairness allocation over worker types that differ
(sw_wf_allocate_types, csrc/sw_wf_types.h).  Plain numpy / scipy (HiGHS); it
shares no code with the header, whose result it checks.

The stage loop of the reference policy
(policies/max_min_fairness_water_filling.py:303-409) on val_j = Σ_k c_jk·x_jk:

  1. one level LP per stage: maximise t with t ≤ val_j for the unfrozen jobs and
     F_j ≤ val_j for the frozen ones, under the capacity and time rows;
  2. one LP per unfrozen job i that maximises val_i with every other unfrozen
     job held at the level L and the frozen ones at theirs.  The relative gain
     (max val_i − L)/L classifies: ≤ BOTTLENECK → bottleneck, ≥ FREE → free,
     otherwise the instance is ambiguous (``allocate`` returns None);
  3. the bottlenecks freeze at L; repeat until every job is frozen.

The reference's MILP maximises the number of jointly raisable jobs; the face is
convex, so that set is the union of the per-job answers.

``centre`` is the analytic centre of the last stage's optimal face, by the
method of tests/mmf_centre_ref.py (one LP per inequality for the tight set,
Newton in its null space), for tiny instances only.
"""
import numpy as np
from scipy.linalg import null_space
from scipy.optimize import linprog

_OPTS = {"primal_feasibility_tolerance": 1e-10, "dual_feasibility_tolerance": 1e-10}
BOTTLENECK = 1e-9
FREE = 1e-6
TIGHT = 1e-7


def _rows(W, sf, c):
    """The capacity and time rows over z = [x (job-major), t]."""
    m, n = c.shape
    nv = m * n + 1
    G, h = [], []
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
    return G, h


def _value_row(c, j, kappa, beta):
    m, n = c.shape
    r = np.zeros(m * n + 1)
    r[j * n:(j + 1) * n] = -c[j]
    r[-1] = kappa
    return r, -beta


def _stage_system(W, sf, c, frozen, F):
    G, h = [], []
    for j in range(c.shape[0]):
        r, b = _value_row(c, j, 0.0 if frozen[j] else 1.0, F[j] if frozen[j] else 0.0)
        G.append(r)
        h.append(b)
    Gc, hc = _rows(W, sf, c)
    return np.array(G + Gc), np.array(h + hc)


def _bounds(W, c):
    m, n = c.shape
    return [(0.0, 0.0 if W[k] == 0 else None) for _ in range(m) for k in range(n)] + [(0.0, None)]


def _solve(obj, G, h, bounds, held, scale):
    """HiGHS on the rows as they are; where it does not end at an optimum (the rows
    `held` at a level are tight on the whole feasible set, and the level carries
    HiGHS's own 1e-10), again with those rows relaxed by 1e-10·max(1, scale), as
    `centre` relaxes them, then by 1e-9·max(1, scale)."""
    for rel in (0.0, 1e-10, 1e-9):
        hr = h.copy()
        hr[held] += rel * max(1.0, scale)
        res = linprog(obj, A_ub=G, b_ub=hr, bounds=bounds, method="highs", options=_OPTS)
        if res.status == 0:
            return res
    raise AssertionError(res.message)


def stage_level(W, sf, c, frozen, F):
    G, h = _stage_system(W, sf, c, frozen, F)
    obj = np.zeros(G.shape[1])
    obj[-1] = -1.0
    held = np.flatnonzero(frozen)
    res = _solve(obj, G, h, _bounds(W, c), held, float(F.max()))
    return float(res.x[-1])


def job_gain(W, sf, c, frozen, F, L, i):
    """(max val_i − L)/L with the other unfrozen jobs held at L."""
    m, n = c.shape
    G, h = [], []
    for j in range(m):
        if j == i:
            continue
        r, b = _value_row(c, j, 0.0, F[j] if frozen[j] else L)
        G.append(r)
        h.append(b)
    Gc, hc = _rows(W, sf, c)
    obj = np.zeros(m * n + 1)
    obj[i * n:(i + 1) * n] = -c[i]
    res = _solve(obj, np.array(G + Gc), np.array(h + hc), _bounds(W, c), np.arange(len(G)), L)
    return (-res.fun - L) / L


def allocate(workers, scale_factors, coefficients):
    """(F[m], froze[m] (1-based stage), stages, ambiguous job tests, job tests, smallest free gain); F is None
    when a job test was ambiguous."""
    W = np.asarray(workers, dtype=np.float64)
    sf = np.asarray(scale_factors, dtype=np.float64)
    c = np.asarray(coefficients, dtype=np.float64)
    m, _ = c.shape
    frozen = np.zeros(m, dtype=bool)
    F = np.zeros(m)
    froze = np.zeros(m, dtype=np.int32)
    stage = tests = amb = 0
    least = np.inf
    while not frozen.all():
        L = stage_level(W, sf, c, frozen, F)
        assert L > 0.0
        stage += 1
        new = []
        for i in np.flatnonzero(~frozen):
            gain = job_gain(W, sf, c, frozen, F, L, i)
            tests += 1
            if gain <= BOTTLENECK:
                new.append(i)
            elif gain < FREE:
                amb += 1
            else:
                least = min(least, gain)
        if amb:
            return None, None, stage, amb, tests, least
        assert new, "a stage without a bottleneck"
        frozen[new] = True
        F[new] = L
        froze[new] = stage
    return F, froze, stage, amb, tests, least


def centre(workers, scale_factors, coefficients, F, froze):
    """The analytic centre of the last stage's optimal face: the jobs that froze
    in the last stage are its unfrozen rows, at the level they froze at."""
    W = np.asarray(workers, dtype=np.float64)
    sf = np.asarray(scale_factors, dtype=np.float64)
    c = np.asarray(coefficients, dtype=np.float64)
    m, n = c.shape
    last = int(froze.max())
    frozen = froze < last
    L = float(F[froze == last][0])
    G, h = _stage_system(W, sf, c, frozen, F)
    act = [j * n + k for j in range(m) for k in range(n) if W[k] > 0] + [m * n]
    G = G[:, act]
    nv = G.shape[1]
    G = np.vstack([G, -np.eye(nv)])
    h = np.append(h, np.zeros(nv))
    face = np.zeros(nv)
    face[-1] = -1.0
    # the frozen rows and the face's bound are relaxed by 1e-10, or HiGHS may call the face empty
    rel = 1e-10 * max(1.0, L)
    hf = np.append(h, -(L - rel))
    hf[:m][frozen] += rel
    Gf = np.vstack([G, face])
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
    z = z0
    if N.shape[1] > 0:
        A = Gf[~tight] @ N
        s0 = hf[~tight] - Gf[~tight] @ z0
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
        z = z0 + N @ y
    x = np.zeros(m * n)
    x[act[:-1]] = z[:-1]
    return x.reshape(m, n)
