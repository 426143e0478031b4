"""tests/p2x_ref.py — TEST INFRASTRUCTURE for the P2 exchange step (DESIGN.md
§3.6; csrc/sw_p2x.h, oracle/p2x_twin.c).

  * ``twin_run`` / ``twin_find_cycle`` / ``twin_edges`` — the sequential
    specification's entry points (oracle/p2x_twin.c) through ctypes.
  * ``probe_run`` / ``probe_find_cycle`` / ``probe_edges`` — the device code
    (csrc/sw_p2x_dev.h) through tests/native/p2x_probe.hip, built by
    csrc/Makefile into shockwave-replication_amd/lib/libp2x_probe.so.
  * ``edges`` / ``cancel`` / ``ref_run`` / ``round_graph`` /
    ``negative_cycle_exists`` / ``cycle_cost`` / ``objective`` /
    ``transport_optimum`` — a plain restatement of the step's
    definitions: Python sets, sorting and exact rationals.  No bitsets and
    nothing from sw_p2x.h; the one rule of the specification it restates is
    the rank order inside a class (c without its 3 lowest mantissa bits,
    descending; then job ascending).
A placement is (T, G, job, w, c, m): per active job its id (ascending), width,
c = p/n and round mask (a Python int, bit t = round t).
Only tests/ may import this module.
"""
import ctypes as C
import os
import struct
import subprocess
from fractions import Fraction
from math import gcd

import numpy as np
import scipy.sparse as sp
from scipy.optimize import Bounds, LinearConstraint, milp

NONE = 1.0e300      # "no edge"
EPS = 2e-4          # δ = ε·P2₀/T·max(1, A/128)
ASCALE = 128
QMAX = 4            # jobs one edge moves
MAX_CANCEL = 256
TMAX = 64
AMAX = 4096
KMAX = 8

_HERE = os.path.dirname(os.path.abspath(__file__))
_ORACLE = os.path.join(os.path.dirname(_HERE), "oracle")
_SO = os.environ.get("SW_TWIN_PATH") or os.path.join(_ORACLE, "_build", "libplan_twin.so")
_LIB = None


def _lib():
    global _LIB
    if _LIB is None:
        if not os.path.exists(_SO):
            subprocess.check_call(["make", "-s", "-C", _ORACLE])
        lib = C.CDLL(_SO)
        dp, ip, up, bp = C.POINTER(C.c_double), C.POINTER(C.c_int32), C.POINTER(C.c_uint64), C.POINTER(C.c_int8)
        lib.twin_p2x_run.argtypes = [C.c_int32, C.c_int32, C.c_int32, ip, ip, dp, up]
        lib.twin_p2x_run.restype = C.c_int32
        lib.twin_p2x_find_cycle.argtypes = [C.c_int32, C.c_int32, dp, ip, dp, C.c_int32, ip]
        lib.twin_p2x_find_cycle.restype = C.c_int32
        lib.twin_p2x_edges.argtypes = [C.c_int32, C.c_int32, C.c_int32, ip, ip, dp, up, C.c_int32, dp, bp]
        lib.twin_p2x_edges.restype = C.c_double
        _LIB = lib
    return _LIB


def _p(a, t):
    return a.ctypes.data_as(C.POINTER(t))


def as_arrays(job, w, c, m):
    """The placement's per-job arrays as the C layouts (fresh copies)."""
    return (np.array(job, dtype=np.int32), np.array(w, dtype=np.int32), np.array(c, dtype=np.float64),
            np.array([int(x) for x in m], dtype=np.uint64))


def twin_run(T, G, job, w, c, m):
    """(final masks as Python ints, ncancel) of twin_p2x_run; the inputs are not modified."""
    j, wa, ca, ma = as_arrays(job, w, c, m)
    keep = (j.copy(), wa.copy(), ca.copy())
    nc = _lib().twin_p2x_run(len(j), T, G, _p(j, C.c_int32), _p(wa, C.c_int32), _p(ca, C.c_double),
                             _p(ma, C.c_uint64))
    assert keep[0].tobytes() == j.tobytes() and keep[1].tobytes() == wa.tobytes() \
        and keep[2].tobytes() == ca.tobytes(), "twin_p2x_run changed an input other than m"
    return [int(x) for x in ma], int(nc)


def twin_find_cycle(T, F, W, room, dw=None):
    """(len, cyc[:len], distances[T + 1]) of the twin's find_cycle on W[T][T]
    (δ included, NONE = no edge); warm from dw when given."""
    Wa = np.ascontiguousarray(W, dtype=np.float64).reshape(T * T).copy()
    ra = np.ascontiguousarray(room, dtype=np.int32).copy()
    d = np.zeros(T + 1) if dw is None else np.array(dw, dtype=np.float64)
    cyc = np.full(T + 1, -1, dtype=np.int32)
    n = _lib().twin_p2x_find_cycle(T, F, _p(Wa, C.c_double), _p(ra, C.c_int32), _p(d, C.c_double),
                                   int(dw is not None), _p(cyc, C.c_int32))
    assert n >= 0
    return int(n), [int(x) for x in cyc[:n]], d


def twin_edges(T, G, job, w, c, m, F):
    """(W[T][T], Wk[T][T], δ) of the twin's set-up and one build_w for load size F."""
    j, wa, ca, ma = as_arrays(job, w, c, m)
    W = np.full(T * T, np.nan)
    Wk = np.full(T * T, -9, dtype=np.int8)
    delta = _lib().twin_p2x_edges(len(j), T, G, _p(j, C.c_int32), _p(wa, C.c_int32), _p(ca, C.c_double),
                                  _p(ma, C.c_uint64), F, _p(W, C.c_double), _p(Wk, C.c_int8))
    return W.reshape(T, T), Wk.reshape(T, T), float(delta)


# ---- the device code through the probe library ------------------------------

_PROBE_SO = os.path.join(os.path.dirname(_HERE), "shockwave-replication_amd", "lib", "libp2x_probe.so")
_PROBE = None


def _probe():
    """libp2x_probe.so; absent means the build is broken (no fall-back)."""
    global _PROBE
    if _PROBE is None:
        lib = C.CDLL(_PROBE_SO)
        dp, ip, up, bp, lp = (C.POINTER(C.c_double), C.POINTER(C.c_int32), C.POINTER(C.c_uint64),
                              C.POINTER(C.c_int8), C.POINTER(C.c_int64))
        lib.p2x_probe_run.argtypes = [C.c_int32, lp, ip, ip, ip, ip, dp, up, ip, C.c_int32]
        lib.p2x_probe_find_cycle.argtypes = [C.c_int32, ip, ip, dp, ip, dp, ip, ip, ip]
        lib.p2x_probe_edges.argtypes = [C.c_int32, lp, ip, ip, ip, ip, ip, dp, up, dp, bp, dp, C.c_int32]
        for f in (lib.p2x_probe_run, lib.p2x_probe_find_cycle, lib.p2x_probe_edges):
            f.restype = C.c_int
        _PROBE = lib
    return _PROBE


def _batch(placements):
    off = np.zeros(len(placements) + 1, dtype=np.int64)
    off[1:] = np.cumsum([len(P["w"]) for P in placements])
    T = np.array([P["T"] for P in placements], dtype=np.int32)
    G = np.array([P["G"] for P in placements], dtype=np.int32)
    cat = lambda k, t: np.array([x for P in placements for x in P[k]], dtype=t)  # noqa: E731
    m = np.array([int(x) for P in placements for x in P["m"]], dtype=np.uint64)
    return off, T, G, cat("w", np.int32), cat("job", np.int32), cat("c", np.float64), m


def probe_run(placements, emax):
    """[(final masks, ncancel)] of sw_p2x_block<SW_WAVES, emax> on the placements, one launch."""
    off, T, G, w, job, c, m = _batch(placements)
    nc = np.full(len(placements), -7, dtype=np.int32)
    rc = _probe().p2x_probe_run(len(placements), _p(off, C.c_int64), _p(T, C.c_int32), _p(G, C.c_int32),
                                _p(w, C.c_int32), _p(job, C.c_int32), _p(c, C.c_double), _p(m, C.c_uint64),
                                _p(nc, C.c_int32), emax)
    assert rc == 0, f"p2x_probe_run: HIP error {rc}"
    return [([int(x) for x in m[off[i]:off[i + 1]]], int(nc[i])) for i in range(len(placements))]


def probe_find_cycle(graphs, dws=None):
    """[(len, cyc[:len], distances[T + 1])] of the device's p2x_find_cycle on
    the graphs (T, F, W, room), one launch; warm from dws[i] where given."""
    n = len(graphs)
    T = np.array([g[0] for g in graphs], dtype=np.int32)
    F = np.array([g[1] for g in graphs], dtype=np.int32)
    W = np.concatenate([np.ascontiguousarray(g[2], dtype=np.float64).reshape(-1) for g in graphs])
    room = np.zeros((n, TMAX), dtype=np.int32)
    dw = np.zeros((n, TMAX + 1))
    warm = np.zeros(n, dtype=np.int32)
    for i, g in enumerate(graphs):
        room[i, :g[0]] = g[3]
        if dws is not None and dws[i] is not None:
            dw[i, :g[0] + 1] = dws[i]
            warm[i] = 1
    ln = np.full(n, -7, dtype=np.int32)
    cyc = np.full((n, TMAX + 1), -7, dtype=np.int32)
    rc = _probe().p2x_probe_find_cycle(n, _p(T, C.c_int32), _p(F, C.c_int32), _p(W, C.c_double),
                                       _p(room, C.c_int32), _p(dw, C.c_double), _p(warm, C.c_int32),
                                       _p(ln, C.c_int32), _p(cyc, C.c_int32))
    assert rc == 0, f"p2x_probe_find_cycle: HIP error {rc}"
    return [(int(ln[i]), [int(x) for x in cyc[i, :max(0, ln[i])]], dw[i, :T[i] + 1].copy()) for i in range(n)]


def probe_edges(placements, Fs, emax):
    """[(W[T][T], Wk[T][T], δ)] of the device's set-up and one full edge build
    for load size Fs[i], one launch (δ = −1 and W = NaN where the step is skipped)."""
    off, T, G, w, job, c, m = _batch(placements)
    F = np.array(Fs, dtype=np.int32)
    woff = np.concatenate([[0], np.cumsum(T.astype(np.int64) ** 2)])
    W = np.full(int(woff[-1]) or 1, np.nan)
    Wk = np.full(int(woff[-1]) or 1, -9, dtype=np.int8)
    delta = np.full(len(placements), np.nan)
    rc = _probe().p2x_probe_edges(len(placements), _p(off, C.c_int64), _p(T, C.c_int32), _p(G, C.c_int32),
                                  _p(F, C.c_int32), _p(w, C.c_int32), _p(job, C.c_int32), _p(c, C.c_double),
                                  _p(m, C.c_uint64), _p(W, C.c_double), _p(Wk, C.c_int8), _p(delta, C.c_double),
                                  emax)
    assert rc == 0, f"p2x_probe_edges: HIP error {rc}"
    return [(W[woff[i]:woff[i + 1]].reshape(T[i], T[i]), Wk[woff[i]:woff[i + 1]].reshape(T[i], T[i]),
             float(delta[i])) for i in range(len(placements))]


# ---- the plain reference --------------------------------------------------

def ckey(c):
    """c without its 3 lowest mantissa bits (the documented rank key)."""
    return struct.unpack("<Q", struct.pack("<d", float(c)))[0] >> 3


def objective(c, m):
    """The exact P2 objective Σ_j c_j·Σ_{t in m_j} t."""
    tot = Fraction(0)
    for cj, mj in zip(c, m):
        mj = int(mj)
        s = sum(t for t in range(mj.bit_length()) if (mj >> t) & 1)
        tot += Fraction(float(cj)) * s
    return tot


def loads(T, w, m):
    return [sum(int(wj) for wj, mj in zip(w, m) if (int(mj) >> t) & 1) for t in range(T)]


def delta_of(T, c, m):
    """δ = ε·P2₀/T·max(1, A/128), from the exact objective (the step's own is a float sum)."""
    A = len(c)
    return EPS * float(objective(c, m)) / T * (A / ASCALE if A > ASCALE else 1.0)


def edges(T, G, w, c, m, F, delta, job=None):
    """(W, Wk, room): for each t ≠ u the cheapest class's cost of moving load F
    from round t to round u, δ included (NONE where no class can), that class's
    index among the ascending widths (−1), and every round's free capacity."""
    A = len(w)
    job = list(range(A)) if job is None else [int(x) for x in job]
    classes = sorted(set(int(x) for x in w))
    # the rank order inside a class, once: (key descending, job ascending)
    order = sorted(range(A), key=lambda i: (-ckey(c[i]), job[i]))
    members = [[set() for _ in range(T)] for _ in classes]
    pos = {}
    for rank, i in enumerate(order):
        pos[i] = rank
        k = classes.index(int(w[i]))
        for t in range(T):
            if (int(m[i]) >> t) & 1:
                members[k][t].add(i)
    W = np.full((T, T), NONE)
    Wk = np.full((T, T), -1, dtype=np.int8)
    for t in range(T):
        for u in range(T):
            if t == u:
                continue
            best, bk = NONE, -1
            for k, wk in enumerate(classes):
                if F % wk or F // wk > QMAX:
                    continue
                q = F // wk
                cand = sorted(members[k][t] - members[k][u], key=pos.__getitem__)
                if len(cand) < q:
                    continue
                # the q largest c first to last when the jobs move earlier, else the q smallest, smallest first
                sel = cand[:q] if u < t else cand[::-1][:q]
                s = 0.0
                for i in sel:
                    s = s + float(c[i])
                cost = s * float(u - t)
                if cost < best:
                    best, bk = cost, k
            if bk >= 0:
                W[t, u] = best + delta
                Wk[t, u] = bk
    room = [G - x for x in loads(T, w, m)]
    return W, Wk, room


MAX_MOVES = 1024    # job moves one cycle may make


def cancel(T, w, c, m, F, Wk, cyc, job=None):
    """The masks after cancelling the cycle cyc (predecessor order: the edge
    cyc[i + 1] → cyc[i]) for load size F: every real edge t → u moves the
    q = F/w_k jobs of its class Wk[t][u] that are in t and not in u with the
    largest c (u < t) or the smallest (u > t), ties by the rank order; all
    edges select from the masks before the cycle.  None when the cycle would
    move more than MAX_MOVES jobs."""
    A = len(w)
    job = list(range(A)) if job is None else [int(x) for x in job]
    classes = sorted(set(int(x) for x in w))
    rank = lambda i: (-ckey(c[i]), job[i])  # noqa: E731
    picks = []
    for i, u in enumerate(cyc):
        t = cyc[(i + 1) % len(cyc)]
        if u == T or t == T:
            continue
        wk = classes[int(Wk[t][u])]
        q = F // wk
        cand = sorted((j for j in range(A) if int(w[j]) == wk and (int(m[j]) >> t) & 1 and not (int(m[j]) >> u) & 1),
                      key=rank)
        assert len(cand) >= q
        picks += [(j, t, u) for j in (cand[:q] if u < t else cand[-q:])]
    if len(picks) > MAX_MOVES:
        return None
    out = [int(x) for x in m]
    for j, t, u in picks:
        out[j] ^= (1 << t) | (1 << u)
    return out


def ref_run(T, G, job, w, c, m, delta, trace=None):
    """The step restated: its loop over load sizes with the edge costs of
    edges() and the moves of cancel() above; only the cycle search is the
    twin's (twin_find_cycle, held to the exact reference by its own tests).
    delta: the step's δ (twin_edges returns it).  Returns (masks, ncancel);
    trace, if a list, receives (F, cycle) per cancel."""
    classes = sorted(set(int(x) for x in w))
    m = [int(x) for x in m]
    dw, cert, nc, changed = {}, {}, 0, True
    while changed and nc < MAX_CANCEL:
        changed = False
        for F in classes:
            if nc >= MAX_CANCEL:
                break
            if cert.get(F) == nc:
                continue  # nothing cancelled since this load size found no cycle
            while nc < MAX_CANCEL:
                W, Wk, room = edges(T, G, w, c, m, F, delta, job)
                n, cyc, dw[F] = twin_find_cycle(T, F, W, room, dw.get(F))
                if n == 0:
                    cert[F] = nc
                    break
                after = cancel(T, w, c, m, F, Wk, cyc, job)
                if after is None:
                    break
                m = after
                nc += 1
                changed = True
                if trace is not None:
                    trace.append((F, cyc))
    return m, nc


def round_graph(T, W, room, F):
    """{(a, b): cost} over rounds 0..T−1 and V = T: the edges of W, t → V at
    cost 0 where round t has F free GPUs, V → u at cost 0 always."""
    g = {}
    for t in range(T):
        for u in range(T):
            if t != u and W[t][u] < NONE:
                g[(t, u)] = float(W[t][u])
        if room[t] >= F:
            g[(t, T)] = 0.0
        g[(T, t)] = 0.0
    return g


def negative_cycle_exists(graph, slack=0):
    """Exact: whether some cycle of {(a, b): cost} costs less than 0 once
    every edge is raised by slack.  Floyd–Warshall over rationals (brought to
    their common denominator, so the arithmetic is on integers)."""
    if not graph:
        return False
    fr = {e: Fraction(v) + Fraction(slack) for e, v in graph.items()}
    den = 1
    for v in fr.values():
        den = den // gcd(den, v.denominator) * v.denominator
    nodes = sorted({a for a, _ in fr} | {b for _, b in fr})
    ix = {v: i for i, v in enumerate(nodes)}
    n = len(nodes)
    d = [[None] * n for _ in range(n)]
    for (a, b), v in fr.items():
        x = int(v * den)
        i, j = ix[a], ix[b]
        if i == j:
            if x < 0:
                return True
            continue
        if d[i][j] is None or x < d[i][j]:
            d[i][j] = x
    for k in range(n):
        dk = d[k]
        cols = [j for j in range(n) if dk[j] is not None]
        for i in range(n):
            dik = d[i][k]
            if dik is None or i == k:
                continue
            di = d[i]
            for j in cols:
                v = dik + dk[j]
                if di[j] is None or v < di[j]:
                    di[j] = v
            if di[i] is not None and di[i] < 0:
                return True
    return False


def cycle_cost(graph, cyc):
    """The exact cost of the cycle cyc, given in predecessor order (the step's:
    cyc[i + 1] is the predecessor of cyc[i], so its edges are cyc[i + 1] →
    cyc[i]); None if a step is not an edge."""
    tot = Fraction(0)
    for i, u in enumerate(cyc):
        t = cyc[(i + 1) % len(cyc)]
        if (t, u) not in graph:
            return None
        tot += Fraction(graph[(t, u)])
    return tot


def transport_optimum(T, slots, c, n):
    """The optimum of one width class's P2: min Σ_j c_j·Σ_t t·y_jt with
    Σ_t y_jt = n_j, Σ_j y_jt ≤ slots, y binary — HiGHS at gap 0 with
    integrality.  Returns (the exact objective of the integral optimum found,
    its masks); an unsolved case is an error of this reference."""
    A = len(c)
    cost = np.array([float(c[j]) * t for j in range(A) for t in range(T)])
    scale = float(np.max(np.abs(cost))) or 1.0
    rows = sp.kron(sp.identity(A), np.ones((1, T)), format="csr")
    cols = sp.kron(np.ones((1, A)), sp.identity(T), format="csr")
    cons = [LinearConstraint(rows, np.array(n, dtype=float), np.array(n, dtype=float)),
            LinearConstraint(cols, -np.inf, float(slots))]
    res = milp(cost / scale, constraints=cons, integrality=np.ones(A * T), bounds=Bounds(0, 1),
               options={"mip_rel_gap": 0.0, "presolve": True})
    if res.status != 0 or res.x is None:
        raise RuntimeError(f"transport_optimum: HiGHS status {res.status}: {res.message}")
    y = np.rint(res.x).astype(np.int64).reshape(A, T)
    if np.max(np.abs(res.x.reshape(A, T) - y)) > 1e-6 or not np.array_equal(y.sum(axis=1), np.array(n)) \
            or y.sum(axis=0).max() > slots:
        raise RuntimeError("transport_optimum: HiGHS returned a point that is not an integral placement")
    masks = [sum(1 << t for t in range(T) if y[j, t]) for j in range(A)]
    return objective(c, masks), masks
