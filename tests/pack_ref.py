"""tests/pack_ref.py — TEST INFRASTRUCTURE for the placement's round loop
(csrc/sw_pack.h, pack() of oracle/plan_twin.c).

  * ``twin_pack`` — the sequential specification's packer
    (twin_pack_arrays_caps of oracle/plan_twin.c) through ctypes;
    ``twin_positions`` — the same on positions already in placement order.
  * ``probe_block`` / ``probe_wave`` / ``probe_one`` / ``probe_room`` /
    ``probe_prims`` — the device code (csrc/sw_pack.h, csrc/sw_block.h) through
    tests/native/pack_probe.hip, built by csrc/Makefile into
    shockwave-replication_amd/lib/libpack_probe.so.
  * ``ref_pack`` / ``ref_room`` / ``gale_ryser`` / ``max_flow_places_all`` /
    ``check_valid`` / ``check_maximal`` — a plain restatement of the placement
    rule and of what a placement must satisfy: Python lists, sets and
    ``sorted()``; the need of a tier straight from its definition.  No
    histogram, no cumulative form and nothing from sw_pack.h.
A case is a dict with T, G, w, n, k1, k2 (per job) and caps (None: every round
holds G).  A position case is a dict with T, G, r, w (numpy, per position in
placement order) and caps.
Only tests/ may import this module.
"""
import ctypes as C
import os
import subprocess

import numpy as np

TMAX = 64
PAD = -12345    # what the capacity rows hold past T: nothing may read it

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
        ip = C.POINTER(C.c_int32)
        lib.twin_pack_arrays_caps.argtypes = [C.c_int32, C.c_int32, C.c_int32, ip, ip, C.POINTER(C.c_uint64),
                                              C.POINTER(C.c_uint32), C.POINTER(C.c_uint8), ip, ip, C.c_int]
        lib.twin_pack_arrays_caps.restype = None
        _LIB = lib
    return _LIB


def _p(a, t):
    return a.ctypes.data_as(C.POINTER(t))


def twin_pack(N, T, G, w, nin, k1, k2, caps=None, unit=False):
    """(y[N][T] as uint8, placed[N]) of the twin's pack(); caps: per-round
    capacities or None; unit: every width counts 1."""
    wa = np.ascontiguousarray(w, dtype=np.int32)
    na = np.ascontiguousarray(nin, dtype=np.int32)
    k1a = np.ascontiguousarray(k1, dtype=np.uint64)
    k2a = np.ascontiguousarray(k2, dtype=np.uint32)
    assert len(wa) == len(na) == len(k1a) == len(k2a) == N and 0 <= T <= TMAX
    y = np.full((max(N, 1), max(T, 1)), 7, dtype=np.uint8)
    placed = np.full(max(N, 1), -7, dtype=np.int32)
    ca = None if caps is None else np.ascontiguousarray(caps, dtype=np.int32)
    assert ca is None or len(ca) == T
    _lib().twin_pack_arrays_caps(N, T, G, _p(wa, C.c_int32), _p(na, C.c_int32), _p(k1a, C.c_uint64),
                                 _p(k2a, C.c_uint32), _p(y, C.c_uint8), _p(placed, C.c_int32),
                                 None if ca is None else _p(ca, C.c_int32), int(bool(unit)))
    return y.reshape(-1)[:N * T].reshape(N, T), placed[:N]


def twin_positions(P):
    """(round masks as uint64[A], residual r as int32[A]) of the twin on the
    position case P: job j is position j, k1 = A − j makes the twin's order the
    position order; with P["unit"] the twin runs its unit form (the positions
    then carry w = 1)."""
    A, T = len(P["r"]), P["T"]
    unit = bool(P.get("unit", False))
    assert not unit or np.all(np.asarray(P["w"]) == 1)
    k1 = (A - np.arange(A)).astype(np.uint64)
    y, placed = twin_pack(A, T, P["G"], P["w"], P["r"], k1, np.zeros(A, dtype=np.uint32), P["caps"], unit)
    bits = (np.uint64(1) << np.arange(T, dtype=np.uint64))
    masks = (y.astype(np.uint64) * bits[None, :]).sum(axis=1, dtype=np.uint64) if A else np.zeros(0, np.uint64)
    return masks, np.asarray(P["r"], dtype=np.int32) - placed


def positions(case):
    """The position case of a case: its jobs with rounds to place in the
    placement order (k1 descending, k2 descending, job ascending); under the
    case's unit flag every position carries w = 1."""
    order = sorted((j for j in range(len(case["n"])) if case["n"][j] > 0),
                   key=lambda j: (-int(case["k1"][j]), -int(case["k2"][j]), j))
    return {"name": case["name"], "T": case["T"], "G": case["G"], "caps": case["caps"], "unit": case["unit"],
            "r": np.array([case["n"][j] for j in order], dtype=np.int32),
            "w": np.array([1 if case["unit"] else case["w"][j] for j in order], dtype=np.int32)}


# ---- the device code through the probe library ------------------------------

_PROBE_SO = os.path.join(os.path.dirname(_HERE), "shockwave-replication_amd", "lib", "libpack_probe.so")
_PROBE = None


def _probe():
    """libpack_probe.so; absent means the build is broken (no fall-back)."""
    global _PROBE
    if _PROBE is None:
        lib = C.CDLL(_PROBE_SO)
        ip, up, lp, sp = C.POINTER(C.c_int32), C.POINTER(C.c_uint64), C.POINTER(C.c_int64), C.POINTER(C.c_uint32)
        for f in (lib.pack_probe_block, lib.pack_probe_wave, lib.pack_probe_one):
            f.argtypes = [C.c_int32, C.c_int32, lp, ip, ip, ip, ip, sp, up, sp]
        lib.pack_probe_room.argtypes = [C.c_int32, ip, ip, ip, ip, ip, ip, ip]
        lib.pack_probe_prims.argtypes = [C.c_int32, ip, ip, ip, C.c_int32, ip, ip, ip]
        for f in (lib.pack_probe_block, lib.pack_probe_wave, lib.pack_probe_one, lib.pack_probe_room,
                  lib.pack_probe_prims):
            f.restype = C.c_int
        _PROBE = lib
    return _PROBE


def _rows(cases):
    """T, G, the capacity rows (PAD past T) and the has-caps flags."""
    n = len(cases)
    T = np.array([P["T"] for P in cases], dtype=np.int32)
    G = np.array([P["G"] for P in cases], dtype=np.int32)
    caps = np.full((max(n, 1), TMAX), PAD, dtype=np.int32)
    has = np.zeros(max(n, 1), dtype=np.int32)
    for i, P in enumerate(cases):
        if P["caps"] is not None:
            caps[i, :P["T"]] = P["caps"]
            has[i] = 1
    return T, G, caps, has


def _loop(fn, sel, cases):
    off = np.zeros(len(cases) + 1, dtype=np.int64)
    off[1:] = np.cumsum([len(P["r"]) for P in cases])
    T, G, caps, has = _rows(cases)
    parts = [np.asarray(P["r"], dtype=np.uint32) | (np.asarray(P["w"], dtype=np.uint32) << np.uint32(8))
             for P in cases]
    st = np.concatenate(parts + [np.zeros(1, dtype=np.uint32)])
    mk = np.full(len(st), 0xDEADBEEFDEADBEEF, dtype=np.uint64)
    sto = np.full(len(st), 0xDEADBEEF, dtype=np.uint32)
    rc = fn(sel, len(cases), _p(off, C.c_int64), _p(T, C.c_int32), _p(G, C.c_int32), _p(caps, C.c_int32),
            _p(has, C.c_int32), _p(st, C.c_uint32), _p(mk, C.c_uint64), _p(sto, C.c_uint32))
    assert rc == 0, f"{fn.__name__}({sel}): HIP error {rc}"
    out = []
    for i in range(len(cases)):
        s = sto[off[i]:off[i + 1]]
        assert np.array_equal(s >> np.uint32(8), st[off[i]:off[i + 1]] >> np.uint32(8)), "the loop changed a width"
        out.append((mk[off[i]:off[i + 1]].copy(), (s & np.uint32(0xFF)).astype(np.int32)))
    return out


def probe_block(E, cases):
    """[(round masks, residual r)] of sw_pack_rounds<E> on the position cases, one launch."""
    return _loop(_probe().pack_probe_block, E, cases)


def probe_wave(E1, cases):
    """The same of sw_pack_rounds_wave<E1>."""
    return _loop(_probe().pack_probe_wave, E1, cases)


def probe_one(multi, cases):
    """The same of sw_pack_rounds_one<multi>."""
    return _loop(_probe().pack_probe_one, int(bool(multi)), cases)


def probe_room(cases):
    """[(room with the row's cbase [T][64], room with cbase = −1 [T][64], that
    cbase)] of sw_pack_room on the cases' capacity rows, one launch."""
    n = len(cases)
    T, G, caps, has = _rows(cases)
    ra = np.full((n, TMAX, 64), PAD, dtype=np.int32)
    rb = np.full((n, TMAX, 64), PAD, dtype=np.int32)
    cb = np.full(n, PAD, dtype=np.int32)
    rc = _probe().pack_probe_room(n, _p(T, C.c_int32), _p(G, C.c_int32), _p(caps, C.c_int32), _p(has, C.c_int32),
                                  _p(ra, C.c_int32), _p(rb, C.c_int32), _p(cb, C.c_int32))
    assert rc == 0, f"pack_probe_room: HIP error {rc}"
    return [(ra[i, :T[i]], rb[i, :T[i]], int(cb[i])) for i in range(n)]


def probe_prims(vs, va, ba, bb):
    """The wave primitives on the rows of vs (sort, min, max) and va (scans,
    sum), both [n][64], and the block primitives on the rows of ba and bb,
    both [m][512].  Returns a dict of arrays: sort, incscan, sufscan, sum, min,
    max [n][64]; exscan_a, total_a, exscan_b, total_b, sum_a, sum_b, min_a,
    min_b [m][512]."""
    vs, va = (np.ascontiguousarray(x, dtype=np.int32).reshape(-1, 64) for x in (vs, va))
    ba, bb = (np.ascontiguousarray(x, dtype=np.int32).reshape(-1, 512) for x in (ba, bb))
    assert vs.shape == va.shape and ba.shape == bb.shape
    wout = np.full((len(vs), 6, 64), PAD, dtype=np.int32)
    bout = np.full((len(ba), 8, 512), PAD, dtype=np.int32)
    rc = _probe().pack_probe_prims(len(vs), _p(vs, C.c_int32), _p(va, C.c_int32), _p(wout, C.c_int32), len(ba),
                                   _p(ba, C.c_int32), _p(bb, C.c_int32), _p(bout, C.c_int32))
    assert rc == 0, f"pack_probe_prims: HIP error {rc}"
    out = {k: wout[:, i] for i, k in enumerate(("sort", "incscan", "sufscan", "sum", "min", "max"))}
    out.update({k: bout[:, i] for i, k in enumerate(("exscan_a", "total_a", "exscan_b", "total_b", "sum_a", "sum_b",
                                                     "min_a", "min_b"))})
    return out


# ---- the plain reference --------------------------------------------------

def ref_room(T, G, caps, t, x):
    """The x smallest capacities of the rounds after t."""
    later = [G] * (T - 1 - t) if caps is None else sorted(int(c) for c in caps[t + 1:T])
    assert 0 <= x <= len(later)
    return sum(later[:x])


def ref_pack(N, T, G, w, nin, k1, k2, caps=None, unit=False):
    """The placement rule restated.  Jobs with rounds to place are visited in
    the order (k1 descending, k2 descending, job ascending).  Round t, with
    R = T − t rounds still open, a job counting min(rounds left, R):

      tiers m = R − 1 … 0: the jobs with more than m rounds left need
        Σ (min(left, R) − m)·w slots after this round's start and have the
        R − 1 − m smallest later capacities besides this round, so they must
        take need = that sum − that room now; q = need − what earlier tiers
        of this round took.  When q > 0, walk the jobs not yet chosen with more
        than m left, in order, counting their widths in ``seen``: a job is
        chosen when seen < q and seen + w fits what the round had free at the
        tier's start;
      fill: the same walk over all jobs not chosen with rounds left, a job
        chosen when seen + w fits;
      tail: while something is free, the first job in order not chosen, with
        rounds left, whose width fits.

    Returns (y[N][T] lists of 0/1, placed[N])."""
    order = sorted((j for j in range(N) if nin[j] > 0), key=lambda j: (-int(k1[j]), -int(k2[j]), j))
    width = {j: 1 if unit else int(w[j]) for j in order}
    left = {j: int(nin[j]) for j in order}
    y = [[0] * T for _ in range(N)]
    for t in range(T):
        R = T - t
        free = int(caps[t]) if caps is not None else G
        chosen = set()
        for m in range(R - 1, -1, -1):
            above = [j for j in order if left[j] > m]
            need = sum((min(left[j], R) - m) * width[j] for j in above) - ref_room(T, G, caps, t, R - 1 - m)
            q = need - sum(width[j] for j in chosen)  # every job chosen so far has more than m left
            if q <= 0:
                continue
            seen, start = 0, free
            for j in above:
                if j in chosen:
                    continue
                if seen < q and seen + width[j] <= start:
                    chosen.add(j)
                    free -= width[j]
                seen += width[j]
        seen, start = 0, free
        for j in order:
            if j in chosen or left[j] <= 0:
                continue
            if seen + width[j] <= start:
                chosen.add(j)
                free -= width[j]
            seen += width[j]
        while free > 0:
            fit = [j for j in order if j not in chosen and left[j] > 0 and width[j] <= free]
            if not fit:
                break
            chosen.add(fit[0])
            free -= width[fit[0]]
        for j in chosen:
            y[j][t] = 1
            left[j] -= 1
    placed = [0] * N
    for j in order:
        placed[j] = int(nin[j]) - left[j]
    return y, placed


def gale_ryser(n, caps):
    """Whether jobs needing n[j] distinct rounds fit rounds holding caps[t]
    jobs each: for every x, what the jobs cannot keep out of the x smallest
    rounds, Σ max(0, n_j − (T − x)), is at most those rounds' capacity."""
    T = len(caps)
    small = sorted(int(c) for c in caps)
    return all(sum(max(0, int(nj) - (T - x)) for nj in n) <= sum(small[:x]) for x in range(T + 1))


def max_flow_places_all(n, caps):
    """The same question answered by a maximum flow (source → job n_j, job →
    round 1, round → sink caps[t]): an independent check of gale_ryser."""
    from scipy.sparse import csr_matrix
    from scipy.sparse.csgraph import maximum_flow

    A, T = len(n), len(caps)
    if A == 0:
        return True
    S, K = A + T, A + T + 1
    rows, cols, val = [], [], []
    for j in range(A):
        rows.append(S), cols.append(j), val.append(int(n[j]))
        for t in range(T):
            rows.append(j), cols.append(A + t), val.append(1)
    for t in range(T):
        rows.append(A + t), cols.append(K), val.append(int(caps[t]))
    g = csr_matrix((np.array(val, dtype=np.int32), (rows, cols)), shape=(K + 1, K + 1))
    return maximum_flow(g, S, K).flow_value == sum(int(x) for x in n)


def _caps_of(T, G, caps):
    return [G] * T if caps is None else [int(c) for c in caps]


def check_valid(T, G, w, n, caps, y, placed, unit=False):
    """Each round's load is at most its capacity, each job is placed at most
    once per round (y is 0/1), placed is the row sum and at most n."""
    cp = _caps_of(T, G, caps)
    y = np.asarray(y, dtype=np.int64).reshape(len(n), T)
    assert np.all((y == 0) | (y == 1))
    wd = np.ones(len(n), dtype=np.int64) if unit else np.asarray(w, dtype=np.int64)
    load = (y * wd[:, None]).sum(axis=0)
    assert np.all(load <= np.array(cp, dtype=np.int64)), (load.tolist(), cp)
    rows = y.sum(axis=1)
    assert np.array_equal(rows, np.asarray(placed, dtype=np.int64))
    assert np.all(rows <= np.maximum(np.asarray(n, dtype=np.int64), 0))


def check_maximal(T, G, w, n, caps, y, unit=False):
    """Per round, no idle job with rounds left whose width fits the round's
    leftover.  Returns the number of (round, job) pairs examined that were
    idle with rounds left."""
    cp = _caps_of(T, G, caps)
    y = np.asarray(y, dtype=np.int64).reshape(len(n), T)
    wd = np.ones(len(n), dtype=np.int64) if unit else np.asarray(w, dtype=np.int64)
    left = np.maximum(np.asarray(n, dtype=np.int64), 0)
    seen = 0
    for t in range(T):
        leftover = cp[t] - int((y[:, t] * wd).sum())
        idle = (y[:, t] == 0) & (left > 0)
        seen += int(idle.sum())
        assert not np.any(idle & (wd <= leftover)), (t, leftover, np.flatnonzero(idle & (wd <= leftover))[:4])
        left = left - y[:, t]
    return seen
