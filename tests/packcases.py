"""Case generators for the placement round loop's own tests (tests/test_pack.py
on the CPU, tests/test_gpu_pack.py on the GPU).  Seeded and small: the shapes
are the smallest that reach each path of csrc/sw_pack.h.

A case is a dict with T, G, w, n, k1, k2 (lists per job), caps (None: every
round holds G) and unit (the widths count 1, whatever w says: the class-wise
repack's form); ``name``, ``wkind`` and ``ckind`` say what it is.  A position
case (see pack_ref.py) holds numpy arrays r, w per position.
"""
import numpy as np

WIDTH_KINDS = ("unit", "equal", "mixed")
CAP_KINDS = ("none", "base", "free")   # uniform G; base + {0, 1}; free in [0, G]
MIXED = (1, 2, 3, 4, 8, 255)
MIXED_P = (0.4, 0.25, 0.1, 0.15, 0.07, 0.03)

BLOCK_E = (2, 4, 8, 20, 32, 64)
WAVE_E1 = (2, 4, 6, 8, 16, 32, 64)
ONE_A = (1, 128, 129, 256, 257, 384, 385, 512)   # sw_pack_rounds_one's selector bounds


def block_sizes(E):
    """E·64 ± 1: where a position's prefix first crosses a wave; E·512: full."""
    return (1, 63, 64, 65, E * 64 - 1, E * 64 + 1, E * 512 - 1, E * 512)


def wave_sizes(E1):
    return (1, E1, E1 + 1, 64 * E1 - 1, 64 * E1)


def _capacities(rng, ckind, T, per_round, mult=1):
    """(G, caps) of a capacity kind around per_round per round; mult: every
    capacity a multiple of it (kinds none and free)."""
    if ckind == "none":
        return per_round // mult * mult, None
    if ckind == "base":
        return per_round + 1, [per_round + int(x) for x in rng.integers(0, 2, size=T)]
    G = 2 * per_round // mult * mult
    palette = rng.integers(0, G // mult + 1, size=int(rng.integers(1, 5))) * mult
    caps = [int(x) for x in rng.choice(palette, size=T)]   # few values: repeats
    if rng.random() < 0.5:
        caps[int(rng.integers(0, T))] = 0
    return G, caps


def _trim(rng, n, w, total):
    """Take single rounds off random jobs until Σ n·w ≤ total."""
    need = sum(a * b for a, b in zip(n, w))
    live = [j for j in range(len(n)) if n[j] > 0]
    while need > total and live:
        i = int(rng.integers(0, len(live)))
        j = live[i]
        n[j] -= 1
        need -= w[j]
        if n[j] == 0:
            live[i] = live[-1]
            live.pop()


def random_case(rng, wkind, ckind, trim, name, small=False, multiples=None, T=None):
    """small: at most 30 jobs and 12 rounds; multiples (one width c): True makes
    every capacity a multiple of c, False redraws until one is not."""
    T0 = int(rng.integers(1, 65)) if rng.random() < 0.3 and not small else int(rng.integers(1, 13))
    T = T0 if T is None else T
    N = int(rng.integers(1, 41)) if rng.random() < 0.6 else int(rng.integers(41, 201))
    N = int(rng.integers(1, 31)) if small else N
    unit = wkind == "unit" and rng.random() < 0.5
    c = int(rng.choice((2, 3, 4, 8)))
    if wkind == "mixed" or unit:   # under unit the widths are not read
        w = [int(x) for x in rng.choice(MIXED, size=N, p=MIXED_P)]
    else:
        w = [1 if wkind == "unit" else c] * N
    full = rng.random(N) < 0.25    # every round
    n = [T if full[j] else int(rng.integers(1, T + 1)) for j in range(N)]
    for j in np.flatnonzero(rng.random(N) < 0.1):
        n[j] = 0   # not active: takes no position
    eff = [1] * N if unit else w
    demand = sum(a * b for a, b in zip(n, eff))
    f = float(rng.choice((0.4, 0.6, 0.8))) if trim else float(rng.choice((0.7, 0.9, 1.0, 1.1, 1.4)))
    mult = c if wkind == "equal" and (rng.random() < 0.5 if multiples is None else multiples) else 1
    while True:
        G, caps = _capacities(rng, ckind, T, int(demand * f / T), mult)
        if multiples is not False or any(x % c for x in ([G] if caps is None else caps)):
            break
        demand += 1   # G = 0, or a base that is a multiple at T = 1: move on
    if trim:   # against what the widths can use: one width c cannot use cap mod c
        u = c if wkind == "equal" else 1
        _trim(rng, n, eff, sum(x // u * u for x in ([G] * T if caps is None else caps)))
    hi = max(2, N // 3)   # few key values: ties down to the job index
    return {"name": name, "wkind": wkind, "ckind": ckind, "T": T, "G": G, "w": w, "n": n, "unit": bool(unit),
            "k1": [int(x) for x in rng.integers(0, hi, size=N)], "k2": [int(x) for x in rng.integers(0, 3, size=N)],
            "caps": caps}


def random_cases(per_cell=24, seed=71):
    """per_cell cases of every (width kind, capacity kind), half of them trimmed
    onto the feasibility edge; the first two of a cell have T = 64 and T = 1."""
    rng = np.random.default_rng(seed)
    return [random_case(rng, wk, ck, i % 2 == 1, f"random_{wk}_{ck}_{i}", T={0: 64, 1: 1}.get(i))
            for wk in WIDTH_KINDS for ck in CAP_KINDS for i in range(per_cell)]


def small_cases(count, wkind, seed, multiples=None):
    """count small cases of one width kind over the capacity kinds, half trimmed
    (for the properties that need only the twin, so there can be many)."""
    rng = np.random.default_rng(seed)
    kinds = ("none", "free") if multiples else CAP_KINDS   # base + {0, 1} has no multiples of c > 1
    return [random_case(rng, wkind, kinds[i % len(kinds)], i % 2 == 1, f"small_{wkind}_{i}", True, multiples)
            for i in range(count)]


def _case(name, T, G, w, n, caps=None, k1=None, k2=None, unit=False):
    N = len(n)
    return {"name": name, "wkind": "edge", "ckind": "none" if caps is None else "edge", "T": T, "G": G,
            "w": list(w), "n": list(n), "k1": list(k1) if k1 is not None else [N - j for j in range(N)],
            "k2": list(k2) if k2 is not None else [0] * N, "caps": None if caps is None else list(caps),
            "unit": unit}


def edge_cases(seed=72):
    rng = np.random.default_rng(seed)
    r64 = [int(x) for x in rng.integers(1, 65, size=90)]
    w64 = [int(x) for x in rng.choice((1, 2, 4), size=90)]
    spread = lambda T, lo, d: [lo + int(x) for x in rng.permutation(np.arange(T) % (d + 1))]  # noqa: E731
    out = [
        _case("A0", 5, 4, [], []),
        _case("A0_of_3", 5, 4, [1, 2, 1], [0, 0, 0]),
        _case("A1", 6, 2, [2], [4]),
        _case("A1_too_wide", 6, 2, [3], [4]),
        _case("T1", 1, 5, [1, 2, 3, 1, 2], [1, 1, 1, 1, 1]),
        _case("T64_n64", 64, 7, [1, 2, 4, 1, 2, 1, 3], [64, 64, 64, 40, 64, 1, 64]),
        _case("T64_n64_caps", 64, 9, [1] * 12, [64] * 8 + [30, 20, 10, 5],
              caps=[8 + (t % 3 == 0) for t in range(64)]),
        _case("G0", 4, 0, [1, 2], [2, 3]),
        _case("caps_all_0", 4, 3, [1, 1], [2, 3], caps=[0, 0, 0, 0]),
        _case("every_n_T", 9, 6, [1, 2, 1, 2, 1, 2], [9] * 6),
        _case("every_n_T_fits", 9, 9, [1, 2, 1, 2, 1, 2], [9] * 6),
        _case("wider_than_every_cap", 5, 8, [1, 9, 2, 1], [3, 5, 2, 4]),
        _case("wider_than_caps", 5, 8, [1, 7, 2, 1], [3, 5, 2, 4], caps=[6, 5, 6, 4, 6]),
        _case("w255", 7, 600, [255, 255, 1, 255, 90], [7, 3, 5, 2, 6]),
        _case("w255_alone", 3, 255, [255, 255], [2, 1]),
        _case("n_above_T", 4, 3, [1, 1, 1, 2], [6, 4, 5, 2]),
        _case("caps_equal", 12, 5, [1] * 9, [12, 11, 9, 7, 7, 5, 3, 2, 2], caps=[5] * 12),
        _case("caps_spread1", 12, 6, [1] * 9, [12, 11, 9, 7, 7, 5, 3, 2, 2], caps=spread(12, 4, 1)),
        _case("caps_spread2", 12, 6, [1] * 9, [12, 11, 9, 7, 7, 5, 3, 2, 2], caps=spread(12, 3, 2)),
        _case("caps_spread1_from_0", 10, 1, [1] * 4, [3, 2, 2, 1], caps=spread(10, 0, 1)),
        _case("caps_T64_sorted_all", 64, 9, w64, r64, caps=[int(x) for x in rng.integers(0, 10, size=64)]),
        _case("caps_T64_descending", 64, 70, w64, r64, caps=[64 - t for t in range(64)]),
        _case("ties", 8, 4, [1, 2, 1, 2, 1, 2, 1, 2], [5, 5, 5, 5, 3, 3, 3, 3], k1=[1] * 8, k2=[2] * 8),
        _case("unit_flag", 8, 3, [4, 255, 2, 8, 1, 3], [8, 6, 5, 4, 2, 1], caps=[3, 2, 3, 1, 3, 2, 3, 3], unit=True),
    ]
    return out


def position_case(rng, A, T, ckind, name, wkind="mixed", f=None):
    """A position case of A positions (numpy): every r in 1..T, a quarter T."""
    r = rng.integers(1, T + 1, size=A).astype(np.int32)
    r[rng.random(A) < 0.25] = T
    w = (np.ones(A, dtype=np.int32) if wkind == "unit"
         else rng.choice(MIXED, size=A, p=MIXED_P).astype(np.int32))
    f = float(rng.choice((0.9, 1.0, 1.15))) if f is None else f
    G, caps = _capacities(rng, ckind, T, int(int((r.astype(np.int64) * w).sum()) * f / T))
    return {"name": name, "T": T, "G": G, "r": r, "w": w, "caps": caps}


def size_cases(sizes, tag, seed):
    """For every A of the form's size list one case per capacity kind at
    T ≤ 16, and one T = 64 case (at the middle size, free capacities)."""
    rng = np.random.default_rng(seed)
    out = [position_case(rng, A, int(rng.integers(2, 17)), ck, f"{tag}_A{A}_{ck}")
           for A in sizes for ck in CAP_KINDS]
    mid = sorted(sizes)[len(sizes) // 2]
    out.append(position_case(rng, mid, 64, "free", f"{tag}_A{mid}_T64"))
    return out


def room_rows(seed=73):
    """Capacity rows for sw_pack_room: spread 0, 1, 2 and large, uniform G,
    zeros, T = 1, 2 and 64 — (name, position-case-like dict with T, G, caps)."""
    rng = np.random.default_rng(seed)
    row = lambda name, T, G, caps: {"name": name, "T": T, "G": G, "caps": caps}  # noqa: E731
    out = [row("uniform_T64", 64, 11, None), row("uniform_T1", 1, 3, None), row("uniform_G0", 7, 0, None)]
    for T in (1, 2, 3, 17, 63, 64):
        out.append(row(f"spread0_T{T}", T, 9, [6] * T))
        out.append(row(f"spread0_zero_T{T}", T, 9, [0] * T))
        out.append(row(f"spread1_T{T}", T, 9, [4 + int(x) for x in rng.integers(0, 2, size=T)]))
        out.append(row(f"spread1_from0_T{T}", T, 9, [int(x) for x in rng.integers(0, 2, size=T)]))
        out.append(row(f"spread2_T{T}", T, 9, [3 + int(x) for x in rng.integers(0, 3, size=T)]))
        out.append(row(f"large_T{T}", T, 9, [int(x) for x in rng.integers(0, 1 << 20, size=T)]))
        out.append(row(f"descending_T{T}", T, 99, [T - t for t in range(T)]))
    out.append(row("spread1_one_high_T64", 64, 9, [5] * 63 + [6]))
    out.append(row("spread1_one_low_T64", 64, 9, [6] + [7] * 63))
    out.append(row("spread2_exact_T3", 3, 9, [2, 4, 3]))
    out.append(row("spread1_exact_T3", 3, 9, [2, 3, 2]))
    return out
