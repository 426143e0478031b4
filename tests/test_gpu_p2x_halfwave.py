"""p2x_find_cycle's relaxation at the edge of its two forms (csrc/sw_p2x_dev.h):
up to T = 32 a wave's ⌈T / 8⌉ rows are split between its half-waves (lanes 0–31
the first ⌈nq / 2⌉, lanes 32–63 the rest) and combined once, and wave 0 joins
the eight waves' partials the same way, four per half-wave; above, each wave
walks its rows in a loop and wave 0 the eight partials.  Given graphs through
the existing probe entry (tests/native/p2x_probe.hip), every case against the
sequential specification (oracle/p2x_twin.c: length, cycle and all T + 1
distances, bit for bit):

  * T = 2, 31, 32, 33 and 64, and every T at which the rows per wave or per
    half-wave change (8 | 9, 16 | 17, 24 | 25);
  * equal best distances through a lower-half row and an upper-half row of one
    wave, and through rows of two waves: the lowest source must win;
  * missing edges (SW_P2X_NONE) beside distances below −SW_P2X_NONE;
  * warm starts; graphs with and without a negative cycle.
One launch per group of cases.
"""
import numpy as np
import pytest

import p2x_ref as pr
import p2xcases as pc

pytestmark = pytest.mark.gpu

NONE = pr.NONE
SIZES = (2, 3, 8, 9, 16, 17, 24, 25, 31, 32, 33, 64)
WAVES = 8


def rows_of(T):
    """(rows per wave, rows of a wave's lower half) of the relaxation."""
    nq = (T + WAVES - 1) // WAVES
    return nq, (nq + 1) // 2 if T <= 32 else nq


def check(graphs, dws, what):
    got = pr.probe_find_cycle(graphs, dws)
    want = []
    for i, g in enumerate(graphs):
        n, cyc, d = pr.twin_find_cycle(g[0], g[1], g[2], g[3], None if dws is None else dws[i])
        assert (got[i][0], got[i][1]) == (n, cyc), (what, i, g[0], got[i][:2], (n, cyc))
        assert got[i][2].tobytes() == d.tobytes(), (what, i, g[0])
        want.append((n, cyc, d))
    return want


def two_preds(T, a, b, u, back=True):
    """u reached at equal cost from a and from b, and (back) both reached from
    u: the cycle found is u's predecessor's, so it names the tie's winner."""
    W = np.full((T, T), NONE)
    W[a, u] = W[b, u] = -1.0
    if back:
        W[u, a] = W[u, b] = -1.0
    return pc._graph(T, 1, W, [0] * T)


def tie_cases():
    """[(graph, the source that must win, the other)]: ties inside one wave
    across its halves, inside one half, and across waves."""
    out = []
    for T in SIZES:
        nq, nh = rows_of(T)
        for wv in range(WAVES):
            t0 = wv * nq
            rows = [t for t in range(t0, min(T, t0 + nq))]
            lower, upper = rows[:nh], rows[nh:]
            pairs = [(lo, up) for lo in lower for up in upper]            # across the halves
            pairs += [(r[0], r[-1]) for r in (lower, upper) if len(r) > 1]  # inside one half
            for a, b in pairs:
                u = next(x for x in range(T) if x not in (a, b)) if T > 2 else None
                if u is not None:
                    out.append((two_preds(T, a, b, u), a, b))
        # across waves, every pair of them (wave 0 joins the partials of waves 0–3 in its lower
        # half and of waves 4–7 in its upper half up to T = 32): their first rows
        firsts = [wv * nq for wv in range(WAVES) if wv * nq < T]
        for i, a in enumerate(firsts):
            for b in firsts[i + 1:]:
                u = next(x for x in range(T) if x not in (a, b)) if T > 2 else None
                if u is not None:
                    out.append((two_preds(T, a, b, u), a, b))
    return out


def test_gpu_lowest_source_wins_ties_in_and_across_half_waves():
    cases = tie_cases()
    assert len(cases) > 100
    want = check([g for g, _, _ in cases], None, "ties")
    for (g, a, b), (n, cyc, _) in zip(cases, want):
        assert n == 2 and a in cyc and b not in cyc, (g[0], a, b, cyc)


def test_gpu_random_graphs_cold_and_warm_at_every_row_split():
    rng = np.random.default_rng(41)
    cold, warm = [], []
    for T in SIZES:
        for _ in range(12):
            g = pc.random_graph(rng, T)
            cold.append(g)
            warm.append(pc.perturb_rows(rng, g))
    want = check(cold, None, "cold")
    with_cycle = sum(1 for n, _, _ in want if n > 0)
    assert 0 < with_cycle < len(cold), "graphs with and without a negative cycle"
    w2 = check(warm, [d for _, _, d in want], "warm")
    assert 0 < sum(1 for n, _, _ in w2 if n > 0) < len(warm)


def test_gpu_missing_edges_beside_distances_below_minus_none():
    """Warm distances of −2e300 and −1.5e300: d + SW_P2X_NONE is below every
    real candidate, so a missing edge taken by its sum would win."""
    rng = np.random.default_rng(43)
    graphs, dws = [], []
    for T in SIZES:
        for dense in (False, True):
            W = rng.integers(-2, 6, size=(T, T)).astype(np.float64)
            W[rng.random((T, T)) >= (0.7 if dense else 0.2)] = NONE
            graphs.append(pc._graph(T, 1, W, [1 if t % 3 == 0 else 0 for t in range(T)]))
            d = rng.integers(-3, 4, size=T + 1).astype(np.float64)
            d[rng.random(T + 1) < 0.4] = -2.0e300
            d[rng.random(T + 1) < 0.2] = -1.5e300
            dws.append(d)
    check(graphs, dws, "sentinel")
    check(graphs, None, "sentinel cold")


def test_gpu_rings_with_and_without_a_negative_cycle():
    graphs = [pc.ring(T, v, cost) for T in SIZES for v in (False, True) for cost in (-1.0, 0.0, 1.0)]
    want = check(graphs, None, "rings")
    for g, (n, _, _) in zip(graphs, want):
        neg = g[2][0, 1] < 0.0
        assert (n > 0) == neg, (g[0], n)
    check(graphs, [d for _, _, d in want], "rings warm")
