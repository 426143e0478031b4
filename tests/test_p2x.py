"""The P2 exchange step's specification (oracle/p2x_twin.c over csrc/sw_p2x.h)
against a plain reference (tests/p2x_ref.py: sets, sorting, exact rationals),
on graphs and placements of the tests' own — not what the placement cascade
leaves.

  a. edge costs: twin_p2x_edges equals the reference bit for bit (W) and
     exactly (Wk) on the shapes of p2xcases.shape_cases;
  b. find_cycle on small-integer graphs: a returned cycle is simple, starts at
     its lowest node, follows edges and costs < 0 exactly, and one is returned
     iff a negative cycle exists (Floyd–Warshall over rationals), cold and
     warm; rings of T and T + 1 nodes; the tie rules;
  c. invariants of twin_p2x_run on random feasible placements;
  d. the termination certificate: after a run below the cancel cap no load
     size's δ-shifted graph has a cycle below −1e-9·P2₀;
  e. inside one width class the result is within δ·D of the HiGHS optimum;
  f. the whole run restated in plain Python (edge costs and the jobs every
     cancelled cycle moves, by sets and sorting) ends in the twin's masks: the
     guard of sw_p2x_start / sw_p2x_next, across the 64-rank word edges.

Measured coverage (an instrumented scratch copy of the twin over this module's
257 run-level placements — shapes, random, single-class, the sentinel case):
237 runs cancel something, 14,530 cycles in all; 12 runs stop at the 256-cancel
cap, 4 of them among the 190 certificate cases (2.1 %, the test asserts ≤ 5 %);
2,488 cycle nodes are V, 599 edges move q = 4 jobs; some round has room exactly
F in 193 and exactly F − 1 in 280 (placement, load size) pairs.  Cycle lengths:
9,530 of 2 nodes, 3,407 of 3, 1,177 of 4, 282 of 5, 91 of 6, 25 of 7, 8 of 8,
2 of 9, 1 of 10, 3 of 11, 2 of 13, 1 of 14 and 1 of 23 — the last three from
the long_cycle_* cases, which a search over rotated geometric c sequences found
(random and dense multi-class placements reached 14 in the same search).  No
run-level placement was found whose cycle has 65 nodes (all of T = 64 and V),
so the move selection's second 64-lane pass in sw_p2x_dev.h is reached only
through find_cycle's output: the 64- and 65-node rings of (b) exercise the
cycle check and read-out on the GPU, not that pass.  find_cycle's 468 random
graphs: 207 have a negative cycle from cold, the longest returned has 11
nodes; the rings give T and T + 1.  Single class (e): 70 cases, 32 saturated,
64 end exactly optimal, the worst (P2_final − optimum)/(δ·D) is 0.484.

The sentinel case (c at and above 1e300) is where a Bellman–Ford that does not
test W entries against the no-edge value goes wrong: distances fall below
−1e300 and a missing edge wins the minimum.  The twin and sw_p2x_dev.h test
every entry.
"""
from fractions import Fraction

import numpy as np
import pytest

import p2x_ref as pr
import p2xcases as pc

SHAPES = pc.shape_cases()
SKIPPED = {"A4097_T8", "nine_classes_T10"}
GRAPHS = pc.random_graphs()
TIES = pc.tie_graphs()
RANDOM = pc.random_placements(120, seed=31)
SINGLE = pc.random_placements(70, seed=32, max_a=60, max_t=12, single=True)
SENTINEL = pc.sentinel_case()

_RUNS = {}


def run(P):
    """twin_p2x_run on a placement, once per placement."""
    k = id(P)
    if k not in _RUNS:
        _RUNS[k] = pr.twin_run(P["T"], P["G"], P["job"], P["w"], P["c"], P["m"])
    return _RUNS[k]


def popcount(x):
    return bin(int(x)).count("1")


def test_cases_are_what_their_names_say():
    """The generators' promises the other tests lean on."""
    for name, P in SHAPES.items():
        assert P["job"] == sorted(set(P["job"])) and all(m > 0 and m >> P["T"] == 0 for m in P["m"]), name
        assert max(pr.loads(P["T"], P["w"], P["m"])) <= P["G"], name
    for F in (1, 2, 4, 8):
        P = SHAPES[f"room_F{F}_T9"]
        room = [P["G"] - x for x in pr.loads(P["T"], P["w"], P["m"])]
        assert F in room and F - 1 in room, (F, room)
    for name in ("saturated_w1_T32", "saturated_w1248_T31", "long_cycle_T63"):
        P = SHAPES[name]
        assert set(pr.loads(P["T"], P["w"], P["m"])) == {P["G"]}, name
    assert len(SHAPES["A4097_T8"]["w"]) == 4097 and len(set(SHAPES["nine_classes_T10"]["w"])) == 9
    assert len(set(SHAPES["eight_classes_T10"]["w"])) == 8
    low = SHAPES["c_low_bits"]["c"]
    assert len({pr.ckey(x) for x in low}) < len(set(low))  # some differ only in the dropped bits


# ---- a. edge costs ---------------------------------------------------------

@pytest.mark.parametrize("name", sorted(SHAPES))
def test_edges_equal_reference(name):
    P = SHAPES[name]
    T, G = P["T"], P["G"]
    classes = sorted(set(P["w"]))
    if name in SKIPPED:
        W, Wk, delta = pr.twin_edges(T, G, P["job"], P["w"], P["c"], P["m"], classes[0])
        assert delta == -1.0 and np.all(np.isnan(W)) and np.all(Wk == -9)
        return
    for F in classes:
        W, Wk, delta = pr.twin_edges(T, G, P["job"], P["w"], P["c"], P["m"], F)
        want = pr.delta_of(T, P["c"], P["m"])
        assert abs(delta - want) <= 1e-12 * want, (delta, want)
        rW, rWk, _ = pr.edges(T, G, P["w"], P["c"], P["m"], F, delta, P["job"])
        assert np.array_equal(Wk, rWk), (name, F, np.argwhere(Wk != rWk)[:4])
        assert W.tobytes() == rW.tobytes(), (name, F, np.argwhere(W != rW)[:4])


def test_edges_sentinel_case_equals_reference():
    """c at and above the no-edge value: a class whose cost reaches it gives no edge."""
    P = SENTINEL
    for F in sorted(set(P["w"])):
        W, Wk, delta = pr.twin_edges(P["T"], P["G"], P["job"], P["w"], P["c"], P["m"], F)
        rW, rWk, _ = pr.edges(P["T"], P["G"], P["w"], P["c"], P["m"], F, delta, P["job"])
        assert np.array_equal(Wk, rWk) and W.tobytes() == rW.tobytes()


# ---- b. find_cycle ---------------------------------------------------------

def check_find_cycle(g, dw=None):
    """The twin's answer on graph g against the exact reference; returns (len, distances)."""
    T, F, W, room = g
    n, cyc, d = pr.twin_find_cycle(T, F, W, room, dw)
    graph = pr.round_graph(T, W, room, F)
    if n > 0:
        assert len(set(cyc)) == n and all(0 <= v <= T for v in cyc), cyc
        assert cyc[0] == min(cyc), cyc
        cost = pr.cycle_cost(graph, cyc)
        assert cost is not None, ("a step of the cycle is not an edge", cyc)
        assert cost < 0, (cost, cyc)
    assert (n > 0) == pr.negative_cycle_exists(graph), (T, n, cyc)
    assert np.all(d <= 0.0)
    return n, d


def test_find_cycle_random_graphs_cold_and_warm():
    found = 0
    for g, g2 in GRAPHS:
        n, d = check_find_cycle(g)
        n2, _ = check_find_cycle(g2, dw=d)
        found += (n > 0) + (n2 > 0)
    # the family has both answers in quantity
    assert 0.25 * 2 * len(GRAPHS) <= found <= 0.75 * 2 * len(GRAPHS), (found, len(GRAPHS))


@pytest.mark.parametrize("T", pc.GRAPH_T)
def test_find_cycle_rings(T):
    """The longest cycles the graph has: all T rounds, and all T rounds and V."""
    n, cyc, _ = pr.twin_find_cycle(*pc.ring(T))
    assert n == T and cyc == [0] + list(range(T - 1, 0, -1))
    n, cyc, _ = pr.twin_find_cycle(*pc.ring(T, through_v=True))
    assert n == T + 1 and cyc == [0, T] + list(range(T - 1, 0, -1))
    for through_v in (False, True):
        check_find_cycle(pc.ring(T, through_v))
        assert pr.twin_find_cycle(*pc.ring(T, through_v, cost=0.0))[0] == 0
        assert pr.twin_find_cycle(*pc.ring(T, through_v, cost=-0.0))[0] == 0


@pytest.mark.parametrize("name", sorted(TIES))
def test_find_cycle_ties(name):
    g = TIES[name]
    n, d = check_find_cycle(g)
    check_find_cycle(g, dw=d)
    T = g[0]
    if name.startswith(("no_edges", "all_zero", "all_minus_zero", "zero_ring")):
        assert n == 0
    if name.startswith("no_edges"):
        assert np.all(d == 0.0)
    if name.startswith("minus_one_ring"):
        assert n == T
    if name.startswith("two_rings"):
        # first predecessor wins: among the equal-cost predecessors u − 1 and u − 2 the lower round
        _, cyc, _ = pr.twin_find_cycle(*g)
        for i, u in enumerate(cyc):
            t = cyc[(i + 1) % len(cyc)]
            assert t == min((u - 1) % T, (u - 2) % T), (u, t)


# ---- c. invariants ---------------------------------------------------------

def check_invariants(P, final, nc):
    T, G, w, c, m0 = P["T"], P["G"], P["w"], P["c"], P["m"]
    assert 0 <= nc <= pr.MAX_CANCEL
    for a, b in zip(m0, final):
        assert popcount(a) == popcount(b)
        assert b >> T == 0
    assert max(pr.loads(T, w, final), default=0) <= G
    p0, p1 = pr.objective(c, m0), pr.objective(c, final)
    assert p1 <= p0
    moved = sum(a != b for a, b in zip(m0, final))
    if nc == 0:
        assert moved == 0
    else:
        # every cancelled cycle gains more than δ per edge and every edge moves ≥ 1 job
        delta = Fraction(pr.twin_edges(T, G, P["job"], w, c, m0, min(w))[2])
        assert moved > 0 and p0 - p1 > delta * moved, (float(p0 - p1), float(delta), moved)
    return p0, p1


@pytest.mark.parametrize("i", range(len(RANDOM)))
def test_run_invariants_random(i):
    P = RANDOM[i]
    final, nc = run(P)
    check_invariants(P, final, nc)


@pytest.mark.parametrize("name", sorted(SHAPES))
def test_run_invariants_shapes(name):
    P = SHAPES[name]
    final, nc = run(P)
    if name in SKIPPED:
        assert nc == 0 and final == P["m"]
    check_invariants(P, final, nc)


def test_run_invariants_sentinel_case():
    """Costs at and above the no-edge value: every invariant holds as elsewhere."""
    final, nc = run(SENTINEL)
    assert nc > 0
    check_invariants(SENTINEL, final, nc)


# The selection of the jobs a cycle moves (sw_p2x_start / sw_p2x_next, shared by
# the twin and the GPU): a feasible but wrong job satisfies every invariant, so
# the run is restated in plain Python (pr.ref_run: edges() and cancel() over
# sets and sorting) and must end in the twin's masks.  Every shape that cancels
# something, less a few large ones whose path another case covers (A511/512/
# 1024 beside A513/1025; the 256-cancel runs at A = 4096 take the plain
# reference too long).
REF_RUN = sorted(set(SHAPES) - SKIPPED - {"A4096_T8", "A1024_T8", "A511_T8", "A512_T8", "T63_M129", "room_F1_T64",
                                          "saturated_w1248_T31"})


_REF = {}


def ref_run(P):
    """pr.ref_run on a placement, once: (masks, ncancel, [(F, cycle)])."""
    if id(P) not in _REF:
        delta = pr.twin_edges(P["T"], P["G"], P["job"], P["w"], P["c"], P["m"], min(P["w"]))[2]
        trace = []
        _REF[id(P)] = pr.ref_run(P["T"], P["G"], P["job"], P["w"], P["c"], P["m"], delta, trace) + (trace,)
    return _REF[id(P)]


@pytest.mark.parametrize("name", REF_RUN + ["sentinel"])
def test_run_equals_plain_reference(name):
    P = SENTINEL if name == "sentinel" else SHAPES[name]
    final, nc = run(P)
    rm, rnc, _ = ref_run(P)
    assert rnc == nc, (nc, rnc)
    assert rm == final, [i for i, (a, b) in enumerate(zip(rm, final)) if a != b][:8]


def test_plain_reference_runs_cross_the_word_edges():
    """The cases above move jobs of ranks below and above 64 and 128, with q = 1, 2 and 4."""
    seen_q, hi_rank = set(), 0
    for name in ("T64_M129", "w1248_T64", "A513_T8"):
        P = SHAPES[name]
        classes = sorted(set(P["w"]))
        trace = ref_run(P)[2]
        seen_q |= {F // wk for F, _ in trace for wk in classes if F % wk == 0 and F // wk <= pr.QMAX}
        final = run(P)[0]
        order = sorted(range(len(P["w"])), key=lambda i: (P["w"][i], -pr.ckey(P["c"][i]), P["job"][i]))
        first = {}
        for pos, i in enumerate(order):
            first.setdefault(P["w"][i], pos)
            if final[i] != P["m"][i]:
                hi_rank = max(hi_rank, pos - first[P["w"][i]])
    assert {1, 2, 4} <= seen_q and hi_rank >= 128, (seen_q, hi_rank)


def test_run_skips():
    for name, P in pc.skip_cases().items():
        final, nc = pr.twin_run(P["T"], P["G"], P["job"], P["w"], P["c"], P["m"])
        assert nc == 0 and final == P["m"], name


# ---- d. termination certificate --------------------------------------------

CERT = [("random", i) for i in range(len(RANDOM))] + [("single", i) for i in range(len(SINGLE))]


def certificate_holds(P, final):
    """No load size's δ-shifted graph on the final placement has a cycle below
    −1e-9·P2₀.  A cycle has at most T + 1 edges, so one below −tol is negative
    once every edge is raised by tol/(T + 1): the exact test is for that."""
    T, G, w, c = P["T"], P["G"], P["w"], P["c"]
    p0 = pr.objective(c, P["m"])
    delta = pr.twin_edges(T, G, P["job"], w, c, P["m"], min(w))[2]
    slack = Fraction(1, 10 ** 9) * p0 / (T + 1)
    for F in sorted(set(w)):
        W, _, room = pr.edges(T, G, w, c, final, F, delta, P["job"])
        if pr.negative_cycle_exists(pr.round_graph(T, W, room, F), slack):
            return False
    return True


def test_cap_share_of_certificate_cases():
    """Runs that stop at the cancel cap are left out of the certificate: at most 5 % of its cases."""
    capped = sum(run((RANDOM if fam == "random" else SINGLE)[i])[1] >= pr.MAX_CANCEL for fam, i in CERT)
    assert capped <= 0.05 * len(CERT), (capped, len(CERT))


@pytest.mark.parametrize("fam,i", CERT)
def test_termination_certificate(fam, i):
    P = (RANDOM if fam == "random" else SINGLE)[i]
    final, nc = run(P)
    if nc >= pr.MAX_CANCEL:
        return  # counted by test_cap_share_of_certificate_cases
    assert certificate_holds(P, final)


# ---- e. exactness inside one class ------------------------------------------

@pytest.mark.parametrize("i", range(len(SINGLE)))
def test_single_class_within_delta_of_optimum(i):
    """P2_final − optimum ≤ δ·D·(1 + 1e-9) + 1e-12·P2₀, D the (job, round)
    memberships in which the final placement differs from the optimal one: the
    difference of the two splits into edge-disjoint residual cycles, and each
    costs ≥ −δ per edge or it would have been cancelled."""
    P = SINGLE[i]
    final, nc = run(P)
    assert nc < pr.MAX_CANCEL  # the bound is for runs that ended on their own; this family has no other
    T, G, w, c = P["T"], P["G"], P["w"], P["c"]
    assert len(set(w)) == 1
    opt, om = pr.transport_optimum(T, G // w[0], c, [popcount(x) for x in P["m"]])
    p0, p1 = pr.objective(c, P["m"]), pr.objective(c, final)
    assert p1 >= opt - Fraction(1, 10 ** 9) * p0  # the reference is the optimum
    delta = Fraction(pr.twin_edges(T, G, P["job"], w, c, P["m"], w[0])[2])
    D = sum(popcount(a ^ b) for a, b in zip(final, om))
    bound = delta * D * (1 + Fraction(1, 10 ** 9)) + Fraction(1, 10 ** 12) * p0
    assert p1 - opt <= bound, (float(p1 - opt), float(delta), D)
