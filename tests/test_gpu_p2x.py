"""The P2 exchange step's device code (csrc/sw_p2x_dev.h) against its
sequential specification (oracle/p2x_twin.c), bit for bit, through the probe
kernels of tests/native/p2x_probe.hip — on the graphs and placements of
tests/test_p2x.py (which holds the specification to a plain reference), not on
what the placement cascade leaves:

  * p2x_find_cycle on every graph of the CPU module, cold and warm: length,
    cycle and all T + 1 distances (rings of 64 and 65 nodes at T = 64 included);
  * the set-up and one full edge build: W, Wk and δ;
  * sw_p2x_block<SW_WAVES, 1> (the batch kernel's instantiation) and
    <SW_WAVES, 8> (the sharded engine's): masks and the cancel count;
  * a batch mixing shapes equals the single launches; the skip cases come back
    byte-identical.
Each comparison is one launch per group of cases.
"""
import numpy as np
import pytest

import p2x_ref as pr
import p2xcases as pc
from test_p2x import GRAPHS, RANDOM, SENTINEL, SHAPES, SINGLE, SKIPPED, TIES, run

pytestmark = pytest.mark.gpu


def assert_same_cycles(graphs, dws, what):
    got = pr.probe_find_cycle(graphs, dws)
    for i, g in enumerate(graphs):
        n, cyc, d = pr.twin_find_cycle(g[0], g[1], g[2], g[3], None if dws is None else dws[i])
        assert (got[i][0], got[i][1]) == (n, cyc), (what, i, g[0], got[i][:2], (n, cyc))
        assert got[i][2].tobytes() == d.tobytes(), (what, i, g[0])


def cold_distances(graphs):
    return [pr.twin_find_cycle(*g)[2] for g in graphs]


def test_gpu_find_cycle_random_graphs_cold_and_warm():
    cold = [g for g, _ in GRAPHS]
    assert_same_cycles(cold, None, "cold")
    # warm: the perturbed graph from the distances the cold run left
    assert_same_cycles([g2 for _, g2 in GRAPHS], cold_distances(cold), "warm")


def test_gpu_find_cycle_rings_and_ties():
    graphs = [pc.ring(T, v, cost) for T in pc.GRAPH_T for v in (False, True) for cost in (-1.0, 0.0, -0.0)]
    graphs += [TIES[k] for k in sorted(TIES)]
    assert_same_cycles(graphs, None, "cold")
    assert_same_cycles(graphs, cold_distances(graphs), "warm")
    got = pr.probe_find_cycle([pc.ring(64), pc.ring(64, through_v=True)])
    assert got[0][0] == 64 and got[1][0] == 65


@pytest.mark.parametrize("emax", [1, 8])
def test_gpu_edges_equal_twin(emax):
    cases = [(n, SHAPES[n], F) for n in sorted(SHAPES) for F in sorted(set(SHAPES[n]["w"]))]
    cases += [("sentinel", SENTINEL, F) for F in sorted(set(SENTINEL["w"]))]
    got = pr.probe_edges([P for _, P, _ in cases], [F for _, _, F in cases], emax)
    for (name, P, F), (W, Wk, delta) in zip(cases, got):
        tW, tWk, tdelta = pr.twin_edges(P["T"], P["G"], P["job"], P["w"], P["c"], P["m"], F)
        assert np.float64(delta).tobytes() == np.float64(tdelta).tobytes(), (name, F, delta, tdelta)
        if name in SKIPPED:
            assert delta == -1.0 and np.all(np.isnan(W)) and np.all(Wk == -9), name
            continue
        assert np.array_equal(Wk, tWk), (name, F, np.argwhere(Wk != tWk)[:4])
        assert W.tobytes() == tW.tobytes(), (name, F, np.argwhere(W != tW)[:4])


RUN_CASES = ([(n, SHAPES[n]) for n in sorted(SHAPES)] + [("sentinel", SENTINEL)]
             + [(f"random{i}", P) for i, P in enumerate(RANDOM)] + [(f"single{i}", P) for i, P in enumerate(SINGLE)])


@pytest.mark.parametrize("emax", [1, 8])
def test_gpu_run_equals_twin(emax):
    got = pr.probe_run([P for _, P in RUN_CASES], emax)
    for (name, P), (masks, nc) in zip(RUN_CASES, got):
        tm, tnc = run(P)
        assert nc == tnc, (name, nc, tnc)
        assert masks == tm, (name, sum(a != b for a, b in zip(masks, tm)))


@pytest.mark.parametrize("emax", [1, 8])
def test_gpu_mixed_batch_equals_single_launches(emax):
    names = ["T64_M129", "A1_T8", "A513_T8", "T2_M64", "nine_classes_T10", "A1025_T8", "w1248_T64", "c_wide",
             "T33_M65", "A4097_T8", "w2_255_T6", "T3_M1"]
    batch = pr.probe_run([SHAPES[n] for n in names], emax)
    for n, b in zip(names, batch):
        assert pr.probe_run([SHAPES[n]], emax)[0] == b, n


@pytest.mark.parametrize("emax", [1, 8])
def test_gpu_skip_cases_come_back_untouched(emax):
    skips = pc.skip_cases()
    names = sorted(skips)
    # between placements that do cancel, so a skipped workgroup sits beside working ones
    batch = [SHAPES["c_equal"]] + [skips[n] for n in names] + [SHAPES["c_equal"]]
    got = pr.probe_run(batch, emax)
    assert got[0][1] > 0 and got[0] == got[-1]
    for n, (masks, nc) in zip(names, got[1:-1]):
        want = np.array([int(x) for x in skips[n]["m"]], dtype=np.uint64)
        assert nc == 0 and np.array(masks, dtype=np.uint64).tobytes() == want.tobytes(), n
