"""The exchange step's set-up with a candidate rank order (csrc/sw_p2x_dev.h,
csrc/sw_p2x_rank.h) through the probe kernels of tests/native/p2x_rank_probe.hip.

On placements at the sizes where the code takes another path — A = 1, 2, 63,
64, 65, 511, 512, classes of 64 and 65 members, K = 1, 8 and 9, widths 3, 5, 6
and 7, T = 2, 30 and 32, all-equal c, near ties, a job table that does not fit
the scratch:

  * the set-up run with and without a candidate gives bit-equal class header,
    ord, pc, rank bitsets, room and δ;
  * the whole step with a candidate equals the twin in masks, cancel count
    and P2;
  * the probe's report of whether the candidate gave the order equals the
    Python restatement's prediction (tests/p2x_rank_ref.py): taken for the
    density order, not taken for near ties, for a reversed candidate and for
    one with two neighbours swapped — the check guards the result.
K = 9 comes back untouched.  One launch per group of cases.
"""
import numpy as np
import pytest

import p2x_rank_ref as rr
import p2x_ref as pr
import p2xcases as pc

pytestmark = pytest.mark.gpu


def near_tie_c(rng, A):
    """Pairs (2i, 2i + 1) equal above the 11 lowest mantissa bits and different
    in bits 3 … 10, the later job the larger."""
    c = rng.uniform(0.5, 4.0, size=A)
    b = c.view(np.uint64).copy()
    for i in range(0, A - 1, 2):
        b[i] &= ~np.uint64(0x7FF)
        b[i + 1] = b[i] | np.uint64(8 << int(rng.integers(0, 8)))
    return [float(x) for x in b.view(np.float64)]


def build_cases():
    rng = np.random.default_rng(41)
    out = {}

    def add(name, T, w, cdist="uniform", job_step=1, tie=False):
        G = max(max(w), int(np.ceil(sum(w) * 1.5 / T)))
        P = pc.placement(rng, T, w, G, "uniform" if tie else cdist, job_step=job_step)
        if tie:
            P = dict(P, c=near_tie_c(rng, len(w)))
        out[name] = pc.shuffle_rounds(rng, P, min(2 * len(w), 200))

    mix = lambda A: [int(x) for x in rng.choice(np.array([1, 1, 1, 2, 4]), size=A)]  # noqa: E731
    for A in (1, 2, 63, 64, 65):
        add(f"A{A}_T8", 8, [1] * A, "ratio")
    for A in (63, 65, 511, 512):
        add(f"A{A}_mix_T30", 30, mix(A))
    add("A512_w1_T32", 32, [1] * 512, "few")
    add("class64_65_T30", 30, pc.widths_of({1: 64, 2: 65}))
    add("K8_T30", 30, pc.widths_of({x: 12 for x in pc.WIDTH_SETS["eight"]}))
    add("w3567_T30", 30, pc.widths_of({3: 30, 5: 20, 6: 12, 7: 9}), "ratio")
    add("equal_c_T30", 30, pc.widths_of({1: 70, 2: 40, 4: 20}), "equal")
    add("few_c_T2", 2, pc.widths_of({1: 90, 2: 37}), "few")
    add("A2_T2", 2, [1, 1])
    add("near_tie_T30", 30, [1] * 130, tie=True)
    add("near_tie_T8", 8, [1] * 64, tie=True)
    add("table_too_large_T2", 2, [1] * 500, "ratio", job_step=3)
    add("job_step3_T32", 32, mix(200), job_step=3)
    return out


CASES = build_cases()
NINE = pc.shape_cases()["nine_classes_T10"]
NAMES = sorted(CASES)


def njobs_of(P):
    return max(P["job"]) + 1


def swapped(P, cand):
    """cand with the first two neighbours of one class swapped (None: no such pair)."""
    wof = dict(zip(P["job"], P["w"]))
    for q in range(len(cand) - 1):
        if wof[cand[q]] == wof[cand[q + 1]]:
            return cand[:q] + [cand[q + 1], cand[q]] + cand[q + 2:]
    return None


def variants(P):
    dens = rr.density_order(P)
    v = {"none": None, "density": dens, "reversed": dens[::-1], "short": dens[:-1]}
    if swapped(P, dens) is not None:
        v["swapped"] = swapped(P, dens)
    if len(dens) >= 2:
        v["repeated"] = dens[:-1] + [dens[0]]
    return v


@pytest.fixture(scope="module")
def setups():
    """{(case, variant): (prediction, probe result)}, one launch."""
    keys, Ps, cands = [], [], []
    for n in NAMES:
        for vn, cd in variants(CASES[n]).items():
            keys.append((n, vn))
            Ps.append(CASES[n])
            cands.append(cd)
    got = rr.probe_setup(Ps, cands, [njobs_of(P) for P in Ps])
    return {k: (rr.predict_ranked(P, cd, njobs_of(P)), g) for k, P, cd, g in zip(keys, Ps, cands, got)}


def test_cases_cover_the_paths(setups):
    pred = {k: v[0] for k, v in setups.items()}
    for n in NAMES:
        assert pred[(n, "none")] == 0 and pred[(n, "short")] == 0
        if (n, "swapped") in pred:
            assert pred[(n, "swapped")] == 0, n
        if len(CASES[n]["job"]) >= 2:
            assert pred[(n, "repeated")] == 0, n
    ordinary = [n for n in NAMES if not n.startswith(("near_tie", "table_too_large"))]
    assert all(pred[(n, "density")] == 1 for n in ordinary), [n for n in ordinary if pred[(n, "density")] != 1]
    assert pred[("near_tie_T30", "density")] == 0 and pred[("near_tie_T8", "density")] == 0
    assert pred[("table_too_large_T2", "density")] == 0
    # reversed: refused wherever a class has two members
    assert all(pred[(n, "reversed")] == 0 for n in NAMES if len(CASES[n]["job"]) >= 2)
    assert pred[("A1_T8", "reversed")] == 1


def test_fast_path_taken_exactly_when_predicted(setups):
    for k, (want, g) in setups.items():
        assert g["ranked"] == want, (k, g["ranked"], want)


def test_setup_equal_with_and_without_candidate(setups):
    for (n, vn), (_, g) in setups.items():
        base = setups[(n, "none")][1]
        for f in ("hdr", "ord", "pc", "B", "room", "delta"):
            assert g[f].tobytes() == base[f].tobytes(), (n, vn, f)
    # and the set-up is the specification's: ord is the rank order
    for n in NAMES:
        P, g = CASES[n], setups[(n, "none")][1]
        assert [P["job"][a] for a in g["ord"]] == rr.rank_order(P), n
        assert g["hdr"][0] == len(set(P["w"])) and list(g["hdr"][1:1 + g["hdr"][0]]) == sorted(set(P["w"])), n


def test_run_with_candidate_equals_twin():
    keys, Ps, cands = [], [], []
    for n in NAMES:
        for vn in ("density", "reversed"):
            keys.append((n, vn))
            Ps.append(CASES[n])
            cands.append(variants(CASES[n])[vn])
    got = rr.probe_run(Ps, cands, [njobs_of(P) for P in Ps])
    twin = {n: pr.twin_run(CASES[n]["T"], CASES[n]["G"], CASES[n]["job"], CASES[n]["w"], CASES[n]["c"],
                           CASES[n]["m"]) for n in NAMES}
    for (n, vn), P, (masks, nc) in zip(keys, Ps, got):
        tm, tnc = twin[n]
        assert nc == tnc, (n, vn, nc, tnc)
        assert masks == tm, (n, vn, sum(a != b for a, b in zip(masks, tm)))
        assert pr.objective(P["c"], masks) == pr.objective(P["c"], tm), (n, vn)


def test_nine_classes_come_back_untouched():
    dens = rr.density_order(NINE)
    assert rr.predict_ranked(NINE, dens, njobs_of(NINE)) == -1
    g = rr.probe_setup([NINE], [dens], [njobs_of(NINE)])[0]
    assert g["ranked"] == -1 and np.all(g["hdr"] == -9) and np.all(g["ord"] == -9) and np.all(np.isnan(g["pc"]))
    masks, nc = rr.probe_run([CASES["K8_T30"], NINE, CASES["K8_T30"]], [None, dens, None],
                             [njobs_of(CASES["K8_T30"]), njobs_of(NINE), njobs_of(CASES["K8_T30"])])[1]
    assert nc == 0 and masks == [int(x) for x in NINE["m"]]
