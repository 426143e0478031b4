"""The size ladder of the sharded engine, on the CPU.

tests/shardcases.py holds instances chosen so that the GPU engine
(csrc/sw_shard.hip) takes every launch form its size dispatch has
(pack_share_any, pack_any, the merge's chunk loop, k_rr's knapsack limits).
Here the CPU shard engine (oracle/shard_twin.c) solves them: each result is a
valid schedule, meets the contract against the single-instance twin, is one
result at every world where the instance takes eight shares — and the record
of what each solve placed, mapped through `launch_forms`, covers every form
name.  tests/test_gpu_shard_ladder.py then holds the GPU engine to these
results bit for bit.
"""
import numpy as np
import pytest

import shardcases as sc
import sw_native as sn
from helpers import check_plan_valid
from test_shard import (P1_BITS, SHARE_P2_RATIO, assert_contract, assert_same_as_single, run_threads,  # noqa: F401
                        shard_lib)

_REF = {}


def reference(lib, case, world):
    """The CPU shard engine's result, record and form names of a case at a
    world: computed once per session, never modified."""
    key = (case[0], world)
    if key not in _REF:
        a = sc.build(case)
        r = run_threads(lib, a, world)
        rec = sc.read_record(lib)
        assert rec["dropped"] == 0, key
        _REF[key] = (a, r, rec, frozenset(sc.launch_forms(a.N, world, a.G, rec)))
    return _REF[key]


@pytest.mark.parametrize("case", sc.CASES, ids=sc.CASE_IDS)
def test_ladder_case_on_cpu(case, shard_lib, twin):
    a = sc.build(case)
    rt = twin.solve(a)
    v8 = sc.share_count(a.N, a.G, 1) == 8
    r1 = None
    for world in (1, 2, 4, 8) if v8 else (1, 2):
        rs = reference(shard_lib, case, world)[1] if world in sc.worlds(a) else run_threads(shard_lib, a, world)
        check_plan_valid(a, rs)
        if v8 and rt["p2_objective"] > 0 and rs["p2_objective"] > 0:
            print(f"{case[0]} W={world}: share P2 / single P2 = {rs['p2_objective'] / rt['p2_objective']:.6f}")
        if case[0] in sc.P2_ABOVE_BAR:  # P1 of the contract; P2 is the recorded finding
            assert (rs["status"] & P1_BITS) == (rt["status"] & P1_BITS), case[0]
            assert np.array_equal(rs["planned_rounds"], rt["planned_rounds"]), case[0]
            for key in ("objective", "utility", "makespan", "bound"):
                assert np.float64(rs[key]).tobytes() == np.float64(rt[key]).tobytes(), (case[0], key)
            ratio = rs["p2_objective"] / rt["p2_objective"]
            assert abs(ratio - sc.P2_ABOVE_BAR[case[0]]) < 5e-7, (case[0], ratio)
        else:
            assert_contract(rs, rt, world, f"{case[0]} W={world}", a.N, a.G)
        if v8:  # one result at every world
            r1 = r1 or rs
            assert_same_as_single(rs, r1, f"{case[0]} W={world} vs W=1")


def test_ladder_cases_cover_every_form(shard_lib):
    """The union of the form names over the cases, their worlds and the
    refusals is the whole name set: every branch of the size dispatch has a
    case that takes it (DESIGN.md §8 names the owner of each)."""
    got = set()
    for case in sc.CASES:
        for world in sc.worlds(sc.build(case)):
            got |= reference(shard_lib, case, world)[3]
    for name, case, world, _ in sc.REFUSALS:
        if name.startswith("eval"):
            continue  # refused before any placement; the CPU engine has nothing to record
        got |= reference(shard_lib, (name,) + case[1:], world)[3]
    assert got == sc.ALL_FORMS, (sorted(sc.ALL_FORMS - got), sorted(got - sc.ALL_FORMS))


def test_refusal_instances_solve_on_the_cpu_engine(shard_lib):
    """The placement refusals are limits of the GPU engine alone: the CPU
    engine solves the same instances, and its record names the form that
    refuses."""
    want = {"share_N32769_G511": "S5/refused", "gathered_N32769_G515": "G7/refused"}
    for name, case, world, _ in sc.REFUSALS:
        if name not in want:
            continue
        a, rs, _, forms = reference(shard_lib, (name,) + case[1:], world)
        check_plan_valid(a, rs)
        assert want[name] in forms, (name, sorted(forms))


def test_eval_refusal_size():
    name, case, _, _ = [r for r in sc.REFUSALS if r[0].startswith("eval")][0]
    assert sc.sizes(case[2]["N"], 1, 511)["q"] == 257 and sc.sizes(131072, 1, 511)["q"] == 256


# ---- launch_forms on hand-made records, at every boundary of the tables ------

def _rec(shares=(), packs=(), local=(), **rr):
    base = dict.fromkeys(sc.RR_KEYS, 0)
    base.update(rr)
    return dict(dropped=0, reround_calls=0, rr=base, p2x_runs=0, p2x_jobs=0,
                shares=[dict(V=V, nsub=nsub, exist=ex, A=[(0, x) for x in A]) for V, nsub, ex, A in shares],
                packs=[dict(mode=1, M=M, A=A) for M, A in packs],
                share_class_packs=[dict(width=1, jobs=0, A=A) for A in local])


SHARE_TABLE = [
    # N (G = 511, world 1: one share of 512·⌈N/512⌉ entries), A, form
    (4096, 0, "S1/wave"), (4096, 512, "S1/wave"), (4096, 513, "S1/body2"), (4096, 1024, "S1/body2"),
    (4096, 1025, "S1/body4"), (4096, 2048, "S1/body4"), (4096, 2049, "S1/body8"), (4096, 4096, "S1/body8"),
    (4097, 512, "S2/wave"), (4097, 513, "S2/body2"), (4097, 1024, "S2/body2"), (4097, 1025, "S2/body4"),
    (4097, 2048, "S2/body4"), (4097, 2049, "S2/body8"), (4097, 4096, "S2/body8"), (4097, 4097, "S2/body20"),
    (10240, 10240, "S2/body20"),
    (10241, 512, "S3/wave"), (10241, 513, "S3/sel2"), (10241, 1025, "S3/sel4"), (10241, 2049, "S3/sel8"),
    (10241, 4096, "S3/sel8"), (10241, 4097, "S3/rounds32"), (16384, 16384, "S3/rounds32"),
    (16385, 512, "S4/wave"), (16385, 513, "S4/sel2"), (16385, 1025, "S4/sel4"), (16385, 2049, "S4/sel8"),
    (16385, 4096, "S4/sel8"), (16385, 4097, "S4/rounds64"), (32768, 32768, "S4/rounds64"),
    (32769, 100, "S5/refused"),
]


@pytest.mark.parametrize("N,A,form", SHARE_TABLE)
def test_launch_forms_share_table(N, A, form):
    got = sc.launch_forms(N, 1, 511, _rec(shares=[(1, 1, 1, [A])]))
    assert form in got and {f for f in got if f[0] == "S"} == {form}, got
    assert ("merge>64" in got) == (16384 < N <= 32768), got


GATHERED_TABLE = [
    (512, 512, "G1/wave"), (513, 512, "G2/wave"), (513, 513, "G2/body2"), (2048, 1025, "G2/body4"),
    (2048, 2048, "G2/body4"), (2049, 0, "G3/body2"), (2049, 1024, "G3/body2"), (2049, 1025, "G3/body4"),
    (4096, 2049, "G3/body8"), (4096, 4096, "G3/body8"), (4097, 1024, "G4/body2"), (4097, 2048, "G4/body4"),
    (4097, 4096, "G4/body8"), (4097, 4097, "G4/body20"), (10240, 10240, "G4/body20"),
    (10241, 1024, "G5/sel2"), (10241, 2048, "G5/sel4"), (10241, 4096, "G5/sel8"), (10241, 4097, "G5/rounds32"),
    (16384, 16384, "G5/rounds32"), (16385, 1024, "G6/sel2"), (16385, 2048, "G6/sel4"),
    (16385, 4096, "G6/sel8"), (16385, 4097, "G6/rounds64"), (32768, 32768, "G6/rounds64"),
    (32769, 5, "G7/refused"),
]


@pytest.mark.parametrize("N,A,form", GATHERED_TABLE)
def test_launch_forms_gathered_table(N, A, form):
    M = sc.sizes(N, 1, 511)["M"]
    got = sc.launch_forms(N, 1, 511, _rec(packs=[(M, A)]))
    assert got - {"merge>64"} == {form}, got
    assert ("merge>64" in got) == (16384 < M <= 32768), got


def test_launch_forms_sizes_and_shares():
    z = sc.sizes(10000, 1, 2848)  # C4: eight shares of 64·20 → 1,280 entries on one rank
    assert (z["V"], z["nsub"], z["Mg"], z["M"]) == (8, 8, 1280, 10240)
    z = sc.sizes(65536, 1, 8192)
    assert (z["V"], z["nsub"], z["Mg"], z["M"]) == (8, 8, 8192, 65536)
    assert sc.sizes(65536, 8, 8192)["Mg"] == 8192 and sc.sizes(65536, 8, 8192)["nsub"] == 1
    assert sc.sizes(65537, 1, 8192)["V"] == 1 and sc.sizes(4095, 1, 8192)["V"] == 1
    assert sc.sizes(4096, 2, 511)["V"] == 2 and sc.sizes(4096, 2, 512)["V"] == 8
    # eight shares above 4,096 entries each: the separate launches, one workgroup per share
    got = sc.launch_forms(40000, 1, 4096, _rec(shares=[(8, 8, 1, [400, 600, 1100, 2100, 4097, 5056, 1, 0])]))
    assert got == {"S2/wave", "S2/body2", "S2/body4", "S2/body8", "S2/body20", "S2/nsub>1"}, got
    # shares that do not exist (sw_share_caps refused) place nothing
    assert sc.launch_forms(3000, 1, 100, _rec(shares=[(1, 1, 0, [3000])])) == set()
    # a class repack inside a share: this rank's P entries
    assert sc.launch_forms(40000, 1, 4096, _rec(shares=[(8, 8, 1, [9] * 8)], local=[700])) == \
        {"S2/wave", "S2/nsub>1", "repair>32768"}
    assert "G6/sel2" in sc.launch_forms(40000, 2, 4096, _rec(shares=[(8, 4, 1, [9] * 4)], local=[700]))
    got = sc.launch_forms(2000, 1, 100, _rec(words2=1, cap512=2, refused_words=1, refused_budget=3,
                                             refused_capmax=1))
    assert got == {"rr/words>=2", "rr/cap>=512", "rr/refused-words", "rr/refused-budget", "rr/refused-capmax"}


def test_record_is_per_solve(shard_lib):
    """A solve's record starts empty: a small instance after a large one."""
    reference(shard_lib, sc.CASES[0], 1)
    a = sc.build(("x", "short", dict(seed=5, N=300, k=1e5)))
    run_threads(shard_lib, a, 1)
    rec = sc.read_record(shard_lib)
    assert [s["A"] for s in rec["shares"]] == [[(300, int((np.asarray(a.w) <= a.G).sum()))]]
    assert rec["packs"] == [] and rec["p2x_runs"] == 1 and rec["p2x_jobs"] == 300
