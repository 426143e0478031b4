"""The placement's round loop on the device (csrc/sw_pack.h) against its
sequential specification (pack() of oracle/plan_twin.c, which tests/test_pack.py
holds to a plain reference), bit for bit on round masks and residual rounds,
through the probe kernels of tests/native/pack_probe.hip — every compiled form
at every size it can hold, not only where a plan solve selects it:

  * sw_pack_rounds<E>, E = 2, 4, 8, 20, 32, 64, at A = 1, 63, 64, 65, E·64 ∓ 1
    (where a position's prefix first crosses a wave), E·512 − 1 and E·512;
  * sw_pack_rounds_wave<E1>, E1 = 2, 4, 6, 8, 16, 32, 64, at A = 1, E1, E1 + 1,
    64·E1 − 1 and 64·E1;
  * sw_pack_rounds_one<true> and <false> at its selector's bounds;
  each in the three capacity kinds, with one T = 64 case, and on the random
  and edge cases of tests/test_pack.py (every one that fits the form), the
  unit-flag cases among them;
  * all forms agree on cases several of them can hold (E = 64 on A = 65,
    E1 = 64 on A = 3 included);
  * sw_pack_room with the row's cbase and with cbase = −1 against "the x
    smallest later capacities" for every t and m, on rows of spread 0, 1, 2
    and large: the shortcut, the sort, and both where both apply;
  * the wave primitives (bitonic sort, scans, sum, min, max) and the block
    primitives (exscan, sum32, min32, each on both slot sets) against numpy;
  * a batch mixing shapes equals the single launches.
Each comparison is one launch per group of cases.
"""
import functools

import numpy as np
import pytest

import pack_ref as pr
import packcases as pc
from test_pack import EDGE, RANDOM

pytestmark = pytest.mark.gpu

_TWIN = {}


def twin(P):
    """The twin's (masks, residual r) on a position case, once per case."""
    k = id(P)
    if k not in _TWIN:
        _TWIN[k] = pr.twin_positions(P)
    return _TWIN[k]


@functools.lru_cache(maxsize=None)
def shared():
    """The CPU module's random and edge cases as position cases (A ≤ 200)."""
    return [pr.positions(c) for c in RANDOM + EDGE]


@functools.lru_cache(maxsize=None)
def block_cases(E):
    return pc.size_cases(pc.block_sizes(E), f"block{E}", seed=100 + E)


@functools.lru_cache(maxsize=None)
def wave_cases(E1):
    return pc.size_cases(pc.wave_sizes(E1), f"wave{E1}", seed=200 + E1)


@functools.lru_cache(maxsize=None)
def one_cases():
    return pc.size_cases(pc.ONE_A, "one", seed=300)


def assert_equals_twin(got, cases, what):
    assert len(got) == len(cases)
    for P, (mk, r) in zip(cases, got):
        tm, tr = twin(P)
        assert np.array_equal(r, tr), (what, P["name"], len(tr), np.flatnonzero(r != tr)[:4])
        assert mk.tobytes() == tm.tobytes(), (what, P["name"], len(tm), np.flatnonzero(mk != tm)[:4])


def fitting(cases, amax):
    return [P for P in cases if len(P["r"]) <= amax]


def test_size_lists_are_what_the_forms_need():
    for E in pc.BLOCK_E:
        sizes = {len(P["r"]) for P in block_cases(E)}
        assert {1, 63, 64, 65, E * 64 - 1, E * 64 + 1, E * 512 - 1, E * 512} == sizes
        assert sum(P["T"] == 64 for P in block_cases(E)) == 1
        for ck in ("none", "base", "free"):
            assert sum(P["name"].endswith(ck) for P in block_cases(E)) == 8
    for E1 in pc.WAVE_E1:
        assert {1, E1, E1 + 1, 64 * E1 - 1, 64 * E1} == {len(P["r"]) for P in wave_cases(E1)}
    assert {len(P["r"]) for P in one_cases()} == set(pc.ONE_A)
    assert any(P["unit"] for P in shared()) and max(len(P["r"]) for P in shared()) <= 200
    # the large cases leave late positions something to do: the last wave's positions are placed somewhere
    P = max(block_cases(64), key=lambda P: len(P["r"]))
    assert twin(P)[0][-64:].any()


@pytest.mark.parametrize("E", pc.BLOCK_E)
def test_gpu_block_loop_equals_twin(E):
    cases = block_cases(E) + shared()
    assert_equals_twin(pr.probe_block(E, cases), cases, f"block E={E}")


@pytest.mark.parametrize("E1", pc.WAVE_E1)
def test_gpu_wave_loop_equals_twin(E1):
    cases = wave_cases(E1) + fitting(shared(), 64 * E1)
    assert len(cases) > len(wave_cases(E1)) + 100
    assert_equals_twin(pr.probe_wave(E1, cases), cases, f"wave E1={E1}")


@pytest.mark.parametrize("multi", [True, False])
def test_gpu_one_position_per_thread_equals_twin(multi):
    cases = one_cases() + shared()
    assert_equals_twin(pr.probe_one(multi, cases), cases, f"one multi={multi}")


def test_gpu_every_form_gives_the_same_result():
    rng = np.random.default_rng(41)
    cases = [pc.position_case(rng, A, T, ck, f"forms_A{A}_{ck}")
             for A, T in ((3, 7), (65, 12), (128, 9)) for ck in pc.CAP_KINDS]
    first = pr.probe_block(64, cases)
    assert_equals_twin(first, cases, "block E=64")
    runs = [(f"block E={E}", pr.probe_block(E, cases)) for E in pc.BLOCK_E[:-1]]
    runs += [(f"wave E1={E1}", pr.probe_wave(E1, cases)) for E1 in pc.WAVE_E1]
    runs += [(f"one multi={m}", pr.probe_one(m, cases)) for m in (True, False)]
    for what, got in runs:
        for P, a, b in zip(cases, first, got):
            assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes(), (what, P["name"])


def want_room(P):
    """(room[t][m] for m < T − t from the definition, cbase as defined)."""
    T, caps = P["T"], P["caps"]
    room = [[pr.ref_room(T, P["G"], caps, t, T - t - 1 - m) for m in range(T - t)] for t in range(T)]
    cbase = min(caps) if caps is not None and T > 0 and max(caps) - min(caps) <= 1 else -1
    return room, cbase


def test_gpu_room_shortcut_and_sort_equal_the_definition():
    rows = pc.room_rows() + [P for P in shared() if P["caps"] is not None]
    got = pr.probe_room(rows)
    short = sort = 0
    for P, (ra, rb, cb) in zip(rows, got):
        room, cbase = want_room(P)
        assert cb == cbase, (P["name"], cb, cbase)
        short += cbase >= 0
        sort += P["caps"] is not None and cbase < 0
        for t in range(P["T"]):
            R = P["T"] - t
            assert ra[t, :R].tolist() == room[t], (P["name"], "cbase", t)
            assert rb[t, :R].tolist() == room[t], (P["name"], "sort", t)
    assert short >= 30 and sort >= 30, (short, sort)


def test_gpu_wave_and_block_primitives_equal_numpy():
    rng = np.random.default_rng(42)
    I32 = np.iinfo(np.int32)
    vs = [rng.integers(I32.min + 1, I32.max, size=64, endpoint=True) for _ in range(24)]   # min's domain: > INT32_MIN
    vs += [rng.integers(-5, 6, size=64) for _ in range(8)]                 # many equal values
    vs += [np.sort(v) for v in vs[:4]] + [np.sort(v)[::-1] for v in vs[4:8]]
    vs += [np.full(64, x) for x in (0, 7, -7, I32.max, I32.min + 1)]
    for k in (0, 1, 2, 31, 62, 63):   # k capacities, INT32_MAX padding above: what sw_pack_room sorts
        v = np.full(64, I32.max)
        v[:k] = rng.integers(0, 1 << 20, size=k)
        vs.append(v)
    vs.append(np.where(np.arange(64) % 2 == 0, I32.max, I32.min + 1))
    vs = np.array(vs, dtype=np.int32)
    va = rng.integers(-(1 << 24), 1 << 24, size=vs.shape).astype(np.int32)   # sums inside 32 bits
    va[0], va[1], va[2] = 0, 1, np.arange(64)
    va[3] = rng.integers(0, 256, size=64)   # widths
    ba = rng.integers(-(1 << 21), 1 << 21, size=(6, 512)).astype(np.int32)
    bb = rng.integers(-(1 << 21), 1 << 21, size=(6, 512)).astype(np.int32)
    ba[0], bb[0] = 0, 1
    ba[1], bb[1] = np.arange(512), np.arange(512)[::-1]
    ba[2] = rng.integers(0, 256 * 64, size=512)   # 64 widths per thread
    bb[2] = 0x7FFFFFFF                               # the width tail's "nothing fits"
    bb[2, 447] = 5
    bb[3, 511], ba[3, 0] = -(1 << 21) - 1, -(1 << 21) - 1   # the minimum in the last / first thread
    got = pr.probe_prims(vs, va, ba, bb)
    one = np.ones((1, 64), dtype=np.int32)
    assert np.array_equal(got["sort"], np.sort(vs, axis=1))
    assert np.array_equal(got["min"], vs.min(axis=1, keepdims=True) * one)
    assert np.array_equal(got["max"], vs.max(axis=1, keepdims=True) * one)
    assert np.array_equal(got["incscan"], np.cumsum(va, axis=1, dtype=np.int32))
    assert np.array_equal(got["sufscan"], np.cumsum(va[:, ::-1], axis=1, dtype=np.int32)[:, ::-1])
    assert np.array_equal(got["sum"], va.sum(axis=1, keepdims=True, dtype=np.int32) * one)
    ones = np.ones((1, 512), dtype=np.int32)
    for k, v in (("a", ba), ("b", bb)):
        v64 = v.astype(np.int64)
        assert np.array_equal(got[f"min_{k}"], v.min(axis=1, keepdims=True) * ones), k
        fits = np.abs(v64).sum(axis=1) < 1 << 31   # row 2 of b is the tail's sentinel: a minimum's input, not a sum's
        assert fits.sum() == len(v) - (k == "b")
        assert np.array_equal(got[f"exscan_{k}"][fits], (np.cumsum(v64, axis=1) - v64)[fits]), k
        assert np.array_equal(got[f"total_{k}"][fits], (v64.sum(axis=1, keepdims=True) * ones)[fits]), k
        assert np.array_equal(got[f"sum_{k}"][fits], (v64.sum(axis=1, keepdims=True) * ones)[fits]), k


@pytest.mark.parametrize("form", ["block8", "wave8", "one"])
def test_gpu_mixed_batch_equals_single_launches(form):
    run = {"block8": lambda cs: pr.probe_block(8, cs), "wave8": lambda cs: pr.probe_wave(8, cs),
           "one": lambda cs: pr.probe_one(True, cs)}[form]
    by_name = {P["name"]: P for P in one_cases() + shared()}
    names = ["one_A512_free", "A0", "one_A1_none", "T64_n64", "one_A385_base", "caps_T64_sorted_all", "T1",
             "one_A129_none", "unit_flag", "one_A257_T64", "w255", "one_A257_free"]
    batch = run([by_name[n] for n in names])
    for n, b in zip(names, batch):
        a = run([by_name[n]])[0]
        assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes(), n
