"""The on-chip row searches (csrc/sw_rowsearch.h in Ctx's cnt / cnt_snap /
kbits) against the CPU twin, on the shapes where a search over a 32-key
register row can go wrong.

T ∈ {1, 2, 31, 32}: 32 is the only horizon where the row's last key is live
and a count of 32 can occur.  N ∈ {1, 2, 65, 513, 1024}: one and two jobs per
thread, partial last waves.  G = 4 with widths up to 8: a job wider than G has
an all-zero row.  Priorities and epoch durations are equal and the epoch counts
come from three values, so whole groups of jobs share a key row and many keys
tie at the price ρ*.  k ∈ {0, 1e-3, 10, 1e5}: k = 0 skips the levels, k = 1e-3
takes about 30 price probes per solve.

A single solve runs the full kernel (sw_plan_kernel); a batch of more than 256
instances runs the split kernels and so sw_level_kernel.
"""
import numpy as np
import pytest

import sw_native as sn
from helpers import assert_same_result, check_plan_valid

TS = (1, 2, 31, 32)
NS = (1, 2, 65, 513, 1024)
KS = (0.0, 1e-3, 10.0, 1e5)
G = 4
SHAPES = [(T, N, k) for T in TS for N in NS for k in KS]
COPIES = 4  # batch instances per shape: 80 shapes × 4 > 256


def make_problem(T, N, k, variant=0):
    rng = np.random.default_rng(1000 * T + N + variant)
    w = rng.choice(np.array([1, 1, 1, 2, 2, 4, 8], dtype=np.int32), size=N)
    E = rng.choice(np.array([5, 20, 200], dtype=np.int32), size=N)
    F = np.zeros(N, dtype=np.int32)
    d = np.full(N, 60.0)
    p = np.ones(N)
    if variant:
        # every other job distinct: many key values between the tied groups,
        # so the price search takes many probes
        odd = np.arange(N) % 2 == 1
        E = np.where(odd, rng.integers(1, 201, size=N), E).astype(np.int32)
        F = np.where(odd, np.floor(rng.uniform(0.0, 1.0, size=N) * E), 0).astype(np.int32)
        d = np.where(odd, np.round(rng.uniform(20.0, 400.0, size=N)), d)
        p = np.where(odd, np.exp(rng.normal(0.0, 1.0, size=N)), p)
    R = (E - F) * d
    return sn.ProblemArrays(w, d, F, E, R, p, T, G, 120.0, k)


@pytest.fixture(scope="module")
def cases(twin):
    """(problem, twin result) per shape and variant, solved once on the CPU —
    which also shows that the twin accepts every shape."""
    out = {}
    for T, N, k in SHAPES:
        for variant in (0, 1):
            a = make_problem(T, N, k, variant)
            out[(T, N, k, variant)] = (a, twin.solve(a))
    return out


def test_twin_accepts_every_shape(cases):
    assert len(cases) == 2 * len(SHAPES)
    for (T, N, k, _), (a, rt) in cases.items():
        check_plan_valid(a, rt)
        assert rt["planned_rounds"].max() <= T
    # the shapes do exercise the searches: some instance plans a full 32-round row
    assert any(rt["planned_rounds"].max() == 32 for (T, _, _, _), (_, rt) in cases.items() if T == 32)


@pytest.mark.gpu
@pytest.mark.parametrize("T", TS)
@pytest.mark.parametrize("N", NS)
def test_gpu_single_solve_matches_twin(T, N, cases, gpu_solver):
    for k in KS:
        for variant in (0, 1):
            a, rt = cases[(T, N, k, variant)]
            rg = gpu_solver.solve(a)
            check_plan_valid(a, rg)
            assert_same_result(rg, rt, f"T={T} N={N} k={k:g} variant {variant}")


@pytest.mark.gpu
def test_gpu_split_batch_matches_twin(cases, gpu_solver):
    keys = [(T, N, k, c & 1) for c in range(COPIES) for T, N, k in SHAPES]
    batch = [make_problem(*key) for key in keys]
    assert len(batch) > 256 and max(a.N for a in batch) <= 1024 and max(a.T for a in batch) <= 32
    for key, a, rg in zip(keys, batch, gpu_solver.solve_batch(batch)):
        assert_same_result(rg, cases[key][1], f"batch {key}")
