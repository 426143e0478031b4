"""The level search's reused counts (csrc/sw_kernels.hip, Ctx::select_level and
Ctx::level_search on the on-chip path) against the CPU twin, on the shapes
where reuse can go wrong.

What the kernel reuses: the tie group takes its counts from the price
bisection's per-job windows (ca, cb) and searches the rows again only when the
bisection never ran; the first windows of an instance come from lo = 0 and
hi = +inf without a search.  The twin does none of this, so bit-equal results
(assert_same_result, `iters` among them) hold the reuse to the plain searches.

Kinds of instance (make_problem), each at T ∈ {1, 2, 31, 32}, N ∈ {1, 65, 512,
1024} (one and two jobs per thread, a partial wave) and k ∈ {0, 1e-3, 10, 1e5}:

  groups  widths up to 8 on G = 4 (a job wider than G has T_j = 0), epoch
          counts from three values with equal priorities and durations, so
          whole groups of jobs share a key row and neighbouring levels share
          ρ* — at k = 1e-3 the branch-and-bound probes between neighbouring
          prices are where the price loop can be entered with plo == phi (the
          tie group's fallback searches).  Jobs 64–127 (N = 512) and 128–255
          (N = 1024) are one wave's jobs and identical, beside waves of
          distinct jobs that stay open.
  flat    job 0 is finished (F == E, cap = 0) with the largest R: its g row is
          flat and above every other, so lb == top and the M_lo loop never
          runs: the first evaluation is at M_lo == top with nothing forced
          and the widest bracket, lo = 0 and hi = +inf, both windows unsearched.
  ample   G = Σ w: every round of every job fits (Wall ≤ bud, no price search
          at any level), M_lo is the lower bound lb, and the job that sets it
          has every round forced (g(T_j − 1) > M_lo: lforce_g's early exit), so
          the windows that come from lo = 0 start at T_j − l = 0 for it.
  ties    four jobs in five are alike (width 2, one key row) and the budget
          G·T cuts the group of their equal keys: ca − cb is one key of
          every such job.  G is odd, so at odd T one GPU-round is left that no
          tied job fits, and the width tail gives it to one of the width-1
          jobs, whose keys are a thousand times lower.

The CPU part shows from the twin's rows (twin_job_rows) and a restatement of
M_lo that flat, ample and ties take their paths.  Not shown on the CPU, since
the twin exposes neither its brackets nor its probes: that a solve enters the
price loop with plo == phi, that a whole wave's windows close while another
stays open, and Wf > C — level_search only evaluates levels ≥ M_lo, where
the M_lo search's own invariant gives Wf ≤ C, so that branch is not reachable
from it; the `groups` instances are built for the first two.
"""
import ctypes

import numpy as np
import pytest

import sw_native as sn
from helpers import assert_same_result, check_plan_valid

TS = (1, 2, 31, 32)
NS = (1, 65, 512, 1024)
KS = (0.0, 1e-3, 10.0, 1e5)
KINDS = ("groups", "flat", "ample", "ties")
SHAPES = [(kind, T, N, k) for kind in KINDS for T in TS for N in NS for k in KS]
EXTRA = 8  # second copies in the batch: 256 shapes + 8 > 256 instances


def make_problem(kind, T, N, k):
    rng = np.random.default_rng(100000 * KINDS.index(kind) + 1000 * T + N)
    G = 4
    w = rng.choice(np.array([1, 1, 1, 2, 2, 4, 8], dtype=np.int32), size=N)
    E = rng.choice(np.array([5, 20, 200], dtype=np.int32), size=N)
    F = np.zeros(N, dtype=np.int32)
    d = np.full(N, 60.0)
    p = np.ones(N)
    if kind == "groups":
        # every other job distinct, so that waves without the identical block stay open
        odd = np.arange(N) % 2 == 1
        E = np.where(odd, rng.integers(1, 201, size=N), E).astype(np.int32)
        F = np.where(odd, np.floor(rng.uniform(0.0, 1.0, size=N) * E), 0).astype(np.int32)
        d = np.where(odd, np.round(rng.uniform(20.0, 60.0, size=N)), d)
        p = np.where(odd, np.exp(rng.normal(0.0, 1.0, size=N)), p)
        E[w > G] = 20  # the jobs that never run stay below the levels that are searched
        F[w > G] = 0
        blk = {512: slice(64, 128), 1024: slice(128, 256)}.get(N)
        if blk is not None:
            w[blk], E[blk], F[blk], d[blk], p[blk] = 1, 150, 0, 60.0, 1.0
    if kind == "ample":
        G = int(w.sum())
    if kind == "ties":
        cheap = np.arange(N) % 5 == 4
        w = np.where(cheap, 1, 2).astype(np.int32)
        p = np.where(cheap, 1e-3, 1.0)
        E[:] = 200
        G = max(5, N // 3) | 1
    R = (E - F) * d
    if kind == "flat":
        F[0] = E[0]
        R[0] = 1e6
    return sn.ProblemArrays(w, d, F, E, R, p, T, G, 120.0, k)


def job_rows(a):
    """g[j][n] (n ≤ T) and key[j][n] (n < T) as the twin builds them."""
    import conftest

    lib = ctypes.CDLL(conftest.TWIN_SO)
    f = np.zeros((a.N, a.T + 1))
    g = np.zeros((a.N, a.T + 1))
    key = np.zeros((a.N, a.T), dtype=np.float32)
    pr = a.c_problem()
    dp = ctypes.POINTER(ctypes.c_double)
    rc = lib.twin_job_rows(ctypes.byref(pr), f.ctypes.data_as(dp), g.ctypes.data_as(dp),
                           key.ctypes.data_as(ctypes.POINTER(ctypes.c_float)))
    assert rc == 0
    return g, key


def m_lo(a, g):
    """(lb, top, M_lo): M_lo is the lowest level in [lb, top], among lb and the
    rows' values, whose forced rounds Σ w_j · #{n < T_j : g_j(n) > M} fit G·T."""
    ok = a.w <= a.G
    Tj = np.where(ok, a.T, 0)
    lb = max(g[j, Tj[j]] for j in range(a.N))
    top = g[:, 0].max()
    live = g[ok, :a.T]
    for M in sorted({lb, *live[(live >= lb)].tolist()}):
        if int((a.w[ok, None] * (live > M)).sum()) <= a.G * a.T:
            return lb, top, M
    raise AssertionError("no feasible level")


@pytest.fixture(scope="module")
def cases(twin):
    """(problem, twin result) per shape, solved once on the CPU."""
    out = {}
    for key in SHAPES:
        a = make_problem(*key)
        out[key] = (a, twin.solve(a))
    return out


def test_twin_accepts_every_shape(cases):
    assert len(cases) == len(SHAPES)
    for (kind, T, N, k), (a, rt) in cases.items():
        check_plan_valid(a, rt)
        assert rt["planned_rounds"].max() <= T
    # jobs wider than G are there and never planned
    a, rt = cases[("groups", 32, 1024, 10.0)]
    assert (a.w > a.G).any() and rt["planned_rounds"][a.w > a.G].max() == 0


def test_groups_hold_an_identical_wave(twin):
    for N, blk in ((512, slice(64, 128)), (1024, slice(128, 256))):
        a = make_problem("groups", 32, N, 1e-3)
        g, key = job_rows(a)
        assert (g[blk] == g[blk][0]).all() and (key[blk] == key[blk][0]).all()
        rest = np.delete(g, np.r_[blk], axis=0)
        assert len(np.unique(rest, axis=0)) > 64  # the other waves hold distinct rows
        # the M_lo loop has levels to search, the block's among them
        lb, top, M = m_lo(a, g)
        assert lb < M <= top and lb < g[blk][0][0] < top


def test_flat_instances_skip_the_m_lo_loop(twin):
    for T in TS:
        for N in NS:
            a = make_problem("flat", T, N, 10.0)
            g, _ = job_rows(a)
            lb, top, M = m_lo(a, g)
            assert lb == top == M == 1e6


def test_ample_instances_skip_the_price_search(twin):
    for T in TS:
        for N in NS:
            a = make_problem("ample", T, N, 10.0)
            assert (a.w <= a.G).all() and int(a.w.sum()) * a.T <= a.G * a.T  # Wall ≤ bud at every level
            g, _ = job_rows(a)
            lb, top, M = m_lo(a, g)
            assert M == lb
            if N > 1:  # the job that sets lb has its last live row value above M_lo
                assert lb < top and (g[:, a.T - 1] > M).any()
    # the early exit is taken somewhere: not every instance is flat at the end
    a = make_problem("ample", 2, 1024, 10.0)
    g, _ = job_rows(a)
    assert (g[:, 1] > m_lo(a, g)[2]).any()


def test_ties_instances_tie_at_the_price(twin):
    """k = 0: one evaluation at +inf with nothing forced; ρ* is the largest
    price at which the strictly dearer rounds fit the budget."""
    for T in TS:
        for N in (65, 512, 1024):
            a = make_problem("ties", T, N, 0.0)
            _, key = job_rows(a)
            alike = a.w == 2
            assert (key[alike] == key[0]).all() and key[~alike].max() < key[alike].min()
            C = a.G * a.T
            assert int(a.w.sum()) * T > C  # a price search is needed
            wk = np.repeat(a.w[:, None], T, axis=1)
            rho = min(r for r in np.unique(key) if int(wk[key > r].sum()) <= C)
            tied = int((key == rho).sum())
            rem = C - int(wk[key > rho].sum())
            assert tied >= alike.sum() >= 52  # one key of every job of the group ties
            assert 0 < rem < int(wk[key == rho].sum())  # the group is cut: job order decides
            assert rem % 2 == T % 2  # odd T: one GPU-round is left to the width tail


@pytest.mark.gpu
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("T", TS)
def test_gpu_single_solve_matches_twin(kind, T, cases, gpu_solver):
    for N in NS:
        for k in KS:
            a, rt = cases[(kind, T, N, k)]
            rg = gpu_solver.solve(a)
            check_plan_valid(a, rg)
            assert_same_result(rg, rt, f"{kind} T={T} N={N} k={k:g}")


@pytest.mark.gpu
def test_gpu_split_batch_matches_twin(cases, gpu_solver):
    keys = SHAPES + SHAPES[:EXTRA]
    batch = [make_problem(*key) for key in keys]
    assert len(batch) > 256 and max(a.N for a in batch) <= 1024 and max(a.T for a in batch) <= 32
    for key, a, rg in zip(keys, batch, gpu_solver.solve_batch(batch)):
        assert_same_result(rg, cases[key][1], f"batch {key}")
