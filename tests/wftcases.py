"""TEST INFRASTRUCTURE for the water-filling MaxMinFairness call over worker
types that differ (sw_wf_allocate_types, csrc/sw_wf_types.h): the CPU twin
(tests/twins/wft_twin.c, built by csrc/Makefile into
shockwave-replication_amd/lib/libwft_twin.so) through ctypes, the seeded input
families of tests/test_wf_types.py and tests/test_gpu_wf_types.py, and the
references computed once and shared.  Only tests/ may import this module."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np

import wf_types_ref as ref

_HERE = os.path.dirname(os.path.abspath(__file__))
_CSRC = os.path.join(os.path.dirname(_HERE), "shockwave-replication_amd", "csrc")
_SO = os.path.join(os.path.dirname(_HERE), "shockwave-replication_amd", "lib", "libwft_twin.so")
_LIB = None

AMBIGUOUS_CAP = 0.02  # of a family's instances


def _lib():
    global _LIB
    if _LIB is None:
        if not os.path.exists(_SO):
            subprocess.check_call(["make", "-s", "-C", _CSRC, "../lib/libwft_twin.so"])
        lib = C.CDLL(_SO)
        dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int32)
        lib.wft_twin_allocate_stats.argtypes = [C.c_int32, C.c_int32, ip, ip, dp, dp, dp, dp, ip, dp, C.c_int32]
        lib.wft_twin_allocate_stats.restype = C.c_int
        for f in ("thresh", "gap_lo", "gap_hi"):
            getattr(lib, "wft_twin_" + f).restype = C.c_double
        for f in ("max_jobs", "max_types", "flag_one", "flag_near", "flag_coarse", "status_stall"):
            getattr(lib, "wft_twin_" + f).restype = C.c_int32
        _LIB = lib
    return _LIB


def const(name):
    return getattr(_lib(), "wft_twin_" + name)()


def twin_allocate_rc(workers, scale_factors, coefficients, stats=False):
    """(x[m][n], F[m], last level, Newton steps, stages, flags, froze[m], rc) from the CPU twin;
    with stats=True also the statistic of every job per stage ([stages][m], −1.0 once frozen)."""
    W = np.ascontiguousarray(workers, dtype=np.int32)
    sf = np.ascontiguousarray(scale_factors, dtype=np.int32)
    c = np.ascontiguousarray(coefficients, dtype=np.float64)
    m, n = c.shape
    assert len(W) == n and len(sf) == m
    x, F, res = np.zeros(m * n), np.zeros(m), np.zeros(4)
    froze = np.zeros(m, dtype=np.int32)
    st = np.full(m * m if stats else 1, -1.0)
    dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int32)
    rc = _lib().wft_twin_allocate_stats(m, n, W.ctypes.data_as(ip), sf.ctypes.data_as(ip), c.ctypes.data_as(dp),
                                        x.ctypes.data_as(dp), F.ctypes.data_as(dp), res.ctypes.data_as(dp),
                                        froze.ctypes.data_as(ip), st.ctypes.data_as(dp) if stats else None,
                                        m if stats else 0)
    out = (x.reshape(m, n), F, float(res[0]), int(res[1]), int(res[2]), int(res[3]), froze, rc)
    return out + (st.reshape(m, m)[:int(res[2]) + (rc != 0)],) if stats else out


def twin_allocate(workers, scale_factors, coefficients):
    *out, rc = twin_allocate_rc(workers, scale_factors, coefficients)
    assert rc == 0, rc
    return tuple(out)


class TwinEngine:
    """The native engine's water-filling calls, backed by the CPU twins."""

    def __init__(self):
        self.calls = []

    def wf_allocate(self, sf, coef, G):
        import wf_ref

        self.calls.append("wf_allocate")
        return wf_ref.twin_allocate(sf, coef, G)

    def wf_allocate_types(self, W, sf, coef):
        self.calls.append("wf_allocate_types")
        x, F, level, steps, stages, flags, _ = twin_allocate(W, sf, coef)
        return x, F, level, steps, stages, flags


def proportional(thr, W):
    """ProportionalPolicy.get_throughputs (proportional.py:15-44)."""
    m, n = thr.shape
    x = np.tile(np.asarray(W, dtype=np.float64) / m, (m, 1))
    x = x / x.sum(axis=1).max()
    return (thr * x).sum(axis=1)


def coefficients(thr, W, sf, weights):
    """c_jk = thr_jk / prop_j · (1 / w_j)·sf_j."""
    mult = (1.0 / np.asarray(weights, dtype=np.float64)) * np.asarray(sf, dtype=np.float64)
    return thr / proportional(thr, W)[:, None] * mult[:, None]


def draw(rng, mmax=24, nmax=4, wmax=8):
    """m 2…mmax, n 2…nmax, workers 1…wmax, scale factors {1,2,4,8}, weights
    {0.5,1,2,4}, throughputs U(0.2, 5) × a per-type U(0.5, 2)."""
    m = int(rng.integers(2, mmax + 1))
    n = int(rng.integers(2, nmax + 1))
    W = rng.integers(1, wmax + 1, size=n).astype(np.int32)
    sf = rng.choice([1, 2, 4, 8], size=m).astype(np.int32)
    w = rng.choice([0.5, 1.0, 2.0, 4.0], size=m)
    thr = rng.uniform(0.2, 5.0, size=(m, n)) * rng.uniform(0.5, 2.0, size=n)[None, :]
    return W, sf, coefficients(thr, W, sf, w)


def _freeze(inst):
    for a in inst:
        a.setflags(write=False)
    return inst


FIT_SEED, HELD_OUT_SEED = 6100, 11  # the second took no part in choosing any constant of the header
SEEDS = {FIT_SEED: 300, HELD_OUT_SEED: 150}  # seed: instances


@functools.lru_cache(maxsize=None)
def fuzz(seed=FIT_SEED):
    rng = np.random.default_rng(seed)
    return [_freeze(draw(rng)) for _ in range(SEEDS[seed])]


@functools.lru_cache(maxsize=None)
def fuzz_refs(seed=FIT_SEED):
    """ref.allocate of every instance of fuzz(seed); computed once."""
    return [ref.allocate(*inst) for inst in fuzz(seed)]


def hard_level_case():
    """Instance 40 of seed 12345: the largest level error met on 1,800 instances."""
    rng = np.random.default_rng(12345)
    return _freeze([draw(rng) for _ in range(41)][40])


def shaped(m, n, seed=0):
    """A generic m × n instance for the bit-exact shapes: workers so that capacity binds."""
    rng = np.random.default_rng(77 + 1000 * m + n + seed)
    W = rng.integers(1, max(2, m // (2 * n) + 2), size=n).astype(np.int32)
    sf = rng.choice([1, 2, 4, 8], size=m).astype(np.int32)
    w = rng.choice([0.5, 1.0, 2.0, 4.0], size=m)
    thr = rng.uniform(0.2, 5.0, size=(m, n)) * rng.uniform(0.5, 2.0, size=n)[None, :]
    return W, sf, coefficients(thr, W, sf, w)


def classes(m, n, groups, seed=0):
    """m jobs in `groups` classes of identical rows: as many stages as classes at most, whatever m is."""
    rng = np.random.default_rng(88 + 1000 * m + n + seed)
    W = rng.integers(max(1, m // (4 * n)), max(2, m // (2 * n) + 2), size=n).astype(np.int32)
    gsf = rng.choice([1, 2, 4], size=groups)
    gw = rng.choice([0.5, 1.0, 2.0, 4.0], size=groups)
    gthr = rng.uniform(0.2, 5.0, size=(groups, n))
    idx = np.arange(m) % groups
    sf = gsf[idx].astype(np.int32)
    return W, sf, coefficients(gthr[idx], W, sf, gw[idx])


def zero_worker_case():
    W, sf, c = shaped(9, 4)
    W = W.copy()
    W[[1, 3]] = 0
    return W, sf, c


def one_stage_case():
    """Identical jobs: capacity fills at the first level for all of them."""
    W = np.array([2, 1, 1], dtype=np.int32)
    sf = np.full(7, 2, dtype=np.int32)
    thr = np.tile(np.array([[1.0, 2.5, 0.7]]), (7, 1))
    return W, sf, coefficients(thr, W, sf, np.ones(7))


def all_capped_case():
    """Σ sf ≤ every type's workers: every job ends at Σ_k x = 1 on its best type."""
    _, sf, c = shaped(6, 3)
    return np.array([64, 64, 64], dtype=np.int32), sf, c


@functools.lru_cache(maxsize=None)
def many_stages_case():
    """The fuzz instance on which the reference takes the most stages."""
    refs = fuzz_refs()
    best = max((i for i in range(len(refs)) if refs[i][0] is not None), key=lambda i: refs[i][2])
    return fuzz()[best]


def last_job_alone_case():
    """One job needs few workers of a type of its own: the others freeze first
    and the last stage has one unfrozen row among m − 1 β-rows."""
    m = 6
    rng = np.random.default_rng(6155)
    W = np.array([1, 1, 4], dtype=np.int32)
    sf = np.ones(m, dtype=np.int32)
    c = np.zeros((m, 3))
    c[:m - 1, :2] = rng.uniform(0.5, 1.0, size=(m - 1, 2))  # five jobs share two workers: levels below 0.5
    c[m - 1, 2] = 1.0  # and one has four workers to itself: its time row stops it at 1
    return W, sf, c


NAMED = {"zero_worker": zero_worker_case, "one_stage": one_stage_case, "all_capped": all_capped_case,
         "many_stages": many_stages_case, "last_job_alone": last_job_alone_case}


def check_rows(W, sf, c, x, F, tol=1e-9):
    """Every row of the program at the returned levels."""
    W = np.asarray(W, dtype=np.float64)
    assert (x >= 0.0).all()
    val = (c * x).sum(axis=1)
    assert (val >= F * (1.0 - tol)).all(), ((val - F) / F).min()
    assert ((sf[:, None] * x).sum(axis=0) <= W + tol * np.maximum(W, 1.0)).all()
    assert (x.sum(axis=1) <= 1.0 + tol).all()
    assert (x[:, W == 0] == 0.0).all()
