"""TEST INFRASTRUCTURE for the FinishTimeFairness call over worker types that
differ (sw_ftf_allocate_types, csrc/sw_ftf_types.h): the CPU twin
(tests/twins/ftft_twin.c, built by csrc/Makefile into
shockwave-replication_amd/lib/libftft_twin.so) through ctypes, the seeded input
families of tests/test_ftf_types.py and tests/test_gpu_ftf_types.py, and the
references computed once and shared.  Only tests/ may import this module."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np

import ftf_types_ref as ref
import mtdtcases as mt

_HERE = os.path.dirname(os.path.abspath(__file__))
_CSRC = os.path.join(os.path.dirname(_HERE), "shockwave-replication_amd", "csrc")
_SO = os.path.join(os.path.dirname(_HERE), "shockwave-replication_amd", "lib", "libftft_twin.so")
_LIB = None

FAMILIES = mt.FAMILIES


def _lib():
    global _LIB
    if _LIB is None:
        if not os.path.exists(_SO):
            subprocess.check_call(["make", "-s", "-C", _CSRC, "../lib/libftft_twin.so"])
        lib = C.CDLL(_SO)
        dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int32)
        lib.ftft_twin_allocate.argtypes = [C.c_int32, C.c_int32, ip, ip, dp, dp, dp, dp, dp, dp]
        lib.ftft_twin_allocate.restype = C.c_int
        lib.ftft_twin_tol.restype = C.c_double
        for f in ("max_solves", "max_jobs", "max_types", "flag_box", "flag_idle", "flag_safe", "status_cap"):
            getattr(lib, "ftft_twin_" + f).restype = C.c_int32
        _LIB = lib
    return _LIB


def const(name):
    return getattr(_lib(), "ftft_twin_" + name)()


def twin_allocate_rc(workers, scale_factors, throughputs, steps, elapsed, expected):
    """(x[m][n], ρ*, t, Newton steps, level solves, flags, rc) from the CPU twin."""
    W = np.ascontiguousarray(workers, dtype=np.int32)
    sf = np.ascontiguousarray(scale_factors, dtype=np.int32)
    thr = np.ascontiguousarray(throughputs, dtype=np.float64)
    st = np.ascontiguousarray(steps, dtype=np.float64)
    a = np.ascontiguousarray(elapsed, dtype=np.float64)
    E = np.ascontiguousarray(expected, dtype=np.float64)
    m, n = thr.shape
    assert len(W) == n and len(sf) == len(st) == len(a) == len(E) == m
    x = np.zeros(m * n)
    res = np.zeros(5)
    dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int32)
    rc = _lib().ftft_twin_allocate(m, n, W.ctypes.data_as(ip), sf.ctypes.data_as(ip), thr.ctypes.data_as(dp),
                                   st.ctypes.data_as(dp), a.ctypes.data_as(dp), E.ctypes.data_as(dp),
                                   x.ctypes.data_as(dp), res.ctypes.data_as(dp))
    return x.reshape(m, n), float(res[0]), float(res[1]), int(res[2]), int(res[3]), int(res[4]), rc


def twin_allocate(workers, scale_factors, throughputs, steps, elapsed, expected):
    *out, rc = twin_allocate_rc(workers, scale_factors, throughputs, steps, elapsed, expected)
    assert rc == 0, rc
    return tuple(out)


class TwinEngine:
    """The native engine's FinishTimeFairness calls, backed by the CPU twins."""

    def __init__(self):
        self.calls = []

    def ftf_allocate(self, sf, full_time, elapsed, expected, G):
        import ftf_ref

        self.calls.append("ftf_allocate")
        return ftf_ref.twin_allocate(sf, full_time, elapsed, expected, G)

    def ftf_allocate_types(self, W, sf, thr, steps, elapsed, expected):
        self.calls.append("ftf_allocate_types")
        return twin_allocate(W, sf, thr, steps, elapsed, expected)


def isolated(W, sf, thr):
    """The throughput of IsolatedPolicy's split (isolated.py:15-52)."""
    m, n = thr.shape
    x = np.asarray(W, dtype=np.float64)[None, :] / m / np.asarray(sf, dtype=np.float64)[:, None]
    x = x / np.maximum(x.sum(axis=1), 1.0)[:, None]
    return (thr * x).sum(axis=1)


def history(rng, W, sf, thr, steps, fresh=0.2):
    """(steps, a, E) of a schedule under way.  Each job has a total of the drawn
    steps (a dead one a redrawn total); a fifth of the live jobs have not
    started (a = 0), the others are 0–90 % done after a time of 0.3–0.8 times
    what the isolated split would have taken; E is the total at the isolated
    throughput."""
    m = len(sf)
    iso = isolated(W, sf, thr)
    dead = ~(steps > 0.0)
    total = np.where(dead, 10.0 ** rng.uniform(4.0, 6.0, size=m), steps)
    done = np.where(rng.random(size=m) < fresh, 0.0, rng.uniform(0.0, 0.9, size=m))
    done[dead] = 1.0
    left = np.where(dead, 0.0, total * (1.0 - done))
    E = total / iso
    a = total * done / iso * rng.uniform(0.3, 0.8, size=m)
    return left, a, E


def draw(rng, i, mmax, nmax, family):
    """Instance i: the draws of mtdtcases.draw (throughputs 0 or in [0.2, 4]·sf
    with a positive one on a type with workers, steps 10^U(4, 6) (narrow) or
    10^U(1, 7.5) (wide), 10 % of the jobs dead) with the history above."""
    W, sf, thr, steps = mt.draw(rng, i, mmax, nmax, family)
    W = (W + 7) // 8  # an eighth of the workers, so that capacity binds on most instances
    left, a, E = history(rng, W, sf, thr, steps)
    return W, sf, thr, left, a, E


def _freeze(inst):
    for a in inst:
        a.setflags(write=False)
    return inst


@functools.lru_cache(maxsize=None)
def level_fuzz(family):
    """150 instances, m < 50, n < 6."""
    rng = np.random.default_rng(5200 + FAMILIES.index(family))
    return [_freeze(draw(rng, i, 50, 6, family)) for i in range(150)]


@functools.lru_cache(maxsize=None)
def level_refs(family):
    """(ρ*, whether it is ρ_box) of the reference for level_fuzz(family); computed once."""
    return [ref.solve_rho(*inst)[:2] for inst in level_fuzz(family)]


@functools.lru_cache(maxsize=None)
def centre_fuzz():
    """60 instances with m·n ≤ 130 (m < 27, n < 6), alternating families."""
    rng = np.random.default_rng(5277)
    out = []
    for i in range(60):
        fam = FAMILIES[i % 2]
        inst = draw(rng, i, 27, 6, fam)
        assert inst[2].size <= 130
        out.append((fam, _freeze(inst)))
    return out


@functools.lru_cache(maxsize=None)
def centre_ref(i):
    """The reference's (x, ρ*, box) of centre_fuzz()[i]; computed once."""
    r = ref.allocate(*centre_fuzz()[i][1])
    r[0].setflags(write=False)
    return r


def shaped(m, n, seed=0, dead=0.1):
    """A generic m × n instance for the bit-exact shapes; above 1000 jobs without
    dead ones, whose ratios would set the level of so many jobs."""
    W, sf, thr, steps = mt.shaped(m, n, seed, dead if 1 < m <= 1000 else 0.0)
    cut = (W + 7) // 8  # an eighth of the workers: capacity binds
    rng = np.random.default_rng(91 + 1000 * m + n + seed)
    # above 100 jobs the history is that of the whole cluster, or E would shrink the demand along
    return (cut, sf, thr) + history(rng, cut if m <= 100 else W, sf, thr, steps)


def no_elapsed_case():
    """Every a_j = 0: t* is linear in ρ, two solves."""
    _, sf, thr, steps = mt.shaped(9, 3)
    W = np.array([2, 1, 1], dtype=np.int32)
    E = steps / isolated(W, sf, thr)
    return W, sf, thr, steps, np.zeros(9), E


def box_case():
    """Capacity does not bind: every job can run at its best type in full."""
    W, sf, thr, left, a, E = shaped(5, 3, dead=0.0)
    return np.array([40, 40, 40], dtype=np.int32), sf, thr, left, a, E


def all_dead_case():
    W, sf, thr, left, a, E = shaped(6, 3)
    return W, sf, thr, np.zeros(6), np.where(a > 0.0, a, 1e4), E


def dead_among_live_case():
    _, sf, thr, left, a, E = shaped(7, 3, dead=0.0)
    W = np.array([1, 2, 1], dtype=np.int32)
    left = left.copy()
    left[[2, 5]] = 0.0
    return W, sf, thr, left, a, E


def zero_worker_case():
    W, sf, thr, steps = mt.zero_worker_case()
    rng = np.random.default_rng(93)
    return (W, sf, thr) + history(rng, W, sf, thr, steps)


def tight_case():
    """Capacity a hundredth of the demand: ρ* ≫ ρ_box."""
    W, sf, thr, left, a, E = shaped(200, 3, dead=0.0)
    return np.array([1, 1, 1], dtype=np.int32), sf, thr, left, a, E


@functools.lru_cache(maxsize=None)
def most_solves_case():
    """The instance of both level families on which the twin takes the most level solves."""
    best = max((inst for f in FAMILIES for inst in level_fuzz(f)), key=lambda inst: twin_allocate(*inst)[4])
    return best


NAMED = {"box": box_case, "all_dead": all_dead_case, "dead_among_live": dead_among_live_case,
         "zero_worker": zero_worker_case, "tight": tight_case, "no_elapsed": no_elapsed_case,
         "most_solves": most_solves_case}


def check_rows(W, sf, thr, steps, elapsed, expected, x, rho, tol=1e-9):
    """Every row of the reference's program at ρ."""
    W = np.asarray(W, dtype=np.float64)
    live = steps > 0.0
    assert (x >= 0.0).all()
    val = (thr * x).sum(axis=1)
    assert (val[live] > 0.0).all()
    d = rho * expected[live] - elapsed[live]
    assert (val[live] * d / steps[live] >= 1.0 - tol).all(), (val[live] * d / steps[live]).min()
    assert ((elapsed[~live] / expected[~live]) <= rho).all()
    assert ((sf[:, None] * x).sum(axis=0) <= W + tol * np.maximum(W, 1.0)).all()
    assert (x.sum(axis=1) <= 1.0 + tol).all()
    assert (x[:, W == 0] == 0.0).all()
