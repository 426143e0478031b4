"""TEST INFRASTRUCTURE for the max-sum-throughput call over worker types that
differ (sw_mst_allocate_types, csrc/sw_mst_types.h): the CPU twin
(tests/twins/mstt_twin.c, built by csrc/Makefile into
shockwave-replication_amd/lib/libmstt_twin.so) through ctypes, the optimality
certificate, the reference's LP through HiGHS, and the instances that
tests/test_mst_types.py and tests/test_gpu_mst_types.py share.  Only tests/ (and
tools/ run by hand) may import this module."""
import ctypes as C
import functools
import math

import numpy as np
from scipy.optimize import linprog
from scipy.sparse import identity, kron, vstack

import twinlib

EPS = 2.0 ** -53


def _declare(lib):
    dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int32)
    lib.mstt_twin_allocate.argtypes = [C.c_int32, C.c_int32, ip, ip, dp, dp, dp, dp, ip]
    lib.mstt_twin_allocate.restype = C.c_int
    for f in ("cap_mult", "lds_cells", "flag_unplaced", "flag_slack"):
        getattr(lib, "mstt_twin_" + f).restype = C.c_int32


def const(name):
    return getattr(twinlib.load("libmstt_twin.so", _declare, built_by="csrc"), "mstt_twin_" + name)()


def twin_allocate(workers, scale_factors, weights):
    """(x [m, n], prices [n], objective, augmentations, row recomputations,
    flags) from the CPU twin, the tuple of Solver.mst_allocate_types."""
    W = np.ascontiguousarray(workers, dtype=np.int32)
    sf = np.ascontiguousarray(scale_factors, dtype=np.int32)
    w = np.ascontiguousarray(weights, dtype=np.float64).reshape(len(sf), len(W))
    m, n = w.shape
    x, p, res = np.zeros(m * n), np.zeros(n), np.zeros(4)
    dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int32)
    rc = twinlib.load("libmstt_twin.so", _declare, built_by="csrc").mstt_twin_allocate(
        m, n, W.ctypes.data_as(ip), sf.ctypes.data_as(ip), w.ctypes.data_as(dp), x.ctypes.data_as(dp),
        p.ctypes.data_as(dp), res.ctypes.data_as(dp), None)
    assert rc == 0, rc
    return x.reshape(m, n), p, float(res[0]), int(res[1]), int(res[2]), int(res[3])


class TwinEngine:
    """The native engine's max-sum-throughput calls, backed by the CPU twins."""

    def __init__(self):
        self.calls = []

    def mst_allocate(self, sf, weights, floors, G):
        import mst_ref

        self.calls.append("mst_allocate")
        return mst_ref.twin_allocate(sf, weights, floors, G)

    def mst_allocate_types(self, W, sf, weights):
        self.calls.append("mst_allocate_types")
        return twin_allocate(W, sf, weights)


def certificate(W, sf, w, out):
    """Primal feasibility in the integers y = sf·x, and the duality gap
    |D(prices) − objective| / objective (D by math.fsum; 0.0 at objective 0)."""
    x, p, obj = out[0], out[1], out[2]
    W, sf, w = np.asarray(W), np.asarray(sf), np.asarray(w, dtype=np.float64).reshape(x.shape)
    y = np.rint(x * sf[:, None]).astype(np.int64)
    assert np.array_equal(y / sf[:, None].astype(np.float64), x), "x is not y / sf with integer y"
    assert (y >= 0).all() and (y.sum(axis=1) <= sf).all() and (y.sum(axis=0) <= W).all()
    assert (x[:, W == 0] == 0.0).all() and (p >= 0.0).all()
    u = np.maximum((w / sf[:, None] - p[None, :]).max(axis=1), 0.0) if len(sf) else np.zeros(0)
    D = math.fsum([float(W[k]) * p[k] for k in range(len(W))] + list(sf * u))
    assert obj == 0.0 or abs(obj - math.fsum((w * x).ravel())) <= 4 * x.size * EPS * obj
    return abs(D - obj) / obj if obj > 0 else abs(D)


def lp_optimum(W, sf, w):
    """(objective, x [m, n]) of the reference's LP (max_sum_throughput.py:66-84
    with policy.py:57-63, no SLOs) through scipy.optimize.linprog (HiGHS)."""
    w = np.asarray(w, dtype=np.float64)
    m, n = w.shape
    rows = kron(identity(m), np.ones((1, n)), format="csr")  # Σ_k x_jk ≤ 1
    caps = kron(np.asarray(sf, dtype=np.float64).reshape(1, m), identity(n), format="csr")  # Σ_j sf_j·x_jk ≤ W_k
    A = vstack([rows, caps], format="csr")
    b = np.concatenate([np.ones(m), np.asarray(W, dtype=np.float64)])
    r = linprog(-w.ravel(), A_ub=A, b_ub=b, bounds=(0, None), method="highs",
                options={"primal_feasibility_tolerance": 1e-9, "dual_feasibility_tolerance": 1e-9})
    assert r.status == 0, r.message
    return -float(r.fun), r.x.reshape(m, n)


def draw(seed, m, n, load=1.6, ints=False):
    """A seeded instance whose capacity binds: Σ sf ≈ load · Σ W.  ints: weights
    and scale factors from small sets, so that many d tie exactly."""
    rng = np.random.default_rng(seed)
    sf = rng.choice([1, 1, 2, 4, 8], size=m).astype(np.int32)
    W = np.maximum(rng.multinomial(max(int(sf.sum() / load), n), np.ones(n) / n), 1).astype(np.int32)
    if ints:
        w = rng.choice([1.0, 2.0, 4.0], size=(m, n)) * np.minimum(sf, 4)[:, None]
    else:
        w = rng.uniform(0.2, 5.0, size=(m, n)) * np.linspace(0.6, 1.8, n)[None, :]
    return W, sf, w


def chain4():
    """Types of one worker each; jobs 0–2 hold types 0–2 and would each lose 1 by
    moving one type up, type 3 is free; job 3 earns only on type 0.  Its best
    path displaces 0 → 1 → 2 → 3 (gain 10 − 3) where evicting job 0 gains 10 − 5."""
    w = np.array([[5.0, 4.0, 0.0, 0.0], [0.0, 5.0, 4.0, 0.0], [0.0, 0.0, 5.0, 4.0], [10.0, 0.0, 0.0, 0.0]])
    return np.ones(4, dtype=np.int32), np.ones(4, dtype=np.int32), w


@functools.lru_cache(maxsize=None)
def cases():
    """name → (W, sf, w): the shapes of the issue, smallest first."""
    lim = const("lds_cells") // 3
    c = {"n1": draw(11, 9, 1)}
    for m in (1, 2, 3):
        c[f"n2_m{m}"] = draw(20 + m, m, 2)
    c["chain4"] = chain4()
    W, sf, w = draw(31, 24, 3)
    c["zero_type"] = (np.array([W[0], 0, W[2]], dtype=np.int32), sf, w)
    c["wide"] = (np.array([2, 3, 1], dtype=np.int32), np.full(6, 4, dtype=np.int32), draw(32, 6, 3)[2])
    c["roomy"] = (np.full(3, 200, dtype=np.int32),) + draw(33, 40, 3)[1:]
    c["ties"] = draw(34, 60, 4, ints=True)
    c["types16"] = draw(35, 100, 16)
    for m in (511, 512, 513):
        c[f"m{m}"] = draw(m, m, 3)
    c["lds_limit"] = draw(41, lim, 3)
    c["lds_limit_plus_1"] = draw(42, lim + 1, 3)
    return c


@functools.lru_cache(maxsize=None)
def twin_of(name):
    return twin_allocate(*cases()[name])
