"""TEST INFRASTRUCTURE for the centred worker-type MaxMinFairness call
(sw_mmf_allocate_types_centred, csrc/sw_mmf_ipm.h): the CPU twin
(tests/twins/mmfc_twin.c, built by csrc/Makefile into
shockwave-replication_amd/lib/libmmfc_twin.so) through ctypes, the seeded input
families of tests/test_mmf_centre.py and tests/test_gpu_mmf_centre.py, and the
references computed once and shared.  Only tests/ may import this module."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np

import mmf_centre_ref
import mmf_ref

_HERE = os.path.dirname(os.path.abspath(__file__))
_CSRC = os.path.join(os.path.dirname(_HERE), "shockwave-replication_amd", "csrc")
_SO = os.path.join(os.path.dirname(_HERE), "shockwave-replication_amd", "lib", "libmmfc_twin.so")
_LIB = None

FAMILIES = ("generic", "identical", "integer")


def _lib():
    global _LIB
    if _LIB is None:
        if not os.path.exists(_SO):
            subprocess.check_call(["make", "-s", "-C", _CSRC, "../lib/libmmfc_twin.so"])
        lib = C.CDLL(_SO)
        dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int32)
        lib.mmfc_twin_allocate.argtypes = [C.c_int32, C.c_int32, ip, ip, dp, dp, dp]
        lib.mmfc_twin_allocate.restype = C.c_int
        lib.mmfc_twin_max_iters.restype = C.c_int32
        lib.mmfc_twin_max_jobs.restype = C.c_int32
        _LIB = lib
    return _LIB


def twin_allocate_rc(workers, scale_factors, coefficients):
    """(x[m][n], t*, Newton steps, rc) from the CPU twin; rc is 0, -3 (the step
    cap) or -4 (a non-positive pivot of the reduced system)."""
    W = np.ascontiguousarray(workers, dtype=np.int32)
    sf = np.ascontiguousarray(scale_factors, dtype=np.int32)
    c = np.ascontiguousarray(coefficients, dtype=np.float64)
    m, n = c.shape
    assert len(W) == n and len(sf) == m
    x = np.zeros(m * n)
    lvl = np.zeros(2)
    dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int32)
    rc = _lib().mmfc_twin_allocate(m, n, W.ctypes.data_as(ip), sf.ctypes.data_as(ip), c.ctypes.data_as(dp),
                                   x.ctypes.data_as(dp), lvl.ctypes.data_as(dp))
    return x.reshape(m, n), float(lvl[0]), int(lvl[1]), rc


def twin_allocate(workers, scale_factors, coefficients):
    x, t, it, rc = twin_allocate_rc(workers, scale_factors, coefficients)
    assert rc == 0, rc
    return x, t, it


def max_iters():
    return int(_lib().mmfc_twin_max_iters())


def max_jobs():
    return int(_lib().mmfc_twin_max_jobs())


class TwinEngine:
    """The native engine's MaxMinFairness calls, backed by the CPU twins."""

    def __init__(self):
        self.calls = []

    def mmf_allocate(self, sf, c, G):
        self.calls.append("mmf_allocate")
        return mmf_ref.twin_allocate(sf, c, G)

    def mmf_allocate_types(self, W, sf, c):
        self.calls.append("mmf_allocate_types")
        return mmf_ref.twin_allocate_types(W, sf, c)

    def mmf_allocate_types_centred(self, W, sf, c):
        self.calls.append("mmf_allocate_types_centred")
        return twin_allocate(W, sf, c)


def family_of(i):
    """Identical types every 5th instance, integer coefficients every 7th."""
    return "identical" if i % 5 == 0 else "integer" if i % 7 == 0 else "generic"


def draw(rng, i, mmax, nmax):
    """Instance i of a seeded fuzz: m < mmax jobs, n < nmax types; worker counts
    with zeros (one type always has workers), coefficients uniform in
    [0.2, 4]·sf with 15 % exact zeros."""
    m, n = int(rng.integers(1, mmax)), int(rng.integers(1, nmax))
    fam = family_of(i)
    W = rng.integers(0, 2 * m + 3, size=n).astype(np.int32)
    W[rng.random(size=n) < 0.15] = 0
    W[rng.integers(0, n)] += 1
    sf = rng.choice([1, 2, 4, 8], size=m).astype(np.int32)
    c = rng.uniform(0.2, 4.0, size=(m, n))
    if fam == "integer":
        c = np.maximum(np.rint(c), 1.0)
    c = c * sf[:, None]
    c[rng.random(size=(m, n)) < 0.15] = 0.0
    if fam == "identical":
        c = np.repeat(c[:, :1], n, axis=1)
        W[:] = max(int(W.max()), 1)
    return fam, W, sf, c


@functools.lru_cache(maxsize=None)
def level_fuzz():
    """150 instances, m < 50, n < 6 (the level and feasibility checks)."""
    rng = np.random.default_rng(2025)
    return [draw(rng, i, 50, 6) for i in range(150)]


@functools.lru_cache(maxsize=None)
def centre_fuzz():
    """105 instances, m < 14, n < 5, each with the reference's centre; computed
    once and left unchanged."""
    rng = np.random.default_rng(77)
    out = []
    for i in range(105):
        fam, W, sf, c = draw(rng, i, 14, 5)
        xr, tr = mmf_centre_ref.face_centre(W, sf, c)
        for a in (W, sf, c, xr):
            a.setflags(write=False)
        out.append((fam, W, sf, c, xr, tr))
    return out


@functools.lru_cache(maxsize=None)
def one_type_fuzz():
    """60 one-type instances with the closed-form centre (oracle/mmf_twin.c)."""
    rng = np.random.default_rng(31)
    out = []
    for _ in range(60):
        m = int(rng.integers(1, 40))
        G = int(rng.integers(1, 3 * m + 3))
        sf = rng.choice([1, 2, 4, 8], size=m).astype(np.int32)
        c = sf / rng.choice([1.0, 2.0, 5.0], size=m)
        x1, t1, _ = mmf_ref.twin_allocate(sf, c, G)
        slack = float((sf * x1).sum()) < G * (1.0 - 1e-9)
        out.append((G, sf, c, x1, t1, slack))
    return out


# the degenerate inputs of the issue
def zero_worker_case():
    W = np.array([4, 0, 2], dtype=np.int32)
    sf = np.array([1, 2, 1, 4], dtype=np.int32)
    c = np.array([[1.0, 2.0, 0.0], [0.5, 0.0, 1.5], [2.0, 1.0, 1.0], [0.0, 3.0, 1.0]])
    return W, sf, c


def level_zero_case():
    W = np.array([3, 0, 2], dtype=np.int32)
    sf = np.array([1, 2, 1, 4], dtype=np.int32)
    c = np.array([[1.0, 2.0, 0.0], [0.0, 5.0, 0.0], [2.0, 1.0, 1.0], [0.5, 3.0, 1.0]])
    return W, sf, c


def shaped(m, n, seed=0):
    """A generic m × n instance for the bit-exact shapes: 10 % zero coefficients,
    but none of its jobs without a positive one (the level is positive)."""
    rng = np.random.default_rng(1000 * m + n + seed)
    W = rng.integers(1, 2 * m + 3, size=n).astype(np.int32)
    sf = rng.choice([1, 2, 4, 8], size=m, p=[0.6, 0.3, 0.09, 0.01]).astype(np.int32)
    full = rng.uniform(0.2, 4.0, size=(m, n)) * sf[:, None]
    c = np.where(rng.random(size=(m, n)) < 0.1, 0.0, full)
    dead = ~(c > 0.0).any(axis=1)
    c[dead, 0] = full[dead, 0]
    return W, sf, c
