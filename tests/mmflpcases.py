"""Seeded inputs for the worker-type MaxMinFairness LP (sw_mmf_allocate_types,
csrc/sw_mmf_lp.h), shared by tests/test_mmf_lp.py (the CPU twin against HiGHS
and exact residuals) and tests/test_gpu_mmf_lp.py (the kernel against the twin).

Every family is ``family(m, n, seed) -> (W, sf, c)``: worker counts per type
(int32, n), scale factors per job (int32, m, in [1, 255]), coefficients
(float64, m × n, finite and ≥ 0) — the envelope the C-ABI accepts.
"""
import numpy as np

# the shapes of the CPU comparison: many types (24/80/150 × 16, 120 × 12), more
# than 512 constraint rows (300 × 2: R = 602; 400 × 3: R = 803), Gavel's 200 × 8
SHAPES = [(24, 16), (80, 16), (120, 12), (150, 16), (300, 2), (400, 3), (200, 8)]
SPARSE_SEEDS = range(6)
# a sparse case kept for what it did under Bland's rule alone with pivot elements
# down to 1e-11: rc = 0 after 14,978 pivots with a constraint violated by 375
# (found by a search over 224 further seeds; the others met 1e-9 or hit the cap)
SPARSE_EXTRA = [(80, 16, 148)]


def _rng(name, m, n, seed):
    return np.random.default_rng([sum(name.encode()), m, n, seed])


def _workers(rng, m, n):
    return rng.integers(1, 3 * m // n + 2, size=n).astype(np.int32)


def _decades(rng, m, n, half_width):
    return 10.0 ** rng.uniform(-half_width, half_width, size=(m, n))


def sparse(m, n, seed):
    """Coefficients over three decades with 40 % zeros, any scale factor, one
    type without workers: the family on which Bland's rule stalls."""
    rng = _rng("sparse", m, n, seed)
    c = _decades(rng, m, n, 1.5)
    c[rng.random(size=(m, n)) < 0.4] = 0.0
    sf = rng.integers(1, 256, size=m).astype(np.int32)
    W = _workers(rng, m, n)
    W[rng.integers(0, n)] = 0
    return W, sf, c


def decades3(m, n, seed):
    rng = _rng("decades3", m, n, seed)
    c = _decades(rng, m, n, 1.5)
    sf = rng.integers(1, 256, size=m).astype(np.int32)
    return _workers(rng, m, n), sf, c


def decades6(m, n, seed):
    rng = _rng("decades6", m, n, seed)
    c = _decades(rng, m, n, 3.0)
    sf = rng.integers(1, 256, size=m).astype(np.int32)
    return _workers(rng, m, n), sf, c


def unit(m, n, seed):
    """The Fig-9 policy: every throughput 1, c[j][k] = sf_j / pw_j for every k
    (fully degenerate: the types are interchangeable)."""
    rng = _rng("unit", m, n, seed)
    sf = rng.choice([1, 2, 4, 8], size=m).astype(np.int32)
    cj = sf / rng.choice([1.0, 2.0, 5.0], size=m)
    return _workers(rng, m, n), sf, np.repeat(cj[:, None], n, axis=1)


def dup(m, n, seed):
    """Half the jobs exact copies of others: ties in the entering rule (equal
    objective entries) and in the leaving rule (equal ratios)."""
    rng = _rng("dup", m, n, seed)
    c = _decades(rng, m, n, 1.5)
    sf = rng.choice([1, 2, 4, 8], size=m).astype(np.int32)
    h = m // 2
    c[m - h:] = c[:h]
    sf[m - h:] = sf[:h]
    return _workers(rng, m, n), sf, c


def tight(m, n, seed):
    """Hardly any workers: W in {0, 1, 2}, at least one positive."""
    rng = _rng("tight", m, n, seed)
    c = _decades(rng, m, n, 1.5)
    sf = rng.choice([1, 2, 4, 8], size=m).astype(np.int32)
    W = rng.integers(0, 3, size=n).astype(np.int32)
    if not W.any():
        W[rng.integers(0, n)] = 1
    return W, sf, c


def zero_type(m, n, seed):
    rng = _rng("zero_type", m, n, seed)
    c = _decades(rng, m, n, 1.5)
    sf = rng.integers(1, 256, size=m).astype(np.int32)
    W = _workers(rng, m, n)
    W[rng.integers(0, n)] = 0
    return W, sf, c


def all_zero_job(m, n, seed):
    """One job can run nowhere, so t* = 0."""
    rng = _rng("all_zero_job", m, n, seed)
    c = _decades(rng, m, n, 1.5)
    c[rng.integers(0, m)] = 0.0
    sf = rng.integers(1, 256, size=m).astype(np.int32)
    return _workers(rng, m, n), sf, c


def stranded_job(m, n, seed):
    """A job whose only nonzero coefficient is on the type without workers
    (t* = 0 although no row of c is zero)."""
    rng = _rng("stranded_job", m, n, seed)
    c = _decades(rng, m, n, 1.5)
    sf = rng.choice([1, 2, 4, 8], size=m).astype(np.int32)
    W = _workers(rng, m, n)
    k = int(rng.integers(0, n))
    W[k] = 0
    j = int(rng.integers(0, m))
    keep = c[j, k]
    c[j] = 0.0
    c[j, k] = keep
    return W, sf, c


FAMILIES = {f.__name__: f for f in (sparse, decades3, decades6, unit, dup, tight, zero_type, all_zero_job)}

# the smallest problems and the two ends of the type range
EDGE_SHAPES = [(m, n) for m in (1, 2, 3) for n in (1, 16)]


def edges():
    """(name, (W, sf, c)) of the edge cases."""
    out = []
    for m, n in EDGE_SHAPES:
        out.append((f"decades3-{m}x{n}", decades3(m, n, 0)))
        if n > 1:
            out.append((f"sparse-{m}x{n}", sparse(m, n, 0)))
    out.append(("stranded-12x4", stranded_job(12, 4, 0)))
    out.append(("stranded-2x2", stranded_job(2, 2, 0)))
    return out


def scaled(case, k):
    """The same problem with every coefficient multiplied by 2^k (exact)."""
    W, sf, c = case
    return W, sf, np.ldexp(c, k)


SCALE_SHAPE = (40, 4)
SCALE_EXPONENTS = [-300, -30, -10, 10, 30, 300]
