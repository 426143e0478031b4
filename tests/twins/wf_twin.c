/*
 * tests/twins/wf_twin.c — TEST INFRASTRUCTURE: CPU bit-exact twin of the
 * water-filling MaxMinFairness allocation kernel
 * (shockwave-replication_amd/csrc/sw_wf.hip).
 *
 * Same algorithm, same per-job arithmetic (sw_wf.h, -ffp-contract=off) and
 * the same deterministic job sums (sw_detsum: 512 contiguous chunks summed
 * left to right, then the halving tree), so it returns the bits the GPU
 * returns.  It is pinned against the reference's stage loop by
 * tests/test_wf.py (tests/wf_ref.py: an exact rational certificate of the
 * level, the sort-based closed form, and the loop restated over HiGHS).
 * Never linked into the product.
 */
#include <math.h>
#include <stdint.h>

#include "../../shockwave-replication_amd/csrc/sw_arith.h"
#include "../../shockwave-replication_amd/csrc/sw_wf.h"
#include "twin_detsum.h"

/* v is caller scratch of N doubles; level receives (L*, Σ sf_j·x_j) */
int wf_twin_allocate(int32_t N, int32_t G, const int32_t* sf, const double* c, double* x, double* level,
                     double* v) {
    if (level) { level[0] = 0.0; level[1] = 0.0; }
    if (N <= 0) return 0;
    double cmax = 0.0;
    for (int32_t j = 0; j < N; ++j) {
        v[j] = (double)sf[j];
        cmax = c[j] > cmax ? c[j] : cmax;
    }
    const double total = detsum(v, N);
    const double Gd = (double)G;
    if (total <= Gd) {
        for (int32_t j = 0; j < N; ++j) x[j] = 1.0;
        if (level) { level[0] = cmax; level[1] = total; }
        return 0;
    }
    uint64_t blo = sw_bits(0.0), bhi = sw_bits(cmax);
    double used = 0.0;
    for (int it = 0; it < SW_WF_ITERS && bhi - blo > 1; ++it) {
        const uint64_t bmid = blo + (bhi - blo) / 2;
        const double L = sw_from_bits(bmid);
        for (int32_t j = 0; j < N; ++j) v[j] = sw_wf_term((double)sf[j], c[j], L);
        const double cap = detsum(v, N);
        if (cap <= Gd) { blo = bmid; used = cap; } else bhi = bmid;
    }
    const double L = sw_from_bits(blo);
    for (int32_t j = 0; j < N; ++j) x[j] = sw_wf_x(c[j], L);
    if (level) { level[0] = L; level[1] = used; }
    return 0;
}
