/*
 * tests/twins/ftf_twin.c — TEST INFRASTRUCTURE: CPU bit-exact twin of the
 * FinishTimeFairness allocation kernel (shockwave-replication_amd/csrc/sw_ftf.hip).
 *
 * Same algorithm, same per-job arithmetic (sw_ftf.h, sw_mmf.h,
 * -ffp-contract=off) and the same deterministic job sums (sw_detsum: 512
 * contiguous chunks summed left to right, then the halving tree), so it
 * returns the bits the GPU returns.  It is pinned against the reference's
 * program by tests/test_ftf.py (tests/ftf_ref.py: an exact rational
 * feasibility certificate of the level, and SLSQP on the program as written).
 * Never linked into the product.
 */
#include <math.h>
#include <stdint.h>

#include "../../shockwave-replication_amd/csrc/sw_arith.h"
#include "../../shockwave-replication_amd/csrc/sw_mmf.h"
#include "../../shockwave-replication_amd/csrc/sw_ftf.h"
#include "twin_detsum.h"

static double cap_at(int32_t N, const int32_t* sf, const double* p, const double* a, const double* E,
                     double rho, double* v) {
    for (int32_t j = 0; j < N; ++j) v[j] = (double)sf[j] * sw_ftf_low(p[j], a[j], E[j], rho);
    return detsum(v, N);
}

/* v is caller scratch of N doubles */
int ftf_twin_allocate(int32_t N, int32_t G, const int32_t* sf, const double* p, const double* a,
                      const double* E, double* x, double* level, double* v) {
    if (level) { level[0] = 0.0; level[1] = 0.0; }
    if (N <= 0) return 0;
    double rho_box = 0.0;
    for (int32_t j = 0; j < N; ++j) {
        const double b = sw_ftf_box(p[j], a[j], E[j]);
        rho_box = b > rho_box ? b : rho_box;
    }
    const double Gd = (double)G;
    for (int32_t j = 0; j < N; ++j) v[j] = (double)sf[j] * sw_ftf_low_box(p[j], a[j], E[j], rho_box);
    const double cap0 = detsum(v, N);
    if (cap0 >= Gd) {
        uint64_t blo = sw_bits(rho_box), bhi = cap0 > Gd ? SW_FTF_RHO_HI : blo;
        for (int it = 0; it < SW_FTF_ITERS && bhi - blo > 1; ++it) {
            const uint64_t bmid = blo + (bhi - blo) / 2;
            if (cap_at(N, sf, p, a, E, sw_from_bits(bmid), v) <= Gd) bhi = bmid; else blo = bmid;
        }
        const double rho = sw_from_bits(bhi);
        for (int32_t j = 0; j < N; ++j)
            x[j] = cap0 > Gd ? sw_ftf_low(p[j], a[j], E[j], rho) : sw_ftf_low_box(p[j], a[j], E[j], rho);
        if (level) { level[0] = rho; level[1] = 0.0; }
        return 0;
    }
    uint64_t blo = SW_MMF_MU_LO, bhi = SW_MMF_MU_HI;
    for (int it = 0; it < SW_MMF_ITERS && bhi - blo > 1; ++it) {
        const uint64_t bmid = blo + (bhi - blo) / 2;
        const double mu = sw_from_bits(bmid);
        for (int32_t j = 0; j < N; ++j)
            v[j] = (double)sf[j] * sw_ftf_x((double)sf[j], p[j], a[j], E[j], rho_box, mu);
        const double slack = Gd - detsum(v, N);
        if (slack > 0.0 && mu * slack >= 1.0) bhi = bmid; else blo = bmid;
    }
    const double mu = sw_from_bits(bhi);
    for (int32_t j = 0; j < N; ++j) x[j] = sw_ftf_x((double)sf[j], p[j], a[j], E[j], rho_box, mu);
    if (level) { level[0] = rho_box; level[1] = mu; }
    return 0;
}
