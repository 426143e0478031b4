/*
 * tests/twins/mst_twin.c — TEST INFRASTRUCTURE: CPU bit-exact twin of the
 * max-sum-throughput allocation kernel
 * (shockwave-replication_amd/csrc/sw_mst.hip).
 *
 * Same searches, same per-job arithmetic (sw_mst.h, -ffp-contract=off) and the
 * same deterministic job sums (sw_detsum: 512 contiguous chunks summed left to
 * right, then the halving tree), so it returns the bits the GPU returns.  It
 * is pinned against the exact-rational optimum of the LP and against the
 * reference's LP through HiGHS by tests/test_mst.py (tests/mst_ref.py).  Never
 * linked into the product.
 */
#include <math.h>
#include <stdint.h>

#include "../../shockwave-replication_amd/csrc/sw_arith.h"
#include "../../shockwave-replication_amd/csrc/sw_mmf.h"
#include "../../shockwave-replication_amd/csrc/sw_mst.h"
#include "twin_detsum.h"

typedef struct {
    int32_t N;
    const int32_t* sf;
    const double* w;
    const double* l; /* null: all zero */
    int dropped;
} mst_in;

static double dens(const mst_in* in, int32_t j) { return sw_mst_density(in->w[j], (double)in->sf[j]); }
static double floor_(const mst_in* in, int32_t j) { return in->l ? sw_mst_floor(in->l[j], in->dropped) : 0.0; }

static double used(const mst_in* in, double lambda, double m, double* v) {
    for (int32_t j = 0; j < in->N; ++j) {
        const double sf = (double)in->sf[j];
        v[j] = sf * sw_mst_alloc(dens(in, j), sf, floor_(in, j), lambda, m);
    }
    return detsum(v, in->N);
}

/* v is caller scratch of N doubles; level is 4 doubles; probes (optional, 2
 * ints) receives the numbers of θ-probes and of multiplier probes */
int mst_twin_allocate(int32_t N, int32_t G, const int32_t* sf, const double* w, const double* l,
                      double* x, double* level, double* v, int32_t* probes) {
    if (level) { level[0] = 0.0; level[1] = 0.0; level[2] = 0.0; level[3] = 0.0; }
    if (probes) { probes[0] = 0; probes[1] = 0; }
    if (N <= 0) return 0;
    const double Gd = (double)G;
    const double inf = sw_from_bits(SW_MST_INF_BITS);
    mst_in in = {N, sf, w, l, 0};
    int32_t np_theta = 0, np_m = 0;

    double maxl = 0.0, mind = inf, maxd = 0.0;
    for (int32_t j = 0; j < N; ++j) {
        const double lj = floor_(&in, j), d = dens(&in, j);
        v[j] = (double)sf[j] * lj;
        maxl = lj > maxl ? lj : maxl;
        mind = d < mind ? d : mind;
        maxd = d > maxd ? d : maxd;
    }
    const double S = detsum(v, N);
    in.dropped = (maxl > 1.0 || S > Gd) ? 1 : 0;

    for (int32_t j = 0; j < N; ++j) v[j] = (double)sf[j] * (dens(&in, j) > 0.0 ? 1.0 : floor_(&in, j));
    const double f0 = detsum(v, N);

    double lambda = 0.0;
    if (f0 > Gd) {
        uint64_t blo = sw_bits(mind) > 0 ? sw_bits(mind) - 1 : 0, bhi = sw_bits(maxd);
        for (int it = 0; it < SW_MST_THETA_ITERS && bhi > blo && bhi - blo > 1; ++it) {
            const uint64_t bmid = blo + (bhi - blo) / 2;
            const double theta = sw_from_bits(bmid);
            double A = -inf, B = inf;
            for (int32_t j = 0; j < N; ++j) {
                const double d = dens(&in, j);
                const int above = d > theta;
                v[j] = (double)sf[j] * (above ? 1.0 : floor_(&in, j));
                if (above) B = d < B ? d : B; else A = d > A ? d : A;
            }
            const double F = detsum(v, N);
            ++np_theta;
            if (F <= Gd) bhi = A >= 0.0 ? sw_bits(A) : bmid;
            else blo = B < inf ? sw_bits(B) - 1 : bmid;
        }
        lambda = sw_from_bits(bhi);
    }

    const double S0 = lambda > 0.0 ? used(&in, lambda, inf, v) : f0;
    double m = 0.0;
    if (S0 < Gd && !(lambda == 0.0 && mind > 0.0)) {
        if (lambda > 0.0) {
            uint64_t klo = SW_MST_NU_LO_KEY, khi = SW_MST_NU_HI_KEY;
            for (int it = 0; it < SW_MST_M_ITERS && khi - klo > 1; ++it) {
                const uint64_t kmid = klo + (khi - klo) / 2;
                ++np_m;
                if (used(&in, lambda, sw_mst_unkey(kmid), v) <= Gd) khi = kmid; else klo = kmid;
            }
            m = sw_mst_unkey(khi);
        } else {
            uint64_t blo = SW_MMF_MU_LO, bhi = SW_MMF_MU_HI;
            for (int it = 0; it < SW_MST_M_ITERS && bhi - blo > 1; ++it) {
                const uint64_t bmid = blo + (bhi - blo) / 2;
                const double mu = sw_from_bits(bmid);
                const double slack = Gd - used(&in, lambda, mu, v);
                ++np_m;
                if (slack > 0.0 && mu * slack >= 1.0) bhi = bmid; else blo = bmid;
            }
            m = sw_from_bits(bhi);
        }
    }

    const double mx = (S0 < Gd) ? m : inf;
    for (int32_t j = 0; j < N; ++j) {
        const double sfj = (double)sf[j];
        x[j] = sw_mst_alloc(dens(&in, j), sfj, floor_(&in, j), lambda, mx);
        v[j] = w[j] * x[j];
    }
    const double obj = detsum(v, N);
    if (level) { level[0] = lambda; level[1] = m; level[2] = obj; level[3] = in.dropped ? 1.0 : 0.0; }
    if (probes) { probes[0] = np_theta; probes[1] = np_m; }
    return 0;
}
