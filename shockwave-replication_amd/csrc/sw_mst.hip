/*
 * sw_mst.hip — the Gavel max-sum-throughput allocation as one HIP workgroup
 * per instance, behind sw_mst_allocate() / sw_mst_allocate_batch().
 *
 * Replaces the ECOS solve (and the second solve without the SLO rows) of
 * policies/max_sum_throughput.py:39-96 for one worker type.  The mathematics
 * and both searches are in sw_mst.h.  One kernel serves both calls: a grid of
 * `count` 512-thread workgroups, each given its instance by an offsets array
 * (CSR); the single call is count = 1.  Thread L owns the contiguous job chunk
 * [L·q, (L+1)·q) of the deterministic sum (q = ⌈N/512⌉), so every reduction is
 * the block's detsum / max / min and the CPU twin (tests/twins/mst_twin.c)
 * returns the same bits.
 *
 *   pass 1   Σ sf·l and max l (are the SLO rows feasible?), min d, max d
 *   f(0)     ≤ G: λ* = 0
 *   search   otherwise ≤ 64 θ-probes, each one pass over the chunk and one
 *            block reduction of (Σ, largest d ≤ θ, smallest d > θ); the
 *            bracket snaps to those densities (sw_mst.h)
 *   floors   the sum with the class at its floors: ≥ G, or an empty class,
 *            ends with m = 0
 *   class    ≤ 64 m-probes (ν by its ordered key when λ* > 0, the bits of μ
 *            when λ* = 0): x_j(m) per class job (bisection in registers) and
 *            the block's detsum of sf_j·x_j over all jobs
 *   emit     x_j, and the objective Σ w·x as one more detsum
 *
 * Every branch is taken on a block-reduced (workgroup-uniform) value, so the
 * whole workgroup takes the same side of each probe and no barrier sits in
 * divergent flow.
 *
 * An instance's d, l and sf (20 B per job) are staged in LDS when the instance
 * has at most SW_MST_LDS_JOBS jobs: every probe re-reads them, and the kernel
 * is latency-bound.  The LDS image is transposed (thread L's k-th job at slot
 * k·512 + L), so a wave reads consecutive words.  Larger instances read w, l
 * and sf from HBM/L2 on each probe and divide again.  The arithmetic and the
 * order of every sum are the same on both paths, so are the bits.
 */
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/shockwave_amd.h"
#include "sw_alloc.h"
#include "sw_mst.h"

#define SW_MST_LDS_JOBS 3072 /* 60 KB of dynamic LDS: with the exchange slots, inside the 64 KB a launch gets without opting in */
#define SW_MST_JOB_BYTES 20  /* d, l (double) and sf (int32) */

namespace {

/* The inputs of one instance, in global memory or in the LDS image: job lo + k
 * of the thread is element at(k) (sw_chunk_at).  dw is the density in the LDS
 * image and the weight in global memory. */
template <bool LDS>
struct MstIn {
    const double* dw;
    const double* l;
    const int32_t* sf;
    int32_t q;
    int32_t dropped;
    __device__ __forceinline__ int32_t at(int32_t k) const { return sw_chunk_at<LDS>(k, q); }
    __device__ __forceinline__ double dens(int32_t i, double sf_) const {
        return LDS ? dw[i] : sw_mst_density(dw[i], sf_);
    }
    __device__ __forceinline__ double floor_(int32_t i) const { return sw_mst_floor(l[i], dropped); }
};

/* Σ_j sf_j·x_j(λ, m) over the thread's chunk */
template <bool LDS>
__device__ __forceinline__ double mst_used(const MstIn<LDS>& in, int32_t cnt, double lambda, double m) {
    double c = 0.0;
    for (int32_t k = 0; k < cnt; ++k) {
        const int32_t i = in.at(k);
        const double sf = (double)in.sf[i];
        c = c + sf * sw_mst_alloc(in.dens(i, sf), sf, in.floor_(i), lambda, m);
    }
    return c;
}

template <bool LDS>
__device__ __forceinline__ void mst_solve(sw_blk& blk, MstIn<LDS>& in, int32_t cnt, int32_t G,
                                          const double* __restrict__ w, double* __restrict__ x,
                                          double* __restrict__ out) {
    const double Gd = (double)G;
    const double inf = sw_from_bits(SW_MST_INF_BITS);

    /* are the SLO rows feasible?  and the range of the densities */
    double c = 0.0, ml = 0.0, dlo = inf, dhi = 0.0;
    in.dropped = 0;
    for (int32_t k = 0; k < cnt; ++k) {
        const int32_t i = in.at(k);
        const double sf = (double)in.sf[i], l = in.floor_(i), d = in.dens(i, sf);
        c = c + sf * l;
        ml = l > ml ? l : ml;
        dlo = d < dlo ? d : dlo;
        dhi = d > dhi ? d : dhi;
    }
    double S, maxl, mind;
    blk.detsum_max_min(c, ml, dlo, S, maxl, mind);
    const double maxd = blk.dmax(dhi);
    in.dropped = (maxl > 1.0 || S > Gd) ? 1 : 0;

    /* f(0) */
    c = 0.0;
    for (int32_t k = 0; k < cnt; ++k) {
        const int32_t i = in.at(k);
        const double sf = (double)in.sf[i];
        c = c + sf * (in.dens(i, sf) > 0.0 ? 1.0 : in.floor_(i));
    }
    const double f0 = blk.detsum(c);

    double lambda = 0.0;
    if (f0 > Gd) {
        /* θ at blo is infeasible, θ at bhi feasible */
        uint64_t blo = sw_bits(mind) > 0 ? sw_bits(mind) - 1 : 0, bhi = sw_bits(maxd);
        for (int it = 0; it < SW_MST_THETA_ITERS && bhi > blo && bhi - blo > 1; ++it) {
            const uint64_t bmid = blo + (bhi - blo) / 2;
            const double theta = sw_from_bits(bmid);
            double a = -inf, b = inf;
            c = 0.0;
            for (int32_t k = 0; k < cnt; ++k) {
                const int32_t i = in.at(k);
                const double sf = (double)in.sf[i], d = in.dens(i, sf);
                const bool above = d > theta;
                c = c + sf * (above ? 1.0 : in.floor_(i));
                if (above) b = d < b ? d : b; else a = d > a ? d : a;
            }
            double F, A, B;
            blk.detsum_max_min(c, a, b, F, A, B);
            if (F <= Gd) bhi = A >= 0.0 ? sw_bits(A) : bmid;
            else blo = B < inf ? sw_bits(B) - 1 : bmid;
        }
        lambda = sw_from_bits(bhi);
    }

    /* the class at its floors; an empty class is λ* = 0 with no zero density */
    const double S0 = lambda > 0.0 ? blk.detsum(mst_used(in, cnt, lambda, inf)) : f0;
    double m = 0.0;
    if (S0 < Gd && !(lambda == 0.0 && mind > 0.0)) {
        if (lambda > 0.0) {
            uint64_t klo = SW_MST_NU_LO_KEY, khi = SW_MST_NU_HI_KEY;
            for (int it = 0; it < SW_MST_M_ITERS && khi - klo > 1; ++it) {
                const uint64_t kmid = klo + (khi - klo) / 2;
                const double used = blk.detsum(mst_used(in, cnt, lambda, sw_mst_unkey(kmid)));
                if (used <= Gd) khi = kmid; else klo = kmid;
            }
            m = sw_mst_unkey(khi);
        } else {
            uint64_t blo = SW_MMF_MU_LO, bhi = SW_MMF_MU_HI;
            for (int it = 0; it < SW_MST_M_ITERS && bhi - blo > 1; ++it) {
                const uint64_t bmid = blo + (bhi - blo) / 2;
                const double mu = sw_from_bits(bmid);
                const double slack = Gd - blk.detsum(mst_used(in, cnt, lambda, mu));
                if (slack > 0.0 && mu * slack >= 1.0) bhi = bmid; else blo = bmid;
            }
            m = sw_from_bits(bhi);
        }
    }

    /* m = 0 with the class at its floors is x(+inf) */
    const double mx = (S0 < Gd) ? m : inf;
    c = 0.0;
    for (int32_t k = 0; k < cnt; ++k) {
        const int32_t i = in.at(k);
        const double sf = (double)in.sf[i];
        const double xj = sw_mst_alloc(in.dens(i, sf), sf, in.floor_(i), lambda, mx);
        x[k] = xj;
        c = c + w[k] * xj;
    }
    const double obj = blk.detsum(c);
    if (threadIdx.x == 0) { out[0] = lambda; out[1] = m; out[2] = obj; out[3] = in.dropped ? 1.0 : 0.0; }
}

/* lds_q: the dynamic LDS holds lds_q·512 jobs (0: no staging) */
__global__ __launch_bounds__(SW_BLOCK) void sw_mst_kernel(const int64_t* __restrict__ offsets,
                                                          const int32_t* __restrict__ workers,
                                                          const int32_t* __restrict__ sf,
                                                          const double* __restrict__ w,
                                                          const double* __restrict__ l,
                                                          double* __restrict__ x,
                                                          double* __restrict__ levels, int32_t lds_q) {
    extern __shared__ double mst_lds[];
    __shared__ sw_xchg X;
    sw_blk blk{&X, 0};
    sw_chunk ch = sw_chunk_of(offsets);
    double* out = levels + 4 * (int64_t)blockIdx.x;
    if (ch.N <= 0) { sw_chunk_zero<4>(out); return; }
    ch.split();
    const int32_t G = workers[blockIdx.x];
    const int64_t base = ch.base;
    const int32_t q = ch.q, lo = ch.lo, cnt = ch.cnt;
    double* xo = x + base + lo;
    const double* wo = w + base + lo;

    if (q <= lds_q) {
        const int32_t slots = lds_q * SW_BLOCK;
        double* ld = mst_lds;
        double* ll = ld + slots;
        int32_t* lsf = (int32_t*)(ll + slots);
        for (int32_t k = 0; k < cnt; ++k) {
            const int32_t s = k * SW_BLOCK + (int32_t)threadIdx.x;
            const int64_t j = base + lo + k;
            ld[s] = sw_mst_density(w[j], (double)sf[j]); ll[s] = l[j]; lsf[s] = sf[j];
        }
        /* each thread reads back only the slots it wrote: no barrier needed */
        MstIn<true> in{ld, ll, lsf, q, 0};
        mst_solve<true>(blk, in, cnt, G, wo, xo, out);
    } else {
        MstIn<false> in{w + base, l + base, sf + base, q, 0};
        mst_solve<false>(blk, in, cnt, G, wo, xo, out);
    }
}

int mst_run(sw_handle* h, const char* who, int32_t count, const int64_t* offsets, const int32_t* workers,
            const int32_t* sf, const double* w, const double* l, double* x, double* levels) {
    /* SW_MST_LDS=0: every instance on the global path (A/B timing, tools/mst_timing.py);
     * null floors are optional: all zero */
    const sw_alloc_call call{who, count, offsets, workers, "worker counts must be >= 1", 3,
                             {{w, 8}, {l, 8, true}, {sf, 4}},
                             x, levels, 4, SW_MST_LDS_JOBS, SW_MST_JOB_BYTES, "SW_MST_LDS"};
    return sw_alloc_run(
        h, call,
        [=](int64_t j) -> const char* {
            if (sf[j] < 1 || sf[j] > SW_MAX_WIDTH) return "scale factors must be in [1,255]";
            if (!(w[j] >= 0.0) || !(w[j] <= SW_MST_WEIGHT_MAX)) return "weights must be finite, >= 0 and <= 1e30";
            if (l && !(l[j] >= 0.0)) return "floors must be >= 0 (+inf allowed) and not NaN";
            return nullptr;
        },
        [](const sw_alloc_dev& d) {
            hipLaunchKernelGGL(sw_mst_kernel, dim3(d.count), dim3(SW_BLOCK), d.lds, d.stream, d.offsets, d.workers,
                               (const int32_t*)d.col[2], (const double*)d.col[0], (const double*)d.col[1], d.x,
                               d.levels, d.maxq);
        });
}

}  // namespace

extern "C" int sw_mst_allocate(sw_handle* h, int32_t num_jobs, int32_t num_workers,
                               const int32_t* scale_factors, const double* weights,
                               const double* floors, double* allocation, double* level) {
    if (!h) return SW_ERR_INVALID;
    if (num_jobs < 0) return sw_fail(h, SW_ERR_INVALID, "sw_mst_allocate: num_jobs < 0");
    const int64_t offsets[2] = {0, num_jobs};
    return mst_run(h, "sw_mst_allocate", 1, offsets, &num_workers, scale_factors, weights, floors,
                   allocation, level);
}

extern "C" int sw_mst_allocate_batch(sw_handle* h, int32_t count, const int64_t* offsets,
                                     const int32_t* num_workers, const int32_t* scale_factors,
                                     const double* weights, const double* floors, double* allocation,
                                     double* levels) {
    if (!h) return SW_ERR_INVALID;
    if (count < 0 || (count > 0 && (!offsets || !num_workers)))
        return sw_fail(h, SW_ERR_INVALID, "sw_mst_allocate_batch: bad count or null pointers");
    if (count == 0) return SW_OK;
    return mst_run(h, "sw_mst_allocate_batch", count, offsets, num_workers, scale_factors, weights,
                   floors, allocation, levels);
}
