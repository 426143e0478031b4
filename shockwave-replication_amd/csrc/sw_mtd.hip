/*
 * sw_mtd.hip — the Gavel MinTotalDuration (makespan) allocation as one HIP
 * workgroup per instance, behind sw_mtd_allocate() / sw_mtd_allocate_batch().
 *
 * Replaces the bisection over ECOS feasibility solves of
 * policies/min_total_duration.py:62-106 for one worker type (or several
 * identical ones).  The mathematics and the search are in sw_mtd.h.  One
 * kernel serves both calls: a grid of `count` 512-thread workgroups, each
 * given its instance by an offsets array (CSR); the single call is count = 1.
 * Thread L owns the contiguous job chunk [L·q, (L+1)·q) of the deterministic
 * sum (q = ⌈N/512⌉), so every reduction is the block's detsum / dmax and the
 * CPU twin (tests/twins/mtd_twin.c) returns the same bits.
 *
 *   pass 1   max_j p_j                                      (block max, once)
 *   search   ≤ 18 T-probes per round (sw_mtd_next): max p ≤ T decides alone
 *            when it fails, otherwise cap(T) = Σ_j sf_j·(p_j/T) ≤ G
 *            (one pass over the chunk, one block detsum)
 *   cap = G  x_j = p_j/T, μ = 0
 *   cap < G  ≤ 64× μ-probe: x_j(μ) per job (bisection in registers) and the
 *            block's detsum of sf_j·x_j → bisection on the bits of μ; x_j(μ*)
 *
 * Every branch is taken on a block-reduced (workgroup-uniform) value, so the
 * whole workgroup takes the same side of each probe and no barrier sits in
 * divergent flow.
 *
 * An instance's two input arrays (12 B per job) are staged in LDS when the
 * instance has at most SW_MTD_LDS_JOBS jobs: every probe re-reads them, and
 * the kernel is latency-bound.  The LDS image is transposed (thread L's k-th
 * job at slot k·512 + L), so a wave reads consecutive words.  Larger
 * instances read HBM/L2 on each probe.  The arithmetic and the order of every
 * sum are the same on both paths, so are the bits.
 */
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/shockwave_amd.h"
#include "sw_alloc.h"
#include "sw_mtd.h"

#define SW_MTD_LDS_JOBS 4096 /* 48 KB of dynamic LDS: below the 64 KB a launch gets without opting in */
#define SW_MTD_JOB_BYTES 12  /* p (double) and sf (int32) */

namespace {

/* The inputs of one instance, in global memory or in the LDS image: job lo + k
 * of the thread is element at(k) (sw_chunk_at). */
template <bool LDS>
struct MtdIn {
    const double* p;
    const int32_t* sf;
    int32_t q;
    __device__ __forceinline__ int32_t at(int32_t k) const { return sw_chunk_at<LDS>(k, q); }
};

template <bool LDS>
__device__ __forceinline__ void mtd_solve(sw_blk& blk, const MtdIn<LDS>& in, int32_t cnt, int32_t G,
                                          double* __restrict__ x, double* __restrict__ out) {
    double m = 0.0;
    for (int32_t k = 0; k < cnt; ++k) {
        const double pj = in.p[in.at(k)];
        m = pj > m ? pj : m;
    }
    const double maxp = blk.dmax(m);
    const double Gd = (double)G;

    sw_mtd_search s;
    sw_mtd_begin(&s);
    double T = 0.0, cap = 0.0; /* cap: cap(T) of the last feasible probe */
    for (int it = 0; it < SW_MTD_MAX_PROBES && sw_mtd_next(&s, &T); ++it) {
        int ok = 0;
        if (maxp <= T) {
            double c = 0.0;
            for (int32_t k = 0; k < cnt; ++k) {
                const int32_t i = in.at(k);
                c = c + (double)in.sf[i] * sw_mtd_low(in.p[i], T);
            }
            const double ct = blk.detsum(c);
            ok = ct <= Gd;
            cap = ok ? ct : cap;
        }
        sw_mtd_feed(&s, T, ok);
    }
    T = sw_mtd_result(&s);
    if (!s.have) { /* unreachable on admitted input (sw_mtd.h); keeps cap consistent with T */
        double c = 0.0;
        for (int32_t k = 0; k < cnt; ++k) {
            const int32_t i = in.at(k);
            c = c + (double)in.sf[i] * sw_mtd_low(in.p[i], T);
        }
        cap = blk.detsum(c);
    }

    if (cap >= Gd) { /* the face is the single point x_j = p_j / T */
        for (int32_t k = 0; k < cnt; ++k) x[k] = sw_mtd_low(in.p[in.at(k)], T);
        if (threadIdx.x == 0) { out[0] = T; out[1] = 0.0; }
        return;
    }

    uint64_t blo = SW_MMF_MU_LO, bhi = SW_MMF_MU_HI;
    for (int it = 0; it < SW_MMF_ITERS && bhi - blo > 1; ++it) {
        const uint64_t bmid = blo + (bhi - blo) / 2;
        const double mu = sw_from_bits(bmid);
        double c = 0.0;
        for (int32_t k = 0; k < cnt; ++k) {
            const int32_t i = in.at(k);
            const double sf = (double)in.sf[i];
            c = c + sf * sw_mtd_x(sf, in.p[i], T, mu);
        }
        const double slack = Gd - blk.detsum(c);
        if (slack > 0.0 && mu * slack >= 1.0) bhi = bmid; else blo = bmid;
    }
    const double mu = sw_from_bits(bhi);
    for (int32_t k = 0; k < cnt; ++k) {
        const int32_t i = in.at(k);
        x[k] = sw_mtd_x((double)in.sf[i], in.p[i], T, mu);
    }
    if (threadIdx.x == 0) { out[0] = T; out[1] = mu; }
}

/* lds_q: the dynamic LDS holds lds_q·512 jobs (0: no staging) */
__global__ __launch_bounds__(SW_BLOCK) void sw_mtd_kernel(const int64_t* __restrict__ offsets,
                                                          const int32_t* __restrict__ workers,
                                                          const int32_t* __restrict__ sf,
                                                          const double* __restrict__ p,
                                                          double* __restrict__ x,
                                                          double* __restrict__ levels, int32_t lds_q) {
    extern __shared__ double mtd_lds[];
    __shared__ sw_xchg X;
    sw_blk blk{&X, 0};
    sw_chunk ch = sw_chunk_of(offsets);
    double* out = levels + 2 * (int64_t)blockIdx.x;
    if (ch.N <= 0) { sw_chunk_zero<2>(out); return; }
    ch.split();
    const int32_t G = workers[blockIdx.x];
    const int64_t base = ch.base;
    const int32_t q = ch.q, lo = ch.lo, cnt = ch.cnt;
    double* xo = x + base + lo;

    if (q <= lds_q) {
        const int32_t slots = lds_q * SW_BLOCK;
        double* lp = mtd_lds;
        int32_t* lsf = (int32_t*)(lp + slots);
        for (int32_t k = 0; k < cnt; ++k) {
            const int32_t s = k * SW_BLOCK + (int32_t)threadIdx.x;
            const int64_t j = base + lo + k;
            lp[s] = p[j]; lsf[s] = sf[j];
        }
        /* each thread reads back only the slots it wrote: no barrier needed */
        const MtdIn<true> in{lp, lsf, q};
        mtd_solve<true>(blk, in, cnt, G, xo, out);
    } else {
        const MtdIn<false> in{p + base, sf + base, q};
        mtd_solve<false>(blk, in, cnt, G, xo, out);
    }
}

int mtd_run(sw_handle* h, const char* who, int32_t count, const int64_t* offsets, const int32_t* workers,
            const int32_t* sf, const double* p, double* x, double* levels) {
    /* SW_MTD_LDS=0: every instance on the L2 path (A/B timing, tools/mtd_timing.py) */
    const sw_alloc_call call{who, count, offsets, workers, "worker counts must be > 0", 2, {{p, 8}, {sf, 4}},
                             x, levels, 2, SW_MTD_LDS_JOBS, SW_MTD_JOB_BYTES, "SW_MTD_LDS"};
    return sw_alloc_run(
        h, call,
        [=](int64_t j) -> const char* {
            if (sf[j] < 1 || sf[j] > SW_MAX_WIDTH || !(p[j] >= 0.0) || !(p[j] <= SW_MTD_FULL_TIME_MAX))
                return "scale factors must be in [1,255], full times finite, >= 0 and <= 1e15";
            return nullptr;
        },
        [](const sw_alloc_dev& d) {
            hipLaunchKernelGGL(sw_mtd_kernel, dim3(d.count), dim3(SW_BLOCK), d.lds, d.stream, d.offsets, d.workers,
                               (const int32_t*)d.col[1], (const double*)d.col[0], d.x, d.levels, d.maxq);
        });
}

}  // namespace

extern "C" int sw_mtd_allocate(sw_handle* h, int32_t num_jobs, int32_t num_workers,
                               const int32_t* scale_factors, const double* full_time,
                               double* allocation, double* level) {
    if (!h) return SW_ERR_INVALID;
    if (num_jobs < 0) return sw_fail(h, SW_ERR_INVALID, "sw_mtd_allocate: num_jobs < 0");
    const int64_t offsets[2] = {0, num_jobs};
    return mtd_run(h, "sw_mtd_allocate", 1, offsets, &num_workers, scale_factors, full_time,
                   allocation, level);
}

extern "C" int sw_mtd_allocate_batch(sw_handle* h, int32_t count, const int64_t* offsets,
                                     const int32_t* num_workers, const int32_t* scale_factors,
                                     const double* full_time, double* allocation, double* levels) {
    if (!h) return SW_ERR_INVALID;
    if (count < 0 || (count > 0 && (!offsets || !num_workers)))
        return sw_fail(h, SW_ERR_INVALID, "sw_mtd_allocate_batch: bad count or null pointers");
    if (count == 0) return SW_OK;
    return mtd_run(h, "sw_mtd_allocate_batch", count, offsets, num_workers, scale_factors, full_time,
                   allocation, levels);
}
