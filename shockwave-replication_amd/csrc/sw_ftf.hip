/*
 * sw_ftf.hip — the Gavel FinishTimeFairness (Themis) allocation as one HIP
 * workgroup per instance, behind sw_ftf_allocate() / sw_ftf_allocate_batch().
 *
 * Replaces the ECOS solve of policies/finish_time_fairness.py:55-140 for one
 * worker type (or several identical ones).  The mathematics is in sw_ftf.h.
 * One kernel serves both calls: a grid of `count` 512-thread workgroups, each
 * given its instance by an offsets array (CSR); the single call is count = 1.
 * Thread L owns the contiguous job chunk [L·q, (L+1)·q) of the deterministic
 * sum (q = ⌈N/512⌉), so every reduction is the block's detsum / dmax and the
 * CPU twin (tests/twins/ftf_twin.c) returns the same bits.
 *
 *   pass 1   ρ_box = max_j (a_j + p_j)/E_j                 (block max)
 *   pass 2   cap(ρ_box) = Σ_j sf_j·low_j(ρ_box)            (block detsum)
 *            = G exactly: x_j = low_j(ρ_box), μ = 0
 *   binds    ≤ 64× ρ-probe: cap(ρ) → bisection on the bits of ρ;
 *            x_j = low_j(ρ*), μ = 0
 *   free     ≤ 64× μ-probe: x_j(μ) per free job (bisection in registers) and
 *            the block's detsum of sf_j·x_j → bisection on the bits of μ;
 *            x_j(μ*), pinned jobs 1
 *
 * An instance's four input arrays (28 B per job) are staged in LDS when the
 * instance has at most SW_FTF_LDS_JOBS jobs: every probe re-reads them, and
 * the kernel is latency-bound.  The LDS image is transposed (thread L's k-th
 * job at slot k·512 + L), so a wave reads consecutive words.  Larger
 * instances read HBM/L2 on each probe, like sw_mmf_kernel.  The arithmetic
 * and the order of every sum are the same on both paths, so are the bits.
 */
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/shockwave_amd.h"
#include "sw_alloc.h"
#include "sw_ftf.h"

#define SW_FTF_LDS_JOBS 2048
#define SW_FTF_JOB_BYTES 28 /* p, a, E (double) and sf (int32) */

namespace {

/* The inputs of one instance, in global memory or in the LDS image: job lo + k
 * of the thread is element at(k) (sw_chunk_at). */
template <bool LDS>
struct FtfIn {
    const double *p, *a, *E;
    const int32_t* sf;
    int32_t q;
    __device__ __forceinline__ int32_t at(int32_t k) const { return sw_chunk_at<LDS>(k, q); }
};

template <bool LDS>
__device__ __forceinline__ void ftf_solve(sw_blk& blk, const FtfIn<LDS>& in, int32_t cnt, int32_t G,
                                          double* __restrict__ x, double* __restrict__ out) {
    double box = 0.0;
    for (int32_t k = 0; k < cnt; ++k) {
        const int32_t i = in.at(k);
        const double b = sw_ftf_box(in.p[i], in.a[i], in.E[i]);
        box = b > box ? b : box;
    }
    const double rho_box = blk.dmax(box);

    double s = 0.0;
    for (int32_t k = 0; k < cnt; ++k) {
        const int32_t i = in.at(k);
        s = s + (double)in.sf[i] * sw_ftf_low_box(in.p[i], in.a[i], in.E[i], rho_box);
    }
    const double cap0 = blk.detsum(s);
    const double Gd = (double)G;

    if (cap0 >= Gd) { /* capacity binds: the unique optimum x_j = p_j / d_j(ρ*) */
        uint64_t blo = sw_bits(rho_box), bhi = cap0 > Gd ? SW_FTF_RHO_HI : blo;
        for (int it = 0; it < SW_FTF_ITERS && bhi - blo > 1; ++it) {
            const uint64_t bmid = blo + (bhi - blo) / 2;
            const double rho = sw_from_bits(bmid);
            double c = 0.0;
            for (int32_t k = 0; k < cnt; ++k) {
                const int32_t i = in.at(k);
                c = c + (double)in.sf[i] * sw_ftf_low(in.p[i], in.a[i], in.E[i], rho);
            }
            if (blk.detsum(c) <= Gd) bhi = bmid; else blo = bmid;
        }
        const double rho = sw_from_bits(bhi);
        for (int32_t k = 0; k < cnt; ++k) {
            const int32_t i = in.at(k);
            x[k] = cap0 > Gd ? sw_ftf_low(in.p[i], in.a[i], in.E[i], rho)
                             : sw_ftf_low_box(in.p[i], in.a[i], in.E[i], rho);
        }
        if (threadIdx.x == 0) { out[0] = rho; out[1] = 0.0; }
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
            c = c + sf * sw_ftf_x(sf, in.p[i], in.a[i], in.E[i], rho_box, mu);
        }
        const double slack = Gd - blk.detsum(c);
        if (slack > 0.0 && mu * slack >= 1.0) bhi = bmid; else blo = bmid;
    }
    const double mu = sw_from_bits(bhi);
    for (int32_t k = 0; k < cnt; ++k) {
        const int32_t i = in.at(k);
        x[k] = sw_ftf_x((double)in.sf[i], in.p[i], in.a[i], in.E[i], rho_box, mu);
    }
    if (threadIdx.x == 0) { out[0] = rho_box; out[1] = mu; }
}

/* lds_q: the dynamic LDS holds lds_q·512 jobs (0: no staging) */
__global__ __launch_bounds__(SW_BLOCK) void sw_ftf_kernel(const int64_t* __restrict__ offsets,
                                                          const int32_t* __restrict__ workers,
                                                          const int32_t* __restrict__ sf,
                                                          const double* __restrict__ p,
                                                          const double* __restrict__ a,
                                                          const double* __restrict__ E,
                                                          double* __restrict__ x,
                                                          double* __restrict__ levels, int32_t lds_q) {
    extern __shared__ double ftf_lds[];
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
        double* lp = ftf_lds;
        double* la = lp + slots;
        double* lE = la + slots;
        int32_t* lsf = (int32_t*)(lE + slots);
        for (int32_t k = 0; k < cnt; ++k) {
            const int32_t s = k * SW_BLOCK + (int32_t)threadIdx.x;
            const int64_t j = base + lo + k;
            lp[s] = p[j]; la[s] = a[j]; lE[s] = E[j]; lsf[s] = sf[j];
        }
        /* each thread reads back only the slots it wrote: no barrier needed */
        const FtfIn<true> in{lp, la, lE, lsf, q};
        ftf_solve<true>(blk, in, cnt, G, xo, out);
    } else {
        const FtfIn<false> in{p + base, a + base, E + base, sf + base, q};
        ftf_solve<false>(blk, in, cnt, G, xo, out);
    }
}

int ftf_run(sw_handle* h, const char* who, int32_t count, const int64_t* offsets, const int32_t* workers,
            const int32_t* sf, const double* p, const double* a, const double* E, double* x,
            double* levels) {
    /* SW_FTF_LDS=0: every instance on the L2 path (A/B timing, tools/ftf_timing.py) */
    const sw_alloc_call call{who, count, offsets, workers, "worker counts must be > 0", 4,
                             {{p, 8}, {a, 8}, {E, 8}, {sf, 4}},
                             x, levels, 2, SW_FTF_LDS_JOBS, SW_FTF_JOB_BYTES, "SW_FTF_LDS"};
    return sw_alloc_run(
        h, call,
        [=](int64_t j) -> const char* {
            if (sf[j] < 1 || sf[j] > SW_MAX_WIDTH || !(p[j] >= 0.0) || !isfinite(p[j]) || !(a[j] >= 0.0) ||
                !isfinite(a[j]) || !(E[j] > 0.0) || !isfinite(E[j]))
                return "scale factors must be in [1,255], full and elapsed times finite "
                       "and >= 0, isolated times finite and > 0";
            return nullptr;
        },
        [](const sw_alloc_dev& d) {
            hipLaunchKernelGGL(sw_ftf_kernel, dim3(d.count), dim3(SW_BLOCK), d.lds, d.stream, d.offsets, d.workers,
                               (const int32_t*)d.col[3], (const double*)d.col[0], (const double*)d.col[1],
                               (const double*)d.col[2], d.x, d.levels, d.maxq);
        });
}

}  // namespace

extern "C" int sw_ftf_allocate(sw_handle* h, int32_t num_jobs, int32_t num_workers,
                               const int32_t* scale_factors, const double* full_time,
                               const double* elapsed, const double* isolated_time,
                               double* allocation, double* level) {
    if (!h) return SW_ERR_INVALID;
    if (num_jobs < 0) return sw_fail(h, SW_ERR_INVALID, "sw_ftf_allocate: num_jobs < 0");
    const int64_t offsets[2] = {0, num_jobs};
    return ftf_run(h, "sw_ftf_allocate", 1, offsets, &num_workers, scale_factors, full_time, elapsed,
                   isolated_time, allocation, level);
}

extern "C" int sw_ftf_allocate_batch(sw_handle* h, int32_t count, const int64_t* offsets,
                                     const int32_t* num_workers, const int32_t* scale_factors,
                                     const double* full_time, const double* elapsed,
                                     const double* isolated_time, double* allocation, double* levels) {
    if (!h) return SW_ERR_INVALID;
    if (count < 0 || (count > 0 && (!offsets || !num_workers)))
        return sw_fail(h, SW_ERR_INVALID, "sw_ftf_allocate_batch: bad count or null pointers");
    if (count == 0) return SW_OK;
    return ftf_run(h, "sw_ftf_allocate_batch", count, offsets, num_workers, scale_factors, full_time,
                   elapsed, isolated_time, allocation, levels);
}
