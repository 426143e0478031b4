/*
 * sw_wf.hip — the Gavel water-filling MaxMinFairness allocation as one HIP
 * workgroup per instance, behind sw_wf_allocate() / sw_wf_allocate_batch().
 *
 * Replaces the stage loop of policies/max_min_fairness_water_filling.py:
 * 303-409 (one ECOS LP and one GLPK MILP per stage, up to one stage per job)
 * for one worker type (or several identical ones).  The mathematics is in
 * sw_wf.h.  One kernel serves both calls: a grid of `count` 512-thread
 * workgroups, each given its instance by an offsets array (CSR); the single
 * call is count = 1.  Thread L owns the contiguous job chunk [L·q, (L+1)·q) of
 * the deterministic sum (q = ⌈N/512⌉), so every reduction is the block's
 * detsum / dmax and the CPU twin (tests/twins/wf_twin.c) returns the same
 * bits.
 *
 *   pass 1   Σ_j sf_j (block detsum, exact) and max_j c_j (block max)
 *            Σ sf ≤ G: x_j = 1, L* = max c
 *   else     ≤ 63× probe: cap(L) = Σ_j sf_j·min(1, L/c_j) → bisection on the
 *            bits of L; x_j = min(1, L* / c_j)
 *
 * An instance's two input arrays (12 B per job) are staged in LDS when the
 * instance has at most SW_WF_LDS_JOBS jobs: every probe re-reads them.  The
 * LDS image is transposed (thread L's k-th job at slot k·512 + L), so a wave
 * reads consecutive words.  Larger instances read L2 on each probe.  The
 * arithmetic and the order of every sum are the same on both paths, so are
 * the bits.
 */
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/shockwave_amd.h"
#include "sw_alloc.h"
#include "sw_wf.h"

#define SW_WF_LDS_JOBS 2048
#define SW_WF_JOB_BYTES 12 /* c (double) and sf (int32) */

namespace {

/* The inputs of one instance, in global memory or in the LDS image: job lo + k
 * of the thread is element at(k) (sw_chunk_at). */
template <bool LDS>
struct WfIn {
    const double* c;
    const int32_t* sf;
    int32_t q;
    __device__ __forceinline__ int32_t at(int32_t k) const { return sw_chunk_at<LDS>(k, q); }
};

template <bool LDS>
__device__ __forceinline__ void wf_solve(sw_blk& blk, const WfIn<LDS>& in, int32_t cnt, int32_t G,
                                         double* __restrict__ x, double* __restrict__ out) {
    double s = 0.0, m = 0.0;
    for (int32_t k = 0; k < cnt; ++k) {
        const int32_t i = in.at(k);
        s = s + (double)in.sf[i];
        m = in.c[i] > m ? in.c[i] : m;
    }
    double total, cmax;
    blk.detsum_max(s, m, total, cmax);
    const double Gd = (double)G;

    if (total <= Gd) { /* the cluster holds every job whole */
        for (int32_t k = 0; k < cnt; ++k) x[k] = 1.0;
        if (threadIdx.x == 0) { out[0] = cmax; out[1] = total; }
        return;
    }

    /* cap(lo) ≤ G < cap(hi) throughout; used = cap(lo) */
    uint64_t blo = sw_bits(0.0), bhi = sw_bits(cmax);
    double used = 0.0;
    for (int it = 0; it < SW_WF_ITERS && bhi - blo > 1; ++it) {
        const uint64_t bmid = blo + (bhi - blo) / 2;
        const double L = sw_from_bits(bmid);
        double c = 0.0;
        for (int32_t k = 0; k < cnt; ++k) {
            const int32_t i = in.at(k);
            c = c + sw_wf_term((double)in.sf[i], in.c[i], L);
        }
        const double cap = blk.detsum(c);
        if (cap <= Gd) { blo = bmid; used = cap; } else bhi = bmid;
    }
    const double L = sw_from_bits(blo);
    for (int32_t k = 0; k < cnt; ++k) x[k] = sw_wf_x(in.c[in.at(k)], L);
    if (threadIdx.x == 0) { out[0] = L; out[1] = used; }
}

/* lds_q: the dynamic LDS holds lds_q·512 jobs (0: no staging) */
__global__ __launch_bounds__(SW_BLOCK) void sw_wf_kernel(const int64_t* __restrict__ offsets,
                                                         const int32_t* __restrict__ workers,
                                                         const int32_t* __restrict__ sf,
                                                         const double* __restrict__ c,
                                                         double* __restrict__ x,
                                                         double* __restrict__ levels, int32_t lds_q) {
    extern __shared__ double wf_lds[];
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
        double* lc = wf_lds;
        int32_t* lsf = (int32_t*)(lc + slots);
        for (int32_t k = 0; k < cnt; ++k) {
            const int32_t s = k * SW_BLOCK + (int32_t)threadIdx.x;
            const int64_t j = base + lo + k;
            lc[s] = c[j]; lsf[s] = sf[j];
        }
        /* each thread reads back only the slots it wrote: no barrier needed */
        const WfIn<true> in{lc, lsf, q};
        wf_solve<true>(blk, in, cnt, G, xo, out);
    } else {
        const WfIn<false> in{c + base, sf + base, q};
        wf_solve<false>(blk, in, cnt, G, xo, out);
    }
}

int wf_run(sw_handle* h, const char* who, int32_t count, const int64_t* offsets, const int32_t* workers,
           const int32_t* sf, const double* c, double* x, double* levels) {
    /* SW_WF_LDS=0: every instance on the L2 path (A/B timing, tools/wf_timing.py) */
    const sw_alloc_call call{who, count, offsets, workers, "worker counts must be > 0", 2, {{c, 8}, {sf, 4}},
                             x, levels, 2, SW_WF_LDS_JOBS, SW_WF_JOB_BYTES, "SW_WF_LDS"};
    return sw_alloc_run(
        h, call,
        [=](int64_t j) -> const char* {
            if (sf[j] < 1 || sf[j] > SW_MAX_WIDTH || !(c[j] > 0.0) || !isfinite(c[j]))
                return "scale factors must be in [1,255], coefficients finite and > 0";
            return nullptr;
        },
        [](const sw_alloc_dev& d) {
            hipLaunchKernelGGL(sw_wf_kernel, dim3(d.count), dim3(SW_BLOCK), d.lds, d.stream, d.offsets, d.workers,
                               (const int32_t*)d.col[1], (const double*)d.col[0], d.x, d.levels, d.maxq);
        });
}

}  // namespace

extern "C" int sw_wf_allocate(sw_handle* h, int32_t num_jobs, int32_t num_workers,
                              const int32_t* scale_factors, const double* coefficients,
                              double* allocation, double* level) {
    if (!h) return SW_ERR_INVALID;
    if (num_jobs < 0) return sw_fail(h, SW_ERR_INVALID, "sw_wf_allocate: num_jobs < 0");
    if (num_jobs == 0) { /* policy.flatten returns None */
        if (level) { level[0] = 0.0; level[1] = 0.0; }
        return SW_OK;
    }
    const int64_t offsets[2] = {0, num_jobs};
    return wf_run(h, "sw_wf_allocate", 1, offsets, &num_workers, scale_factors, coefficients, allocation,
                  level);
}

extern "C" int sw_wf_allocate_batch(sw_handle* h, int32_t count, const int64_t* offsets,
                                    const int32_t* num_workers, const int32_t* scale_factors,
                                    const double* coefficients, double* allocation, double* levels) {
    if (!h) return SW_ERR_INVALID;
    if (count < 0 || (count > 0 && (!offsets || !num_workers)))
        return sw_fail(h, SW_ERR_INVALID, "sw_wf_allocate_batch: bad count or null pointers");
    if (count == 0) return SW_OK;
    return wf_run(h, "sw_wf_allocate_batch", count, offsets, num_workers, scale_factors, coefficients,
                  allocation, levels);
}
