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
#include <stdlib.h>
#include <string.h>

#include <string>

#include "../../include/shockwave_amd.h"
#include "sw_block.h"
#include "sw_handle.h"
#include "sw_wf.h"

#define SW_WF_LDS_JOBS 2048
#define SW_WF_JOB_BYTES 12 /* c (double) and sf (int32) */

namespace {

/* The inputs of one instance: job lo + k of thread L is element
 * k·ks + L·ls — (1, q) in global memory, (512, 1) in the LDS image. */
template <bool LDS>
struct WfIn {
    const double* c;
    const int32_t* sf;
    int32_t q;
    __device__ __forceinline__ int32_t at(int32_t k) const {
        return LDS ? k * SW_BLOCK + (int32_t)threadIdx.x : (int32_t)threadIdx.x * q + k;
    }
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
    const int64_t inst = blockIdx.x;
    const int64_t base = offsets[inst];
    const int32_t N = (int32_t)(offsets[inst + 1] - base);
    double* out = levels + 2 * inst;
    if (N <= 0) { /* an empty instance (policy.flatten returns None) */
        if (threadIdx.x == 0) { out[0] = 0.0; out[1] = 0.0; }
        return;
    }
    const int32_t G = workers[inst];
    const int32_t q = (N + SW_BLOCK - 1) / SW_BLOCK;
    const int32_t lo = (int32_t)threadIdx.x * q;
    const int32_t hi = lo + q < N ? lo + q : N;
    const int32_t cnt = hi > lo ? hi - lo : 0;
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

/* One input block and one output block per call (one copy each way):
 *   in : offsets[count+1] (int64) | c [total] (double) | sf [total],
 *        workers [count] (int32)
 *   out: x [total] | levels [count][2] (double) */
struct WfBufs {
    DevBuf<unsigned char> in, out;
    HostBuf<unsigned char> hin, hout;
};

int wf_fail(sw_handle* h, int code, const std::string& msg) {
    h->err = msg;
    return code;
}

#define WF_HIP(h, call)                                                                     \
    do {                                                                                    \
        hipError_t _e = (call);                                                             \
        if (_e != hipSuccess)                                                               \
            return wf_fail((h), SW_ERR_HIP, std::string(#call) + ": " + hipGetErrorString(_e)); \
    } while (0)

int wf_run(sw_handle* h, const char* who, int32_t count, const int64_t* offsets, const int32_t* workers,
           const int32_t* sf, const double* c, double* x, double* levels) {
    const std::string w(who);
    if (offsets[0] != 0) return wf_fail(h, SW_ERR_INVALID, w + ": offsets must start at 0");
    int32_t maxq = 0;
    for (int32_t i = 0; i < count; ++i) {
        const int64_t n = offsets[i + 1] - offsets[i];
        if (n < 0 || n > (int64_t)INT32_MAX - SW_BLOCK)
            return wf_fail(h, SW_ERR_INVALID, w + ": offsets must not decrease");
        if (workers[i] <= 0) return wf_fail(h, SW_ERR_INVALID, w + ": worker counts must be > 0");
        const int32_t q = (int32_t)((n + SW_BLOCK - 1) / SW_BLOCK);
        if (q <= SW_WF_LDS_JOBS / SW_BLOCK && q > maxq) maxq = q;
    }
    /* SW_WF_LDS=0: every instance on the L2 path (A/B timing, tools/wf_timing.py) */
    const char* lds_env = getenv("SW_WF_LDS");
    if (lds_env && lds_env[0] == '0') maxq = 0;
    const int64_t total = offsets[count];
    if (total > 0 && (!sf || !c || !x)) return wf_fail(h, SW_ERR_INVALID, w + ": null pointers");
    for (int64_t j = 0; j < total; ++j) {
        if (sf[j] < 1 || sf[j] > SW_MAX_WIDTH || !(c[j] > 0.0) || !isfinite(c[j]))
            return wf_fail(h, SW_ERR_INVALID,
                           w + ": scale factors must be in [1,255], coefficients finite and > 0");
    }
    if (levels)
        for (int64_t i = 0; i < 2 * (int64_t)count; ++i) levels[i] = 0.0;
    if (total == 0) return SW_OK; /* only empty instances */
    WF_HIP(h, hipSetDevice(h->device));
    if (!h->wf) h->wf = new WfBufs();
    WfBufs* b = (WfBufs*)h->wf;
    const size_t T = (size_t)total, C = (size_t)count;
    const size_t o_c = (C + 1) * 8, o_sf = o_c + T * 8, o_w = o_sf + T * 4, in_bytes = o_w + C * 4;
    const size_t o_lv = T * 8, out_bytes = o_lv + C * 16;
    WF_HIP(h, b->in.reserve(in_bytes));
    WF_HIP(h, b->out.reserve(out_bytes));
    WF_HIP(h, b->hin.reserve(in_bytes));
    WF_HIP(h, b->hout.reserve(out_bytes));
    memcpy(b->hin.p, offsets, (C + 1) * 8);
    memcpy(b->hin.p + o_c, c, T * 8);
    memcpy(b->hin.p + o_sf, sf, T * 4);
    memcpy(b->hin.p + o_w, workers, C * 4);
    WF_HIP(h, hipMemcpyAsync(b->in.p, b->hin.p, in_bytes, hipMemcpyHostToDevice, h->stream));
    unsigned char* d = b->in.p;
    const size_t lds = (size_t)maxq * SW_BLOCK * SW_WF_JOB_BYTES;
    hipLaunchKernelGGL(sw_wf_kernel, dim3((unsigned)count), dim3(SW_BLOCK), lds, h->stream,
                       (const int64_t*)d, (const int32_t*)(d + o_w), (const int32_t*)(d + o_sf),
                       (const double*)(d + o_c), (double*)b->out.p, (double*)(b->out.p + o_lv), maxq);
    WF_HIP(h, hipGetLastError());
    WF_HIP(h, hipMemcpyAsync(b->hout.p, b->out.p, out_bytes, hipMemcpyDeviceToHost, h->stream));
    WF_HIP(h, hipStreamSynchronize(h->stream));
    memcpy(x, b->hout.p, T * 8);
    if (levels) memcpy(levels, b->hout.p + o_lv, C * 16);
    return SW_OK;
}

}  // namespace

void sw_wf_release(sw_handle* h) {
    if (!h || !h->wf) return;
    WfBufs* b = (WfBufs*)h->wf;
    b->in.release(); b->out.release(); b->hin.release(); b->hout.release();
    delete b;
    h->wf = nullptr;
}

extern "C" int sw_wf_allocate(sw_handle* h, int32_t num_jobs, int32_t num_workers,
                              const int32_t* scale_factors, const double* coefficients,
                              double* allocation, double* level) {
    if (!h) return SW_ERR_INVALID;
    if (num_jobs < 0) return wf_fail(h, SW_ERR_INVALID, "sw_wf_allocate: num_jobs < 0");
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
        return wf_fail(h, SW_ERR_INVALID, "sw_wf_allocate_batch: bad count or null pointers");
    if (count == 0) return SW_OK;
    return wf_run(h, "sw_wf_allocate_batch", count, offsets, num_workers, scale_factors, coefficients,
                  allocation, levels);
}
