/*
 * sw_mmf_ipm.hip — the centred MaxMinFairness allocation over worker types as
 * one HIP workgroup per instance, behind sw_mmf_allocate_types_centred() /
 * sw_mmf_allocate_types_centred_batch().
 *
 * The method and all of its arithmetic are in sw_mmf_ipm.h: a primal–dual
 * interior-point method on the LP of sw_mmf_lp.h that ends at the analytic
 * centre of the optimal face.  One launch per call, the whole iteration inside
 * the kernel (the simplex of sw_mmf.hip takes two launches per pivot).  A grid
 * of `count` 512-thread workgroups, each given its instance by an offsets
 * array (CSR); the single call is count = 1.  Thread L owns the contiguous job
 * chunk [L·q, (L+1)·q) of the deterministic sum (q = ⌈m/512⌉), so the CPU twin
 * (tests/twins/mmfc_twin.c) returns the same bits.
 *
 *   per job    x, s, the slacks, their steps and scalings: 8·na + 21 doubles in
 *              a workspace on the handle (HBM, L2-resident at these sizes),
 *              structure of arrays
 *   LDS        sw_ipm_glob (t, the capacity slacks, the reduced system: 4 KB)
 *              and the reduction scratch
 *   a step     pass A (residuals, μ)            1 reduction of na + 2 sums, 3 maxes
 *              pass B (scalings)                no reduction
 *              pass R_k, k < na (row k of the   1 reduction of ≤ na + 4 sums each
 *                reduced system)
 *              thread 0: L·D·Lᵀ of the na × na system, dt, dy_C
 *              pass C (back-substitution)       1 reduction of 2 maxes
 *              pass D (the step)                fused with the next pass A
 *   the end    the two points of the path extrapolated to μ = 0 under a ratio
 *              test                             1 reduction of na sums, 1 max
 * The reduction's helpers are in sw_mmf_ipm_dev.h (shared with sw_mtd_types.hip).
 * A reduction is the block's deterministic tree for sums (wave_dettree, then
 * the halving tree over the eight waves) and exact maxima, two barriers: one
 * before thread 0 combines the waves' values and runs the one-thread part of
 * the step, one after it.  No grid-wide synchronisation, no inline assembly.
 */
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <string.h>

#include <string>
#include <vector>

#include "../../include/shockwave_amd.h"
#include "sw_block.h"
#include "sw_handle.h"
#include "sw_mmf_ipm.h"
#include "sw_mmf_ipm_dev.h"

namespace {

/* levels: [count][3] = t*, Newton steps, status (SW_IPM_OK / _CAP / _BREAK) */
__global__ __launch_bounds__(SW_BLOCK) void sw_mmf_ipm_kernel(const int64_t* __restrict__ offsets, int32_t n,
                                                              const int32_t* __restrict__ workers,
                                                              const int32_t* __restrict__ shifts,
                                                              const int32_t* __restrict__ sfs,
                                                              const double* __restrict__ coef,
                                                              double* __restrict__ ws, double* __restrict__ x,
                                                              double* __restrict__ levels) {
    __shared__ sw_ipm_glob G;
    __shared__ IpmRed R;
    sw_ipm_glob* g = &G;
    const int64_t inst = blockIdx.x;
    const int64_t base = offsets[inst];
    const int32_t m = (int32_t)(offsets[inst + 1] - base);
    const int tid = threadIdx.x;
    double* out = levels + 3 * inst;
    if (m <= 0) { /* uniform */
        if (tid == 0) { out[0] = 0.0; out[1] = 0.0; out[2] = 0.0; }
        return;
    }
    const int32_t q = (m + SW_BLOCK - 1) / SW_BLOCK;
    const int32_t lo = tid * q < m ? tid * q : m;
    const int32_t hi = lo + q < m ? lo + q : m;
    const int32_t shift = shifts[inst];
    const int32_t* sf = sfs + base;
    const double* cf = coef + base * n;
    double* xo = x + base * n;

    if (tid == 0) sw_ipm_setup(g, m, n, workers + inst * n);
    __syncthreads();
    const int32_t na = g->na;
    if (na == 0) { /* uniform: no type has workers */
        for (int32_t j = lo; j < hi; ++j)
            for (int32_t k = 0; k < n; ++k) xo[(int64_t)j * n + k] = 0.0;
        if (tid == 0) { out[0] = 0.0; out[1] = 0.0; out[2] = 0.0; }
        return;
    }
    sw_ipm_job J{ws + (int64_t)SW_IPM_FIELDS(n) * base, m, 0, na, 0.0};
    double acc[SW_IPM_NRED], mx[SW_IPM_NMAX];
    double v[SW_IPM_NRED], w[SW_IPM_NMAX];

    /* the start */
    ipm_clear(acc, mx);
    for (int32_t j = lo; j < hi; ++j) {
        J.j = j; J.sf = (double)sf[j];
        sw_ipm_job_load(g, &J, cf + (int64_t)j * n, shift, v, w);
        ipm_take(acc, v, 2, mx, w, 1);
    }
    ipm_publish(R, acc, 2, mx, 1);
    if (tid == 0) { ipm_combine(R, 2, 1); sw_ipm_glob_load(g, R.sums, R.maxes); }
    __syncthreads();
    ipm_clear(acc, mx);
    for (int32_t j = lo; j < hi; ++j) {
        J.j = j; J.sf = (double)sf[j];
        sw_ipm_job_start(g, &J, w);
        ipm_take(acc, v, 0, mx, w, 1);
    }
    ipm_publish(R, acc, 0, mx, 1);
    if (tid == 0) { ipm_combine(R, 0, 1); sw_ipm_glob_start(g, R.maxes); }
    __syncthreads();
    for (int32_t j = lo; j < hi; ++j) {
        J.j = j; J.sf = (double)sf[j];
        sw_ipm_job_start2(g, &J);
    }

    /* the steps; `moved`: pass D of the step before is still to do */
    bool moved = false;
    for (int32_t guard = 0; guard <= SW_IPM_MAX_ITERS + 1; ++guard) {
        ipm_clear(acc, mx);
        for (int32_t j = lo; j < hi; ++j) {
            J.j = j; J.sf = (double)sf[j];
            if (moved) sw_ipm_job_step(g, &J);
            sw_ipm_job_resid(g, &J, v, w);
            ipm_take(acc, v, na + 2, mx, w, 3);
        }
        ipm_publish(R, acc, na + 2, mx, 3);
        if (tid == 0) { ipm_combine(R, na + 2, 3); sw_ipm_glob_resid(g, R.sums, R.maxes); }
        __syncthreads();
        if (g->done) break; /* uniform */
        for (int32_t j = lo; j < hi; ++j) {
            J.j = j; J.sf = (double)sf[j];
            sw_ipm_job_prep(g, &J);
        }
        for (int32_t k = 0; k < na; ++k) {
            const int32_t cnt = sw_ipm_row_count(na, k, g->has_t);
            ipm_clear(acc, mx);
            for (int32_t j = lo; j < hi; ++j) {
                J.j = j; J.sf = (double)sf[j];
                const sw_ipm_rowctx rc = sw_ipm_row_begin(&J, k);
#pragma unroll
                for (int i = 0; i < SW_IPM_NRED; ++i)
                    if (i < cnt) acc[i] = acc[i] + sw_ipm_row_val(&J, &rc, i);
            }
            ipm_publish(R, acc, cnt, mx, 0);
            if (tid == 0) {
                ipm_combine(R, cnt, 0);
                sw_ipm_glob_row(g, k, R.sums);
                if (k == na - 1) sw_ipm_glob_solve(g);
            }
            __syncthreads();
        }
        if (g->done) break; /* uniform: the reduced system broke down */
        ipm_clear(acc, mx);
        for (int32_t j = lo; j < hi; ++j) {
            J.j = j; J.sf = (double)sf[j];
            sw_ipm_job_back(g, &J, w);
            ipm_take(acc, v, 0, mx, w, 2);
        }
        ipm_publish(R, acc, 0, mx, 2);
        if (tid == 0) { ipm_combine(R, 0, 2); sw_ipm_glob_step(g, R.maxes); }
        __syncthreads();
        moved = true;
    }

    if (sw_ipm_two_points(g)) { /* uniform: the ratio test of the extrapolation */
        ipm_clear(acc, mx);
        for (int32_t j = lo; j < hi; ++j) {
            J.j = j; J.sf = (double)sf[j];
            sw_ipm_job_final(g, &J, v, w);
            ipm_take(acc, v, na, mx, w, 1);
        }
        ipm_publish(R, acc, na, mx, 1);
        if (tid == 0) { ipm_combine(R, na, 1); sw_ipm_glob_final(g, R.sums, R.maxes); }
        __syncthreads();
    }
    for (int32_t j = lo; j < hi; ++j) {
        J.j = j; J.sf = (double)sf[j];
        sw_ipm_job_emit(g, &J, xo + (int64_t)j * n);
    }
    if (tid == 0) {
        out[0] = sw_ipm_level(g, shift);
        out[1] = (double)g->iters;
        out[2] = (double)g->status;
    }
}

struct MmfcBufs {
    DevBuf<double> ws;
    std::vector<int32_t> shifts;
};

int mmfc_run(sw_handle* h, const std::string& who, int32_t count, int32_t n, const int64_t* offsets,
             const int32_t* workers, const int32_t* sf, const double* coef, double* x, double* levels) {
    if (n < 1 || n > SW_IPM_MAX_TYPES || !offsets || !workers)
        return sw_fail(h, SW_ERR_INVALID, who + ": bad sizes or null pointers");
    if (offsets[0] != 0) return sw_fail(h, SW_ERR_INVALID, who + ": offsets must start at 0");
    for (int32_t i = 0; i < count; ++i) {
        const int64_t m = offsets[i + 1] - offsets[i];
        if (m < 0) return sw_fail(h, SW_ERR_INVALID, who + ": offsets must not decrease");
        if (m > SW_IPM_MAX_JOBS) return sw_fail(h, SW_ERR_INVALID, who + ": more than 16384 jobs in an instance");
        for (int32_t k = 0; k < n; ++k)
            if (workers[(size_t)i * n + k] < 0)
                return sw_fail(h, SW_ERR_INVALID, who + ": worker counts must be >= 0");
    }
    const int64_t total = offsets[count];
    if (total > 0 && (!sf || !coef || !x)) return sw_fail(h, SW_ERR_INVALID, who + ": null pointers");
    if (!h->mmfc) h->mmfc = new MmfcBufs();
    MmfcBufs* mb = (MmfcBufs*)h->mmfc;
    mb->shifts.assign((size_t)count, 0);
    for (int32_t i = 0; i < count; ++i) {
        double cmax = 0.0; /* the normalisation of sw_mmf_ipm.h: over the types that have workers */
        for (int64_t j = offsets[i]; j < offsets[i + 1]; ++j) {
            if (sf[j] < 1 || sf[j] > SW_MAX_WIDTH)
                return sw_fail(h, SW_ERR_INVALID, who + ": scale factors must be in [1,255]");
            for (int32_t k = 0; k < n; ++k) {
                const double c = coef[(size_t)j * n + k];
                if (!(c >= 0.0) || !isfinite(c))
                    return sw_fail(h, SW_ERR_INVALID, who + ": coefficients must be finite and >= 0");
                if (workers[(size_t)i * n + k] > 0 && c > cmax) cmax = c;
            }
        }
        mb->shifts[(size_t)i] = sw_lp_shift(cmax);
    }
    if (levels)
        for (int64_t i = 0; i < 2 * (int64_t)count; ++i) levels[i] = 0.0;
    if (total == 0) return SW_OK; /* only empty instances: policy.flatten returns None */
    SW_HIP(h, hipSetDevice(h->device));
    /* in : offsets[count+1] (int64) | coef[total·n] (double) | workers[count·n] | shifts[count] | sf[total] (int32)
     * out: x[total·n] | levels[count][3] (double) */
    const size_t C = (size_t)count, T = (size_t)total, N = (size_t)n;
    const size_t o_coef = (C + 1) * 8, o_w = o_coef + T * N * 8, o_sh = o_w + C * N * 4, o_sf = o_sh + C * 4;
    const size_t in_bytes = ipm_align8(o_sf + T * 4);
    const size_t o_lv = T * N * 8, out_bytes = o_lv + C * 3 * 8;
    sw_io_bufs* b = &h->io;
    SW_HIP(h, b->in.reserve(in_bytes));
    SW_HIP(h, b->out.reserve(out_bytes));
    SW_HIP(h, b->hin.reserve(in_bytes));
    SW_HIP(h, b->hout.reserve(out_bytes));
    SW_HIP(h, mb->ws.reserve((size_t)SW_IPM_FIELDS(n) * T));
    memcpy(b->hin.p, offsets, (C + 1) * 8);
    memcpy(b->hin.p + o_coef, coef, T * N * 8);
    memcpy(b->hin.p + o_w, workers, C * N * 4);
    memcpy(b->hin.p + o_sh, mb->shifts.data(), C * 4);
    memcpy(b->hin.p + o_sf, sf, T * 4);
    SW_HIP(h, hipMemcpyAsync(b->in.p, b->hin.p, in_bytes, hipMemcpyHostToDevice, h->stream));
    hipLaunchKernelGGL(sw_mmf_ipm_kernel, dim3((unsigned)count), dim3(SW_BLOCK), 0, h->stream,
                       (const int64_t*)b->in.p, n, (const int32_t*)(b->in.p + o_w), (const int32_t*)(b->in.p + o_sh),
                       (const int32_t*)(b->in.p + o_sf), (const double*)(b->in.p + o_coef), mb->ws.p,
                       (double*)b->out.p, (double*)(b->out.p + o_lv));
    SW_HIP(h, hipGetLastError());
    SW_HIP(h, hipMemcpyAsync(b->hout.p, b->out.p, out_bytes, hipMemcpyDeviceToHost, h->stream));
    SW_HIP(h, hipStreamSynchronize(h->stream));
    const double* lv = (const double*)(b->hout.p + o_lv);
    for (int32_t i = 0; i < count; ++i) {
        const int status = (int)lv[3 * (size_t)i + 2];
        if (status != SW_IPM_OK)
            return sw_fail(h, SW_ERR_CAPACITY,
                            who + (status == SW_IPM_CAP ? ": step cap reached"
                                                        : ": the reduced system lost positive definiteness") +
                                " (instance " + std::to_string(i) + ")");
    }
    memcpy(x, b->hout.p, T * N * 8);
    if (levels)
        for (int32_t i = 0; i < count; ++i) {
            levels[2 * (size_t)i] = lv[3 * (size_t)i];
            levels[2 * (size_t)i + 1] = lv[3 * (size_t)i + 1];
        }
    return SW_OK;
}

}  // namespace

void sw_mmfc_release(sw_handle* h) {
    if (!h || !h->mmfc) return;
    MmfcBufs* b = (MmfcBufs*)h->mmfc;
    b->ws.release();
    delete b;
    h->mmfc = nullptr;
}

extern "C" int sw_mmf_allocate_types_centred(sw_handle* h, int32_t num_jobs, int32_t num_types,
                                             const int32_t* workers, const int32_t* scale_factors,
                                             const double* coefficients, double* allocation, double* level) {
    if (!h) return SW_ERR_INVALID;
    if (num_jobs < 0) return sw_fail(h, SW_ERR_INVALID, "sw_mmf_allocate_types_centred: num_jobs < 0");
    const int64_t offsets[2] = {0, num_jobs};
    return mmfc_run(h, "sw_mmf_allocate_types_centred", 1, num_types, offsets, workers, scale_factors,
                    coefficients, allocation, level);
}

extern "C" int sw_mmf_allocate_types_centred_batch(sw_handle* h, int32_t count, int32_t num_types,
                                                   const int64_t* offsets, const int32_t* workers,
                                                   const int32_t* scale_factors, const double* coefficients,
                                                   double* allocation, double* levels) {
    if (!h) return SW_ERR_INVALID;
    if (count < 0) return sw_fail(h, SW_ERR_INVALID, "sw_mmf_allocate_types_centred_batch: count < 0");
    if (count == 0) return SW_OK;
    return mmfc_run(h, "sw_mmf_allocate_types_centred_batch", count, num_types, offsets, workers,
                    scale_factors, coefficients, allocation, levels);
}
