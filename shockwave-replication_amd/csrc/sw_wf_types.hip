/*
 * sw_wf_types.hip — the water-filling MaxMinFairness allocation over worker
 * types that differ as one HIP workgroup per instance, behind
 * sw_wf_allocate_types() / sw_wf_allocate_types_batch().
 *
 * The method and its arithmetic are in sw_wf_types.h: the lexicographic
 * max-min vector of the jobs' values by stages, every stage a cold-started
 * level solve of the interior-point engine of sw_mmf_ipm.h on the rows
 * t ≤ val_j (unfrozen) and F_j ≤ val_j (frozen), the bottlenecks of a stage
 * read off its strictly complementary end point.  One launch per call; a grid
 * of `count` 512-thread workgroups, each given its instance by an offsets array
 * (CSR); the single call is count = 1.  Thread L owns the contiguous job chunk
 * [L·q, (L+1)·q) of the deterministic sum (q = ⌈m/512⌉), so the CPU twin
 * (tests/twins/wft_twin.c) returns the same bits.
 *
 *   per job    the engine's workspace, two more fields (the stage the job
 *              froze in, its level) and the last stage's shares: 9·na + 23
 *              doubles on the handle (HBM, L2-resident at these sizes),
 *              structure of arrays
 *   LDS        sw_ipm_glob (4 KB), sw_wft_glob (the stage loop) and the
 *              reduction scratch (sw_mmf_ipm_dev.h)
 *   a stage    thread 0 alone decides whether there is one; the engine's three
 *              start passes on the current κ and β; the Newton loop of
 *              sw_mmf_ipm.hip, pass for pass; the extrapolation's ratio test
 *              with the eased rows' lift (1 reduction); the classifying pass
 *              (1 reduction: the count of the jobs that froze, the ends of the
 *              statistic)
 *   a retry    a stage whose solve broke down is done again (thread 0 decides)
 *              with the ease and μ₁ eight times larger, at most twice
 *   the repeat with more than one stage: the last stage's shares are kept (1
 *              reduction: the capacity rows' slack), the stage is solved again
 *              at twice the ease, and the blend's ratio test (1 reduction)
 * Every loop exit is decided from LDS state after a barrier, so it is uniform
 * across the workgroup.  No grid-wide synchronisation, no inline assembly.
 *
 * Measured (profiles/wf_types_timing.json, wall time per call with the host's
 * checks and copies): 0.76 / 0.95 / 1.19 / 553 ms at (jobs, types) = (30, 3) /
 * (120, 3) / (400, 3) / (400, 8) in 1 / 1 / 1 / 62 stages (1 / 1 / 1 / 63 level
 * solves) and 19 – 2,076 Newton steps, next to 0.72 / 0.89 / 1.16 / 6.51 ms of
 * sw_mmf_allocate_types_centred on the first stage's rows: 1.03–1.35 of level
 * solves × one centred call; 256 instances of (30, 3) in one launch 4.43 ms,
 * 57.8k allocations/s.  250 VGPRs, none spilled, 443 SGPRs spilled to VGPR
 * lanes, 176 bytes of scratch per lane, 5.9 KB of LDS, 2 waves per SIMD.
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
#include "sw_mmf_ipm_dev.h"
#include "sw_wf_types.h"

namespace {

/* results: [count][5] = last level, Newton steps, stages, flags, status (SW_IPM_OK / _CAP / _BREAK, SW_WFT_STALL) */
__global__ __launch_bounds__(SW_BLOCK) void sw_wf_types_kernel(const int64_t* __restrict__ offsets, int32_t n,
                                                               const int32_t* __restrict__ workers,
                                                               const int32_t* __restrict__ shifts,
                                                               const int32_t* __restrict__ sfs,
                                                               const double* __restrict__ coef,
                                                               double* __restrict__ ws, double* __restrict__ x,
                                                               double* __restrict__ levels,
                                                               double* __restrict__ results) {
    __shared__ sw_ipm_glob G;
    __shared__ sw_wft_glob Q;
    __shared__ IpmRed R;
    __shared__ int32_t go;
    sw_ipm_glob* g = &G;
    sw_wft_glob* qs = &Q;
    const int64_t inst = blockIdx.x;
    const int64_t base = offsets[inst];
    const int32_t m = (int32_t)(offsets[inst + 1] - base);
    const int tid = threadIdx.x;
    double* out = results + 5 * inst;
    if (m <= 0) { /* uniform */
        if (tid == 0)
            for (int i = 0; i < 5; ++i) out[i] = 0.0;
        return;
    }
    const int32_t q = (m + SW_BLOCK - 1) / SW_BLOCK;
    const int32_t lo = tid * q < m ? tid * q : m;
    const int32_t hi = lo + q < m ? lo + q : m;
    const int32_t* sf = sfs + base;
    const double* cf = coef + base * n;
    double* xo = x + base * n;
    double* lv = levels + base;

    if (tid == 0) {
        sw_ipm_setup(g, m, n, workers + inst * n);
        sw_wft_begin(qs, m, shifts[inst]);
    }
    __syncthreads();
    const int32_t na = g->na; /* the same at every stage */
    if (na == 0) {            /* uniform: no type has workers */
        for (int32_t j = lo; j < hi; ++j) {
            for (int32_t k = 0; k < n; ++k) xo[(int64_t)j * n + k] = 0.0;
            lv[j] = 0.0;
        }
        if (tid == 0)
            for (int i = 0; i < 5; ++i) out[i] = 0.0;
        return;
    }
    sw_ipm_job J{ws + (int64_t)SW_WFT_FIELDS(n) * base, m, 0, na, 0.0};
    double acc[SW_IPM_NRED], mx[SW_IPM_NMAX];
    double v[SW_IPM_NRED], w[SW_IPM_NMAX];
    for (int32_t j = lo; j < hi; ++j) {
        J.j = j;
        sw_wft_job_begin(&J);
    }

    /* the stages: each freezes at least one job, so at most m; then the repeat of the last */
    for (int32_t stage = 0; stage <= (SW_WFT_TRIES + 1) * m; ++stage) {
        if (tid == 0) go = sw_wft_next(qs) ? 1 : sw_wft_repeat(qs) ? 2 : 0;
        __syncthreads();
        if (!go) break; /* uniform */
        if (go == 2) { /* uniform: the engine's end point of the last stage is still in place */
            ipm_clear(acc, mx);
            for (int32_t j = lo; j < hi; ++j) {
                J.j = j; J.sf = (double)sf[j];
                sw_wft_job_keep(g, qs, &J, v);
                ipm_take(acc, v, na, mx, w, 0);
            }
            ipm_publish(R, acc, na, mx, 0);
            if (tid == 0) { ipm_combine(R, na, 0); sw_wft_glob_keep(g, qs, R.sums); }
        }
        __syncthreads();
        if (tid == 0) {
            sw_ipm_setup(g, m, n, workers + inst * n);
            sw_wft_setup(g, qs);
        }
        __syncthreads();
        /* the engine's start on the stage's rows */
        ipm_clear(acc, mx);
        for (int32_t j = lo; j < hi; ++j) {
            J.j = j; J.sf = (double)sf[j];
            sw_wft_job_load(g, qs, &J, cf + (int64_t)j * n, v, w);
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
        if (g->status != SW_IPM_OK) { /* uniform: again at a larger ease, or the end */
            if (tid == 0) go = sw_wft_retry(g, qs);
            __syncthreads();
            const int32_t again = go;
            __syncthreads(); /* every wave has read `go` before the loop's head writes it */
            if (again == 1) continue;
            break;
        }
        /* the level is reached (every job has a positive coefficient on a type with workers and a
         * stage has an unfrozen job, so the level is a variable and both path points were taken):
         * the ratio test of the extrapolation and the eased rows' lift */
        ipm_clear(acc, mx);
        for (int32_t j = lo; j < hi; ++j) {
            J.j = j; J.sf = (double)sf[j];
            sw_ipm_job_final(g, &J, v, w);
            v[na] = sw_wft_job_lift(&J);
            ipm_take(acc, v, na + 1, mx, w, 1);
        }
        ipm_publish(R, acc, na + 1, mx, 1);
        if (tid == 0) {
            ipm_combine(R, na + 1, 1);
            sw_ipm_glob_final(g, R.sums, R.maxes);
            sw_wft_glob_level(g, qs, R.sums[na]);
        }
        __syncthreads();
        if (qs->rep == 1) { /* uniform: the repeat ends the call with the blend's ratio test */
            ipm_clear(acc, mx);
            for (int32_t j = lo; j < hi; ++j) {
                J.j = j; J.sf = (double)sf[j];
                sw_wft_job_blend(g, qs, &J, v, w);
                ipm_take(acc, v, na, mx, w, 1);
            }
            ipm_publish(R, acc, na, mx, 1);
            if (tid == 0) { ipm_combine(R, na, 1); sw_wft_glob_blend(g, qs, R.sums, R.maxes); }
            break;
        }
        /* the bottlenecks of the stage freeze */
        ipm_clear(acc, mx);
        for (int32_t j = lo; j < hi; ++j) {
            J.j = j; J.sf = (double)sf[j];
            sw_wft_job_classify(g, qs, &J, v, w);
            ipm_take(acc, v, 1, mx, w, 2);
        }
        ipm_publish(R, acc, 1, mx, 2);
        if (tid == 0) { ipm_combine(R, 1, 2); sw_wft_feed(qs, R.sums[0], R.maxes); }
    }
    __syncthreads(); /* thread 0's last words on g and qs */

    for (int32_t j = lo; j < hi; ++j) {
        J.j = j; J.sf = (double)sf[j];
        sw_wft_job_emit(g, qs, &J, xo + (int64_t)j * n);
        lv[j] = sw_wft_job_level(qs, &J);
    }
    if (tid == 0) {
        sw_wft_result(qs, out);
        out[4] = (double)qs->status;
    }
}

struct WftBufs {
    DevBuf<double> ws;
    std::vector<int32_t> shifts;
};

int wft_run(sw_handle* h, const std::string& who, int32_t count, int32_t n, const int64_t* offsets,
            const int32_t* workers, const int32_t* sf, const double* coef, double* x, double* levels,
            double* results) {
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
    if (total > 0 && (!sf || !coef || !x || !levels)) return sw_fail(h, SW_ERR_INVALID, who + ": null pointers");
    if (!h->wft) h->wft = new WftBufs();
    WftBufs* wb = (WftBufs*)h->wft;
    wb->shifts.assign((size_t)count, 0);
    for (int32_t i = 0; i < count; ++i) {
        const int32_t* wk = workers + (size_t)i * n;
        bool any = false;
        for (int32_t k = 0; k < n; ++k) any = any || wk[k] > 0;
        double cmax = 0.0; /* the normalisation of sw_wf_types.h: over the types that have workers */
        for (int64_t j = offsets[i]; j < offsets[i + 1]; ++j) {
            const auto job = [&] { return " (job " + std::to_string(j - offsets[i]) + " of instance " + std::to_string(i) + ")"; };
            if (sf[j] < 1 || sf[j] > SW_MAX_WIDTH)
                return sw_fail(h, SW_ERR_INVALID, who + ": scale factors must be in [1,255]" + job());
            double best = 0.0;
            for (int32_t k = 0; k < n; ++k) {
                const double c = coef[(size_t)j * n + k];
                if (!(c >= 0.0) || !isfinite(c))
                    return sw_fail(h, SW_ERR_INVALID, who + ": coefficients must be finite and >= 0" + job());
                if (wk[k] > 0 && c > best) best = c;
            }
            if (any && !(best > 0.0))
                return sw_fail(h, SW_ERR_INVALID,
                               who + ": a job has no positive coefficient on a type with workers" + job());
            if (best > cmax) cmax = best;
        }
        wb->shifts[(size_t)i] = sw_lp_shift(cmax);
    }
    if (results)
        for (int64_t i = 0; i < 4 * (int64_t)count; ++i) results[i] = 0.0;
    if (total == 0) return SW_OK;
    SW_HIP(h, hipSetDevice(h->device));
    /* in : offsets[count+1] (int64) | coef[total·n] (double) | workers[count·n] | shifts[count] | sf[total] (int32)
     * out: x[total·n] | levels[total] | results[count][5] (double) */
    const size_t C = (size_t)count, T = (size_t)total, N = (size_t)n;
    const size_t o_coef = (C + 1) * 8, o_w = o_coef + T * N * 8, o_sh = o_w + C * N * 4, o_sf = o_sh + C * 4;
    const size_t in_bytes = ipm_align8(o_sf + T * 4);
    const size_t o_lv = T * N * 8, o_rs = o_lv + T * 8, out_bytes = o_rs + C * 5 * 8;
    sw_io_bufs* b = &h->io;
    SW_HIP(h, b->in.reserve(in_bytes));
    SW_HIP(h, b->out.reserve(out_bytes));
    SW_HIP(h, b->hin.reserve(in_bytes));
    SW_HIP(h, b->hout.reserve(out_bytes));
    SW_HIP(h, wb->ws.reserve((size_t)SW_WFT_FIELDS(n) * T));
    memcpy(b->hin.p, offsets, (C + 1) * 8);
    memcpy(b->hin.p + o_coef, coef, T * N * 8);
    memcpy(b->hin.p + o_w, workers, C * N * 4);
    memcpy(b->hin.p + o_sh, wb->shifts.data(), C * 4);
    memcpy(b->hin.p + o_sf, sf, T * 4);
    SW_HIP(h, hipMemcpyAsync(b->in.p, b->hin.p, in_bytes, hipMemcpyHostToDevice, h->stream));
    hipLaunchKernelGGL(sw_wf_types_kernel, dim3((unsigned)count), dim3(SW_BLOCK), 0, h->stream,
                       (const int64_t*)b->in.p, n, (const int32_t*)(b->in.p + o_w), (const int32_t*)(b->in.p + o_sh),
                       (const int32_t*)(b->in.p + o_sf), (const double*)(b->in.p + o_coef), wb->ws.p,
                       (double*)b->out.p, (double*)(b->out.p + o_lv), (double*)(b->out.p + o_rs));
    SW_HIP(h, hipGetLastError());
    SW_HIP(h, hipMemcpyAsync(b->hout.p, b->out.p, out_bytes, hipMemcpyDeviceToHost, h->stream));
    SW_HIP(h, hipStreamSynchronize(h->stream));
    const double* rs = (const double*)(b->hout.p + o_rs);
    for (int32_t i = 0; i < count; ++i) {
        const int status = (int)rs[5 * (size_t)i + 4];
        if (status != SW_IPM_OK)
            return sw_fail(h, SW_ERR_CAPACITY,
                           who + (status == SW_IPM_CAP     ? ": step cap reached"
                                  : status == SW_WFT_STALL ? ": a stage froze no job"
                                                           : ": the reduced system lost positive definiteness") +
                               " (instance " + std::to_string(i) + ")");
    }
    memcpy(x, b->hout.p, T * N * 8);
    memcpy(levels, b->hout.p + o_lv, T * 8);
    if (results)
        for (int32_t i = 0; i < count; ++i)
            for (int c = 0; c < 4; ++c) results[4 * (size_t)i + c] = rs[5 * (size_t)i + c];
    return SW_OK;
}

}  // namespace

void sw_wft_release(sw_handle* h) {
    if (!h || !h->wft) return;
    WftBufs* b = (WftBufs*)h->wft;
    b->ws.release();
    delete b;
    h->wft = nullptr;
}

extern "C" int sw_wf_allocate_types(sw_handle* h, int32_t num_jobs, int32_t num_types, const int32_t* workers,
                                    const int32_t* scale_factors, const double* coefficients, double* allocation,
                                    double* levels, double* result) {
    if (!h) return SW_ERR_INVALID;
    if (num_jobs < 0) return sw_fail(h, SW_ERR_INVALID, "sw_wf_allocate_types: num_jobs < 0");
    const int64_t offsets[2] = {0, num_jobs};
    return wft_run(h, "sw_wf_allocate_types", 1, num_types, offsets, workers, scale_factors, coefficients,
                   allocation, levels, result);
}

extern "C" int sw_wf_allocate_types_batch(sw_handle* h, int32_t count, int32_t num_types, const int64_t* offsets,
                                          const int32_t* workers, const int32_t* scale_factors,
                                          const double* coefficients, double* allocation, double* levels,
                                          double* results) {
    if (!h) return SW_ERR_INVALID;
    if (count < 0) return sw_fail(h, SW_ERR_INVALID, "sw_wf_allocate_types_batch: count < 0");
    if (count == 0) return SW_OK;
    return wft_run(h, "sw_wf_allocate_types_batch", count, num_types, offsets, workers, scale_factors, coefficients,
                   allocation, levels, results);
}
