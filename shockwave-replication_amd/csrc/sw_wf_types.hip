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
 *   a stage    thread 0 alone decides whether there is one; the load pass on the
 *              current κ and β and ipm_start_tail; ipm_solve
 *              (sw_mmf_ipm_dev.h); the extrapolation's ratio test
 *              with the eased rows' lift (1 reduction); the classifying pass
 *              (1 reduction: the count of the jobs that froze, the ends of the
 *              statistic)
 *   a retry    a stage whose solve broke down is done again (thread 0 decides)
 *              with the ease and μ₁ eight times larger, at most twice
 *   the repeat with more than one stage: the last stage's shares are kept (1
 *              reduction: the capacity rows' slack), the stage is solved again
 *              at twice the ease, and the blend's ratio test (1 reduction)
 * Every loop exit is decided from LDS state after a barrier, so it is uniform
 * across the workgroup.  The host side of the call is the worker-type frame of
 * sw_types.h.  No grid-wide synchronisation, no inline assembly.
 *
 * Measured (profiles/wf_types_timing.json, wall time per call with the host's
 * checks and copies): 0.76 / 0.95 / 1.19 / 553 ms at (jobs, types) = (30, 3) /
 * (120, 3) / (400, 3) / (400, 8) in 1 / 1 / 1 / 62 stages (1 / 1 / 1 / 63 level
 * solves) and 19 – 2,076 Newton steps, next to 0.72 / 0.89 / 1.16 / 6.51 ms of
 * sw_mmf_allocate_types_centred on the first stage's rows: 1.03–1.35 of level
 * solves × one centred call; 256 instances of (30, 3) in one launch 4.43 ms,
 * 57.8k allocations/s.
 * Compile report (gfx950): 181 VGPRs, no VGPR spill, 454 SGPRs spilled to VGPR
 * lanes, 176 bytes of scratch per lane, 5.9 KB of LDS, 2 waves per SIMD.
 */
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/shockwave_amd.h"
#include "sw_block.h"
#include "sw_handle.h"
#include "sw_mmf_ipm_dev.h"
#include "sw_types.h"
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
    const ipm_chunk ch = ipm_chunk_of(offsets);
    const int64_t inst = ch.inst, base = ch.base;
    const int32_t m = ch.m, lo = ch.lo, hi = ch.hi;
    const int tid = threadIdx.x;
    double* out = results + 5 * inst;
    if (m <= 0) { /* uniform */
        ipm_zero_results<5>(out);
        return;
    }
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
        ipm_zero_results<5>(out);
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
        ipm_start_tail(g, R, J, sf, lo, hi, acc, mx, v, w);
        ipm_solve(g, R, J, sf, lo, hi, acc, mx, v, w);
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

int wft_run(sw_handle* h, const char* who, int32_t count, int32_t n, const int64_t* offsets, const int32_t* workers,
            const int32_t* sf, const double* coef, double* x, double* levels, double* results) {
    const sw_types_call c{who, count, n, offsets, workers, sf, {1, {{coef, true}}, true, true, 4},
                          x, levels, results, SW_WFT_FIELDS(n), SW_WFT_STALL, "a stage froze no job"};
    return sw_types_run(
        h, c,
        [&](int32_t i, int32_t* shift, int64_t* job) -> const char* {
            const int32_t* wk = workers + (size_t)i * n;
            bool any = false;
            for (int32_t k = 0; k < n; ++k) any = any || wk[k] > 0;
            double cmax = 0.0; /* the normalisation of sw_wf_types.h: over the types that have workers */
            for (int64_t j = offsets[i]; j < offsets[i + 1]; ++j) {
                *job = j - offsets[i];
                if (sf[j] < 1 || sf[j] > SW_MAX_WIDTH) return "scale factors must be in [1,255]";
                double best = 0.0;
                for (int32_t k = 0; k < n; ++k) {
                    const double cf = coef[(size_t)j * n + k];
                    if (!(cf >= 0.0) || !isfinite(cf)) return "coefficients must be finite and >= 0";
                    if (wk[k] > 0 && cf > best) best = cf;
                }
                if (any && !(best > 0.0)) return "a job has no positive coefficient on a type with workers";
                if (best > cmax) cmax = best;
            }
            *shift = sw_lp_shift(cmax);
            return nullptr;
        },
        [](const sw_types_dev& d) {
            hipLaunchKernelGGL(sw_wf_types_kernel, dim3(d.count), dim3(SW_BLOCK), 0, d.stream, d.offsets, d.n,
                               d.workers, d.shifts, d.sf, d.col[0], d.ws, d.x, d.levels, d.results);
        });
}

}  // namespace

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
