/*
 * sw_ftf_types.hip — the FinishTimeFairness (Themis) allocation over worker
 * types that differ as one HIP workgroup per instance, behind
 * sw_ftf_allocate_types() / sw_ftf_allocate_types_batch().
 *
 * The method and its arithmetic are in sw_ftf_types.h: ρ* is the root of
 * t*(ρ) = 1, t* the max-min level of the rows thr_jk·(ρ·E_j − a_j)/s_j by the
 * interior-point engine of sw_mmf_ipm.h, found by Newton steps on t* from the
 * aggregate lower bound, every probe a cold start of the engine.  One launch
 * per call; a grid of `count` 512-thread workgroups, each given its instance by
 * an offsets array (CSR); the single call is count = 1.  Thread L owns the
 * contiguous job chunk [L·q, (L+1)·q) of the deterministic sum (q = ⌈m/512⌉),
 * so the CPU twin (tests/twins/ftft_twin.c) returns the same bits.
 *
 *   per job    the engine's workspace, 8·na + 21 doubles on the handle (HBM,
 *              L2-resident at these sizes), structure of arrays
 *   LDS        sw_ipm_glob (4 KB), sw_ftft_glob (the outer iteration, the
 *              start's bisection) and the reduction scratch (sw_mmf_ipm_dev.h)
 *   start      ρ_box (1 reduction), then at most 66 reductions of the one-type
 *              capacity sum: the bisection over the bits of ρ
 *   a probe    thread 0 alone takes the next level from the outer iteration;
 *              the normalising shift at that level (1 reduction); the engine's
 *              load pass and ipm_start_tail; ipm_solve (sw_mmf_ipm_dev.h); the
 *              extrapolation's ratio test with the slope's sum (1 reduction);
 *              thread 0 feeds level and slope back
 *   centring   only when t*(ρ_box) > 1: one pass over the jobs instead of the
 *              start passes, then ipm_solve once more in the engine's
 *              objective-free mode
 * Every loop exit is decided from LDS state after a barrier, so it is uniform
 * across the workgroup.  The host side of the call is the worker-type frame of
 * sw_types.h.  No grid-wide synchronisation, no inline assembly.
 *
 * Measured (profiles/ftf_types_timing.json, wall time per call with the host's
 * checks and copies): 1.98 / 2.58 / 3.29 / 22.8 / 8.88 ms at (jobs, types) =
 * (30, 3) / (120, 3) / (400, 3) / (400, 8) / (2048, 3) in 3 / 3 / 3 / 3 / 2 level
 * solves and 51–87 Newton steps, next to 0.71 / 0.92 / 1.20 / 8.01 / 4.72 ms of
 * sw_mmf_allocate_types_centred on the rows at ρ*, one level solve: 0.92–0.95 of
 * solves × one centred call; 256 instances of (30, 3) in one launch 3.43 ms,
 * 74.6k allocations/s.
 * Compile report (gfx950): 158 VGPRs, no VGPR spill, 446 SGPRs spilled to VGPR
 * lanes, 176 bytes of scratch per lane, 5.8 KB of LDS, room for 3 waves per
 * SIMD (a workgroup is 2).
 */
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/shockwave_amd.h"
#include "sw_block.h"
#include "sw_handle.h"
#include "sw_mmf_ipm_dev.h"
#include "sw_ftf_types.h"
#include "sw_types.h"

namespace {

/* results: [count][6] = ρ*, t, Newton steps, level solves, flags, status (SW_IPM_OK / _CAP / _BREAK, SW_FTFT_CAP) */
__global__ __launch_bounds__(SW_BLOCK) void sw_ftf_types_kernel(const int64_t* __restrict__ offsets, int32_t n,
                                                                const int32_t* __restrict__ workers,
                                                                const int32_t* __restrict__ sfs,
                                                                const double* __restrict__ thr,
                                                                const double* __restrict__ steps,
                                                                const double* __restrict__ elapsed,
                                                                const double* __restrict__ expected,
                                                                double* __restrict__ ws, double* __restrict__ x,
                                                                double* __restrict__ results) {
    __shared__ sw_ipm_glob G;
    __shared__ sw_ftft_glob Q;
    __shared__ IpmRed R;
    __shared__ int32_t go;
    sw_ipm_glob* g = &G;
    sw_ftft_glob* qs = &Q;
    const ipm_chunk ch = ipm_chunk_of(offsets);
    const int64_t inst = ch.inst, base = ch.base;
    const int32_t m = ch.m, lo = ch.lo, hi = ch.hi;
    const int tid = threadIdx.x;
    double* out = results + 6 * inst;
    if (m <= 0) { /* uniform */
        ipm_zero_results<6>(out);
        return;
    }
    const int32_t* sf = sfs + base;
    const double* tp = thr + base * n;
    const double* st = steps + base;
    const double* el = elapsed + base;
    const double* ex = expected + base;
    double* xo = x + base * n;
#define SW_FTFT_JOB_IN tp + (int64_t)j * n, st[j], el[j], ex[j]

    if (tid == 0) sw_ipm_setup(g, m, n, workers + inst * n);
    __syncthreads();
    const int32_t na = g->na; /* the same at every probe */
    sw_ipm_job J{ws + (int64_t)SW_IPM_FIELDS(n) * base, m, 0, na, 0.0};
    double acc[SW_IPM_NRED], mx[SW_IPM_NMAX];
    double v[SW_IPM_NRED], w[SW_IPM_NMAX];

    /* ρ_box, then the aggregate start */
    ipm_clear(acc, mx);
    for (int32_t j = lo; j < hi; ++j) {
        sw_ftft_job_box(g, SW_FTFT_JOB_IN, v, w);
        ipm_take(acc, v, 1, mx, w, 1);
    }
    ipm_publish(R, acc, 1, mx, 1);
    if (tid == 0) { ipm_combine(R, 1, 1); sw_ftft_glob_box(g, qs, R.sums, R.maxes); }
    __syncthreads();
    if (na == 0) { /* uniform: no type has workers, so (validated) no job is live */
        for (int32_t j = lo; j < hi; ++j)
            for (int32_t k = 0; k < n; ++k) xo[(int64_t)j * n + k] = 0.0;
        if (tid == 0) {
            sw_ftft_result(qs, out);
            out[5] = 0.0;
        }
        return;
    }
    for (int32_t it = 0; it < SW_FTF_ITERS + 4; ++it) {
        if (tid == 0) go = sw_ftft_start_next(qs);
        __syncthreads();
        if (!go) break; /* uniform */
        ipm_clear(acc, mx);
        for (int32_t j = lo; j < hi; ++j) acc[0] = acc[0] + sw_ftft_job_cap(g, qs, (double)sf[j], SW_FTFT_JOB_IN);
        ipm_publish(R, acc, 1, mx, 0);
        if (tid == 0) { ipm_combine(R, 1, 0); sw_ftft_start_feed(qs, R.sums[0]); }
    }
    __syncthreads(); /* every wave has read the start loop's last `go` before the probe loop writes it */

    /* the probes; at most one centring run after the last */
    for (int32_t probe = 0; probe < SW_FTFT_MAX_SOLVES + 2; ++probe) {
        if (tid == 0) {
            go = qs->centring ? 2 : sw_ftft_next(&qs->s, &qs->rho);
            if (go == 1) sw_ipm_setup(g, m, n, workers + inst * n);
        }
        __syncthreads();
        if (!go) break; /* uniform */
        if (go == 2) {
            for (int32_t j = lo; j < hi; ++j) {
                J.j = j; J.sf = (double)sf[j];
                sw_mtdt_job_switch(g, &J);
            }
        } else {
            /* the normalisation at this level, then the engine's start */
            ipm_clear(acc, mx);
            for (int32_t j = lo; j < hi; ++j) {
                w[0] = sw_ftft_job_rowmax(g, qs, SW_FTFT_JOB_IN);
                ipm_take(acc, v, 0, mx, w, 1);
            }
            ipm_publish(R, acc, 0, mx, 1);
            if (tid == 0) { ipm_combine(R, 0, 1); sw_ftft_glob_shift(qs, R.maxes); }
            __syncthreads();
            ipm_clear(acc, mx);
            for (int32_t j = lo; j < hi; ++j) {
                J.j = j; J.sf = (double)sf[j];
                sw_ftft_job_load(g, qs, &J, SW_FTFT_JOB_IN, v, w);
                ipm_take(acc, v, 2, mx, w, 1);
            }
            ipm_publish(R, acc, 2, mx, 1);
            if (tid == 0) { ipm_combine(R, 2, 1); sw_ftft_glob_load(g, qs, R.sums, R.maxes); }
            __syncthreads();
            ipm_start_tail(g, R, J, sf, lo, hi, acc, mx, v, w);
        }
        ipm_solve(g, R, J, sf, lo, hi, acc, mx, v, w);
        if (g->status != SW_IPM_OK) break; /* uniform */
        if (!g->has_t) {                   /* uniform: an objective-free run ends the call */
            if (tid == 0) sw_ftft_glob_free(g, qs);
            break;
        }
        /* the level is reached: the ratio test of the extrapolation and the slope, then the outer step */
        ipm_clear(acc, mx);
        for (int32_t j = lo; j < hi; ++j) {
            J.j = j; J.sf = (double)sf[j];
            sw_ipm_job_final(g, &J, v, w);
            v[na] = sw_ftft_job_slope(g, qs, &J, SW_FTFT_JOB_IN);
            ipm_take(acc, v, na + 1, mx, w, 1);
        }
        ipm_publish(R, acc, na + 1, mx, 1);
        if (tid == 0) {
            ipm_combine(R, na + 1, 1);
            sw_ipm_glob_final(g, R.sums, R.maxes);
            sw_ftft_glob_feed(g, qs, R.sums[na]);
            sw_ftft_glob_switch(g, qs);
        }
    }
    __syncthreads(); /* thread 0's last words on g and qs */

    for (int32_t j = lo; j < hi; ++j) {
        J.j = j; J.sf = (double)sf[j];
        sw_ipm_job_emit(g, &J, xo + (int64_t)j * n);
    }
    if (tid == 0) {
        sw_ftft_result(qs, out);
        out[5] = (double)(g->status != SW_IPM_OK ? g->status : qs->s.status);
    }
#undef SW_FTFT_JOB_IN
}

int ftft_run(sw_handle* h, const char* who, int32_t count, int32_t n, const int64_t* offsets, const int32_t* workers,
             const int32_t* sf, const double* thr, const double* steps, const double* elapsed, const double* expected,
             double* x, double* results) {
    const sw_types_call c{who, count, n, offsets, workers, sf,
                          {4, {{thr, true}, {steps, false}, {elapsed, false}, {expected, false}}, false, false, 5},
                          x, nullptr, results, SW_IPM_FIELDS(n), SW_FTFT_CAP, "level solve cap reached"};
    return sw_types_run(
        h, c,
        [&](int32_t i, int32_t*, int64_t* job) -> const char* {
            const int32_t* wk = workers + (size_t)i * n;
            double box = 0.0;
            for (int pass = 0; pass < 2; ++pass) /* 0: every value and ρ_box; 1: the rows at ρ_box */
                for (int64_t j = offsets[i]; j < offsets[i + 1]; ++j) {
                    *job = j - offsets[i];
                    const double s = steps[j], a = elapsed[j], E = expected[j];
                    double best = 0.0;
                    for (int32_t k = 0; k < n; ++k) {
                        const double t = thr[(size_t)j * n + k];
                        if (!(t >= 0.0) || !isfinite(t)) return "throughputs must be finite and >= 0";
                        if (wk[k] > 0 && t > best) best = t;
                    }
                    if (pass == 1) {
                        if (s > 0.0 && !isfinite(sw_ftft_coef(best, sw_ftft_d(s / best, a, E, box), s)))
                            return "throughput x time / steps overflows";
                        continue;
                    }
                    if (sf[j] < 1 || sf[j] > SW_MAX_WIDTH) return "scale factors must be in [1,255]";
                    if (!(s >= 0.0) || !isfinite(s)) return "steps must be finite and >= 0";
                    if (!(a >= 0.0) || !isfinite(a)) return "elapsed times must be finite and >= 0";
                    if (!(E > 0.0) || !isfinite(E)) return "expected times must be finite and > 0";
                    if (s > 0.0) {
                        if (!(best > 0.0)) return "a job with steps left has no throughput on a type with workers";
                        if (!(s / best <= SW_MTD_FULL_TIME_MAX)) return "steps / throughput above 1e15 seconds";
                    }
                    const double b = sw_ftf_box(s > 0.0 ? s / best : 0.0, a, E);
                    if (!isfinite(b)) return "(elapsed + steps / throughput) / expected overflows";
                    if (b > box) box = b;
                }
            return nullptr;
        },
        [](const sw_types_dev& d) {
            hipLaunchKernelGGL(sw_ftf_types_kernel, dim3(d.count), dim3(SW_BLOCK), 0, d.stream, d.offsets, d.n,
                               d.workers, d.sf, d.col[0], d.col[1], d.col[2], d.col[3], d.ws, d.x, d.results);
        });
}

}  // namespace

extern "C" int sw_ftf_allocate_types(sw_handle* h, int32_t num_jobs, int32_t num_types, const int32_t* workers,
                                     const int32_t* scale_factors, const double* throughputs, const double* steps,
                                     const double* elapsed, const double* expected, double* allocation,
                                     double* result) {
    if (!h) return SW_ERR_INVALID;
    if (num_jobs < 0) return sw_fail(h, SW_ERR_INVALID, "sw_ftf_allocate_types: num_jobs < 0");
    const int64_t offsets[2] = {0, num_jobs};
    return ftft_run(h, "sw_ftf_allocate_types", 1, num_types, offsets, workers, scale_factors, throughputs, steps,
                    elapsed, expected, allocation, result);
}

extern "C" int sw_ftf_allocate_types_batch(sw_handle* h, int32_t count, int32_t num_types, const int64_t* offsets,
                                           const int32_t* workers, const int32_t* scale_factors,
                                           const double* throughputs, const double* steps, const double* elapsed,
                                           const double* expected, double* allocation, double* results) {
    if (!h) return SW_ERR_INVALID;
    if (count < 0) return sw_fail(h, SW_ERR_INVALID, "sw_ftf_allocate_types_batch: count < 0");
    if (count == 0) return SW_OK;
    return ftft_run(h, "sw_ftf_allocate_types_batch", count, num_types, offsets, workers, scale_factors,
                    throughputs, steps, elapsed, expected, allocation, results);
}
