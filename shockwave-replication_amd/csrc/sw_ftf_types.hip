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
 *              three start passes; the Newton loop of sw_mtd_types.hip, pass
 *              for pass; the extrapolation's ratio test with the slope's sum
 *              (1 reduction); thread 0 feeds level and slope back
 *   centring   only when t*(ρ_box) > 1: one pass over the jobs, then the same
 *              loop body once more in the engine's objective-free mode
 * Every loop exit is decided from LDS state after a barrier, so it is uniform
 * across the workgroup.  No grid-wide synchronisation, no inline assembly.
 *
 * Measured (profiles/ftf_types_timing.json, wall time per call with the host's
 * checks and copies): 1.98 / 2.58 / 3.29 / 22.8 / 8.88 ms at (jobs, types) =
 * (30, 3) / (120, 3) / (400, 3) / (400, 8) / (2048, 3) in 3 / 3 / 3 / 3 / 2 level
 * solves and 51–87 Newton steps, next to 0.71 / 0.92 / 1.20 / 8.01 / 4.72 ms of
 * sw_mmf_allocate_types_centred on the rows at ρ*, one level solve: 0.92–0.95 of
 * solves × one centred call; 256 instances of (30, 3) in one launch 3.43 ms,
 * 74.6k allocations/s.  171 VGPRs, no VGPR spill, 435 SGPRs spilled to VGPR
 * lanes, 176 bytes of scratch per lane, 5.8 KB of LDS, 2 waves per SIMD (the
 * worker-type MinTotalDuration kernel: 213 VGPRs, no VGPR spill, 5.8 KB).
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
#include "sw_ftf_types.h"

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
    const int64_t inst = blockIdx.x;
    const int64_t base = offsets[inst];
    const int32_t m = (int32_t)(offsets[inst + 1] - base);
    const int tid = threadIdx.x;
    double* out = results + 6 * inst;
    if (m <= 0) { /* uniform */
        if (tid == 0)
            for (int i = 0; i < 6; ++i) out[i] = 0.0;
        return;
    }
    const int32_t q = (m + SW_BLOCK - 1) / SW_BLOCK;
    const int32_t lo = tid * q < m ? tid * q : m;
    const int32_t hi = lo + q < m ? lo + q : m;
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

struct FtftBufs {
    DevBuf<double> ws;
};

int ftft_run(sw_handle* h, const std::string& who, int32_t count, int32_t n, const int64_t* offsets,
             const int32_t* workers, const int32_t* sf, const double* thr, const double* steps, const double* elapsed,
             const double* expected, double* x, double* results) {
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
    if (total > 0 && (!sf || !thr || !steps || !elapsed || !expected || !x))
        return sw_fail(h, SW_ERR_INVALID, who + ": null pointers");
    for (int32_t i = 0; i < count; ++i) {
        const int32_t* wk = workers + (size_t)i * n;
        double box = 0.0;
        for (int pass = 0; pass < 2; ++pass) /* 0: every value and ρ_box; 1: the rows at ρ_box */
            for (int64_t j = offsets[i]; j < offsets[i + 1]; ++j) {
                const auto job = [&] { return " (job " + std::to_string(j - offsets[i]) + " of instance " + std::to_string(i) + ")"; };
                const double s = steps[j], a = elapsed[j], E = expected[j];
                double best = 0.0;
                for (int32_t k = 0; k < n; ++k) {
                    const double c = thr[(size_t)j * n + k];
                    if (!(c >= 0.0) || !isfinite(c))
                        return sw_fail(h, SW_ERR_INVALID, who + ": throughputs must be finite and >= 0" + job());
                    if (wk[k] > 0 && c > best) best = c;
                }
                if (pass == 1) {
                    if (s > 0.0 && !isfinite(sw_ftft_coef(best, sw_ftft_d(s / best, a, E, box), s)))
                        return sw_fail(h, SW_ERR_INVALID, who + ": throughput x time / steps overflows" + job());
                    continue;
                }
                if (sf[j] < 1 || sf[j] > SW_MAX_WIDTH)
                    return sw_fail(h, SW_ERR_INVALID, who + ": scale factors must be in [1,255]" + job());
                if (!(s >= 0.0) || !isfinite(s))
                    return sw_fail(h, SW_ERR_INVALID, who + ": steps must be finite and >= 0" + job());
                if (!(a >= 0.0) || !isfinite(a))
                    return sw_fail(h, SW_ERR_INVALID, who + ": elapsed times must be finite and >= 0" + job());
                if (!(E > 0.0) || !isfinite(E))
                    return sw_fail(h, SW_ERR_INVALID, who + ": expected times must be finite and > 0" + job());
                if (s > 0.0) {
                    if (!(best > 0.0))
                        return sw_fail(h, SW_ERR_INVALID,
                                       who + ": a job with steps left has no throughput on a type with workers" + job());
                    if (!(s / best <= SW_MTD_FULL_TIME_MAX))
                        return sw_fail(h, SW_ERR_INVALID, who + ": steps / throughput above 1e15 seconds" + job());
                }
                const double b = sw_ftf_box(s > 0.0 ? s / best : 0.0, a, E);
                if (!isfinite(b))
                    return sw_fail(h, SW_ERR_INVALID, who + ": (elapsed + steps / throughput) / expected overflows" + job());
                if (b > box) box = b;
            }
    }
    if (results)
        for (int64_t i = 0; i < 5 * (int64_t)count; ++i) results[i] = 0.0;
    if (total == 0) return SW_OK;
    SW_HIP(h, hipSetDevice(h->device));
    if (!h->ftft) h->ftft = new FtftBufs();
    FtftBufs* fb = (FtftBufs*)h->ftft;
    /* in : offsets[count+1] (int64) | thr[total·n] | steps, elapsed, expected[total] (double) | workers[count·n] |
     *      sf[total] (int32)
     * out: x[total·n] | results[count][6] (double) */
    const size_t C = (size_t)count, T = (size_t)total, N = (size_t)n;
    const size_t o_thr = (C + 1) * 8, o_st = o_thr + T * N * 8, o_el = o_st + T * 8, o_ex = o_el + T * 8,
                 o_w = o_ex + T * 8, o_sf = o_w + C * N * 4;
    const size_t in_bytes = ipm_align8(o_sf + T * 4);
    const size_t o_rs = T * N * 8, out_bytes = o_rs + C * 6 * 8;
    sw_io_bufs* b = &h->io;
    SW_HIP(h, b->in.reserve(in_bytes));
    SW_HIP(h, b->out.reserve(out_bytes));
    SW_HIP(h, b->hin.reserve(in_bytes));
    SW_HIP(h, b->hout.reserve(out_bytes));
    SW_HIP(h, fb->ws.reserve((size_t)SW_IPM_FIELDS(n) * T));
    memcpy(b->hin.p, offsets, (C + 1) * 8);
    memcpy(b->hin.p + o_thr, thr, T * N * 8);
    memcpy(b->hin.p + o_st, steps, T * 8);
    memcpy(b->hin.p + o_el, elapsed, T * 8);
    memcpy(b->hin.p + o_ex, expected, T * 8);
    memcpy(b->hin.p + o_w, workers, C * N * 4);
    memcpy(b->hin.p + o_sf, sf, T * 4);
    SW_HIP(h, hipMemcpyAsync(b->in.p, b->hin.p, in_bytes, hipMemcpyHostToDevice, h->stream));
    hipLaunchKernelGGL(sw_ftf_types_kernel, dim3((unsigned)count), dim3(SW_BLOCK), 0, h->stream,
                       (const int64_t*)b->in.p, n, (const int32_t*)(b->in.p + o_w), (const int32_t*)(b->in.p + o_sf),
                       (const double*)(b->in.p + o_thr), (const double*)(b->in.p + o_st),
                       (const double*)(b->in.p + o_el), (const double*)(b->in.p + o_ex), fb->ws.p, (double*)b->out.p,
                       (double*)(b->out.p + o_rs));
    SW_HIP(h, hipGetLastError());
    SW_HIP(h, hipMemcpyAsync(b->hout.p, b->out.p, out_bytes, hipMemcpyDeviceToHost, h->stream));
    SW_HIP(h, hipStreamSynchronize(h->stream));
    const double* rs = (const double*)(b->hout.p + o_rs);
    for (int32_t i = 0; i < count; ++i) {
        const int status = (int)rs[6 * (size_t)i + 5];
        if (status != SW_IPM_OK)
            return sw_fail(h, SW_ERR_CAPACITY,
                           who + (status == SW_IPM_CAP     ? ": step cap reached"
                                  : status == SW_FTFT_CAP ? ": level solve cap reached"
                                                          : ": the reduced system lost positive definiteness") +
                               " (instance " + std::to_string(i) + ")");
    }
    memcpy(x, b->hout.p, T * N * 8);
    if (results)
        for (int32_t i = 0; i < count; ++i)
            for (int c = 0; c < 5; ++c) results[5 * (size_t)i + c] = rs[6 * (size_t)i + c];
    return SW_OK;
}

}  // namespace

void sw_ftft_release(sw_handle* h) {
    if (!h || !h->ftft) return;
    FtftBufs* b = (FtftBufs*)h->ftft;
    b->ws.release();
    delete b;
    h->ftft = nullptr;
}

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
