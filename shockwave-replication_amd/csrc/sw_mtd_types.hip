/*
 * sw_mtd_types.hip — the MinTotalDuration allocation over worker types that
 * differ as one HIP workgroup per instance, behind sw_mtd_allocate_types() /
 * sw_mtd_allocate_types_batch().
 *
 * The method and its arithmetic are in sw_mtd_types.h: the max-min level of
 * steps-normalised throughput by the interior-point engine of sw_mmf_ipm.h,
 * the reference's search over T as scalar work on that level, and the analytic
 * centre of the feasible polytope at the found T by the engine's objective-free
 * mode from the level's second path point.  One launch per call; a grid of
 * `count` 512-thread workgroups, each given its instance by an offsets array
 * (CSR); the single call is count = 1.  Thread L owns the contiguous job chunk
 * [L·q, (L+1)·q) of the deterministic sum (q = ⌈m/512⌉), so the CPU twin
 * (tests/twins/mtdt_twin.c) returns the same bits.
 *
 *   per job    the engine's workspace, 8·na + 21 doubles on the handle (HBM,
 *              L2-resident at these sizes), structure of arrays
 *   LDS        sw_ipm_glob (4 KB), sw_mtdt_glob (T, t*, flags) and the
 *              reduction scratch (sw_mmf_ipm_dev.h)
 *   a phase    the Newton loop of sw_mmf_ipm.hip, pass for pass
 *   between    the extrapolation's ratio test (1 reduction), then thread 0
 *              alone between two barriers: the level, the search (at most
 *              SW_MTD_MAX_PROBES multiplications and comparisons), the thin
 *              rule or the switch of the global state; then one pass over the
 *              jobs (duals onto z·s = 1, value slacks onto the fixed level)
 * Both phases are the same loop body run at most twice: the phase is a field
 * of the LDS state, not a register carried through the loop.  No grid-wide
 * synchronisation, no inline assembly.
 *
 * Measured (profiles/mtd_types_timing.json, wall time per call with the host's
 * checks and copies): 0.87 / 0.94 / 1.20 / 6.38 / 4.17 ms at (jobs, types) =
 * (30, 3) / (120, 3) / (400, 3) / (400, 8) / (2048, 3) in 23–26 Newton steps of
 * both phases, next to 0.79 / 0.81 / 1.01 / 6.13 / 3.65 ms of
 * sw_mmf_allocate_types_centred on the level program alone; 256 instances of
 * (30, 3) in one launch 1.70 ms, 151k allocations/s.  213 VGPRs, no VGPR spill,
 * 5.8 KB of LDS (the centred MaxMinFairness kernel: 241, none, 5.7 KB).
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
#include "sw_mtd_types.h"

namespace {

/* results: [count][5] = T, t*, Newton steps, flags, status (SW_IPM_OK / _CAP / _BREAK) */
__global__ __launch_bounds__(SW_BLOCK) void sw_mtd_types_kernel(const int64_t* __restrict__ offsets, int32_t n,
                                                                const int32_t* __restrict__ workers,
                                                                const int32_t* __restrict__ shifts,
                                                                const int32_t* __restrict__ sfs,
                                                                const double* __restrict__ thr,
                                                                const double* __restrict__ steps,
                                                                double* __restrict__ ws, double* __restrict__ x,
                                                                double* __restrict__ results) {
    __shared__ sw_ipm_glob G;
    __shared__ sw_mtdt_glob Q;
    __shared__ IpmRed R;
    __shared__ int32_t go;
    sw_ipm_glob* g = &G;
    sw_mtdt_glob* qs = &Q;
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
    const int32_t shift = shifts[inst];
    const int32_t* sf = sfs + base;
    const double* tp = thr + base * n;
    const double* st = steps + base;
    double* xo = x + base * n;

    if (tid == 0) {
        sw_ipm_setup(g, m, n, workers + inst * n);
        sw_mtdt_setup(qs);
    }
    __syncthreads();
    const int32_t na = g->na;
    if (na == 0) { /* uniform: no type has workers, so (validated) no job is live */
        for (int32_t j = lo; j < hi; ++j)
            for (int32_t k = 0; k < n; ++k) xo[(int64_t)j * n + k] = 0.0;
        if (tid == 0) {
            qs->flags = SW_MTDT_IDLE;
            sw_mtdt_search(qs, 0.0, 1);
            sw_mtdt_result(g, qs, out);
            out[4] = 0.0;
        }
        return;
    }
    sw_ipm_job J{ws + (int64_t)SW_IPM_FIELDS(n) * base, m, 0, na, 0.0};
    double acc[SW_IPM_NRED], mx[SW_IPM_NMAX];
    double v[SW_IPM_NRED], w[SW_IPM_NMAX];

    /* the start */
    ipm_clear(acc, mx);
    for (int32_t j = lo; j < hi; ++j) {
        J.j = j; J.sf = (double)sf[j];
        sw_mtdt_job_load(g, &J, tp + (int64_t)j * n, st[j], shift, v, w);
        ipm_take(acc, v, 3, mx, w, 1);
    }
    ipm_publish(R, acc, 3, mx, 1);
    if (tid == 0) { ipm_combine(R, 3, 1); sw_mtdt_glob_load(g, qs, R.sums, R.maxes); }
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

    for (int32_t phase = 0; phase < 2; ++phase) {
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
        if (g->status != SW_IPM_OK || !g->has_t) break; /* uniform: an error, or the centre is reached */
        /* the level is reached: the ratio test of the extrapolation, then the search */
        ipm_clear(acc, mx);
        for (int32_t j = lo; j < hi; ++j) {
            J.j = j; J.sf = (double)sf[j];
            sw_ipm_job_final(g, &J, v, w);
            ipm_take(acc, v, na, mx, w, 1);
        }
        ipm_publish(R, acc, na, mx, 1);
        if (tid == 0) {
            ipm_combine(R, na, 1);
            sw_ipm_glob_final(g, R.sums, R.maxes);
            go = sw_mtdt_glob_switch(g, qs, shift);
        }
        __syncthreads();
        if (!go) break; /* uniform: the thin rule, the extrapolated point is the answer */
        for (int32_t j = lo; j < hi; ++j) {
            J.j = j; J.sf = (double)sf[j];
            sw_mtdt_job_switch(g, &J);
        }
    }

    for (int32_t j = lo; j < hi; ++j) {
        J.j = j; J.sf = (double)sf[j];
        sw_ipm_job_emit(g, &J, xo + (int64_t)j * n);
    }
    if (tid == 0) {
        sw_mtdt_result(g, qs, out);
        out[4] = (double)g->status;
    }
}

struct MtdtBufs {
    DevBuf<double> ws;
    std::vector<int32_t> shifts;
};

int mtdt_run(sw_handle* h, const std::string& who, int32_t count, int32_t n, const int64_t* offsets,
             const int32_t* workers, const int32_t* sf, const double* thr, const double* steps, double* x,
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
    if (total > 0 && (!sf || !thr || !steps || !x)) return sw_fail(h, SW_ERR_INVALID, who + ": null pointers");
    if (!h->mtdt) h->mtdt = new MtdtBufs();
    MtdtBufs* mb = (MtdtBufs*)h->mtdt;
    mb->shifts.assign((size_t)count, 0);
    for (int32_t i = 0; i < count; ++i) {
        const int32_t* wk = workers + (size_t)i * n;
        double cmin = 0.0; /* the normalisation of sw_mtd_types.h */
        for (int64_t j = offsets[i]; j < offsets[i + 1]; ++j) {
            if (sf[j] < 1 || sf[j] > SW_MAX_WIDTH)
                return sw_fail(h, SW_ERR_INVALID, who + ": scale factors must be in [1,255]");
            const double s = steps[j];
            if (!(s >= 0.0) || !isfinite(s)) return sw_fail(h, SW_ERR_INVALID, who + ": steps must be finite and >= 0");
            double best = 0.0;
            for (int32_t k = 0; k < n; ++k) {
                const double c = thr[(size_t)j * n + k];
                if (!(c >= 0.0) || !isfinite(c))
                    return sw_fail(h, SW_ERR_INVALID, who + ": throughputs must be finite and >= 0");
                if (wk[k] > 0 && c > best) best = c;
            }
            if (s > 0.0) {
                const std::string job = " (job " + std::to_string(j - offsets[i]) + " of instance " + std::to_string(i) + ")";
                if (!(best > 0.0))
                    return sw_fail(h, SW_ERR_INVALID,
                                   who + ": a job with steps left has no throughput on a type with workers" + job);
                if (!(s / best <= SW_MTD_FULL_TIME_MAX))
                    return sw_fail(h, SW_ERR_INVALID, who + ": steps / throughput above 1e15 seconds" + job);
                const double rm = sw_mtdt_rowmax(n, wk, thr + (size_t)j * n, s);
                if (!isfinite(rm)) return sw_fail(h, SW_ERR_INVALID, who + ": throughput / steps overflows" + job);
                cmin = sw_mtdt_shift_take(cmin, rm);
            }
        }
        mb->shifts[(size_t)i] = sw_lp_shift(cmin);
    }
    if (results)
        for (int64_t i = 0; i < 4 * (int64_t)count; ++i) results[i] = 0.0;
    if (total == 0) return SW_OK;
    SW_HIP(h, hipSetDevice(h->device));
    /* in : offsets[count+1] (int64) | thr[total·n] | steps[total] (double) | workers[count·n] | shifts[count] |
     *      sf[total] (int32)
     * out: x[total·n] | results[count][5] (double) */
    const size_t C = (size_t)count, T = (size_t)total, N = (size_t)n;
    const size_t o_thr = (C + 1) * 8, o_st = o_thr + T * N * 8, o_w = o_st + T * 8, o_sh = o_w + C * N * 4,
                 o_sf = o_sh + C * 4;
    const size_t in_bytes = ipm_align8(o_sf + T * 4);
    const size_t o_rs = T * N * 8, out_bytes = o_rs + C * 5 * 8;
    sw_io_bufs* b = &h->io;
    SW_HIP(h, b->in.reserve(in_bytes));
    SW_HIP(h, b->out.reserve(out_bytes));
    SW_HIP(h, b->hin.reserve(in_bytes));
    SW_HIP(h, b->hout.reserve(out_bytes));
    SW_HIP(h, mb->ws.reserve((size_t)SW_IPM_FIELDS(n) * T));
    memcpy(b->hin.p, offsets, (C + 1) * 8);
    memcpy(b->hin.p + o_thr, thr, T * N * 8);
    memcpy(b->hin.p + o_st, steps, T * 8);
    memcpy(b->hin.p + o_w, workers, C * N * 4);
    memcpy(b->hin.p + o_sh, mb->shifts.data(), C * 4);
    memcpy(b->hin.p + o_sf, sf, T * 4);
    SW_HIP(h, hipMemcpyAsync(b->in.p, b->hin.p, in_bytes, hipMemcpyHostToDevice, h->stream));
    hipLaunchKernelGGL(sw_mtd_types_kernel, dim3((unsigned)count), dim3(SW_BLOCK), 0, h->stream,
                       (const int64_t*)b->in.p, n, (const int32_t*)(b->in.p + o_w), (const int32_t*)(b->in.p + o_sh),
                       (const int32_t*)(b->in.p + o_sf), (const double*)(b->in.p + o_thr),
                       (const double*)(b->in.p + o_st), mb->ws.p, (double*)b->out.p, (double*)(b->out.p + o_rs));
    SW_HIP(h, hipGetLastError());
    SW_HIP(h, hipMemcpyAsync(b->hout.p, b->out.p, out_bytes, hipMemcpyDeviceToHost, h->stream));
    SW_HIP(h, hipStreamSynchronize(h->stream));
    const double* rs = (const double*)(b->hout.p + o_rs);
    for (int32_t i = 0; i < count; ++i) {
        const int status = (int)rs[5 * (size_t)i + 4];
        if (status != SW_IPM_OK)
            return sw_fail(h, SW_ERR_CAPACITY,
                            who + (status == SW_IPM_CAP ? ": step cap reached"
                                                        : ": the reduced system lost positive definiteness") +
                                " (instance " + std::to_string(i) + ")");
    }
    memcpy(x, b->hout.p, T * N * 8);
    if (results)
        for (int32_t i = 0; i < count; ++i)
            for (int c = 0; c < 4; ++c) results[4 * (size_t)i + c] = rs[5 * (size_t)i + c];
    return SW_OK;
}

}  // namespace

void sw_mtdt_release(sw_handle* h) {
    if (!h || !h->mtdt) return;
    MtdtBufs* b = (MtdtBufs*)h->mtdt;
    b->ws.release();
    delete b;
    h->mtdt = nullptr;
}

extern "C" int sw_mtd_allocate_types(sw_handle* h, int32_t num_jobs, int32_t num_types, const int32_t* workers,
                                     const int32_t* scale_factors, const double* throughputs, const double* steps,
                                     double* allocation, double* result) {
    if (!h) return SW_ERR_INVALID;
    if (num_jobs < 0) return sw_fail(h, SW_ERR_INVALID, "sw_mtd_allocate_types: num_jobs < 0");
    const int64_t offsets[2] = {0, num_jobs};
    return mtdt_run(h, "sw_mtd_allocate_types", 1, num_types, offsets, workers, scale_factors, throughputs, steps,
                    allocation, result);
}

extern "C" int sw_mtd_allocate_types_batch(sw_handle* h, int32_t count, int32_t num_types, const int64_t* offsets,
                                           const int32_t* workers, const int32_t* scale_factors,
                                           const double* throughputs, const double* steps, double* allocation,
                                           double* results) {
    if (!h) return SW_ERR_INVALID;
    if (count < 0) return sw_fail(h, SW_ERR_INVALID, "sw_mtd_allocate_types_batch: count < 0");
    if (count == 0) return SW_OK;
    return mtdt_run(h, "sw_mtd_allocate_types_batch", count, num_types, offsets, workers, scale_factors,
                    throughputs, steps, allocation, results);
}
