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
 *   the start  the load pass (1 reduction of 3 sums, 1 max), then ipm_start_tail
 *   a phase    ipm_solve (sw_mmf_ipm_dev.h)
 *   between    the extrapolation's ratio test (1 reduction), then thread 0
 *              alone between two barriers: the level, the search (at most
 *              SW_MTD_MAX_PROBES multiplications and comparisons), the thin
 *              rule or the switch of the global state; then one pass over the
 *              jobs (duals onto z·s = 1, value slacks onto the fixed level)
 * Both phases are the same loop body run at most twice: the phase is a field
 * of the LDS state, not a register carried through the loop.  The host side of
 * the call is the worker-type frame of sw_types.h.  No grid-wide
 * synchronisation, no inline assembly.
 *
 * Measured (profiles/mtd_types_timing.json, wall time per call with the host's
 * checks and copies): 0.87 / 0.94 / 1.20 / 6.38 / 4.17 ms at (jobs, types) =
 * (30, 3) / (120, 3) / (400, 3) / (400, 8) / (2048, 3) in 23–26 Newton steps of
 * both phases, next to 0.79 / 0.81 / 1.01 / 6.13 / 3.65 ms of
 * sw_mmf_allocate_types_centred on the level program alone; 256 instances of
 * (30, 3) in one launch 1.70 ms, 151k allocations/s.
 * Compile report (gfx950): 198 VGPRs, no VGPR spill, 335 SGPRs spilled to VGPR
 * lanes, 176 bytes of scratch per lane, 5.6 KB of LDS, 2 waves per SIMD.
 */
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/shockwave_amd.h"
#include "sw_block.h"
#include "sw_handle.h"
#include "sw_mmf_ipm_dev.h"
#include "sw_mtd_types.h"
#include "sw_types.h"

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
    const ipm_chunk ch = ipm_chunk_of(offsets);
    const int64_t inst = ch.inst, base = ch.base;
    const int32_t m = ch.m, lo = ch.lo, hi = ch.hi;
    const int tid = threadIdx.x;
    double* out = results + 5 * inst;
    if (m <= 0) { /* uniform */
        ipm_zero_results<5>(out);
        return;
    }
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
    ipm_start_tail(g, R, J, sf, lo, hi, acc, mx, v, w);

    for (int32_t phase = 0; phase < 2; ++phase) {
        ipm_solve(g, R, J, sf, lo, hi, acc, mx, v, w);
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

int mtdt_run(sw_handle* h, const char* who, int32_t count, int32_t n, const int64_t* offsets, const int32_t* workers,
             const int32_t* sf, const double* thr, const double* steps, double* x, double* results) {
    const sw_types_call c{who, count, n, offsets, workers, sf, {2, {{thr, true}, {steps, false}}, true, false, 4},
                          x, nullptr, results, SW_IPM_FIELDS(n), 0, nullptr};
    return sw_types_run(
        h, c,
        [&](int32_t i, int32_t* shift, int64_t* job) -> const char* {
            const int32_t* wk = workers + (size_t)i * n;
            double cmin = 0.0; /* the normalisation of sw_mtd_types.h */
            for (int64_t j = offsets[i]; j < offsets[i + 1]; ++j) {
                if (sf[j] < 1 || sf[j] > SW_MAX_WIDTH) return "scale factors must be in [1,255]";
                const double s = steps[j];
                if (!(s >= 0.0) || !isfinite(s)) return "steps must be finite and >= 0";
                double best = 0.0;
                for (int32_t k = 0; k < n; ++k) {
                    const double t = thr[(size_t)j * n + k];
                    if (!(t >= 0.0) || !isfinite(t)) return "throughputs must be finite and >= 0";
                    if (wk[k] > 0 && t > best) best = t;
                }
                if (s > 0.0) {
                    *job = j - offsets[i];
                    if (!(best > 0.0)) return "a job with steps left has no throughput on a type with workers";
                    if (!(s / best <= SW_MTD_FULL_TIME_MAX)) return "steps / throughput above 1e15 seconds";
                    const double rm = sw_mtdt_rowmax(n, wk, thr + (size_t)j * n, s);
                    if (!isfinite(rm)) return "throughput / steps overflows";
                    cmin = sw_mtdt_shift_take(cmin, rm);
                    *job = -1;
                }
            }
            *shift = sw_lp_shift(cmin);
            return nullptr;
        },
        [](const sw_types_dev& d) {
            hipLaunchKernelGGL(sw_mtd_types_kernel, dim3(d.count), dim3(SW_BLOCK), 0, d.stream, d.offsets, d.n,
                               d.workers, d.shifts, d.sf, d.col[0], d.col[1], d.ws, d.x, d.results);
        });
}

}  // namespace

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
