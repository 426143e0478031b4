/*
 * sw_mmf_ipm_dev.h — the device side of the interior-point engine
 * (sw_mmf_ipm.h), shared by its four kernels: sw_mmf_ipm.hip, sw_mtd_types.hip,
 * sw_ftf_types.hip and sw_wf_types.hip.
 *
 *   ipm_chunk        a workgroup's instance and a thread's job chunk of it
 *   the reduction    of one pass over the jobs: the block's deterministic tree
 *                    for sums (wave_dettree, then the halving tree over the
 *                    eight waves) and exact maxima, two barriers: one before
 *                    thread 0 combines the waves' values and runs the
 *                    one-thread part of the step, one after it
 *   ipm_start_tail   the engine's two start passes after a kernel's own load
 *   ipm_solve        the Newton loop
 * The loads, the extrapolation's pass and whatever a policy does between two
 * solves stay in the kernels.
 */
#ifndef SW_MMF_IPM_DEV_H
#define SW_MMF_IPM_DEV_H

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "sw_block.h"
#include "sw_mmf_ipm.h"

namespace {

constexpr double kNegHuge = -1.7976931348623157e308;

struct IpmRed {
    double s[SW_WAVES][SW_IPM_NRED];
    double m[SW_WAVES][SW_IPM_NMAX];
    double sums[SW_IPM_NRED];
    double maxes[SW_IPM_NMAX];
};

/* The first half of a reduction: the waves' trees into LDS and the barrier;
 * then thread 0 combines them (ipm_combine) and goes on alone. */
__device__ __forceinline__ void ipm_publish(IpmRed& R, const double (&acc)[SW_IPM_NRED], int32_t cnt,
                                            const double (&mx)[SW_IPM_NMAX], int32_t nmx) {
    const int lane = lane_id(), wv = wave_id();
#pragma unroll
    for (int i = 0; i < SW_IPM_NRED; ++i)
        if (i < cnt) { /* uniform */
            const double v = wave_dettree(acc[i]);
            if (lane == 0) R.s[wv][i] = v;
        }
#pragma unroll
    for (int i = 0; i < SW_IPM_NMAX; ++i)
        if (i < nmx) {
            const double v = wave_max_f64(mx[i]);
            if (lane == 0) R.m[wv][i] = v;
        }
    __syncthreads();
}

/* thread 0 only: the halving tree over the waves, the maxima */
__device__ __forceinline__ void ipm_combine(IpmRed& R, int32_t cnt, int32_t nmx) {
    for (int32_t i = 0; i < cnt; ++i) {
        double s[SW_WAVES];
#pragma unroll
        for (int w = 0; w < SW_WAVES; ++w) s[w] = R.s[w][i];
#pragma unroll
        for (int h = SW_WAVES / 2; h >= 1; h >>= 1)
#pragma unroll
            for (int k = 0; k < h; ++k) s[k] = s[k] + s[k + h];
        R.sums[i] = s[0];
    }
    for (int32_t i = 0; i < nmx; ++i) {
        double m = R.m[0][i];
#pragma unroll
        for (int w = 1; w < SW_WAVES; ++w) m = R.m[w][i] > m ? R.m[w][i] : m;
        R.maxes[i] = m;
    }
}

__device__ __forceinline__ void ipm_clear(double (&acc)[SW_IPM_NRED], double (&mx)[SW_IPM_NMAX]) {
#pragma unroll
    for (int i = 0; i < SW_IPM_NRED; ++i) acc[i] = 0.0;
#pragma unroll
    for (int i = 0; i < SW_IPM_NMAX; ++i) mx[i] = kNegHuge;
}

/* acc += v[0 … cnt), mx = max(mx, w[0 … nmx)) with the arrays kept in registers */
__device__ __forceinline__ void ipm_take(double (&acc)[SW_IPM_NRED], const double* v, int32_t cnt,
                                         double (&mx)[SW_IPM_NMAX], const double* w, int32_t nmx) {
#pragma unroll
    for (int i = 0; i < SW_IPM_NRED; ++i)
        if (i < cnt) acc[i] = acc[i] + v[i];
#pragma unroll
    for (int i = 0; i < SW_IPM_NMAX; ++i)
        if (i < nmx) mx[i] = w[i] > mx[i] ? w[i] : mx[i];
}

/* The instance of workgroup blockIdx.x: m jobs at base; thread threadIdx.x owns
 * the jobs [lo, hi) of it, the contiguous chunk [L·q, (L+1)·q), q = ⌈m/512⌉. */
struct ipm_chunk {
    int64_t inst, base;
    int32_t m, lo, hi;
};

__device__ __forceinline__ ipm_chunk ipm_chunk_of(const int64_t* __restrict__ offsets) {
    const int64_t inst = blockIdx.x;
    const int64_t base = offsets[inst];
    const int32_t m = (int32_t)(offsets[inst + 1] - base);
    const int32_t tid = threadIdx.x;
    const int32_t q = (m + SW_BLOCK - 1) / SW_BLOCK;
    const int32_t lo = tid * q < m ? tid * q : m;
    const int32_t hi = lo + q < m ? lo + q : m;
    return {inst, base, m, lo, hi};
}

/* the W result words of an instance without jobs or without workers */
template <int W>
__device__ __forceinline__ void ipm_zero_results(double* __restrict__ out) {
    if (threadIdx.x == 0)
        for (int i = 0; i < W; ++i) out[i] = 0.0;
}

/* The engine's start after a kernel's own load pass (which ends in a barrier):
 * x = θ and the level's start (1 reduction of 1 max), then the slacks and a
 * dual-feasible start.  acc, mx, v, w are the caller's: see ipm_solve. */
__device__ __forceinline__ void ipm_start_tail(sw_ipm_glob* g, IpmRed& R, sw_ipm_job& J,
                                               const int32_t* __restrict__ sf, int32_t lo, int32_t hi,
                                               double (&acc)[SW_IPM_NRED], double (&mx)[SW_IPM_NMAX],
                                               double (&v)[SW_IPM_NRED], double (&w)[SW_IPM_NMAX]) {
    ipm_clear(acc, mx);
    for (int32_t j = lo; j < hi; ++j) {
        J.j = j; J.sf = (double)sf[j];
        sw_ipm_job_start(g, &J, w);
        ipm_take(acc, v, 0, mx, w, 1);
    }
    ipm_publish(R, acc, 0, mx, 1);
    if (threadIdx.x == 0) { ipm_combine(R, 0, 1); sw_ipm_glob_start(g, R.maxes); }
    __syncthreads();
    for (int32_t j = lo; j < hi; ++j) {
        J.j = j; J.sf = (double)sf[j];
        sw_ipm_job_start2(g, &J);
    }
}

/* The Newton loop: steps from the state in g and the workspace until g->done,
 * which thread 0 sets (the criterion, the step cap, a breakdown of the reduced
 * system: g->status).  Every exit is read from LDS after a barrier, so it is
 * uniform across the workgroup.
 *   pass A (residuals, μ)            1 reduction of na + 2 sums, 3 maxes
 *   pass B (scalings)                no reduction
 *   pass R_k, k < na (row k of the   1 reduction of ≤ na + 4 sums each
 *     reduced system)
 *   thread 0: L·D·Lᵀ of the na × na system, dt, dy_C
 *   pass C (back-substitution)       1 reduction of 2 maxes
 *   pass D (the step)                fused with the next pass A (`moved`)
 * acc, mx, v, w are the caller's accumulators and per-job values, passed by
 * reference: the kernels use them in their own passes too, and copies local to
 * this function were a second set in scratch (336 instead of 176 bytes per lane
 * in sw_mtd_types.hip). */
__device__ __forceinline__ void ipm_solve(sw_ipm_glob* g, IpmRed& R, sw_ipm_job& J,
                                          const int32_t* __restrict__ sf, int32_t lo, int32_t hi,
                                          double (&acc)[SW_IPM_NRED], double (&mx)[SW_IPM_NMAX],
                                          double (&v)[SW_IPM_NRED], double (&w)[SW_IPM_NMAX]) {
    const int tid = threadIdx.x;
    const int32_t na = J.na;
    bool moved = false; /* pass D of the step before is still to do */
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
}

}  // namespace

#endif /* SW_MMF_IPM_DEV_H */
