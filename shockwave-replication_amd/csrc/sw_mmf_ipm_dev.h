/*
 * sw_mmf_ipm_dev.h — the device helpers of the interior-point kernels
 * (sw_mmf_ipm.hip, sw_mtd_types.hip): the reduction of one pass over the jobs.
 * A reduction is the block's deterministic tree for sums (wave_dettree, then
 * the halving tree over the eight waves) and exact maxima, two barriers: one
 * before thread 0 combines the waves' values and runs the one-thread part of
 * the step, one after it.
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

inline size_t ipm_align8(size_t o) { return (o + 7) & ~(size_t)7; }

}  // namespace

#endif /* SW_MMF_IPM_DEV_H */
