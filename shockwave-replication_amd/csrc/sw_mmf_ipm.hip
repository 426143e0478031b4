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
 *   the start  the load pass (1 reduction of 2 sums, 1 max), then ipm_start_tail
 *   the steps  ipm_solve (sw_mmf_ipm_dev.h)
 *   the end    the two points of the path extrapolated to μ = 0 under a ratio
 *              test                             1 reduction of na sums, 1 max
 * The reduction, the start's tail and the Newton loop are in sw_mmf_ipm_dev.h,
 * shared with the three other kernels of the engine; the host side of the call
 * is the worker-type frame of sw_types.h.  No grid-wide synchronisation, no
 * inline assembly.
 *
 * Compile report (gfx950): 222 VGPRs, no VGPR spill, 314 SGPRs spilled to VGPR
 * lanes, 176 bytes of scratch per lane, 5.6 KB of LDS, 2 waves per SIMD.
 */
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/shockwave_amd.h"
#include "sw_block.h"
#include "sw_handle.h"
#include "sw_mmf_ipm.h"
#include "sw_mmf_ipm_dev.h"
#include "sw_types.h"

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
    const ipm_chunk ch = ipm_chunk_of(offsets);
    const int64_t inst = ch.inst, base = ch.base;
    const int32_t m = ch.m, lo = ch.lo, hi = ch.hi;
    const int tid = threadIdx.x;
    double* out = levels + 3 * inst;
    if (m <= 0) { /* uniform */
        ipm_zero_results<3>(out);
        return;
    }
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
        ipm_zero_results<3>(out);
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
    ipm_start_tail(g, R, J, sf, lo, hi, acc, mx, v, w);
    ipm_solve(g, R, J, sf, lo, hi, acc, mx, v, w);

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

int mmfc_run(sw_handle* h, const char* who, int32_t count, int32_t n, const int64_t* offsets, const int32_t* workers,
             const int32_t* sf, const double* coef, double* x, double* levels) {
    const sw_types_call c{who, count, n, offsets, workers, sf, {1, {{coef, true}}, true, false, 2},
                          x, nullptr, levels, SW_IPM_FIELDS(n), 0, nullptr};
    return sw_types_run(
        h, c,
        [&](int32_t i, int32_t* shift, int64_t*) -> const char* {
            double cmax = 0.0; /* the normalisation of sw_mmf_ipm.h: over the types that have workers */
            for (int64_t j = offsets[i]; j < offsets[i + 1]; ++j) {
                if (sf[j] < 1 || sf[j] > SW_MAX_WIDTH) return "scale factors must be in [1,255]";
                for (int32_t k = 0; k < n; ++k) {
                    const double cf = coef[(size_t)j * n + k];
                    if (!(cf >= 0.0) || !isfinite(cf)) return "coefficients must be finite and >= 0";
                    if (workers[(size_t)i * n + k] > 0 && cf > cmax) cmax = cf;
                }
            }
            *shift = sw_lp_shift(cmax);
            return nullptr;
        },
        [](const sw_types_dev& d) {
            hipLaunchKernelGGL(sw_mmf_ipm_kernel, dim3(d.count), dim3(SW_BLOCK), 0, d.stream, d.offsets, d.n, d.workers,
                               d.shifts, d.sf, d.col[0], d.ws, d.x, d.results);
        });
}

}  // namespace

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
