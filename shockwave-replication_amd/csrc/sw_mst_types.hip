/*
 * sw_mst_types.hip — the max-sum-throughput allocation over worker types that
 * differ as one HIP workgroup per instance, behind sw_mst_allocate_types() /
 * sw_mst_allocate_types_batch().
 *
 * The method is in sw_mst_types.h: the LP as a transportation problem, solved
 * exactly in integers by successive best paths on the sink graph (at most 17
 * nodes).  One launch per call; a grid of `count` 512-thread workgroups, each
 * given its instance by an offsets array (CSR); the single call is count = 1.
 *
 *   per job    d[n] (double) in the call's workspace on the handle (HBM,
 *              L2-resident at these sizes); the flow y[n] (int32) in LDS when
 *              the instance has at most SW_MSTT_LDS_CELLS cells (48 KB),
 *              otherwise behind d in the workspace.  Same code on both: the
 *              flow is reached through one pointer.
 *   LDS        the flow, sw_mstt_state (4.0 KB: g, its arg jobs, two distance
 *              rows, the predecessors per round, residuals), the control words of an
 *              augmentation (two sets, by parity), the cross-wave slots of the
 *              row reduction (two sets), sw_xchg for the objective's sum
 *   an         wave 0 alone, waves 1–7 wait at the one barrier: lane l ≤ n
 *   augmen-    holds sink l; at most n Bellman–Ford rounds, each a loop over
 *   tation     the n predecessors on LDS and a wave fence, ended early by a
 *              ballot; lane 0 walks the path, moves the units and lists the
 *              created arcs and the stale rows; lane l updates its column of g
 *              for each created arc.  Then the barrier, and every thread reads
 *              the control words.
 *   a stale    all 512 threads: thread t holds sink t mod P of job slice
 *   row        t div P (P the power of two ≥ n + 1), a running lexicographic
 *              max over the slice's jobs with flow on the row's type, xor
 *              shuffles at distances P … 32 inside the wave, one LDS slot per
 *              wave and sink, a barrier, lane l of wave 0 combines the 8 slots
 *              into g.  Rows are recomputed only when the push emptied an arc
 *              whose job was a row's arg-max, never all n² pairs.
 *   the end    the duals by the same rounds on q (lane k holds type k), the
 *              column maxima for types without workers by the row reduction's
 *              second mode, x = y / sf and the objective as the block's
 *              deterministic sum over contiguous job chunks.
 * Every branch that holds a barrier is taken on a control word read after a
 * barrier (workgroup-uniform).  No grid-wide synchronisation, no inline
 * assembly, no matrix instructions: the work is arg-max reductions and integer
 * moves.  The host side of the call is the worker-type frame of sw_types.h; the
 * prices travel as n more words of the frame's result row.
 *
 * Measured (profiles/mst_types_timing.json, wall time per call with the host's
 * checks and copies): 0.26 / 0.79 / 2.52 / 6.12 / 17.1 ms at (jobs, types) =
 * (30, 3) / (120, 3) / (400, 3) / (400, 8) / (2048, 3) in 41 / 149 / 479 / 537 /
 * 2506 augmentations, about 6.8 µs each: the kernel is bound by the latency of
 * one wave's rounds and one barrier per augmentation, not by the reductions.
 * HiGHS on one core takes 1.31 / 2.10 / 5.05 / 9.28 / 59.8 ms on the same LPs;
 * 256 instances of (30, 3) in one launch 0.81 ms, 316k allocations/s.
 */
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include <vector>

#include "../../include/shockwave_amd.h"
#include "sw_alloc.h"
#include "sw_block.h"
#include "sw_handle.h"
#include "sw_mst_types.h"
#include "sw_types.h"

#define SW_MSTT_W 4 /* result words before the prices */

static_assert(SW_MSTT_MAX_TYPES == SW_TYPES_MAX_TYPES && SW_MSTT_CAP == SW_IPM_CAP, "the frame's limits and cap status");

namespace {

struct MsttCtl {
    int32_t dirty, rem, status;
};
struct MsttRed {
    double val[SW_WAVES][32];
    int32_t arg[SW_WAVES][32];
};

/* Row k of g from all jobs (ROW), or the column maxima of d (not ROW), into
 * R's slots of this wave; the caller's barrier follows. */
template <bool ROW>
__device__ __forceinline__ void mstt_reduce(MsttRed& R, const double* __restrict__ D, const int32_t* y, int32_t m,
                                            int32_t n, int32_t P, int32_t k) {
    const int32_t l = (int32_t)threadIdx.x & (P - 1);
    const int32_t slice = (int32_t)threadIdx.x / P, nsl = SW_BLOCK / P;
    double best = sw_mstt_neg_inf();
    int32_t bi = SW_MSTT_NO_JOB;
    if (l <= n && !(ROW && l == k))
        for (int32_t i = slice; i < m; i += nsl) {
            if (ROW && y[(int64_t)i * n + k] <= 0) continue;
            const double c = ROW ? sw_mstt_d(D, n, i, l) - sw_mstt_d(D, n, i, k) : sw_mstt_d(D, n, i, l);
            if (sw_mstt_better(c, i, best, bi)) { best = c; bi = i; }
        }
    for (int32_t off = P; off < 64; off <<= 1) {
        const double ob = __shfl_xor(best, off, 64);
        const int32_t oi = __shfl_xor(bi, off, 64);
        if (sw_mstt_better(ob, oi, best, bi)) { best = ob; bi = oi; }
    }
    if (lane_id() < P) { R.val[wave_id()][lane_id()] = best; R.arg[wave_id()][lane_id()] = bi; }
}

/* after the barrier: sink l's maximum over the waves */
__device__ __forceinline__ void mstt_combine(const MsttRed& R, int32_t l, double& best, int32_t& bi) {
    best = R.val[0][l];
    bi = R.arg[0][l];
    for (int w = 1; w < SW_WAVES; ++w)
        if (sw_mstt_better(R.val[w][l], R.arg[w][l], best, bi)) { best = R.val[w][l]; bi = R.arg[w][l]; }
}

/* results: [count][4 + n + 1] = objective, augmentations, row recomputations,
 * flags, price[n], status */
__global__ __launch_bounds__(SW_BLOCK) void sw_mst_types_kernel(const int64_t* __restrict__ offsets, int32_t n,
                                                                const int32_t* __restrict__ workers,
                                                                const int32_t* __restrict__ sfs,
                                                                const double* __restrict__ weights,
                                                                double* __restrict__ ws, double* __restrict__ x,
                                                                double* __restrict__ results) {
    __shared__ int32_t ylds[SW_MSTT_LDS_CELLS];
    __shared__ sw_mstt_state S;
    __shared__ MsttCtl ctl[2];
    __shared__ MsttRed R[2];
    __shared__ sw_xchg X;
    sw_mstt_state* s = &S;
    sw_chunk ch = sw_chunk_of(offsets);
    const int64_t inst = blockIdx.x, base = ch.base;
    const int32_t m = ch.N;
    const int32_t tid = (int32_t)threadIdx.x;
    double* out = results + (SW_MSTT_W + n + 1) * inst;
    if (m <= 0) { /* uniform */
        if (tid <= SW_MSTT_W + n) out[tid] = 0.0;
        return;
    }
    ch.split();
    const int32_t* sf = sfs + base;
    const double* w = weights + base * n;
    const int32_t* wk = workers + inst * n;
    double* D = ws + (int64_t)SW_MSTT_FIELDS(n) * base;
    const int32_t cells = m * n;
    int32_t* y = cells <= SW_MSTT_LDS_CELLS ? ylds : (int32_t*)(D + cells);
    int32_t P = 1;
    while (P < n + 1) P <<= 1;

    for (int32_t c = tid; c < cells; c += SW_BLOCK) {
        D[c] = sw_mstt_density(w[c], (double)sf[c / n]);
        y[c] = 0;
    }
    if (tid == 0) sw_mstt_setup(s, m, n, wk);
    __syncthreads();

    int32_t j = 0, par = 0, rpar = 0;
    bool fresh = true;
    while (j < m) {
        if (tid < 64) {
            if (tid == 0 && fresh) s->rem = sf[j];
            if (tid <= n) sw_mstt_start(s, D, j, tid);
            wave_sync(); /* also orders the row writes of the last recomputation before the rounds */
            int buf = 0;
            int32_t r = 0;
            while (r < n) {
                const int changed = tid <= n ? sw_mstt_relax(s, tid, r, buf) : 0;
                wave_sync();
                buf ^= 1;
                ++r;
                if (!__any(changed)) break;
            }
            if (tid == 0) {
                sw_mstt_push(s, y, j, r, buf);
                ctl[par].dirty = s->dirty;
                ctl[par].rem = s->rem;
                ctl[par].status = s->status;
            }
            wave_sync();
            const int32_t nnew = s->nnew;
            if (tid <= n)
                for (int32_t a = 0; a < nnew; ++a) sw_mstt_arc_add(s, D, s->new_job[a], s->new_type[a], tid);
        }
        __syncthreads();
        const MsttCtl c = ctl[par];
        par ^= 1;
        if (c.status != SW_MSTT_OK) break; /* uniform */
        for (int32_t k = 0; k < n; ++k) {
            if (!((c.dirty >> k) & 1)) continue; /* uniform */
            mstt_reduce<true>(R[rpar], D, y, m, n, P, k);
            __syncthreads();
            if (tid <= n && tid != k) mstt_combine(R[rpar], tid, s->g[k][tid], s->arg[k][tid]);
            if (tid == 0) ++s->rows;
            rpar ^= 1;
        }
        fresh = c.rem == 0;
        if (fresh) ++j;
    }
    __syncthreads();
    const int32_t status = s->status;

    /* the duals */
    if (status == SW_MSTT_OK) {
        if (tid < 64) {
            if (tid <= n) sw_mstt_dual_start(s, tid);
            wave_sync();
            int buf = 0;
            for (int32_t r = 0; r < n; ++r) {
                const int changed = tid <= n ? sw_mstt_dual_relax(s, tid, buf) : 0;
                wave_sync();
                buf ^= 1;
                if (!__any(changed)) break;
            }
            if (tid == 0) {
                int32_t none = 0;
                for (int32_t k = 0; k < n; ++k)
                    if (sw_bits(s->dist[buf][k]) == SW_MSTT_NEG_INF_BITS) none |= 1 << k;
                ctl[par].dirty = none;
                ctl[par].rem = buf;
            }
        }
        __syncthreads();
        const int32_t none = ctl[par].dirty, buf = ctl[par].rem;
        if (none) { /* uniform */
            mstt_reduce<false>(R[rpar], D, y, m, n, P, 0);
            __syncthreads();
        }
        if (tid < n) {
            double cm = 0.0;
            int32_t bi;
            if ((none >> tid) & 1) mstt_combine(R[rpar], tid, cm, bi);
            out[SW_MSTT_W + tid] = sw_mstt_price(s->dist[buf][tid], cm);
        }
    } else if (tid < n) {
        out[SW_MSTT_W + tid] = 0.0;
    }

    /* x and the objective */
    sw_blk blk{&X, 0};
    double acc = 0.0;
    for (int32_t i = ch.lo; i < ch.lo + ch.cnt; ++i)
        acc = acc + sw_mstt_emit(n, y + (int64_t)i * n, (double)sf[i], w + (int64_t)i * n, x + (base + i) * n);
    const double objective = blk.detsum(acc);
    if (tid == 0) {
        sw_mstt_result(s, wk, objective, out);
        out[SW_MSTT_W + n] = (double)status;
    }
}

int mstt_run(sw_handle* h, const char* who, int32_t count, int32_t n, const int64_t* offsets, const int32_t* workers,
             const int32_t* sf, const double* weights, double* x, double* prices, double* results) {
    /* the frame's result row carries the prices behind the four result words */
    const int W = SW_MSTT_W + (n >= 1 && n <= SW_MSTT_MAX_TYPES ? n : 0);
    std::vector<double> rows((size_t)(count > 0 ? count : 0) * W);
    const sw_types_call c{who, count, n, offsets, workers, sf, {1, {{weights, true}}, false, false, W},
                          x, nullptr, rows.data(), SW_MSTT_FIELDS(n), 0, nullptr};
    const int rc = sw_types_run(
        h, c,
        [&](int32_t i, int32_t*, int64_t* job) -> const char* {
            for (int64_t j = offsets[i]; j < offsets[i + 1]; ++j) {
                *job = j - offsets[i];
                if (sf[j] < 1 || sf[j] > SW_MAX_WIDTH) return "scale factors must be in [1,255]";
                for (int32_t k = 0; k < n; ++k) {
                    const double v = weights[(size_t)j * n + k];
                    if (!(v >= 0.0) || !(v <= SW_MSTT_WEIGHT_MAX)) return "weights must be finite, >= 0 and <= 1e30";
                }
            }
            *job = -1;
            return nullptr;
        },
        [](const sw_types_dev& d) {
            hipLaunchKernelGGL(sw_mst_types_kernel, dim3(d.count), dim3(SW_BLOCK), 0, d.stream, d.offsets, d.n,
                               d.workers, d.sf, d.col[0], d.ws, d.x, d.results);
        });
    if (rc != SW_OK) return rc;
    for (int32_t i = 0; i < count; ++i) {
        const double* r = rows.data() + (size_t)i * W;
        if (results)
            for (int a = 0; a < SW_MSTT_W; ++a) results[(size_t)i * SW_MSTT_W + a] = r[a];
        if (prices)
            for (int32_t k = 0; k < n; ++k) prices[(size_t)i * n + k] = r[SW_MSTT_W + k];
    }
    return SW_OK;
}

}  // namespace

extern "C" int sw_mst_allocate_types(sw_handle* h, int32_t num_jobs, int32_t num_types, const int32_t* workers,
                                     const int32_t* scale_factors, const double* weights, double* allocation,
                                     double* prices, double* result) {
    if (!h) return SW_ERR_INVALID;
    if (num_jobs < 0) return sw_fail(h, SW_ERR_INVALID, "sw_mst_allocate_types: num_jobs < 0");
    const int64_t offsets[2] = {0, num_jobs};
    return mstt_run(h, "sw_mst_allocate_types", 1, num_types, offsets, workers, scale_factors, weights, allocation,
                    prices, result);
}

extern "C" int sw_mst_allocate_types_batch(sw_handle* h, int32_t count, int32_t num_types, const int64_t* offsets,
                                           const int32_t* workers, const int32_t* scale_factors,
                                           const double* weights, double* allocation, double* prices,
                                           double* results) {
    if (!h) return SW_ERR_INVALID;
    if (count < 0) return sw_fail(h, SW_ERR_INVALID, "sw_mst_allocate_types_batch: count < 0");
    if (count == 0) return SW_OK;
    return mstt_run(h, "sw_mst_allocate_types_batch", count, num_types, offsets, workers, scale_factors, weights,
                    allocation, prices, results);
}
