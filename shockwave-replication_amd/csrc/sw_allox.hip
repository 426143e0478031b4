/*
 * sw_allox.hip — the AlloX min-cost assignment as one HIP workgroup per
 * instance, behind sw_allox_assign() / sw_allox_assign_batch().
 *
 * Replaces the dense m × (m·n) matrix and scipy's linear_sum_assignment of
 * policies/allox.py:71-103.  The method, the pruned column set, the tie rule
 * and the arithmetic are in sw_allox.h.  One kernel serves both calls: a grid
 * of `count` workgroups, each given its instance by offsets arrays (CSR); the
 * single call is count = 1.
 *
 *   rows     in job order, one shortest-path search each
 *   step     thread L relaxes its slots L, L + NT, … from the current row
 *            (cost computed from p[i][type], the position and d[i]; nothing
 *            is stored per (row, column)) and keeps its best (distance,
 *            slot); the workgroup reduces the arg-min: DPP inside a wave,
 *            then one LDS exchange and ONE barrier, with two alternating
 *            exchange sets as in sw_block.h
 *   duals    every visited assigned slot, in parallel (distinct rows)
 *   augment  thread 0 walks the path (≤ r + 1 slots)
 *   emit     per assigned slot, then the in-order cost sum by thread 0
 *
 * A slot's distance, predecessor and visited flag are only ever touched by
 * the thread that owns it, so a search step needs no barrier besides the
 * reduction's.  The current row, the winning slot and the distance are read
 * back through v_readfirstlane: the row's p and d are then scalar loads.
 *
 * All column and row state is in dynamic LDS (sw_allox_bytes: 25 B a slot,
 * 8 B a row, 59,392 B at the caps m = n = 1024, inside the 64 KB a launch
 * gets without opting in).  Every search step reads one row of p and d[i]:
 * they are copied into LDS behind that state when both fit (900 jobs, 256
 * workers and 3 types do: 64,900 B) and are read from global memory by
 * address-uniform loads otherwise.  Instances whose slots number at most
 * SW_ALLOX_WAVE_SLOTS run as a single wave: the reduction then needs no LDS
 * exchange and the workgroup barrier is the wave's own.
 */
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

#include "../../include/shockwave_amd.h"
#include "sw_allox.h"
#include "sw_block.h"
#include "sw_handle.h"

#define SW_ALLOX_WAVE_SLOTS 256 /* m + n up to which a batch runs one wave per instance */
#define SW_ALLOX_LDS_BYTES (65536 - 256) /* dynamic LDS of a launch: 64 KB less the exchange slots */

namespace {

template <int NW>
struct AlloxXchg {
    double v[2][NW];
    int32_t s[2][NW];
};

/* arg-min of (distance, slot) over the wave, valid in every lane */
__device__ __forceinline__ void allox_wave_argmin(double& v, int32_t& s) {
    uint64_t xv = __builtin_bit_cast(uint64_t, v);
    int32_t xs = s;
#define SW_ALLOX_STEP_(c, rm)                                                                   \
    {                                                                                           \
        const uint64_t yv_ = SW_DPP64(xv, SW_ALLOX_INF_BITS, c, rm);                            \
        const int32_t ys_ = __builtin_amdgcn_update_dpp(SW_ALLOX_NO_SLOT, xs, c, rm, 0xF, false); \
        if (sw_allox_less(__builtin_bit_cast(double, yv_), ys_, __builtin_bit_cast(double, xv), xs)) { \
            xv = yv_;                                                                           \
            xs = ys_;                                                                           \
        }                                                                                       \
    }
    SW_DPP64_STEPS(SW_ALLOX_STEP_)
#undef SW_ALLOX_STEP_
    v = __builtin_bit_cast(double, sw_readlane63_u64(xv));
    s = __builtin_amdgcn_readlane(xs, 63);
}

template <int NW>
__device__ __forceinline__ void allox_argmin(AlloxXchg<NW>* X, int& par, double& v, int32_t& s) {
    allox_wave_argmin(v, s);
    if (NW > 1) {
        if (lane_id() == 0) { X->v[par][wave_id()] = v; X->s[par][wave_id()] = s; }
        __syncthreads();
        v = X->v[par][0];
        s = X->s[par][0];
#pragma unroll
        for (int w = 1; w < NW; ++w) {
            const double vw = X->v[par][w];
            const int32_t sw = X->s[par][w];
            if (sw_allox_less(vw, sw, v, s)) { v = vw; s = sw; }
        }
        par ^= 1;
    }
    v = sw_f64u(v);
    s = sw_u32(s);
}

/* One instance on the workgroup; p and d point to global memory or to their
 * LDS copies (the same values: the same bits either way). */
template <int NW>
__device__ __forceinline__ void allox_solve(AlloxXchg<NW>* X, const sw_allox_cols& c, int32_t m, int32_t n,
                                            int32_t T, const int32_t* __restrict__ fw,
                                            const double* __restrict__ p, const double* __restrict__ d,
                                            int32_t* __restrict__ jw, int32_t* __restrict__ jp,
                                            int32_t* __restrict__ wf, double* __restrict__ cost,
                                            int32_t* __restrict__ status) {
    constexpr int NT = 64 * NW;
    const int tid = (int)threadIdx.x;
    int par = 0;
    const double inf = sw_from_bits(SW_ALLOX_INF_BITS);
    for (int32_t j = tid; j < n; j += NT) sw_allox_init_frontier(&c, j, sw_allox_worker_type(fw, T, j));
    for (int32_t i = tid; i < m; i += NT) c.u[i] = 0.0;
    __syncthreads();

    for (int32_t r = 0; r < m; ++r) {
        const int32_t ncol = n + r;
        for (int32_t s = tid; s < ncol; s += NT) { c.sh[s] = inf; c.seen[s] = 0; }
        double minv = 0.0;
        int32_t i = r, via = -1, sink = -1;
        for (int32_t it = 0; it <= r && sink < 0; ++it) {
            const double ui = c.u[i], di = d[i];
            double pr[SW_ALLOX_MAX_TYPES];
#pragma unroll
            for (int t = 0; t < SW_ALLOX_MAX_TYPES; ++t) pr[t] = t < T ? p[(size_t)i * (size_t)T + t] : 0.0;
            double bv = inf;
            int32_t bs = SW_ALLOX_NO_SLOT;
            for (int32_t s = tid; s < ncol; s += NT) {
                if (c.seen[s]) continue;
                const int32_t ty = c.wt[s] >> SW_ALLOX_TYPE_SHIFT;
                double pk = pr[0];
#pragma unroll
                for (int t = 1; t < SW_ALLOX_MAX_TYPES; ++t) pk = ty == t ? pr[t] : pk;
                const double sh = sw_allox_relax(&c, s, minv, ui, pk, di, via);
                if (sw_allox_less(sh, s, bv, bs)) { bv = sh; bs = s; }
            }
            allox_argmin<NW>(X, par, bv, bs);
            if (bs >= ncol) break; /* no finite distance: cannot happen with validated inputs */
            minv = bv;
            if (tid == (bs & (NT - 1))) c.seen[bs] = 1;
            if (bs < n) sink = bs;
            else { i = sw_u32(c.row[bs]); via = bs; }
        }
        if (sink < 0) { /* workgroup-uniform */
            if (tid == 0) *status = 1;
            return;
        }
        for (int32_t s = tid; s < ncol; s += NT) /* by the slot's owner, as in the search */
            if (s >= n && c.seen[s]) sw_allox_dual(&c, s, minv);
        if (tid == 0) c.u[r] = minv;
        __syncthreads();
        if (tid == 0) sw_allox_augment(&c, n, r, sink);
        __syncthreads();
    }

    for (int32_t s = n + tid; s < n + m; s += NT) sw_allox_emit(&c, s, T, p, d, jw, jp, wf);
    __syncthreads();
    if (tid == 0) {
        double total = 0.0;
        for (int32_t i = 0; i < m; ++i) total = total + c.u[i];
        *cost = total;
    }
}

template <int NW>
__global__ __launch_bounds__(64 * NW) void sw_allox_kernel(
    const int64_t* __restrict__ job_off, const int64_t* __restrict__ wrk_off,
    const int64_t* __restrict__ p_off, const int32_t* __restrict__ num_types,
    const int32_t* __restrict__ free_workers, const double* __restrict__ p_all,
    const double* __restrict__ d_all, int32_t* __restrict__ job_worker,
    int32_t* __restrict__ job_position, int32_t* __restrict__ worker_first,
    double* __restrict__ costs, int32_t* __restrict__ status, uint32_t stage_limit) {
    constexpr int NT = 64 * NW;
    extern __shared__ double allox_lds[];
    __shared__ AlloxXchg<NW> X;
    const int tid = (int)threadIdx.x;
    const int64_t inst = blockIdx.x;
    const int64_t jb = job_off[inst], wb = wrk_off[inst];
    const int32_t m = (int32_t)(job_off[inst + 1] - jb);
    const int32_t n = (int32_t)(wrk_off[inst + 1] - wb);
    const int32_t T = num_types[inst];
    const int32_t* fw = free_workers + inst * SW_ALLOX_MAX_TYPES;
    const double* p = p_all + p_off[inst];
    const double* d = d_all + jb;
    int32_t* jw = job_worker + jb;
    int32_t* jp = job_position + jb;
    int32_t* wf = worker_first + wb;

    for (int32_t i = tid; i < m; i += NT) { jw[i] = -1; jp[i] = 0; }
    for (int32_t j = tid; j < n; j += NT) wf[j] = -1;
    if (tid == 0) { costs[inst] = 0.0; status[inst] = 0; }
    if (m <= 0 || n <= 0) return; /* nothing to assign (allox.py:49: the previous rows are copied) */

    const sw_allox_cols c = sw_allox_layout(allox_lds, m, n);
    /* every search step reads one row of p and d: staged behind the column state when the
     * launch's LDS holds them (stage_limit: its dynamic LDS bytes, 0 = never) */
    const size_t cols = sw_allox_bytes(m, n), np = (size_t)m * (size_t)T;
    if (cols + (np + (size_t)m) * 8 <= (size_t)stage_limit) {
        double* lp = allox_lds + cols / 8;
        double* ld = lp + np;
        for (size_t k = tid; k < np; k += NT) lp[k] = p[k];
        for (int32_t i = tid; i < m; i += NT) ld[i] = d[i];
        allox_solve<NW>(&X, c, m, n, T, fw, lp, ld, jw, jp, wf, costs + inst, status + inst);
    } else {
        allox_solve<NW>(&X, c, m, n, T, fw, p, d, jw, jp, wf, costs + inst, status + inst);
    }
}

/* One input block and one output block per call (one copy each way):
 *   in : job_off[count+1] | wrk_off[count+1] | p_off[count] (int64) | p [P] | d [M] (double)
 *        | free [count][8] | num_types [count] (int32)
 *   out: costs [count] (double) | job_worker [M] | job_position [M] | worker_first [W]
 *        | status [count] (int32) */
/* free_stride: ints between two instances' worker counts */
int allox_run(sw_handle* h, const char* who, int32_t count, const int64_t* job_off,
              const int32_t* num_types, const int32_t* free_workers, int32_t free_stride,
              const double* p, const double* d, int32_t* job_worker, int32_t* job_position,
              int32_t* worker_first, const int64_t* wrk_off_in, double* costs) {
    const std::string n(who);
    if (job_off[0] != 0) return sw_fail(h, SW_ERR_INVALID, n + ": job offsets must start at 0");
    if (wrk_off_in && wrk_off_in[0] != 0)
        return sw_fail(h, SW_ERR_INVALID, n + ": worker offsets must start at 0");
    const size_t C = (size_t)count;
    std::vector<int64_t> off_store(2 * C + 1, 0);
    int64_t* wrk_off = off_store.data();
    int64_t* p_off = wrk_off + C + 1;
    /* SW_ALLOX_STAGE=0: p and d stay in global memory (A/B timing, tools/allox_timing.py) */
    const char* st_env = getenv("SW_ALLOX_STAGE");
    const bool stage = !(st_env && st_env[0] == '0');
    size_t lds = 0;
    int32_t max_slots = 0;
    int64_t P = 0;
    wrk_off[0] = 0;
    for (int32_t i = 0; i < count; ++i) {
        const int64_t m = job_off[i + 1] - job_off[i];
        if (m < 0) return sw_fail(h, SW_ERR_INVALID, n + ": job offsets must not decrease");
        const int32_t T = num_types[i];
        if (T < 1 || T > SW_ALLOX_MAX_TYPES)
            return sw_fail(h, SW_ERR_INVALID, n + ": num_types must be in [1, 8]");
        int64_t nw = 0;
        for (int32_t t = 0; t < T; ++t) {
            const int32_t f = free_workers[(size_t)i * free_stride + t];
            if (f < 0) return sw_fail(h, SW_ERR_INVALID, n + ": worker counts must be >= 0");
            nw += f;
        }
        if (wrk_off_in && wrk_off_in[i + 1] - wrk_off_in[i] != nw)
            return sw_fail(h, SW_ERR_INVALID, n + ": worker offsets must step by the sum of the worker counts");
        if (m > SW_ALLOX_MAX_JOBS || nw > SW_ALLOX_MAX_WORKERS)
            return sw_fail(h, SW_ERR_CAPACITY, n + ": more than 1024 jobs or 1024 free workers in one instance");
        wrk_off[i + 1] = wrk_off[i] + nw;
        p_off[i] = P;
        P += m * T;
        if (m > 0 && nw > 0) {
            size_t b = sw_allox_bytes((int32_t)m, (int32_t)nw);
            const size_t staged = b + (size_t)(m * T + m) * 8;
            if (stage && staged <= SW_ALLOX_LDS_BYTES) b = staged;
            if (b > lds) lds = b;
            if ((int32_t)(m + nw) > max_slots) max_slots = (int32_t)(m + nw);
        }
    }
    const int64_t M = job_off[count], W = wrk_off[count];
    if (M > 0 && (!p || !d || !job_worker || !job_position))
        return sw_fail(h, SW_ERR_INVALID, n + ": null pointers");
    if (W > 0 && !worker_first) return sw_fail(h, SW_ERR_INVALID, n + ": null pointers");
    for (int64_t k = 0; k < P; ++k)
        if (!(p[k] >= 0.0) || !(p[k] <= SW_ALLOX_PROC_MAX))
            return sw_fail(h, SW_ERR_INVALID, n + ": processing times must be finite, >= 0 and <= 1e30");
    for (int64_t j = 0; j < M; ++j)
        if (!(d[j] >= 0.0) || !(d[j] <= SW_ALLOX_DELAY_MAX))
            return sw_fail(h, SW_ERR_INVALID, n + ": delays must be finite, >= 0 and <= 1e15");
    for (int64_t j = 0; j < M; ++j) { job_worker[j] = -1; job_position[j] = 0; }
    for (int64_t j = 0; j < W; ++j) worker_first[j] = -1;
    if (costs)
        for (int32_t i = 0; i < count; ++i) costs[i] = 0.0;
    if (lds == 0) return SW_OK; /* no instance has both a job and a free worker */

    int32_t wave_slots = SW_ALLOX_WAVE_SLOTS;
    /* SW_ALLOX_WAVE_SLOTS=<k>: the one-wave threshold (A/B timing, tools/allox_timing.py) */
    const char* ws_env = getenv("SW_ALLOX_WAVE_SLOTS");
    if (ws_env && ws_env[0]) wave_slots = atoi(ws_env);

    SW_HIP(h, hipSetDevice(h->device));
    sw_io_bufs* b = &h->io;
    const size_t Ms = (size_t)M, Ws = (size_t)W, Ps = (size_t)P;
    const size_t o_wo = (C + 1) * 8, o_po = o_wo + (C + 1) * 8, o_p = o_po + C * 8, o_d = o_p + Ps * 8,
                 o_f = o_d + Ms * 8, o_t = o_f + C * SW_ALLOX_MAX_TYPES * 4, in_bytes = o_t + C * 4;
    const size_t o_jw = C * 8, o_jp = o_jw + Ms * 4, o_wf = o_jp + Ms * 4, o_st = o_wf + Ws * 4,
                 out_bytes = o_st + C * 4;
    SW_HIP(h, b->in.reserve(in_bytes));
    SW_HIP(h, b->out.reserve(out_bytes));
    SW_HIP(h, b->hin.reserve(in_bytes));
    SW_HIP(h, b->hout.reserve(out_bytes));
    memcpy(b->hin.p, job_off, (C + 1) * 8);
    memcpy(b->hin.p + o_wo, wrk_off, (C + 1) * 8);
    memcpy(b->hin.p + o_po, p_off, C * 8);
    if (Ps) memcpy(b->hin.p + o_p, p, Ps * 8);
    if (Ms) memcpy(b->hin.p + o_d, d, Ms * 8);
    int32_t* hf = (int32_t*)(b->hin.p + o_f);
    for (size_t i = 0; i < C; ++i)
        for (int32_t t = 0; t < SW_ALLOX_MAX_TYPES; ++t)
            hf[i * SW_ALLOX_MAX_TYPES + t] = t < num_types[i] ? free_workers[i * free_stride + t] : 0;
    memcpy(b->hin.p + o_t, num_types, C * 4);
    SW_HIP(h, hipMemcpyAsync(b->in.p, b->hin.p, in_bytes, hipMemcpyHostToDevice, h->stream));
    unsigned char* di = b->in.p;
    unsigned char* dout = b->out.p;
    if (max_slots <= wave_slots)
        hipLaunchKernelGGL(sw_allox_kernel<1>, dim3((unsigned)count), dim3(64), lds, h->stream,
                           (const int64_t*)di, (const int64_t*)(di + o_wo), (const int64_t*)(di + o_po),
                           (const int32_t*)(di + o_t), (const int32_t*)(di + o_f), (const double*)(di + o_p),
                           (const double*)(di + o_d), (int32_t*)(dout + o_jw), (int32_t*)(dout + o_jp),
                           (int32_t*)(dout + o_wf), (double*)dout, (int32_t*)(dout + o_st),
                           stage ? (uint32_t)lds : 0u);
    else
        hipLaunchKernelGGL(sw_allox_kernel<SW_WAVES>, dim3((unsigned)count), dim3(SW_BLOCK), lds, h->stream,
                           (const int64_t*)di, (const int64_t*)(di + o_wo), (const int64_t*)(di + o_po),
                           (const int32_t*)(di + o_t), (const int32_t*)(di + o_f), (const double*)(di + o_p),
                           (const double*)(di + o_d), (int32_t*)(dout + o_jw), (int32_t*)(dout + o_jp),
                           (int32_t*)(dout + o_wf), (double*)dout, (int32_t*)(dout + o_st),
                           stage ? (uint32_t)lds : 0u);
    SW_HIP(h, hipGetLastError());
    SW_HIP(h, hipMemcpyAsync(b->hout.p, b->out.p, out_bytes, hipMemcpyDeviceToHost, h->stream));
    SW_HIP(h, hipStreamSynchronize(h->stream));
    const int32_t* st = (const int32_t*)(b->hout.p + o_st);
    for (size_t i = 0; i < C; ++i)
        if (st[i] != 0) return sw_fail(h, SW_ERR_INVALID, n + ": a search found no column");
    if (Ms) memcpy(job_worker, b->hout.p + o_jw, Ms * 4);
    if (Ms) memcpy(job_position, b->hout.p + o_jp, Ms * 4);
    if (Ws) memcpy(worker_first, b->hout.p + o_wf, Ws * 4);
    if (costs) memcpy(costs, b->hout.p, C * 8);
    return SW_OK;
}

}  // namespace

extern "C" int sw_allox_assign(sw_handle* h, int32_t num_jobs, int32_t num_types,
                               const int32_t* free_workers, const double* proc_time,
                               const double* delay, int32_t* job_worker, int32_t* job_position,
                               int32_t* worker_first, double* cost) {
    if (!h) return SW_ERR_INVALID;
    if (num_jobs < 0) return sw_fail(h, SW_ERR_INVALID, "sw_allox_assign: num_jobs < 0");
    if (num_types < 1 || num_types > SW_ALLOX_MAX_TYPES)
        return sw_fail(h, SW_ERR_INVALID, "sw_allox_assign: num_types must be in [1, 8]");
    if (!free_workers) return sw_fail(h, SW_ERR_INVALID, "sw_allox_assign: null pointers");
    const int64_t offsets[2] = {0, num_jobs};
    return allox_run(h, "sw_allox_assign", 1, offsets, &num_types, free_workers, 0, proc_time, delay,
                     job_worker, job_position, worker_first, nullptr, cost);
}

extern "C" int sw_allox_assign_batch(sw_handle* h, int32_t count, const int64_t* job_offsets,
                                     const int32_t* num_types, const int32_t* free_workers,
                                     const double* proc_time, const double* delay,
                                     int32_t* job_worker, int32_t* job_position,
                                     int32_t* worker_first, const int64_t* worker_offsets,
                                     double* costs) {
    if (!h) return SW_ERR_INVALID;
    if (count < 0 || (count > 0 && (!job_offsets || !num_types || !free_workers || !worker_offsets)))
        return sw_fail(h, SW_ERR_INVALID, "sw_allox_assign_batch: bad count or null pointers");
    if (count == 0) return SW_OK;
    return allox_run(h, "sw_allox_assign_batch", count, job_offsets, num_types, free_workers,
                     SW_ALLOX_MAX_TYPES, proc_time, delay, job_worker, job_position, worker_first,
                     worker_offsets, costs);
}
