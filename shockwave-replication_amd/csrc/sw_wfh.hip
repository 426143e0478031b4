/*
 * sw_wfh.hip — the hierarchical (entity) water-filling MaxMinFairness
 * allocation as one HIP workgroup per instance, behind sw_wfh_allocate() /
 * sw_wfh_allocate_batch().
 *
 * Replaces the stage loop of policies/max_min_fairness_water_filling.py:
 * 303-409 with its per-stage reweighting (:21-77) for one worker type (or
 * several identical ones).  The mathematics and the order of every sum are in
 * sw_wfh.h.  One kernel serves both calls: a grid of `count` 512-thread
 * workgroups on a CSR grid of jobs and one of entities; the single call is
 * count = 1.
 *
 * The host puts every instance in member order (entity 0's jobs in ascending
 * job index, then entity 1's, …): position p holds job mem[p], and entity e
 * owns the positions [ebeg[e], ebeg[e+1]).  The scale factors and the
 * coefficients travel in that order, so a wave reads an entity's members as
 * consecutive words, and no device step depends on the order of atomics (there
 * are none).  The same host pass adds up D_e (int64: exact in any order).  The
 * host arithmetic (checks, block layout, packing) is in sw_wfh_layout.h.
 *
 *   pass 1   thread L owns the entity chunk [L·qE, (L+1)·qE), qE = ⌈E/512⌉:
 *            k_e = D_e / W_e; block: Σ_e D_e (exact) and max_e k_e;
 *            Σ_e D_e ≤ G: x_j = 1
 *   outer    ≤ 63× probe: cap_out(C) = block detsum over the entity chunks →
 *            bisection on the bits of C; g_e = the term at C*.  An entity of
 *            one job is finished here by its chunk's thread (the fifo formula,
 *            one division)
 *   inner    one wave per entity of two jobs or more (wave v looks at entities
 *            v, v + 8, …, 64 of them at a time, and visits those).  g_e ≥ D_e:
 *            x_j = 1.  fifo: int64 prefix of sf over the members, 64 at a
 *            time, then the clamp.  fairness: ≤ 63× probe of cap_e(τ) = the
 *            lanes' strided partial sums and the wave's halving tree →
 *            bisection on the bits of τ_e; x_j = min(1, τ_e / c_j)
 *   last     Σ_p sf_p·x_p, block detsum over the position chunks
 *
 * Nothing is staged in LDS: the probes of an entity read 12 B per member from
 * L2, consecutive across the wave (DESIGN.md §19 has the timing).
 */
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <string.h>

#include "../../include/shockwave_amd.h"
#include "sw_alloc.h"
#include "sw_wfh.h"
#include "sw_wfh_layout.h"

static_assert(SW_WFH_MAX_WIDTH == SW_MAX_WIDTH, "the layout header's copy of the width bound");

namespace {

/* the views of one call's blocks */
struct WfhDev {
    const int64_t *offsets, *eoffs, *ebeg;
    const int32_t* workers;
    const double* c;   /* [T] member order */
    const double* W;   /* [Etot] */
    const int32_t* sf; /* [T] member order */
    const int32_t* mem; /* [T] job index within the instance */
    const int32_t* mode; /* [Etot] */
    const int64_t* D; /* [Etot] Σ sf of the entity */
    double *x, *g, *levels;
    double* K; /* [Etot] workspace: k_e, written and read by the entity's chunk thread */
};

/* the wave's halving tree, its lane-0 result in every lane */
__device__ __forceinline__ double wfh_wave_detsum(double v) { return sw_f64u(wave_dettree(v)); }

__global__ __launch_bounds__(SW_BLOCK) void sw_wfh_kernel(const WfhDev d) {
    __shared__ sw_xchg X;
    sw_blk blk{&X, 0};
    sw_chunk ch = sw_chunk_of(d.offsets);
    double* out = d.levels + 2 * (int64_t)blockIdx.x;
    const int64_t e0 = d.eoffs[blockIdx.x];
    const int32_t E = (int32_t)(d.eoffs[blockIdx.x + 1] - e0);
    const int32_t tid = (int32_t)threadIdx.x;
    if (ch.N <= 0) {
        for (int32_t e = tid; e < E; e += SW_BLOCK) d.g[e0 + e] = 0.0;
        sw_chunk_zero<2>(out);
        return;
    }
    ch.split();
    const double Gd = (double)d.workers[blockIdx.x];
    const int64_t base = ch.base;
    const int32_t lane = lane_id();
    const int32_t wv = sw_u32(wave_id());
    /* the thread's chunk of the entities */
    const int32_t qe = (E + SW_BLOCK - 1) / SW_BLOCK;
    const int32_t elo = tid * qe;
    const int32_t ecnt = elo + qe <= E ? qe : (E > elo ? E - elo : 0);
    const int64_t* __restrict__ Dv = d.D + e0 + elo;
    double* Kv = d.K + e0 + elo;

    /* pass 1 */
    double s = 0.0, m = 0.0;
    for (int32_t k = 0; k < ecnt; ++k) {
        const double kk = sw_wfh_coef(Dv[k], d.W[e0 + elo + k]);
        Kv[k] = kk;
        s = s + (double)Dv[k];
        m = kk > m ? kk : m;
    }
    double total, kmax;
    blk.detsum_max(s, m, total, kmax);

    if (total <= Gd) { /* the cluster holds every job whole */
        for (int32_t k = 0; k < ecnt; ++k) d.g[e0 + elo + k] = (double)Dv[k];
        for (int32_t k = 0; k < ch.cnt; ++k) d.x[base + ch.lo + k] = 1.0;
        if (tid == 0) { out[0] = kmax; out[1] = total; }
        return;
    }

    /* outer: cap_out(lo) ≤ G < cap_out(hi) throughout */
    uint64_t blo = sw_bits(0.0), bhi = sw_bits(kmax);
    for (int it = 0; it < SW_WF_ITERS && bhi - blo > 1; ++it) {
        const uint64_t bmid = blo + (bhi - blo) / 2;
        const double C = sw_from_bits(bmid);
        double c = 0.0;
        for (int32_t k = 0; k < ecnt; ++k) c = c + sw_wfh_outer_term(Dv[k], Kv[k], C);
        const double cap = blk.detsum(c);
        if (cap <= Gd) blo = bmid; else bhi = bmid;
    }
    const double Cs = sw_from_bits(blo);
    for (int32_t k = 0; k < ecnt; ++k) {
        const double gk = sw_wfh_outer_term(Dv[k], Kv[k], Cs);
        d.g[e0 + elo + k] = gk;
        const int64_t b = d.ebeg[e0 + elo + k];
        if (d.ebeg[e0 + elo + k + 1] - b == 1) /* an entity of one job */
            d.x[base + d.mem[b]] = gk >= (double)Dv[k] ? 1.0 : sw_wfh_fifo_x(gk, 0, d.sf[b]);
    }
    __syncthreads();

    /* inner: wave v's entities are v, v + 8, …; lane l of a tile looks at the
     * (t + l)-th of them, and the wave visits those of two jobs or more */
    for (int32_t t = 0; wv + SW_WAVES * t < E; t += 64) {
        const int32_t el = wv + SW_WAVES * (t + lane);
        int32_t bl = 0, nl = 0; /* the entity's first position within the instance, its jobs */
        if (el < E) {
            const int64_t b = d.ebeg[e0 + el];
            bl = (int32_t)(b - base);
            nl = (int32_t)(d.ebeg[e0 + el + 1] - b);
        }
        uint64_t todo = sw_u64(__ballot(nl > 1));
        while (todo) {
            const int32_t bit = sw_u32(__builtin_ctzll(todo));
            todo &= todo - 1;
            const int32_t e = wv + SW_WAVES * (t + bit);
            const int64_t b = base + __builtin_amdgcn_readlane(bl, bit);
            const int32_t n = __builtin_amdgcn_readlane(nl, bit);
            const int64_t De = d.D[e0 + e];
            const double ge = d.g[e0 + e];
            const int32_t* __restrict__ sfe = d.sf + b;
            const double* __restrict__ ce = d.c + b;
            const int32_t* __restrict__ me = d.mem + b;
            if (ge >= (double)De) {
                for (int32_t i = lane; i < n; i += 64) d.x[base + me[i]] = 1.0;
            } else if (d.mode[e0 + e] == SW_WFH_FIFO) {
                int64_t pre = 0;
                for (int32_t u = 0; u < n; u += 64) { /* every lane takes every tile: the scan is wave-wide */
                    const int32_t i = u + lane;
                    const int32_t sfi = i < n ? sfe[i] : 0;
                    const int32_t inc = wave_incscan_i32(sfi);
                    if (i < n) d.x[base + me[i]] = sw_wfh_fifo_x(ge, pre + (int64_t)(inc - sfi), sfi);
                    pre += (int64_t)__builtin_amdgcn_readlane(inc, 63);
                }
            } else {
                double cm = 0.0;
                for (int32_t i = lane; i < n; i += 64) cm = ce[i] > cm ? ce[i] : cm;
                cm = wave_max_f64(cm);
                /* cap_e(lo) ≤ g_e < cap_e(hi) = D_e throughout */
                uint64_t lo = sw_bits(0.0), hi = sw_bits(cm);
                for (int it = 0; it < SW_WF_ITERS && hi - lo > 1; ++it) {
                    const uint64_t mid = lo + (hi - lo) / 2;
                    const double tau = sw_from_bits(mid);
                    double p = 0.0;
                    for (int32_t i = lane; i < n; i += 64) p = p + sw_wf_term((double)sfe[i], ce[i], tau);
                    const double cap = wfh_wave_detsum(p);
                    if (cap <= ge) lo = mid; else hi = mid;
                }
                const double tau = sw_from_bits(lo);
                for (int32_t i = lane; i < n; i += 64) d.x[base + me[i]] = sw_wf_x(ce[i], tau);
            }
        }
    }
    __syncthreads();

    /* the allocated capacity, over the position chunks */
    double u = 0.0;
    for (int32_t k = 0; k < ch.cnt; ++k) {
        const int64_t p = base + ch.lo + k;
        u = u + (double)d.sf[p] * d.x[base + d.mem[p]];
    }
    const double used = blk.detsum(u);
    if (tid == 0) { out[0] = Cs; out[1] = used; }
}

int wfh_run(sw_handle* h, const char* who, int32_t count, const int64_t* offsets, const int64_t* eoffs,
            const int32_t* workers, const int32_t* sf, const double* c, const int32_t* ent, const double* W,
            const int32_t* modes, double* x, double* g, double* levels) {
    const std::string w = std::string(who) + ": ";
    int32_t maxq = 0; /* nothing is staged */
    if (const char* e = sw_alloc_scan(count, offsets, workers, "worker counts must be > 0", 0, "SW_WFH_LDS", &maxq))
        return sw_fail(h, SW_ERR_INVALID, w + e);
    if (const char* e = sw_wfh_check(count, offsets, eoffs, sf, c, ent, W, modes, x))
        return sw_fail(h, SW_ERR_INVALID, w + e);
    const sw_wfh_layout L = sw_wfh_plan(count, offsets[count], eoffs[count]);
    if (levels)
        for (size_t i = 0; i < 2 * L.C; ++i) levels[i] = 0.0;
    if (g)
        for (size_t e = 0; e < L.Et; ++e) g[e] = 0.0;
    if (L.T == 0) return SW_OK; /* only empty instances */

    SW_HIP(h, hipSetDevice(h->device));
    sw_io_bufs* b = &h->io;
    SW_HIP(h, b->in.reserve(L.in_bytes));
    SW_HIP(h, b->out.reserve(L.out_bytes));
    SW_HIP(h, b->hin.reserve(L.in_bytes));
    SW_HIP(h, b->hout.reserve(L.back_bytes));
    sw_wfh_pack(L, offsets, eoffs, workers, sf, c, ent, W, modes, b->hin.p);
    SW_HIP(h, hipMemcpyAsync(b->in.p, b->hin.p, L.in_bytes, hipMemcpyHostToDevice, h->stream));
    const unsigned char* di = b->in.p;
    unsigned char* dout = b->out.p;
    const WfhDev dv{(const int64_t*)di, (const int64_t*)(di + L.eoffs), (const int64_t*)(di + L.ebeg),
                    (const int32_t*)(di + L.workers), (const double*)(di + L.c), (const double*)(di + L.W),
                    (const int32_t*)(di + L.sf), (const int32_t*)(di + L.mem), (const int32_t*)(di + L.mode),
                    (const int64_t*)(di + L.D), (double*)dout, (double*)(dout + L.g), (double*)(dout + L.levels),
                    (double*)(dout + L.K)};
    hipLaunchKernelGGL(sw_wfh_kernel, dim3((unsigned)count), dim3(SW_BLOCK), 0, h->stream, dv);
    SW_HIP(h, hipGetLastError());
    SW_HIP(h, hipMemcpyAsync(b->hout.p, dout, L.back_bytes, hipMemcpyDeviceToHost, h->stream));
    SW_HIP(h, hipStreamSynchronize(h->stream));
    memcpy(x, b->hout.p, L.T * 8);
    if (g && L.Et) memcpy(g, b->hout.p + L.g, L.Et * 8);
    if (levels) memcpy(levels, b->hout.p + L.levels, L.C * 16);
    return SW_OK;
}

}  // namespace

extern "C" int sw_wfh_allocate(sw_handle* h, int32_t num_jobs, int32_t num_entities, int32_t num_workers,
                               const int32_t* scale_factors, const double* coefficients,
                               const int32_t* entity_of_job, const double* entity_weights,
                               const int32_t* entity_modes, double* allocation, double* entity_capacity,
                               double* level) {
    if (!h) return SW_ERR_INVALID;
    if (num_jobs < 0 || num_entities < 0)
        return sw_fail(h, SW_ERR_INVALID, "sw_wfh_allocate: num_jobs < 0 or num_entities < 0");
    if (num_jobs == 0) { /* policy.flatten returns None */
        if (level) { level[0] = 0.0; level[1] = 0.0; }
        if (entity_capacity)
            for (int32_t e = 0; e < num_entities; ++e) entity_capacity[e] = 0.0;
        return SW_OK;
    }
    const int64_t offsets[2] = {0, num_jobs}, eoffs[2] = {0, num_entities};
    return wfh_run(h, "sw_wfh_allocate", 1, offsets, eoffs, &num_workers, scale_factors, coefficients,
                   entity_of_job, entity_weights, entity_modes, allocation, entity_capacity, level);
}

extern "C" int sw_wfh_allocate_batch(sw_handle* h, int32_t count, const int64_t* job_offsets,
                                     const int64_t* entity_offsets, const int32_t* num_workers,
                                     const int32_t* scale_factors, const double* coefficients,
                                     const int32_t* entity_of_job, const double* entity_weights,
                                     const int32_t* entity_modes, double* allocation,
                                     double* entity_capacity, double* levels) {
    if (!h) return SW_ERR_INVALID;
    if (count < 0 || (count > 0 && (!job_offsets || !entity_offsets || !num_workers)))
        return sw_fail(h, SW_ERR_INVALID, "sw_wfh_allocate_batch: bad count or null pointers");
    if (count == 0) return SW_OK;
    return wfh_run(h, "sw_wfh_allocate_batch", count, job_offsets, entity_offsets, num_workers, scale_factors,
                   coefficients, entity_of_job, entity_weights, entity_modes, allocation, entity_capacity,
                   levels);
}
