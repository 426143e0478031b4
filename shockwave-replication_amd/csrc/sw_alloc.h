/*
 * sw_alloc.h — the allocation frame: what the per-job Gavel baselines
 * (sw_ftf.hip, sw_wf.hip, sw_mtd.hip, sw_mst.hip) share around their solve
 * bodies.  One 512-thread workgroup per instance of a CSR batch; thread L owns
 * the job chunk [L·q, (L+1)·q), q = ⌈N/512⌉; the results are x[total] and
 * levels[count][W].
 *
 *   host    sw_alloc_run: the checks of a call in one order, the input block
 *           packed and copied, the policy's launch, the output block copied
 *           back (the arithmetic is in sw_alloc_layout.h)
 *   device  sw_chunk: a workgroup's instance and a thread's chunk of it;
 *           sw_chunk_at: where the chunk's k-th job is read
 */
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <string>

#include "../../include/shockwave_amd.h"
#include "sw_alloc_layout.h"
#include "sw_block.h"
#include "sw_handle.h"

static_assert(SW_ALLOC_LANES == SW_BLOCK, "the frame's chunks are one per thread of the workgroup");

/* One call, single (count = 1) or batch. */
struct sw_alloc_call {
    const char* who; /* the entry point, for the error texts */
    int32_t count;
    const int64_t* offsets;
    const int32_t* workers;
    const char* workers_rule; /* the text for a worker count < 1 */
    int ncols;
    sw_alloc_col cols[SW_ALLOC_MAX_COLS];
    double* x;
    double* levels; /* [count][W], may be null */
    int W;
    int32_t lds_jobs;    /* instances of at most this many jobs are staged in LDS */
    int32_t job_bytes;   /* LDS bytes per staged job */
    const char* lds_env; /* "0" there: nothing is staged */
};

/* What a policy's launch receives: the device views of the two blocks (col[] in
 * the order of sw_alloc_call.cols), and the dynamic LDS for maxq jobs per thread. */
struct sw_alloc_dev {
    unsigned count;
    hipStream_t stream;
    const int64_t* offsets;
    const int32_t* workers;
    const void* col[SW_ALLOC_MAX_COLS];
    double *x, *levels;
    int32_t maxq;
    size_t lds;
};

/* rule(j): the error text for job j, or null.  launch(d): enqueues the policy's
 * kernel on d.stream.  The first error of a bad call is the first in this
 * order: offsets and worker counts, null pointers, the per-job rule. */
template <class Rule, class Launch>
int sw_alloc_run(sw_handle* h, const sw_alloc_call& c, Rule rule, Launch launch) {
    const std::string w = std::string(c.who) + ": ";
    int32_t maxq = 0;
    if (const char* e = sw_alloc_scan(c.count, c.offsets, c.workers, c.workers_rule, c.lds_jobs, c.lds_env, &maxq))
        return sw_fail(h, SW_ERR_INVALID, w + e);
    const int64_t total = c.offsets[c.count];
    bool missing = !c.x;
    for (int k = 0; k < c.ncols; ++k) missing = missing || (!c.cols[k].p && !c.cols[k].optional);
    if (total > 0 && missing) return sw_fail(h, SW_ERR_INVALID, w + "null pointers");
    for (int64_t j = 0; j < total; ++j)
        if (const char* e = rule(j)) return sw_fail(h, SW_ERR_INVALID, w + e);
    if (c.levels)
        for (int64_t i = 0; i < c.W * (int64_t)c.count; ++i) c.levels[i] = 0.0;
    if (total == 0) return SW_OK; /* only empty instances */
    SW_HIP(h, hipSetDevice(h->device));
    sw_io_bufs* b = &h->io;
    const sw_alloc_layout L = sw_alloc_plan(c.cols, c.ncols, c.count, total, c.W);
    const size_t in_bytes = L.in_bytes, out_bytes = L.out_bytes;
    SW_HIP(h, b->in.reserve(in_bytes));
    SW_HIP(h, b->out.reserve(out_bytes));
    SW_HIP(h, b->hin.reserve(in_bytes));
    SW_HIP(h, b->hout.reserve(out_bytes));
    sw_alloc_pack(L, c.cols, c.offsets, c.workers, b->hin.p);
    SW_HIP(h, hipMemcpyAsync(b->in.p, b->hin.p, in_bytes, hipMemcpyHostToDevice, h->stream));
    sw_alloc_dev d{(unsigned)c.count, h->stream, (const int64_t*)b->in.p, (const int32_t*)(b->in.p + L.workers),
                   {}, (double*)b->out.p, (double*)(b->out.p + L.levels), maxq,
                   (size_t)maxq * SW_BLOCK * (size_t)c.job_bytes};
    for (int k = 0; k < c.ncols; ++k) d.col[k] = b->in.p + L.col[k];
    launch(d);
    SW_HIP(h, hipGetLastError());
    SW_HIP(h, hipMemcpyAsync(b->hout.p, b->out.p, out_bytes, hipMemcpyDeviceToHost, h->stream));
    SW_HIP(h, hipStreamSynchronize(h->stream));
    sw_alloc_unpack(L, b->hout.p, c.x, c.levels);
    return SW_OK;
}

/* The instance of workgroup blockIdx.x, the N jobs at base, and after split()
 * the chunk of thread threadIdx.x: jobs base + lo + [0, cnt).  A kernel takes
 * the instance with sw_chunk_of, leaves an empty one (N <= 0: policy.flatten
 * returns None) through sw_chunk_zero, and splits the others. */
struct sw_chunk {
    int64_t base;
    int32_t N, q, lo, cnt;
    __device__ __forceinline__ void split() {
        q = (N + SW_BLOCK - 1) / SW_BLOCK;
        lo = (int32_t)threadIdx.x * q;
        const int32_t hi = lo + q < N ? lo + q : N;
        cnt = hi > lo ? hi - lo : 0;
    }
};

__device__ __forceinline__ sw_chunk sw_chunk_of(const int64_t* __restrict__ offsets) {
    const int64_t inst = blockIdx.x;
    const int64_t base = offsets[inst];
    return {base, (int32_t)(offsets[inst + 1] - base), 0, 0, 0};
}

/* the W levels of an empty instance */
template <int W>
__device__ __forceinline__ void sw_chunk_zero(double* __restrict__ out) {
    if (threadIdx.x == 0)
        for (int i = 0; i < W; ++i) out[i] = 0.0;
}

/* Where thread L reads job lo + k of its chunk: element L·q + k of the
 * instance's arrays in global memory, slot k·512 + L of the transposed LDS
 * image (a wave reads consecutive words). */
template <bool LDS>
__device__ __forceinline__ int32_t sw_chunk_at(int32_t k, int32_t q) {
    return LDS ? k * SW_BLOCK + (int32_t)threadIdx.x : (int32_t)threadIdx.x * q + k;
}
