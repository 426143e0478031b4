/*
 * sw_types.h — the worker-type frame: what the four calls over worker types
 * that differ (sw_mmf_ipm.hip, sw_mtd_types.hip, sw_ftf_types.hip,
 * sw_wf_types.hip) share around their kernels.  One 512-thread workgroup per
 * instance of a CSR batch; the results are x[total][n], for water filling
 * levels[total], and results[count][W].
 *
 *   the frame   sw_types_run: the checks of a call in one order, the input
 *               block packed and copied, the engine's workspace reserved, the
 *               policy's launch, the output block copied back, the status
 *               column turned into an error text, the results unpacked (the
 *               arithmetic is in sw_types_layout.h)
 *   a policy    its columns and result width (sw_types_call), the check of an
 *               instance's values with the instance's normalising shift (scan),
 *               and its kernel's launch on the device views (launch)
 *
 * The four calls share one workspace on the handle (sw_handle::types), as they
 * share sw_io_bufs: every call ends in a stream synchronise, so no two are in
 * flight on one handle, and reserve only grows.  A call therefore finds the
 * words of an earlier call, of any of the four policies, in its workspace.
 * None reads them: every solve is a cold start.  Each field of a job is written
 * by the kernel's load pass, by the engine's start passes (x, the slacks, the
 * duals), by pass B (the scalings) or by pass C (the steps) before the pass
 * that reads it, the first path point's copies (X1, SU1, U1) are read only
 * after sw_ipm_two_points says that they were taken, and water filling's three
 * extra fields are written by sw_wft_job_begin and sw_wft_job_keep before they
 * are read.  An instance without jobs or without workers touches none.
 */
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <string>

#include "../../include/shockwave_amd.h"
#include "sw_block.h"
#include "sw_handle.h"
#include "sw_mmf_ipm.h"
#include "sw_types_layout.h"

static_assert(SW_TYPES_MAX_TYPES == SW_IPM_MAX_TYPES && SW_TYPES_MAX_JOBS == SW_IPM_MAX_JOBS,
              "the frame's limits are the engine's");

/* One call, single (count = 1) or batch. */
struct sw_types_call {
    const char* who; /* the entry point, for the error texts */
    int32_t count, n;
    const int64_t* offsets;
    const int32_t* workers; /* [count][n] */
    const int32_t* sf;      /* [total] */
    sw_types_shape shape;
    double* x;       /* [total][n] */
    double* levels;  /* [total], only with shape.levels */
    double* results; /* [count][W], may be null */
    int fields;      /* doubles of workspace per job */
    int status;      /* the policy's own status next to SW_IPM_CAP and SW_IPM_BREAK, 0 for none */
    const char* status_text;
};

/* What a policy's launch receives: the device views of the two blocks (col[] in
 * the order of sw_types_shape.cols) and the workspace. */
struct sw_types_dev {
    unsigned count;
    int32_t n;
    hipStream_t stream;
    const int64_t* offsets;
    const int32_t *workers, *shifts, *sf;
    const double* col[SW_TYPES_MAX_COLS];
    double *ws, *x, *levels, *results;
};

/* scan(i, &shift, &job): checks the values of instance i; returns the error
 * text or null, with job >= 0 when the text is about that job of the instance,
 * and yields the instance's shift (ignored without shape.shifts).
 * launch(d): enqueues the policy's kernel on d.stream.  The first error of a
 * bad call is the first in this order: sizes, offsets and worker counts; null
 * pointers; the scans, instance by instance. */
template <class Scan, class Launch>
int sw_types_run(sw_handle* h, const sw_types_call& c, Scan scan, Launch launch) {
    const std::string w = std::string(c.who) + ": ";
    if (const char* e = sw_types_check(c.count, c.n, c.offsets, c.workers)) return sw_fail(h, SW_ERR_INVALID, w + e);
    const int64_t total = c.offsets[c.count];
    bool missing = !c.sf || !c.x || (c.shape.levels && !c.levels);
    for (int k = 0; k < c.shape.ncols; ++k) missing = missing || !c.shape.cols[k].p;
    if (total > 0 && missing) return sw_fail(h, SW_ERR_INVALID, w + "null pointers");
    sw_types_bufs* tb = &h->types;
    tb->shifts.assign((size_t)c.count, 0);
    for (int32_t i = 0; i < c.count; ++i) {
        int64_t job = -1;
        if (const char* e = scan(i, &tb->shifts[(size_t)i], &job))
            return sw_fail(h, SW_ERR_INVALID,
                           w + e + (job < 0 ? std::string() : " (job " + std::to_string(job) + " of instance " +
                                                                  std::to_string(i) + ")"));
    }
    if (c.results)
        for (int64_t i = 0; i < c.shape.W * (int64_t)c.count; ++i) c.results[i] = 0.0;
    if (total == 0) return SW_OK; /* only empty instances: policy.flatten returns None */
    SW_HIP(h, hipSetDevice(h->device));
    sw_io_bufs* b = &h->io;
    const sw_types_layout L = sw_types_plan(c.shape, c.count, c.n, total);
    const size_t in_bytes = L.in_bytes, out_bytes = L.out_bytes;
    SW_HIP(h, b->in.reserve(in_bytes));
    SW_HIP(h, b->out.reserve(out_bytes));
    SW_HIP(h, b->hin.reserve(in_bytes));
    SW_HIP(h, b->hout.reserve(out_bytes));
    SW_HIP(h, tb->ws.reserve((size_t)c.fields * L.T));
    sw_types_pack(L, c.shape, c.offsets, c.workers, tb->shifts.data(), c.sf, b->hin.p);
    SW_HIP(h, hipMemcpyAsync(b->in.p, b->hin.p, in_bytes, hipMemcpyHostToDevice, h->stream));
    sw_types_dev d{(unsigned)c.count, c.n, h->stream, (const int64_t*)b->in.p,
                   (const int32_t*)(b->in.p + L.workers), (const int32_t*)(b->in.p + L.shifts),
                   (const int32_t*)(b->in.p + L.sf), {}, tb->ws.p, (double*)b->out.p,
                   (double*)(b->out.p + L.levels), (double*)(b->out.p + L.results)};
    for (int k = 0; k < L.ncols; ++k) d.col[k] = (const double*)(b->in.p + L.col[k]);
    launch(d);
    SW_HIP(h, hipGetLastError());
    SW_HIP(h, hipMemcpyAsync(b->hout.p, b->out.p, out_bytes, hipMemcpyDeviceToHost, h->stream));
    SW_HIP(h, hipStreamSynchronize(h->stream));
    for (int32_t i = 0; i < c.count; ++i) {
        const int status = sw_types_status(L, b->hout.p, (size_t)i);
        if (status != SW_IPM_OK)
            return sw_fail(h, SW_ERR_CAPACITY,
                           w + (status == SW_IPM_CAP               ? "step cap reached"
                                : c.status && status == c.status ? c.status_text
                                                                 : "the reduced system lost positive definiteness") +
                               " (instance " + std::to_string(i) + ")");
    }
    sw_types_unpack(L, b->hout.p, c.x, c.levels, c.results);
    return SW_OK;
}
