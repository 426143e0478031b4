/*
 * sw_alloc_layout.h — the arithmetic of the allocation frame (sw_alloc.h): the
 * checks on a call's CSR offsets and worker counts, the LDS staging bound, and
 * the layout, packing and unpacking of the one input block and the one output
 * block of a call.  No HIP in here: a plain host compiler builds it
 * (tests/native/alloc_layout_check.cpp).
 */
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#define SW_ALLOC_LANES 512 /* the frame's workgroup (SW_BLOCK): one job chunk per thread */
#define SW_ALLOC_MAX_COLS 4

/* One per-job input column of `size` bytes per element, 8 or 4.  A null p
 * packs as zeros; the frame rejects it unless the column is optional. */
struct sw_alloc_col {
    const void* p;
    size_t size;
    bool optional;
};

/* The first checks of a call, in the order their errors are reported: the
 * offsets start at 0; then per instance, they do not decrease and span at most
 * INT32_MAX − 512 jobs, and the worker count is positive (workers_rule: the
 * policy's wording of that).  Returns the error text, or null.
 * *maxq receives the largest chunk length q = ⌈n/512⌉ among the instances of
 * at most lds_jobs jobs (a multiple of 512): the jobs per thread that the
 * launch's LDS must hold.  It is 0, nothing staged, when the environment
 * variable lds_env begins with '0' (A/B timing, tools/). */
inline const char* sw_alloc_scan(int32_t count, const int64_t* offsets, const int32_t* workers,
                                 const char* workers_rule, int32_t lds_jobs, const char* lds_env,
                                 int32_t* maxq) {
    *maxq = 0;
    if (offsets[0] != 0) return "offsets must start at 0";
    int32_t mq = 0;
    for (int32_t i = 0; i < count; ++i) {
        const int64_t n = offsets[i + 1] - offsets[i];
        if (n < 0 || n > (int64_t)INT32_MAX - SW_ALLOC_LANES) return "offsets must not decrease";
        if (workers[i] <= 0) return workers_rule;
        const int32_t q = (int32_t)((n + SW_ALLOC_LANES - 1) / SW_ALLOC_LANES);
        if (q <= lds_jobs / SW_ALLOC_LANES && q > mq) mq = q;
    }
    const char* env = getenv(lds_env);
    if (!(env && env[0] == '0')) *maxq = mq;
    return nullptr;
}

/* Byte offsets of the views in the two blocks of a call over T jobs in C
 * instances with W levels per instance:
 *   in : offsets[C+1] (int64) | the 8-byte columns [T] | the 4-byte columns [T]
 *        | workers[C] (int32)
 *   out: x[T] | levels[C][W] (double)
 * The widest elements come first, so every view is aligned to its element
 * size; the columns are therefore listed 8-byte ones first. */
struct sw_alloc_layout {
    size_t T, C, W;
    int ncols;
    size_t col[SW_ALLOC_MAX_COLS];
    size_t workers, in_bytes;
    size_t levels, out_bytes; /* x is at 0 */
};

inline sw_alloc_layout sw_alloc_plan(const sw_alloc_col* cols, int ncols, int32_t count, int64_t total,
                                     int W) {
    sw_alloc_layout L{};
    L.T = (size_t)total;
    L.C = (size_t)count;
    L.W = (size_t)W;
    L.ncols = ncols;
    size_t o = (L.C + 1) * 8;
    for (int c = 0; c < ncols; ++c) {
        L.col[c] = o;
        o += L.T * cols[c].size;
    }
    L.workers = o;
    L.in_bytes = o + L.C * 4;
    L.levels = L.T * 8;
    L.out_bytes = L.levels + L.C * L.W * 8;
    return L;
}

inline void sw_alloc_pack(const sw_alloc_layout& L, const sw_alloc_col* cols, const int64_t* offsets,
                          const int32_t* workers, unsigned char* in) {
    memcpy(in, offsets, (L.C + 1) * 8);
    for (int c = 0; c < L.ncols; ++c) {
        if (cols[c].p) memcpy(in + L.col[c], cols[c].p, L.T * cols[c].size);
        else memset(in + L.col[c], 0, L.T * cols[c].size);
    }
    memcpy(in + L.workers, workers, L.C * 4);
}

/* levels may be null */
inline void sw_alloc_unpack(const sw_alloc_layout& L, const unsigned char* out, double* x, double* levels) {
    memcpy(x, out, L.T * 8);
    if (levels) memcpy(levels, out + L.levels, L.C * L.W * 8);
}
