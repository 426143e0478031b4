/*
 * sw_types_layout.h — the arithmetic of the worker-type frame (sw_types.h): the
 * checks that the four worker-type calls share, and the layout, packing and
 * unpacking of the one input block and the one output block of a call.  No HIP
 * in here: a plain host compiler builds it (tests/native/types_layout_check.cpp).
 */
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#define SW_TYPES_MAX_COLS 4
#define SW_TYPES_MAX_TYPES 16   /* SW_IPM_MAX_TYPES */
#define SW_TYPES_MAX_JOBS 16384 /* SW_IPM_MAX_JOBS, spelled out in the text below */

/* One input column of doubles: [T·n] (a value per job and type) or [T]. */
struct sw_types_col {
    const double* p;
    bool per_type;
};

/* What a policy's blocks hold besides the offsets, the worker counts, the scale
 * factors, x and the results. */
struct sw_types_shape {
    int ncols;
    sw_types_col cols[SW_TYPES_MAX_COLS];
    bool shifts; /* in : one normalising shift per instance */
    bool levels; /* out: one level per job */
    int W;       /* the caller's result words per instance; the kernel's row has one more, the status */
};

/* The first checks of a call, in the order their errors are reported: the sizes
 * and the two arrays every instance is read from; the offsets start at 0; then
 * per instance, they do not decrease and span at most SW_TYPES_MAX_JOBS jobs,
 * and no worker count is negative.  Returns the error text, or null. */
inline const char* sw_types_check(int32_t count, int32_t n, const int64_t* offsets, const int32_t* workers) {
    if (n < 1 || n > SW_TYPES_MAX_TYPES || !offsets || !workers) return "bad sizes or null pointers";
    if (offsets[0] != 0) return "offsets must start at 0";
    for (int32_t i = 0; i < count; ++i) {
        const int64_t m = offsets[i + 1] - offsets[i];
        if (m < 0) return "offsets must not decrease";
        if (m > SW_TYPES_MAX_JOBS) return "more than 16384 jobs in an instance";
        for (int32_t k = 0; k < n; ++k)
            if (workers[(size_t)i * n + k] < 0) return "worker counts must be >= 0";
    }
    return nullptr;
}

/* Byte offsets of the views in the two blocks of a call over T jobs in C
 * instances of n types:
 *   in : offsets[C+1] (int64) | the columns [T·n] or [T] (double) | workers[C·n]
 *        | shifts[C] when the policy has them | sf[T] (int32), padded to 8
 *   out: x[T·n] | levels[T] when the policy has them | results[C][W+1] (double)
 * The 8-byte views come first, so every view is aligned to its element size. */
struct sw_types_layout {
    size_t C, T, N, W;
    int ncols;
    size_t col[SW_TYPES_MAX_COLS], col_bytes[SW_TYPES_MAX_COLS];
    bool has_shifts, has_levels;
    size_t workers, shifts, sf, in_bytes; /* shifts == sf when the policy has none */
    size_t levels, results, out_bytes;    /* x is at 0; levels == results when the policy has none */
};

inline sw_types_layout sw_types_plan(const sw_types_shape& s, int32_t count, int32_t n, int64_t total) {
    sw_types_layout L{};
    L.C = (size_t)count;
    L.T = (size_t)total;
    L.N = (size_t)n;
    L.W = (size_t)s.W;
    L.ncols = s.ncols;
    L.has_shifts = s.shifts;
    L.has_levels = s.levels;
    size_t o = (L.C + 1) * 8;
    for (int c = 0; c < s.ncols; ++c) {
        L.col[c] = o;
        L.col_bytes[c] = L.T * (s.cols[c].per_type ? L.N : 1) * 8;
        o += L.col_bytes[c];
    }
    L.workers = o;
    L.shifts = L.workers + L.C * L.N * 4;
    L.sf = L.shifts + (s.shifts ? L.C * 4 : 0);
    L.in_bytes = (L.sf + L.T * 4 + 7) & ~(size_t)7;
    L.levels = L.T * L.N * 8;
    L.results = L.levels + (s.levels ? L.T * 8 : 0);
    L.out_bytes = L.results + L.C * (L.W + 1) * 8;
    return L;
}

/* shifts is read only when the policy has them; the padding is left as it is */
inline void sw_types_pack(const sw_types_layout& L, const sw_types_shape& s, const int64_t* offsets,
                          const int32_t* workers, const int32_t* shifts, const int32_t* sf, unsigned char* in) {
    memcpy(in, offsets, (L.C + 1) * 8);
    for (int c = 0; c < L.ncols; ++c) memcpy(in + L.col[c], s.cols[c].p, L.col_bytes[c]);
    memcpy(in + L.workers, workers, L.C * L.N * 4);
    if (L.has_shifts) memcpy(in + L.shifts, shifts, L.C * 4);
    memcpy(in + L.sf, sf, L.T * 4);
}

/* results[C][W] from the kernel's [C][W+1]; results may be null, levels is
 * written only when the policy has them */
inline void sw_types_unpack(const sw_types_layout& L, const unsigned char* out, double* x, double* levels,
                            double* results) {
    memcpy(x, out, L.T * L.N * 8);
    if (L.has_levels) memcpy(levels, out + L.levels, L.T * 8);
    if (results)
        for (size_t i = 0; i < L.C; ++i) memcpy(results + L.W * i, out + L.results + (L.W + 1) * i * 8, L.W * 8);
}

/* the status word of instance i in the output block */
inline int sw_types_status(const sw_types_layout& L, const unsigned char* out, size_t i) {
    double v;
    memcpy(&v, out + L.results + ((L.W + 1) * i + L.W) * 8, 8);
    return (int)v;
}
