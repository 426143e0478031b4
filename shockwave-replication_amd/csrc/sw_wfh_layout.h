/*
 * sw_wfh_layout.h — the host arithmetic of a hierarchical water-filling call
 * (sw_wfh.hip): the checks that follow the frame's scan of the job offsets and
 * worker counts (sw_alloc_layout.h), the layout of the call's input and output
 * blocks, and the packing of the input block in member order.  No HIP in here:
 * a plain host compiler builds it (tests/native/wfh_layout_check.cpp).
 */
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include <vector>

#include "sw_alloc_layout.h"

#define SW_WFH_MAX_WIDTH 255 /* SW_MAX_WIDTH of include/shockwave_amd.h */

/* The checks of a call after sw_alloc_scan, in the order their errors are
 * reported: the entity offsets start at 0 and, per instance, do not decrease
 * and span at most INT32_MAX − 512 entities; null pointers with jobs or
 * entities present; the per-job rule; the per-entity rules; every job's entity
 * within its instance's range.  Returns the error text, or null. */
inline const char* sw_wfh_check(int32_t count, const int64_t* offsets, const int64_t* eoffs, const int32_t* sf,
                                const double* c, const int32_t* ent, const double* W, const int32_t* modes,
                                const double* x) {
    if (eoffs[0] != 0) return "entity offsets must start at 0";
    for (int32_t i = 0; i < count; ++i) {
        const int64_t n = eoffs[i + 1] - eoffs[i];
        if (n < 0 || n > (int64_t)INT32_MAX - SW_ALLOC_LANES) return "entity offsets must not decrease";
    }
    const int64_t T = offsets[count], Et = eoffs[count];
    if ((T > 0 && (!sf || !c || !ent || !x)) || (Et > 0 && (!W || !modes))) return "null pointers";
    for (int64_t j = 0; j < T; ++j)
        if (sf[j] < 1 || sf[j] > SW_WFH_MAX_WIDTH || !(c[j] > 0.0) || !isfinite(c[j]))
            return "scale factors must be in [1,255], coefficients finite and > 0";
    for (int64_t e = 0; e < Et; ++e) {
        if (!(W[e] > 0.0) || !isfinite(W[e])) return "entity weights must be finite and > 0";
        if (modes[e] != 0 && modes[e] != 1) return "entity modes must be 0 (fairness) or 1 (fifo)";
    }
    for (int32_t i = 0; i < count; ++i) {
        const int64_t E = eoffs[i + 1] - eoffs[i];
        for (int64_t j = offsets[i]; j < offsets[i + 1]; ++j)
            if (ent[j] < 0 || ent[j] >= E) return "entity_of_job must be in [0, num_entities)";
    }
    return nullptr;
}

/* Byte offsets of the views in the two blocks of a call over T jobs and Et
 * entities in C instances:
 *   in : offsets[C+1] | eoffs[C+1] | ebeg[Et+1] | D[Et] (int64) | c[T] | W[Et] (double)
 *        | sf[T] | mem[T] | mode[Et] | workers[C] (int32)
 *   out: x[T] | g[Et] | levels[C][2] (double): back_bytes of it are copied back;
 *        then the workspace K[Et] (double)
 * The widest elements come first, so every view is aligned to its element size. */
struct sw_wfh_layout {
    size_t C, T, Et;
    size_t eoffs, ebeg, D, c, W, sf, mem, mode, workers, in_bytes; /* offsets is at 0 */
    size_t g, levels, back_bytes, K, out_bytes;                    /* x is at 0 */
};

inline sw_wfh_layout sw_wfh_plan(int32_t count, int64_t total, int64_t entities) {
    sw_wfh_layout L{};
    L.C = (size_t)count;
    L.T = (size_t)total;
    L.Et = (size_t)entities;
    L.eoffs = (L.C + 1) * 8;
    L.ebeg = L.eoffs + (L.C + 1) * 8;
    L.D = L.ebeg + (L.Et + 1) * 8;
    L.c = L.D + L.Et * 8;
    L.W = L.c + L.T * 8;
    L.sf = L.W + L.Et * 8;
    L.mem = L.sf + L.T * 4;
    L.mode = L.mem + L.T * 4;
    L.workers = L.mode + L.Et * 4;
    L.in_bytes = L.workers + L.C * 4;
    L.g = L.T * 8;
    L.levels = L.g + L.Et * 8;
    L.back_bytes = L.levels + L.C * 16;
    L.K = L.back_bytes;
    L.out_bytes = L.K + L.Et * 8;
    return L;
}

/* Packs a checked call.  Member order: a counting sort of every instance's jobs
 * by entity, stable in job order.  Position p (counted over the whole call,
 * like the jobs) holds job mem[p] of its instance with sf[p] and c[p]; entity e
 * (counted over the whole call) owns the positions [ebeg[e], ebeg[e+1]) and
 * D[e] = Σ sf over them. */
inline void sw_wfh_pack(const sw_wfh_layout& L, const int64_t* offsets, const int64_t* eoffs,
                        const int32_t* workers, const int32_t* sf, const double* c, const int32_t* ent,
                        const double* W, const int32_t* modes, unsigned char* in) {
    memcpy(in, offsets, (L.C + 1) * 8);
    memcpy(in + L.eoffs, eoffs, (L.C + 1) * 8);
    if (L.Et) memcpy(in + L.W, W, L.Et * 8);
    if (L.Et) memcpy(in + L.mode, modes, L.Et * 4);
    memcpy(in + L.workers, workers, L.C * 4);
    int64_t* ebeg = (int64_t*)(in + L.ebeg);
    int64_t* hD = (int64_t*)(in + L.D);
    double* hc = (double*)(in + L.c);
    int32_t* hsf = (int32_t*)(in + L.sf);
    int32_t* hmem = (int32_t*)(in + L.mem);
    std::vector<int64_t> next;
    for (size_t i = 0; i < L.C; ++i) {
        const int64_t j0 = offsets[i], j1 = offsets[i + 1], e0 = eoffs[i];
        const size_t E = (size_t)(eoffs[i + 1] - e0);
        next.assign(E + 1, 0);
        for (int64_t j = j0; j < j1; ++j) next[(size_t)ent[j] + 1]++;
        int64_t p = j0;
        for (size_t e = 0; e < E; ++e) {
            const int64_t n = next[e + 1];
            ebeg[e0 + (int64_t)e] = p;
            hD[e0 + (int64_t)e] = 0;
            next[e] = p;
            p += n;
        }
        for (int64_t j = j0; j < j1; ++j) {
            const int64_t q = next[(size_t)ent[j]]++;
            hmem[q] = (int32_t)(j - j0);
            hsf[q] = sf[j];
            hc[q] = c[j];
            hD[e0 + ent[j]] += sf[j];
        }
    }
    ebeg[L.Et] = (int64_t)L.T;
}
