/*
 * tests/twins/twin_detsum.h — TEST INFRASTRUCTURE: the deterministic job sum
 * of the CPU twins, in the order of the kernels' block detsum (sw_block.h): 512
 * contiguous chunks summed left to right, a halving tree over each wave's 64
 * partials, then a halving tree over the waves.
 */
#pragma once
#include <stdint.h>

#include "../../shockwave-replication_amd/csrc/sw_arith.h"

static double detsum(const double* v, int32_t N) {
    double part[SW_DET_LANES];
    double wsum[SW_DET_LANES / 64];
    int32_t q = (N + SW_DET_LANES - 1) / SW_DET_LANES;
    for (int32_t lane = 0; lane < SW_DET_LANES; ++lane) {
        double s = 0.0;
        int32_t lo = lane * q, hi = lo + q < N ? lo + q : N;
        for (int32_t j = lo; j < hi; ++j) s = s + v[j];
        part[lane] = s;
    }
    for (int32_t w = 0; w < SW_DET_LANES / 64; ++w) {
        double* p = part + 64 * w;
        for (int32_t h = 32; h >= 1; h >>= 1)
            for (int32_t i = 0; i < h; ++i) p[i] = p[i] + p[i + h];
        wsum[w] = p[0];
    }
    for (int32_t h = SW_DET_LANES / 128; h >= 1; h >>= 1)
        for (int32_t i = 0; i < h; ++i) wsum[i] = wsum[i] + wsum[i + h];
    return wsum[0];
}
