/*
 * tests/twins/wfh_twin.c — TEST INFRASTRUCTURE: CPU bit-exact twin of the
 * hierarchical (entity) water-filling allocation kernel
 * (shockwave-replication_amd/csrc/sw_wfh.hip).
 *
 * Same algorithm, same arithmetic (sw_wfh.h, -ffp-contract=off) and the same
 * order of every sum: the member order, sw_detsum over the entities and over
 * the positions, and the wave sum of an entity's members (64 strided lane
 * partials, then the halving tree).  It is pinned by tests/test_wfh.py against
 * the reference's staged process in exact rationals and against the stage
 * loop restated over HiGHS (tests/wfh_ref.py).  Never linked into the product.
 */
#include <math.h>
#include <stdint.h>
#include <stdlib.h>

#include "../../shockwave-replication_amd/csrc/sw_arith.h"
#include "../../shockwave-replication_amd/csrc/sw_wfh.h"
#include "twin_detsum.h"

/* cap_e(τ): lane l adds members l, l + 64, … left to right, then the tree */
static double wave_cap(const int32_t* sf, const double* c, int32_t n, double tau) {
    double p[64];
    for (int32_t l = 0; l < 64; ++l) {
        double s = 0.0;
        for (int32_t i = l; i < n; i += 64) s = s + sw_wf_term((double)sf[i], c[i], tau);
        p[l] = s;
    }
    for (int32_t h = 32; h >= 1; h >>= 1)
        for (int32_t i = 0; i < h; ++i) p[i] = p[i] + p[i + h];
    return p[0];
}

/* ent[j] in [0, E), W > 0, mode 0 fairness / 1 fifo (the caller checks);
 * gcap receives g_e, level (C*, Σ sf·x).  Returns 0, or -1 out of memory. */
int wfh_twin_allocate(int32_t N, int32_t E, int32_t G, const int32_t* sf, const double* c, const int32_t* ent,
                      const double* W, const int32_t* mode, double* x, double* gcap, double* level) {
    if (level) { level[0] = 0.0; level[1] = 0.0; }
    for (int32_t e = 0; e < E; ++e) gcap[e] = 0.0;
    if (N <= 0) return 0;
    const int32_t V = N > E ? N : E;
    int32_t* ebeg = (int32_t*)malloc(sizeof(int32_t) * ((size_t)E + 2));
    int32_t* next = (int32_t*)malloc(sizeof(int32_t) * ((size_t)E + 2));
    int32_t* mem = (int32_t*)malloc(sizeof(int32_t) * (size_t)N);
    int32_t* msf = (int32_t*)malloc(sizeof(int32_t) * (size_t)N);
    double* mc = (double*)malloc(sizeof(double) * (size_t)N);
    double* v = (double*)calloc((size_t)V, sizeof(double));
    int64_t* D = (int64_t*)malloc(sizeof(int64_t) * ((size_t)E + 1));
    double* K = (double*)malloc(sizeof(double) * ((size_t)E + 1));
    int rc = -1;
    if (!ebeg || !next || !mem || !msf || !mc || !v || !D || !K) goto done;
    rc = 0;

    /* member order */
    for (int32_t e = 0; e <= E; ++e) ebeg[e] = 0;
    for (int32_t j = 0; j < N; ++j) ebeg[ent[j] + 1]++;
    for (int32_t e = 0; e < E; ++e) ebeg[e + 1] += ebeg[e];
    for (int32_t e = 0; e < E; ++e) next[e] = ebeg[e];
    for (int32_t j = 0; j < N; ++j) {
        const int32_t q = next[ent[j]]++;
        mem[q] = j; msf[q] = sf[j]; mc[q] = c[j];
    }

    /* pass 1 */
    double kmax = 0.0;
    for (int32_t e = 0; e < E; ++e) {
        int64_t s = 0;
        for (int32_t p = ebeg[e]; p < ebeg[e + 1]; ++p) s += msf[p];
        D[e] = s;
        K[e] = sw_wfh_coef(s, W[e]);
        v[e] = (double)s;
        kmax = K[e] > kmax ? K[e] : kmax;
    }
    const double total = detsum(v, E);
    const double Gd = (double)G;
    if (total <= Gd) {
        for (int32_t e = 0; e < E; ++e) gcap[e] = (double)D[e];
        for (int32_t j = 0; j < N; ++j) x[j] = 1.0;
        if (level) { level[0] = kmax; level[1] = total; }
        goto done;
    }

    /* outer */
    uint64_t blo = sw_bits(0.0), bhi = sw_bits(kmax);
    for (int it = 0; it < SW_WF_ITERS && bhi - blo > 1; ++it) {
        const uint64_t bmid = blo + (bhi - blo) / 2;
        const double C = sw_from_bits(bmid);
        for (int32_t e = 0; e < E; ++e) v[e] = sw_wfh_outer_term(D[e], K[e], C);
        if (detsum(v, E) <= Gd) blo = bmid; else bhi = bmid;
    }
    const double Cs = sw_from_bits(blo);
    for (int32_t e = 0; e < E; ++e) gcap[e] = sw_wfh_outer_term(D[e], K[e], Cs);

    /* inner */
    for (int32_t e = 0; e < E; ++e) {
        const int32_t b = ebeg[e], n = ebeg[e + 1] - b;
        if (n == 0) continue;
        const double ge = gcap[e];
        if (ge >= (double)D[e]) {
            for (int32_t i = 0; i < n; ++i) x[mem[b + i]] = 1.0;
        } else if (n == 1 || mode[e] == SW_WFH_FIFO) {
            int64_t pre = 0;
            for (int32_t i = 0; i < n; ++i) {
                x[mem[b + i]] = sw_wfh_fifo_x(ge, pre, msf[b + i]);
                pre += msf[b + i];
            }
        } else {
            double cm = 0.0;
            for (int32_t i = 0; i < n; ++i) cm = mc[b + i] > cm ? mc[b + i] : cm;
            uint64_t lo = sw_bits(0.0), hi = sw_bits(cm);
            for (int it = 0; it < SW_WF_ITERS && hi - lo > 1; ++it) {
                const uint64_t mid = lo + (hi - lo) / 2;
                if (wave_cap(msf + b, mc + b, n, sw_from_bits(mid)) <= ge) lo = mid; else hi = mid;
            }
            const double tau = sw_from_bits(lo);
            for (int32_t i = 0; i < n; ++i) x[mem[b + i]] = sw_wf_x(mc[b + i], tau);
        }
    }

    /* the allocated capacity, over the positions */
    for (int32_t p = 0; p < N; ++p) v[p] = (double)msf[p] * x[mem[p]];
    if (level) { level[0] = Cs; level[1] = detsum(v, N); }

done:
    free(ebeg); free(next); free(mem); free(msf); free(mc); free(v); free(D); free(K);
    return rc;
}
