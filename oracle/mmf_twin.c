/*
 * oracle/mmf_twin.c — TEST INFRASTRUCTURE: CPU bit-exact twin of the
 * MaxMinFairness allocation kernel (shockwave-replication_amd/csrc/sw_mmf.hip).
 *
 * Same algorithm, same per-job arithmetic (sw_mmf.h, -ffp-contract=off) and
 * the same deterministic job sums (sw_detsum), so it returns the bits the GPU
 * returns.  It is pinned against the LP itself by tests/test_mmf.py: the
 * optimum level t* matches scipy's HiGHS solution of the reference's LP
 * (policies/max_min_fairness.py:68-93) and the allocation satisfies the
 * analytic-centre optimality conditions.  Never linked into the product.
 */
#include <math.h>
#include <stdint.h>

#include "../shockwave-replication_amd/csrc/sw_mmf.h"
#include "../tests/twins/twin_detsum.h"

/* v is caller scratch of N doubles */
int mmf_twin_allocate(int32_t N, int32_t G, const int32_t* sf, const double* c, double* x,
                      double* level, double* v) {
    if (N <= 0) {
        if (level) { level[0] = 0.0; level[1] = 0.0; }
        return 0;
    }
    double minc = INFINITY;
    for (int32_t j = 0; j < N; ++j) {
        v[j] = (double)sf[j] / c[j];
        minc = c[j] < minc ? c[j] : minc;
    }
    const double capb = (double)G / detsum(v, N);
    if (capb <= minc) {
        for (int32_t j = 0; j < N; ++j) x[j] = capb / c[j];
        if (level) { level[0] = capb; level[1] = 0.0; }
        return 0;
    }
    const double t = minc;
    int64_t pinned = 0;
    for (int32_t j = 0; j < N; ++j) pinned += c[j] <= t ? sf[j] : 0;
    const double gfree = (double)((int64_t)G - pinned);
    uint64_t blo = SW_MMF_MU_LO, bhi = SW_MMF_MU_HI;
    for (int it = 0; it < SW_MMF_ITERS && bhi - blo > 1; ++it) {
        const uint64_t bmid = blo + (bhi - blo) / 2;
        const double mu = sw_from_bits(bmid);
        for (int32_t j = 0; j < N; ++j)
            v[j] = c[j] <= t ? 0.0 : (double)sf[j] * sw_mmf_x(c[j], (double)sf[j], t, mu);
        const double slack = gfree - detsum(v, N);
        if (slack > 0.0 && mu * slack >= 1.0) bhi = bmid; else blo = bmid;
    }
    const double mu = sw_from_bits(bhi);
    for (int32_t j = 0; j < N; ++j) x[j] = c[j] <= t ? 1.0 : sw_mmf_x(c[j], (double)sf[j], t, mu);
    if (level) { level[0] = t; level[1] = mu; }
    return 0;
}

/* ---- the heterogeneity-aware LP over worker types (sw_mmf_lp.h) ---------- */
#include <stdlib.h>

#include "../shockwave-replication_amd/csrc/sw_mmf_lp.h"

/* the pivot cap of an m × n problem, for the tests' bound on the pivots taken */
int64_t mmf_twin_lp_max_pivots(int32_t m, int32_t n) {
    const sw_lp_dims d = sw_lp_dims_of(m, n);
    return sw_lp_max_pivots(&d);
}

/* the entering column of the objective row obj[0 … C) (k_lp_select's
 * reduction, in column order), SW_LP_NO_COLUMN at the optimum */
static int32_t lp_enter(const double* obj, int32_t C, int bland) {
    int32_t e = SW_LP_NO_COLUMN;
    double ev = 0.0;
    for (int32_t c = 0; c < C; ++c) {
        if (!sw_lp_enters(obj[c])) continue;
        const double v = sw_lp_enter_key(obj[c], bland);
        if (sw_lp_enter_before(v, c, ev, e)) { e = c; ev = v; }
    }
    return e;
}

/* the pieces of the pivot rule and of the normalisation, for tests/test_mmf_lp.py */
int32_t mmf_twin_lp_enter(const double* obj, int32_t C, int32_t bland) { return lp_enter(obj, C, bland); }
int32_t mmf_twin_lp_shift(double cmax) { return sw_lp_shift(cmax); }
double mmf_twin_lp_scale(double v, int32_t k) { return sw_lp_scale(v, k); }
/* feeds the objective values z[0 … n) after n pivots to the stall counter;
 * bland[i] = whether pivot i + 1 enters by Bland's rule */
void mmf_twin_lp_stall(const double* z, int32_t n, int32_t* bland) {
    int64_t stall = 0;
    double best = 0.0;
    for (int32_t i = 0; i < n; ++i) {
        sw_lp_note(z[i], &best, &stall);
        bland[i] = sw_lp_bland(stall);
    }
}

/* The kernel's pivots, one after the other (sw_mmf.hip k_lp_select and
 * k_lp_update), by the pivot rule and the normalisation of sw_mmf_lp.h.
 * x: m·n doubles (row-major), level[0] = t*; *pivots the pivots taken.
 * Returns 0, or -2 (no leaving row: cannot happen on this bounded LP) /
 * -3 (pivot cap) / -1 (allocation). */
int mmf_twin_allocate_types(int32_t m, int32_t n, const int32_t* workers, const int32_t* sf,
                            const double* coef, double* x, double* level, int64_t* pivots) {
    const sw_lp_dims d = sw_lp_dims_of(m, n);
    const size_t W = (size_t)d.W, R1 = (size_t)d.R + 1;
    double* a = (double*)malloc(R1 * W * sizeof(double));
    double* f = (double*)malloc(R1 * sizeof(double));
    int32_t* basis = (int32_t*)malloc((size_t)(d.R > 0 ? d.R : 1) * sizeof(int32_t));
    if (!a || !f || !basis) { free(a); free(f); free(basis); return -1; }
    double cmax = 0.0;
    for (int32_t j = 0; j < m * n; ++j) cmax = coef[j] > cmax ? coef[j] : cmax;
    const int32_t shift = sw_lp_shift(cmax);
    for (size_t i = 0; i < R1; ++i)
        for (size_t c = 0; c < W; ++c)
            a[i * W + c] = sw_lp_init(&d, workers, sf, coef, shift, (int32_t)i, (int32_t)c);
    for (int32_t i = 0; i < d.R; ++i) basis[i] = m * n + 1 + i;
    const int64_t maxp = sw_lp_max_pivots(&d);
    int64_t piv = 0, stall = 0;
    double best = 0.0;
    int rc = 0;
    const double* obj = a + (size_t)d.R * W;
    for (;;) {
        if (piv > 0) sw_lp_note(obj[d.C], &best, &stall);
        const int32_t e = lp_enter(obj, d.C, sw_lp_bland(stall));
        if (e == SW_LP_NO_COLUMN) break; /* optimal */
        int32_t r = -1, bb = 0;
        double rb = 0.0;
        for (int32_t i = 0; i < d.R; ++i) {
            const double v = a[(size_t)i * W + e];
            if (sw_lp_leaves(v)) {
                const double ratio = a[(size_t)i * W + d.C] / v;
                if (r < 0 || sw_lp_before(ratio, basis[i], rb, bb)) { r = i; rb = ratio; bb = basis[i]; }
            }
        }
        if (r < 0) { rc = -2; break; }
        if (++piv > maxp) { rc = -3; break; }
        for (size_t i = 0; i < R1; ++i) f[i] = a[i * W + (size_t)e];
        const double pe = f[r];
        double* pr = a + (size_t)r * W;
        for (size_t c = 0; c < W; ++c) pr[c] = pr[c] / pe;
        for (size_t i = 0; i < R1; ++i) {
            const double fi = f[i];
            if ((int32_t)i == r || fi == 0.0) continue;
            double* ai = a + i * W;
            for (size_t c = 0; c < W; ++c) ai[c] = ai[c] - fi * pr[c];
        }
        basis[r] = e;
    }
    double t = 0.0;
    for (int32_t j = 0; j < m * n; ++j) x[j] = 0.0;
    for (int32_t i = 0; i < d.R; ++i) {
        const double v = a[(size_t)i * W + d.C];
        if (basis[i] < m * n) x[basis[i]] = v;
        else if (basis[i] == m * n) t = v;
    }
    level[0] = sw_lp_scale(t, -shift);
    *pivots = piv;
    free(a); free(f); free(basis);
    return rc;
}
