/*
 * sw_mmf_lp.h — the heterogeneity-aware MaxMinFairness LP over several worker
 * types (policies/max_min_fairness.py:44-100, MaxMinFairnessPolicyWithPerf;
 * base constraints policy.py:57-63), solved by the primal simplex method on a
 * dense tableau.  Shared by the HIP kernel (sw_mmf.hip, one workgroup, the
 * tableau in HBM/L2) and the CPU twin (oracle/mmf_twin.c), which run the same
 * pivots with the same per-element arithmetic (-ffp-contract=off), so they
 * return the same bits.
 *
 * The LP, m jobs × n worker types, x[j][k] = share of time job j runs on
 * type k (coef[j][k] = throughput · priority weight · scale factor, the
 * caller's normalisation, max_min_fairness.py:57-73):
 *     maximise t
 *     s.t.  t − Σ_k coef[j][k]·x[j][k] ≤ 0      (m value rows)
 *           Σ_j sf_j·x[j][k] ≤ workers[k]       (n capacity rows)
 *           Σ_k x[j][k] ≤ 1                     (m time rows)
 *           x ≥ 0, t ≥ 0
 * Tableau: rows 0 … R−1 the constraints (value rows, capacity rows, time rows;
 * R = 2m + n), row R the objective (z − c form: −1 under t); columns x[j][k]
 * at j·n + k, t at m·n, the slack of row i at m·n + 1 + i, the right-hand
 * side last (row stride SW_LP_W = m·n + 2 + R).  The slack basis is feasible
 * (right-hand sides 0, workers, 1).
 *
 * Normalisation: on entry every coefficient is multiplied by the power of two
 * that brings the largest of them into [1, 2) (sw_lp_shift, sw_lp_scale: exact,
 * so t*(s·coef) = s·t*(coef) bit for bit for s a power of two, and the
 * allocation does not depend on s); the level is scaled back at the end.
 * SW_LP_EPS is then relative to the largest coefficient.  All-zero
 * coefficients are left alone.
 *
 * Pivot rule.  Entering column (sw_lp_enters, sw_lp_enter_before): among the
 * columns whose objective entry is below −SW_LP_EPS, the most negative entry,
 * ties to the lowest index (Dantzig's rule, here "the steep rule": comparisons
 * only, so a reduction in any order finds the same column).  This LP is
 * degenerate — every value row starts tight at t = 0 — and the steep rule
 * alone can cycle, so a stall counter guards it (sw_lp_note): after SW_LP_STALL
 * consecutive pivots that did not raise the objective value above the best
 * seen so far, the entering column is Bland's (the lowest index below
 * −SW_LP_EPS) until the next pivot that does raise it.  The leaving row is
 * always the one of least ratio rhs_i / a_ie over a_ie > SW_LP_PIV_EPS, ties
 * to the lowest basic variable index (Bland's leaving rule).
 *   The pivot element's bar is higher than the objective's: an entry that is
 * zero in exact arithmetic is left at 1e-11 … 1e-10 by the cancellations of a
 * few hundred updates, and in a degenerate row (right-hand side 0: every type
 * without workers gives one) its ratio 0 wins the ratio test.  Dividing by
 * such an entry destroys the tableau: with the bar at SW_LP_EPS, problems with
 * W in {0, 1, 2} ended 1e-3 below the optimum or at the pivot cap with levels
 * of −3,692.  After the normalisation the genuine pivot elements seen on
 * every test family are ≥ 2e-6 (coefficients over six decades), so 1e-9
 * separates the two; a coefficient below 1e-9 of the largest can no longer be
 * pivoted on, which costs at most that fraction of the level.
 *   Termination: a run of Bland pivots cannot cycle (Bland 1977: lowest-index
 * entering and leaving variables visit no basis twice), so it either reaches
 * the optimum or a pivot that raises the objective strictly above the best
 * value seen.  Each return to the steep rule therefore costs one strict
 * increase of the best value, which is the objective at a vertex; the LP has
 * finitely many vertices, so finitely many such increases, and between two of
 * them at most SW_LP_STALL steep pivots and one finite Bland run.  The pivot
 * cap (sw_lp_max_pivots) stays as the guard against rounding.
 *   Why not Bland's rule throughout: on m × 16 problems with coefficients over
 * three decades it takes 20 to 130 times the pivots (20,302 at 80 × 16, the
 * cap at 120 × 12), and the tableau drifts to constraint violations of 7e-4
 * (DESIGN.md §12).
 *
 * A pivot divides the pivot row by the pivot element
 * (p_j = a_rj / a_re), then every other row i subtracts f_i·p_j with f_i its
 * entry in the entering column before the pivot.  The optimum found is a
 * vertex of the LP: its level t* is the LP's (unique) optimum; the allocation
 * is one optimal vertex (the reference's ECOS returns an interior point of
 * the same optimal face, so allocations agree only where the optimum is
 * unique — tests/test_mmf.py checks the level against HiGHS and the
 * allocation for feasibility and optimality).
 */
#ifndef SW_MMF_LP_H
#define SW_MMF_LP_H

#include "sw_arith.h"

#define SW_LP_EPS 1e-11
#define SW_LP_PIV_EPS 1e-9    /* least pivot element, see the pivot rule above */
#define SW_LP_STALL 8         /* pivots without a rise of the objective before Bland's rule takes over */
#define SW_LP_MAX_TYPES 16    /* worker types the call accepts */
#define SW_LP_MAX_JOBS 2048   /* jobs (the tableau: (2m + n + 1)·(m·n + 2m + n + 2) doubles) */

typedef struct {
    int32_t m, n, R, C, W; /* jobs, types, constraint rows, columns (no rhs), row stride */
} sw_lp_dims;

SW_HD sw_lp_dims sw_lp_dims_of(int32_t m, int32_t n) {
    sw_lp_dims d;
    d.m = m;
    d.n = n;
    d.R = 2 * m + n;
    d.C = m * n + 1 + d.R;
    d.W = d.C + 1;
    return d;
}

/* The normalisation: k = −⌊log2 cmax⌋ for the largest coefficient cmax > 0
 * (read off its bits; subnormals by their leading bit), 0 for cmax = 0. */
SW_HD int32_t sw_lp_shift(double cmax) {
    const uint64_t u = sw_bits(cmax);
    const int32_t ex = (int32_t)((u >> 52) & 0x7FF);
    uint64_t mant = u & 0xFFFFFFFFFFFFFull;
    int32_t top = -1;
    if (ex > 0) return 1023 - ex;
    for (; mant; mant >>= 1) ++top;
    return top < 0 ? 0 : 1074 - top;
}

/* v·2^k, k in [−2046, 2046], as two multiplications by powers of two in the
 * normal range (exact unless the result itself is subnormal or overflows) */
SW_HD double sw_lp_pow2(int32_t k) { return sw_from_bits((uint64_t)(k + 1023) << 52); }
SW_HD double sw_lp_scale(double v, int32_t k) {
    const int32_t k1 = k / 2;
    return v * sw_lp_pow2(k1) * sw_lp_pow2(k - k1);
}

/* Entry (i, c) of the initial tableau; shift = sw_lp_shift(max coef). */
SW_HD double sw_lp_init(const sw_lp_dims* d, const int32_t* workers, const int32_t* sf,
                        const double* coef, int32_t shift, int32_t i, int32_t c) {
    const int32_t m = d->m, n = d->n, tcol = m * n, rhs = d->C;
    if (i == d->R) return c == tcol ? -1.0 : 0.0; /* objective: maximise t */
    if (c == tcol + 1 + i) return 1.0;            /* the row's slack */
    if (i < m) {                                  /* value row of job i */
        if (c == tcol) return 1.0;
        if (c >= i * n && c < (i + 1) * n) return -sw_lp_scale(coef[c], shift);
        return 0.0;
    }
    if (i < m + n) { /* capacity row of type k */
        const int32_t k = i - m;
        if (c == rhs) return (double)workers[k];
        if (c < tcol && c % n == k) return (double)sf[c / n];
        return 0.0;
    }
    { /* time row of job j */
        const int32_t j = i - m - n;
        if (c == rhs) return 1.0;
        if (c >= j * n && c < (j + 1) * n) return 1.0;
        return 0.0;
    }
}

/* The entering rule.  A column enters only if its objective entry o is below
 * −SW_LP_EPS; its key is o under the steep rule and 0 under Bland's, so that
 * one order — smaller key, then lower column — serves both.  The empty
 * candidate is (0, INT32_MAX): it loses to every column that may enter. */
#define SW_LP_NO_COLUMN 0x7FFFFFFF
SW_HD int sw_lp_bland(int64_t stall) { return stall >= SW_LP_STALL; }
SW_HD int sw_lp_enters(double o) { return o < -SW_LP_EPS; }
SW_HD double sw_lp_enter_key(double o, int bland) { return bland ? 0.0 : o; }
SW_HD int sw_lp_enter_before(double v, int32_t c, double vb, int32_t cb) {
    return v < vb || (v == vb && c < cb);
}

/* The stall counter, once per pivot taken: z is the objective value after the
 * pivot, *best the largest seen so far (0 at the slack basis). */
SW_HD void sw_lp_note(double z, double* best, int64_t* stall) {
    if (z > *best) {
        *best = z;
        *stall = 0;
    } else if (*stall < SW_LP_STALL) {
        *stall = *stall + 1;
    }
}

/* a row may leave only on a pivot element above the rounding residue */
SW_HD int sw_lp_leaves(double a_ie) { return a_ie > SW_LP_PIV_EPS; }

/* the leaving-row order: smaller ratio, then smaller basic variable */
SW_HD int sw_lp_before(double r, int32_t b, double rb, int32_t bb) {
    return r < rb || (r == rb && b < bb);
}

/* pivots the call may take before it gives up (SW_ERR_CAPACITY) */
SW_HD int64_t sw_lp_max_pivots(const sw_lp_dims* d) { return 50 * (int64_t)(d->R + d->C) + 1000; }

#endif /* SW_MMF_LP_H */
