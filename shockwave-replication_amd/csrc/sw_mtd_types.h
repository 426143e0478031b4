/*
 * sw_mtd_types.h — the Gavel MinTotalDuration (makespan) allocation over worker
 * types whose throughputs differ, shared by the HIP kernel (sw_mtd_types.hip,
 * one workgroup per instance, one launch) and the CPU twin
 * (tests/twins/mtdt_twin.c).  Only IEEE +, −, ×, ÷ and comparisons
 * (-ffp-contract=off on both sides), every sum over jobs through the
 * deterministic tree, so the two return the same bits.  It builds on the
 * interior-point engine of sw_mmf_ipm.h and the search of sw_mtd.h.
 *
 * The reference (policies/min_total_duration.py:41-106) bisects T and solves
 * per probe the feasibility LP
 *     Σ_k thr_jk·x_jk ≥ steps_j / T,  Σ_j sf_j·x_jk ≤ workers_k,  Σ_k x_jk ≤ 1,  x ≥ 0.
 * That LP is feasible at T exactly when T·t* ≥ 1, t* the max-min level of
 * Σ_k (thr_jk / steps_j)·x_jk over the live jobs (steps_j > 0) under the same
 * capacity and time rows: scale a maximiser of the level by 1/(T·t*).
 *
 * Phase 1, the level.  The engine's two-point path on the rows
 *     κ_j·t ≤ Σ_k c_jk·x_jk,   live: κ = 1, c = thr/steps;  dead: κ = 0, c = thr/max_k thr,
 * normalised by a power of two (sw_mtdt_rowmax).  A dead job's row does not
 * bound t (κ = 0) and never pins it; it is kept so that both phases run on the same rows, and because it is a row of
 * the reference's LP.  t* is the extrapolated level (relative error 8e-7 at
 * coefficients that span six decades).
 *
 * The search.  The reference's two loops through sw_mtd_begin / _next / _feed /
 * _result with feasible(T) = (T·t* ≥ 1.0), one multiplication and one
 * comparison on the unnormalised t*: scalar work of one thread.  Without a live
 * job every probe is feasible, T ends at the last midpoint above 100
 * (103.814…), the level is 0.0 and SW_MTDT_IDLE is set.
 *   SW_MTD_ROUNDS stays a proven bound.  The validator admits a live job only
 * with a positive throughput on a type with workers and a best full time
 * steps_j / max_k thr_jk ≤ SW_MTD_FULL_TIME_MAX = 1e15 (the maximum over types
 * with workers), m ≤ 16384 and sf ≤ 255.  The point x_j,best(j) = 1/(255·m)
 * meets every capacity row (Σ sf·x ≤ 1 ≤ workers_k) and time row, and gives
 * every live job a value ≥ 1e-15/(255·16384) > 2.3e-22, so t* > 2.3e-22 and,
 * with the level's error far below a factor 2, every T ≥ 1e22 is feasible.  The
 * first probe of round r ≥ 1 is 5.5·10^(5+r): the search has ended by round 17,
 * inside the 23 rounds of sw_mtd.h.
 *
 * Phase 2, the centre.  The point returned is the maximiser of Σ log(slack)
 * over every inequality of the reference's LP at the found T, the sum without
 * those tight on the whole polytope (x ≥ 0 on a type without workers: exactly
 * 0.0; the value row of a dead job without throughput on any type with
 * workers).  It is the engine's objective-free mode (has_t = 0) with the level
 * held at the constant 1/T: Newton steps towards every z·s = 1 on the rows
 * Σ c·x − κ/T ≥ 0, the rows of phase 1 (row scaling does not move the centre:
 * a live row has right side 1/T instead of steps/T, a dead one 0).
 *   The start is the second path point of phase 1, not a fresh one.  At that
 * point x, the capacity and time slacks are strictly positive, and with
 * u ← u + κ·(t₂ − 1/T) so are the value slacks as soon as the margin
 * T·t* − 1 exceeds the path's own distance t* − t₂ ≤ (pairs)·μ₂; below that
 * u is kept and the row starts with a residual κ·(t₂ − 1/T) that the Newton
 * steps remove.  Without an objective the dual equations are homogeneous, so
 * the duals of the path point divided by μ₂ are dual feasible again and every
 * pair starts at z·s = 1 except the value rows that bound the level: at a
 * small margin, where a fresh start would be far outside the thin polytope,
 * the start is nearly centred.  A fresh start (x = θ) has value residuals of
 * the level's own size at every margin.
 *   The duals at the centre are of size 1/slack, up to 1/(t* − 1/T): the dual
 * residual bound SW_IPM_RES is taken relative to that (g->scale).
 *
 * The thin polytope.  margin = T·t* − 1 can be arbitrarily small, or negative
 * by the level's own error.  Below SW_MTDT_THIN phase 2 is skipped, the
 * allocation is phase 1's extrapolated point (the centre of the level LP's
 * optimal face, feasible at T up to the level's error) and SW_MTDT_THIN_FLAG is
 * set.  The threshold is measured (SW_MTDT_THIN below).
 *
 * Measured against an independent computation (tests/mtd_types_ref.py: HiGHS,
 * a replay of the search, a null-space Newton centre; tests/test_mtd_types.py):
 * T equal on 150 of 150 instances of each family (steps 10^U(4, 6) and
 * 10^U(1, 7.5)), none excluded by the near-probe rule; shares within 1.8e-10
 * (narrow) and 8.9e-11 (wide) of the centre on 105 instances, bar 1e-6; every
 * row of the LP within 1e-9.  Phase 2 takes 4–15 Newton steps (median 6) from
 * the start above, 2–9 (median 2) at a margin of 1e-8.
 *
 * result[4] = T, t* (1/seconds), Newton steps of both phases, flags.
 */
#ifndef SW_MTD_TYPES_H
#define SW_MTD_TYPES_H

#include "sw_arith.h"
#include "sw_mmf_ipm.h"
#include "sw_mtd.h"

/* Measured on the twin built with the rule switched off, over the 300
 * instances of both families of tests/mtdtcases.py (m < 50, n < 6), all steps
 * multiplied so that the margin comes out at the target: at 1e-4, 1e-5, 1e-6,
 * 1e-7 and 1e-8 phase 2 converged on every instance (at most 47 Newton steps
 * in all, every row within 1e-9); at 1e-9 the step cap was reached on 4 of 300,
 * at 1e-12 on 13, at 1e-13 on 108.  The break-down margin is between 1e-9 and
 * 1e-8; the threshold is a decade above the smallest margin at which every
 * instance converged. */
#ifndef SW_MTDT_THIN
#define SW_MTDT_THIN 1e-7
#endif

#define SW_MTDT_IDLE 1      /* flags: no live job */
#define SW_MTDT_THIN_FLAG 2 /* flags: margin below SW_MTDT_THIN, phase 2 skipped */

/* The state of a call that is not the engine's (LDS in the kernel). */
typedef struct {
    double T, tstar, margin;
    int32_t flags, iters1, phase, pad;
} sw_mtdt_glob;

SW_HD void sw_mtdt_setup(sw_mtdt_glob* q) {
    q->T = 0.0;
    q->tstar = 0.0;
    q->margin = 0.0;
    q->flags = 0;
    q->iters1 = 0;
    q->phase = 0;
}

/* The coefficient of a live job on a type. */
SW_HD double sw_mtdt_coef(double thr, double steps) { return thr / steps; }

/* The normalisation: the power of two that brings the SMALLEST live row's
 * largest coefficient (on a type with workers) into [1, 2).  That coefficient
 * bounds the level from above (x ≤ 1), so the normalised level is at most 2 and
 * in practice within a few decades of 1, where the engine's tolerances, which
 * are measured against the level, mean what they say.  Row scaling leaves the
 * central path where it is; with the largest coefficient of all at [1, 2)
 * (sw_mmf_ipm.h) steps that span 6.5 decades put the level at 1e-7 and the
 * dual residual bound 1e-10·level below the rounding of duals of size 1: the
 * step cap was reached on 66 of 150 instances of the wide family. */
SW_HD double sw_mtdt_rowmax(int32_t n, const int32_t* workers, const double* thr, double steps) {
    double mx = 0.0;
    for (int32_t k = 0; k < n; ++k)
        if (workers[k] > 0) mx = sw_max(mx, sw_mtdt_coef(thr[k], steps));
    return mx;
}
SW_HD double sw_mtdt_shift_take(double cmin, double rowmax) {
    return cmin > 0.0 && cmin < rowmax ? cmin : rowmax;
}

/* The search on a known level: T and the margin T·t* − 1. */
SW_HD void sw_mtdt_search(sw_mtdt_glob* q, double tstar, int idle) {
    sw_mtd_search s;
    double T = 0.0;
    sw_mtd_begin(&s);
    for (int32_t it = 0; it < SW_MTD_MAX_PROBES && sw_mtd_next(&s, &T); ++it)
        sw_mtd_feed(&s, T, idle ? 1 : (T * tstar >= 1.0));
    q->T = sw_mtd_result(&s);
    q->tstar = idle ? 0.0 : tstar;
    q->margin = idle ? 0.0 : q->T * tstar - 1.0;
}

/* Init pass 1 (in place of sw_ipm_job_load): the job's normalised rows.  Sums:
 * [0] sf, [1] whether the job has a value row, [2] whether it is live; max:
 * [0] −(largest coefficient) of a live job, −DBL_MAX of a dead one. */
SW_HD void sw_mtdt_job_load(const sw_ipm_glob* g, sw_ipm_job* J, const double* thr, double steps, int32_t shift,
                            double* sums, double* maxes) {
    const int live = steps > 0.0;
    double mx = 0.0, tmx = 0.0;
    for (int32_t k = 0; k < J->na; ++k) tmx = sw_max(tmx, thr[g->act[k]]);
    for (int32_t k = 0; k < J->na; ++k) {
        const double t = thr[g->act[k]];
        const double c = live ? sw_lp_scale(sw_mtdt_coef(t, steps), shift) : (tmx > 0.0 ? t / tmx : 0.0);
        SW_IPM_C(J, k) = c;
        mx = sw_max(mx, c);
    }
    SW_IPM_Q(J, SW_IPM_HASV) = mx > 0.0 ? 1.0 : 0.0;
    SW_IPM_Q(J, SW_IPM_KAP) = live ? 1.0 : 0.0;
    SW_IPM_Q(J, SW_IPM_BET) = 0.0;
    {
        const int32_t k = sw_lp_shift(mx);
        SW_IPM_Q(J, SW_IPM_RSC) = mx > 0.0 && k < 0 ? sw_lp_scale(1.0, k) : 1.0;
    }
    sums[0] = J->sf;
    sums[1] = mx > 0.0 ? 1.0 : 0.0;
    sums[2] = live ? 1.0 : 0.0;
    maxes[0] = live ? -mx : -1.7976931348623157e308;
}

/* After pass 1 (one thread).  Without a live job there is no level: the
 * engine's objective-free mode from its own start, and the search at once. */
SW_HD void sw_mtdt_glob_load(sw_ipm_glob* g, sw_mtdt_glob* q, const double* sums, const double* maxes) {
    sw_ipm_glob_load(g, sums, maxes);
    if (!(sums[2] > 0.0)) {
        g->has_t = 0;
        g->mu_end = 1.0;
        g->npairs = (double)g->m * (double)g->na + g->nv + (double)g->m + (double)g->na;
        q->flags = SW_MTDT_IDLE;
        q->phase = 1;
        sw_mtdt_search(q, 0.0, 1);
    }
}

/* The engine's state from the second path point of a level solve to its
 * objective-free mode at the constant (normalised) level tc, width = t* − tc > 0
 * (one thread; shared with sw_ftf_types.h).  g->tau receives 1/μ₂ for the jobs'
 * pass (sw_mtdt_job_switch), g->rhst the amount κ-rows' slacks grow by. */
SW_HD void sw_mtdt_glob_centre(sw_ipm_glob* g, double tc, double width) {
    const double inv = 1.0 / g->mu_end;
    g->rhst = g->t > tc ? g->t - tc : 0.0;
    g->tau = inv;
    g->npairs = g->npairs - 1.0;
    g->has_t = 0;
    g->t = tc;
    g->st = 0.0;
    g->dt = 0.0;
    g->dst = 0.0;
    g->mu_end = 1.0;
    g->scale = width < 1.0 ? 1.0 / width : 1.0;
    g->stage = 0;
    g->save = 0;
    g->done = 0;
    g->iters = 0;
    for (int32_t k = 0; k < g->na; ++k) g->sw[k] = g->sw[k] * inv;
}

/* After phase 1 and its final pass (one thread): the search, and either the
 * thin rule (returns 0: the extrapolated point is the answer) or the switch of
 * the engine's state to phase 2 (returns 1: sw_mtdt_job_switch on every job,
 * then the Newton loop again).  g->tau receives 1/μ₂ for the jobs' pass,
 * g->rhst the amount κ-rows' slacks grow by. */
SW_HD int sw_mtdt_glob_switch(sw_ipm_glob* g, sw_mtdt_glob* q, int32_t shift) {
    sw_mtdt_search(q, sw_ipm_level(g, shift), 0);
    q->phase = 1;
    const double tc = sw_lp_scale(1.0 / q->T, shift);
    const double ts = sw_lp_scale(q->tstar, shift);
    const double width = ts - tc;
    if (!(q->margin >= SW_MTDT_THIN) || !(width > 0.0)) {
        q->flags = q->flags | SW_MTDT_THIN_FLAG;
        return 0;
    }
    q->iters1 = g->iters;
    sw_mtdt_glob_centre(g, tc, width);
    return 1;
}

/* The switch, per job: the duals onto z·s = 1, the value slack onto the row
 * at the constant level. */
SW_HD void sw_mtdt_job_switch(const sw_ipm_glob* g, sw_ipm_job* J) {
    const double inv = g->tau;
    for (int32_t k = 0; k < J->na; ++k) SW_IPM_S(J, k) = SW_IPM_S(J, k) * inv;
    SW_IPM_Q(J, SW_IPM_SV) = SW_IPM_Q(J, SW_IPM_SV) * inv;
    if (SW_IPM_Q(J, SW_IPM_HASV) != 0.0) {
        SW_IPM_Q(J, SW_IPM_SU) = SW_IPM_Q(J, SW_IPM_SU) * inv;
        SW_IPM_Q(J, SW_IPM_U) = SW_IPM_Q(J, SW_IPM_U) + SW_IPM_Q(J, SW_IPM_KAP) * g->rhst;
    }
}

/* result[4] */
SW_HD void sw_mtdt_result(const sw_ipm_glob* g, const sw_mtdt_glob* q, double* out) {
    out[0] = q->T;
    out[1] = q->tstar;
    out[2] = (double)(q->iters1 + g->iters);
    out[3] = (double)q->flags;
}

#endif /* SW_MTD_TYPES_H */
