/*
 * sw_ftf_types.h — the Gavel FinishTimeFairness (Themis) allocation over worker
 * types whose throughputs differ, shared by the HIP kernel (sw_ftf_types.hip,
 * one workgroup per instance, one launch) and the CPU twin
 * (tests/twins/ftft_twin.c).  Only IEEE +, −, ×, ÷ and comparisons
 * (-ffp-contract=off on both sides), every sum over jobs through the
 * deterministic tree, so the two return the same bits.  It builds on the
 * interior-point engine of sw_mmf_ipm.h and the one-type arithmetic of sw_ftf.h.
 *
 * The reference (policies/finish_time_fairness.py:55-140) solves
 *     minimise ρ  s.t.  a_j + s_j / Σ_k thr_jk·x_jk ≤ ρ·E_j,
 *                       Σ_j sf_j·x_jk ≤ W_k,   Σ_k x_jk ≤ 1,   x ≥ 0,
 * s_j the steps remaining, a_j the time since start, E_j > 0 the expected
 * isolated time.  With d_j(ρ) = ρ·E_j − a_j (sw_ftf.h) the program at a fixed ρ
 * is the feasibility LP Σ_k c_jk(ρ)·x_jk ≥ 1, c_jk(ρ) = thr_jk·d_j(ρ)/s_j, which
 * is feasible exactly when the max-min level t*(ρ) of these rows is ≥ 1: the
 * rows of the engine with κ_j = 1.  A job with s_j = 0 is a dead row (κ = 0,
 * c = thr/max thr, as in sw_mtd_types.h); its constant ratio a_j/E_j only
 * bounds ρ from below.  ρ* is the root of t*(ρ) = 1.
 *
 * The slope.  With y_j the dual of job j's value row (the engine's SW_IPM_SU)
 * and val_j = Σ_k c_jk·x_jk,  dt* / dρ = Σ_j y_j·val_j·E_j/d_j: one more sum in
 * the reduction of the final pass, taken at the second path point.  Its error
 * costs outer steps, never accuracy.
 *
 * The start.  ρ_box = max_j (a_j + p_j)/E_j, p_j = s_j / max{thr_jk : W_k > 0}
 * (dead jobs: a_j/E_j), is the least level the time rows admit; the job that
 * sets it has a largest coefficient of 1, so t*(ρ_box) ≤ 1.  In this arithmetic
 * d_j is max(ρ·E_j − a_j, p_j): the two are equal for ρ ≥ ρ_box up to the
 * rounding of ρ·E_j − a_j, and with the maximum every live row's largest
 * coefficient is ≥ 1 at every probe.  The closer start is the aggregate bound:
 * the least ρ ≥ ρ_box with Σ_j sf_j·min(1, p_j/d_j(ρ)) ≤ Σ_k W_k (every feasible
 * x has Σ_k x_jk ≥ p_j/d_j), the one-type program of sw_ftf.h on p_j by its
 * bisection over the bits of ρ.  It is a lower bound on ρ*, and ρ* itself when
 * the types are identical.
 *
 * The outer iteration (sw_ftft_begin / _next / _feed / _result, scalar work of
 * one thread).  Probe the start; while t < 1 − tol take the Newton step on t*,
 * ρ ← ρ + (1 − t)/t' (exact in one step when every a_j = 0: t* is then linear
 * in ρ).  1/t*(ρ) is convex and decreasing, so the Newton step on φ = 1/t*,
 * ρ ← ρ + t·(1 − t)/t', never overshoots from the left; the t-step can.  If a
 * probe comes out above 1 + tol it is remembered as an upper end, the iteration
 * returns to the largest probed level with t < 1 and takes only φ-steps from
 * there on (SW_FTFT_SAFE); a step that would reach the upper end all the same
 * (the slope's own error) is replaced by the midpoint.  It stops at
 * |t − 1| ≤ tol or when the step no longer changes ρ.  The last probe is always
 * the one at the returned ρ, so the engine's state at the end is the answer's.
 *
 * Every probe is a cold start of the engine (sw_ipm_setup … start2).  The rows
 * are normalised per probe by the power of two that brings the smallest live
 * row's largest coefficient into [1, 2) (as sw_mtd_types.h; it depends on ρ, so
 * it is one more reduction of the probe, not host work).
 *
 * No second phase where t*(ρ*) = 1.  The optimal face of the program is the
 * feasible set of the LP at ρ*, and that is the optimal face of the level LP at
 * ρ* (t* = 1), inequality for inequality; row scaling does not move an analytic
 * centre.  The point returned is the engine's extrapolated point of the last
 * level solve: the centre under the linear barrier, the convention sw_ftf.h
 * fixes for one type.
 *   One case has t*(ρ*) > 1: a dead job's ratio a_j/E_j sets ρ_box and leaves
 * the live jobs room.  ρ* = ρ_box, the feasible set has an interior in the value
 * rows and its centre is not that of the level LP's face: it is found as
 * sw_mtd_types.h finds its second phase, by the engine's objective-free mode at
 * the constant level 1 from the level's second path point (sw_ftft_glob_switch,
 * with that header's thin rule and its measured SW_MTDT_THIN).
 *
 * Flags.  SW_FTFT_BOX: ρ* = ρ_box.  SW_FTFT_IDLE: no live job; ρ* = max a_j/E_j
 * and the point is the centre of the whole polytope by the engine's
 * objective-free mode (as SW_MTDT_IDLE).  SW_FTFT_SAFE: the φ-step fallback
 * was taken.
 *
 * result[5] = ρ* (the last probe's ρ, divided by its t where t < 1:
 * sw_ftft_rho), t of the last probe, Newton steps of all probes, level solves,
 * flags.
 */
#ifndef SW_FTF_TYPES_H
#define SW_FTF_TYPES_H

#include "sw_arith.h"
#include "sw_ftf.h"
#include "sw_mmf_ipm.h"
#include "sw_mtd_types.h"

/* Measured on the twin over the 300 instances of both families of
 * tests/ftftcases.py (m < 50, n < 6; steps 10^U(4, 6) and 10^U(1, 7.5), mixed
 * a_j, 10 % dead): the engine's level at the probed ρ differs from HiGHS's on
 * the same rows by at most 2.0e-9 relative (narrow) and 7.7e-9 (wide)
 * (tests/test_ftf_types.py prints both).  The engine's value is the smaller:
 * its point is feasible.  The tolerance is a decade above the worst.  At 1e-9
 * every instance still converged, in at most 8 solves. */
#ifndef SW_FTFT_TOL
#define SW_FTFT_TOL 1e-7
#endif
#define SW_FTFT_ROUND 1e-12

/* Level solves of one call.  Measured on the same 300 instances: 1–5 on both
 * families, the SAFE path on none (1–8 and on 5 at a tolerance of 1e-9); the
 * cap is four times the worst of either. */
#define SW_FTFT_MAX_SOLVES 32

#define SW_FTFT_BOX 1  /* flags: ρ* = ρ_box */
#define SW_FTFT_IDLE 2 /* flags: no live job */
#define SW_FTFT_SAFE 4 /* flags: a probe overshot, φ-steps from then on */

#define SW_FTFT_CAP (-5) /* SW_FTFT_MAX_SOLVES level solves without reaching the tolerance */

/* The outer iteration's state. */
typedef struct {
    double rho, rho_box, lo, t_lo, tp_lo, hi, t, tol;
    int32_t have_lo, have_hi, safe, solves, done, status, wide, pad;
} sw_ftft_search;

SW_HD void sw_ftft_begin(sw_ftft_search* s, double rho_box, double start, double tol) {
    s->rho = start;
    s->rho_box = rho_box;
    s->lo = 0.0;
    s->t_lo = 0.0;
    s->tp_lo = 0.0;
    s->hi = 0.0;
    s->t = 0.0;
    s->tol = tol;
    s->have_lo = 0;
    s->have_hi = 0;
    s->safe = 0;
    s->solves = 0;
    s->done = 0;
    s->status = 0;
    s->wide = 0;
}

/* Whether another probe is needed, and its level. */
SW_HD int sw_ftft_next(sw_ftft_search* s, double* rho) {
    if (s->done || s->status != 0) return 0;
    if (s->solves >= SW_FTFT_MAX_SOLVES) {
        s->status = SW_FTFT_CAP;
        return 0;
    }
    *rho = s->rho;
    return 1;
}

/* a step from (rho, t, tp) that stays below a known upper end */
SW_HD double sw_ftft_step(const sw_ftft_search* s, double rho, double t, double tp) {
    const double step = s->safe ? t * (1.0 - t) / tp : (1.0 - t) / tp;
    double nxt = rho + step;
    if (s->have_hi && !(nxt < s->hi)) nxt = rho + 0.5 * (s->hi - rho);
    return nxt;
}

/* The probe at rho gave the level t with slope tp. */
SW_HD void sw_ftft_feed(sw_ftft_search* s, double rho, double t, double tp) {
    s->solves = s->solves + 1;
    s->rho = rho;
    s->t = t;
    if (t >= 1.0 - s->tol && t <= 1.0 + s->tol) {
        s->done = 1;
        return;
    }
    if (t < 1.0) {
        if (!(tp > 0.0)) { /* no live row carries a dual: not a level program */
            s->status = SW_FTFT_CAP;
            return;
        }
        s->have_lo = 1;
        s->lo = rho;
        s->t_lo = t;
        s->tp_lo = tp;
        {
            const double nxt = sw_ftft_step(s, rho, t, tp);
            if (nxt == rho || (s->have_hi && nxt == s->hi)) s->done = 1;
            else s->rho = nxt;
        }
        return;
    }
    /* above 1 + tol */
    if (rho == s->rho_box) { /* the time rows admit nothing lower: a dead job's ratio set ρ_box */
        s->done = 1;
        s->wide = 1;
        return;
    }
    if (!s->have_hi || rho < s->hi) s->hi = rho;
    s->have_hi = 1;
    s->safe = 1;
    if (!s->have_lo) {
        s->rho = s->rho_box;
        return;
    }
    {
        const double nxt = sw_ftft_step(s, s->lo, s->t_lo, s->tp_lo);
        if (nxt == s->lo || nxt == s->hi) s->done = 1; /* the ends are neighbours: the feasible one is kept */
        else s->rho = nxt;
    }
}

/* The level returned for the last probe (ρ, t).  The engine's t is the least
 * row value of its own point, so that point meets every row of the program at
 * any ρ' with d_j(ρ') ≥ d_j(ρ)/t; for t < 1, ρ' = ρ/t is one (a_j/t ≥ a_j).  The
 * accepted probe can have t as low as 1 − tol: returning ρ/t keeps every row
 * within the engine's own residual instead of within tol.  Below
 * SW_FTFT_ROUND, the rounding of the level itself, ρ is returned as probed, so
 * that ρ_box is returned bit for bit. */
SW_HD int sw_ftft_lifted(const sw_ftft_search* s) { return s->t < 1.0 - SW_FTFT_ROUND; }
SW_HD double sw_ftft_rho(const sw_ftft_search* s) { return sw_ftft_lifted(s) ? s->rho / s->t : s->rho; }
SW_HD int32_t sw_ftft_flags(const sw_ftft_search* s) {
    return (s->rho == s->rho_box && !sw_ftft_lifted(s) ? SW_FTFT_BOX : 0) | (s->safe ? SW_FTFT_SAFE : 0);
}

/* The state of a call that is not the engine's (LDS in the kernel). */
typedef struct {
    sw_ftft_search s;
    double rho, G, cap0;
    uint64_t blo, bhi;
    int32_t shift, iters, flags, idle, bis, bisdone, centring, pad;
} sw_ftft_glob;

/* The largest throughput on a type with workers, the time at a full allocation. */
SW_HD double sw_ftft_best(const sw_ipm_glob* g, const double* thr) {
    double mx = 0.0;
    for (int32_t k = 0; k < g->na; ++k) mx = sw_max(mx, thr[g->act[k]]);
    return mx;
}
SW_HD double sw_ftft_p(double steps, double best) { return steps > 0.0 ? steps / best : 0.0; }

/* d_j(ρ) of a live job, never below p_j */
SW_HD double sw_ftft_d(double p, double a, double E, double rho) { return sw_max(sw_ftf_d(a, E, rho), p); }

/* The coefficient of a live job on a type. */
SW_HD double sw_ftft_coef(double thr, double d, double steps) { return thr * d / steps; }

/* Pass P1.  Sums: [0] whether the job is live; max: [0] its ratio at a full
 * allocation. */
SW_HD void sw_ftft_job_box(const sw_ipm_glob* g, const double* thr, double steps, double a, double E, double* sums,
                           double* maxes) {
    sums[0] = steps > 0.0 ? 1.0 : 0.0;
    maxes[0] = sw_ftf_box(sw_ftft_p(steps, sw_ftft_best(g, thr)), a, E);
}

/* After pass P1 (one thread). */
SW_HD void sw_ftft_glob_box(const sw_ipm_glob* g, sw_ftft_glob* q, const double* sums, const double* maxes) {
    double G = 0.0;
    for (int32_t k = 0; k < g->na; ++k) G = G + g->Wk[k];
    q->G = G;
    q->idle = !(sums[0] > 0.0);
    q->rho = maxes[0];
    q->shift = 0;
    q->iters = 0;
    q->flags = 0;
    q->bis = 0;
    q->bisdone = 0;
    q->centring = 0;
    q->blo = 0;
    q->bhi = 0;
    q->cap0 = 0.0;
    sw_ftft_begin(&q->s, maxes[0], maxes[0], SW_FTFT_TOL);
}

/* The aggregate start: its probes (q->rho) and their answers.  Pass P2 sums
 * [0] sf_j·min(1, p_j/d_j(q->rho)). */
SW_HD double sw_ftft_job_cap(const sw_ipm_glob* g, const sw_ftft_glob* q, double sf, const double* thr, double steps,
                             double a, double E) {
    return sf * sw_ftf_low(sw_ftft_p(steps, sw_ftft_best(g, thr)), a, E, q->rho);
}
SW_HD int sw_ftft_start_next(sw_ftft_glob* q) {
    if (q->idle || q->bisdone) return 0;
    if (q->bis == 0) {
        q->rho = q->s.rho_box;
        return 1;
    }
    if (q->bis > SW_FTF_ITERS || q->bhi - q->blo <= 1) {
        q->s.rho = sw_from_bits(q->bhi);
        q->bisdone = 1;
        return 0;
    }
    q->rho = sw_from_bits(q->blo + (q->bhi - q->blo) / 2);
    return 1;
}
SW_HD void sw_ftft_start_feed(sw_ftft_glob* q, double cap) {
    if (q->bis == 0) {
        q->cap0 = cap;
        if (cap <= q->G) q->bisdone = 1; /* the start is ρ_box */
        q->blo = sw_bits(q->s.rho_box);
        q->bhi = SW_FTF_RHO_HI;
    } else if (cap <= q->G) {
        q->bhi = sw_bits(q->rho);
    } else {
        q->blo = sw_bits(q->rho);
    }
    q->bis = q->bis + 1;
}

/* Pass S of a probe.  Max: [0] −(largest coefficient) of a live job, −DBL_MAX
 * of a dead one. */
SW_HD double sw_ftft_job_rowmax(const sw_ipm_glob* g, const sw_ftft_glob* q, const double* thr, double steps, double a,
                                double E) {
    const double best = sw_ftft_best(g, thr);
    if (!(steps > 0.0)) return -1.7976931348623157e308;
    return -sw_ftft_coef(best, sw_ftft_d(sw_ftft_p(steps, best), a, E, q->rho), steps);
}
SW_HD void sw_ftft_glob_shift(sw_ftft_glob* q, const double* maxes) {
    q->shift = q->idle ? 0 : sw_lp_shift(-maxes[0]);
}

/* Init pass 1 of a probe (in place of sw_ipm_job_load): the job's normalised
 * rows at q->rho.  Sums: [0] sf, [1] whether the job has a value row; max: [0]
 * −(largest coefficient) of a live job, −DBL_MAX of a dead one. */
SW_HD void sw_ftft_job_load(const sw_ipm_glob* g, const sw_ftft_glob* q, sw_ipm_job* J, const double* thr,
                            double steps, double a, double E, double* sums, double* maxes) {
    const int live = steps > 0.0;
    const double best = sw_ftft_best(g, thr);
    const double d = live ? sw_ftft_d(sw_ftft_p(steps, best), a, E, q->rho) : 0.0;
    double mx = 0.0;
    for (int32_t k = 0; k < J->na; ++k) {
        const double t = thr[g->act[k]];
        const double c = live ? sw_lp_scale(sw_ftft_coef(t, d, steps), q->shift) : (best > 0.0 ? t / best : 0.0);
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
    maxes[0] = live ? -mx : -1.7976931348623157e308;
}

/* After init pass 1 (one thread).  Without a live job there is no level: the
 * engine's objective-free mode from its own start. */
SW_HD void sw_ftft_glob_load(sw_ipm_glob* g, const sw_ftft_glob* q, const double* sums, const double* maxes) {
    sw_ipm_glob_load(g, sums, maxes);
    if (q->idle) {
        g->has_t = 0;
        g->mu_end = 1.0;
        g->npairs = (double)g->m * (double)g->na + g->nv + (double)g->m + (double)g->na;
    }
}

/* The slope's term of a job, at the engine's current point: y_j·val_j·E_j/d_j
 * in the normalised rows. */
SW_HD double sw_ftft_job_slope(const sw_ipm_glob* g, const sw_ftft_glob* q, const sw_ipm_job* J, const double* thr,
                               double steps, double a, double E) {
    double val = 0.0;
    if (!(steps > 0.0) || SW_IPM_Q(J, SW_IPM_HASV) == 0.0) return 0.0;
    for (int32_t k = 0; k < J->na; ++k) val = val + SW_IPM_C(J, k) * SW_IPM_X(J, k);
    {
        const double best = sw_ftft_best(g, thr);
        return SW_IPM_Q(J, SW_IPM_SU) * val * E / sw_ftft_d(sw_ftft_p(steps, best), a, E, q->rho);
    }
}

/* After a probe's final pass (one thread): the level and its slope to the
 * outer iteration. */
SW_HD void sw_ftft_glob_feed(const sw_ipm_glob* g, sw_ftft_glob* q, double slope) {
    q->iters = q->iters + g->iters;
    sw_ftft_feed(&q->s, q->rho, sw_ipm_level(g, q->shift), sw_lp_scale(slope, -q->shift));
}

/* An objective-free run is over (one thread): the only probe of a call
 * without a live job, or the centring at ρ_box. */
SW_HD void sw_ftft_glob_free(const sw_ipm_glob* g, sw_ftft_glob* q) {
    q->iters = q->iters + g->iters;
    if (!q->s.done) q->s.solves = q->s.solves + 1;
    q->s.done = 1;
    q->centring = 0;
}

/* After the last probe (one thread): whether the polytope at ρ* has an
 * interior to centre in.  That is so only when t*(ρ_box) > 1, the level a dead
 * job's ratio a_j/E_j left to the live ones.  Then the engine's state is
 * switched to its objective-free mode at the constant level 1 by
 * sw_mtdt_glob_centre (returns 1: sw_mtdt_job_switch on every job, then
 * the Newton loop again), under the same thin rule: below a margin of
 * SW_MTDT_THIN the extrapolated point is kept. */
SW_HD int sw_ftft_glob_switch(sw_ipm_glob* g, sw_ftft_glob* q) {
    if (!q->s.wide || q->centring) return 0;
    {
        const double tc = sw_lp_scale(1.0, q->shift);
        const double ts = sw_lp_scale(q->s.t, q->shift);
        const double width = ts - tc;
        if (!(q->s.t - 1.0 >= SW_MTDT_THIN) || !(width > 0.0)) return 0;
        q->centring = 1;
        sw_mtdt_glob_centre(g, tc, width);
    }
    return 1;
}

/* result[5] */
SW_HD void sw_ftft_result(const sw_ftft_glob* q, double* out) {
    out[0] = q->idle ? q->s.rho : sw_ftft_rho(&q->s);
    out[1] = q->idle ? 0.0 : q->s.t;
    out[2] = (double)q->iters;
    out[3] = (double)q->s.solves;
    out[4] = (double)(q->idle ? SW_FTFT_IDLE : sw_ftft_flags(&q->s));
}

#endif /* SW_FTF_TYPES_H */
