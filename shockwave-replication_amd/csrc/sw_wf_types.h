/*
 * sw_wf_types.h — the Gavel water-filling MaxMinFairness allocation over worker
 * types whose throughputs differ, shared by the HIP kernel (sw_wf_types.hip,
 * one workgroup per instance, one launch) and the CPU twin
 * (tests/twins/wft_twin.c).  Only IEEE +, −, ×, ÷ and comparisons
 * (-ffp-contract=off on both sides), every sum over jobs through the
 * deterministic tree, so the two return the same bits.  It builds on the
 * interior-point engine of sw_mmf_ipm.h.
 *
 * The reference (policies/max_min_fairness_water_filling.py:303-409, the
 * WithPerf class without entities) raises every unfrozen job by a common
 * amount per stage, finds the jobs that cannot rise any further with a MILP,
 * freezes them and goes on.  With c_jk = thr_jk/prop_j · (1/w_j)·sf_j (the
 * caller's coefficients) and val_j(x) = Σ_k c_jk·x_jk its fixed point is the
 * LEXICOGRAPHIC MAX-MIN vector of val_j over
 *     Σ_j sf_j·x_jk ≤ W_k,   Σ_k x_jk ≤ 1,   x ≥ 0.
 * That vector is unique; the shares are not, and the reference returns the
 * last stage's ECOS point, the analytic centre of the last LP's optimal face.
 *
 * A stage is one level solve of the engine, cold-started: an unfrozen job's
 * row is t ≤ val_j (κ = 1, β = 0), a job frozen at the level F_j has the row
 * F_j ≤ val_j (κ = 0, β = F_j: the constant sw_mmf_ipm.h holds per value row).
 * The unfrozen jobs that are bottlenecks at the stage's level are frozen at it;
 * the loop ends when every job is frozen.  The allocation returned is the
 * extrapolated point of the LAST level solve: the centre of the last LP's
 * optimal face (with more than one stage, corrected for the ease by a repeat
 * of that solve: "The repeat" below).
 *
 * The ease.  A frozen job cannot exceed its level while the others keep
 * theirs, and what stops it (a time row, a type it fills with other frozen
 * jobs) is then tight on the whole feasible set of every later stage: those
 * LPs have no interior and no central path.  Measured with β = F_j exactly: the
 * duals grow without bound below μ of about 5e-8 and 42 of the first 60 fuzz
 * instances end at the step cap.  So a frozen row is eased: β_j = F_j·(1 − ε),
 * ε = SW_WFT_EASE = 2^-30, the width of the later stages' interior; the levels
 * returned are eased likewise, so the shares meet every row at them to the
 * engine's residual.
 *   The eased rows lift a later stage's level: by Σ_j y_j·F_j·ε/(1 − ε) over
 * the frozen jobs, y_j the row's dual, where the dual is unique.  The
 * sensitivity is not small (a level rises by up to 470 times what an earlier
 * one is lowered by), so the lift is taken off before the stage's level is
 * used: one more sum of the final pass, with y_j extrapolated to μ = 0 from
 * the two path points as the shares are (SW_IPM_SU1).  Where the dual is not
 * unique the path's dual is the centre of the dual face and the lift it gives
 * is not the level's one-sided slope: that is the worst case below.
 *   Measured against HiGHS on 6 seeds of the fuzz family (1,800 instances): the
 * relative error of a level is at most 9.7e-8 on all but one instance and
 * 8.6e-7 on that one (seed 12345, instance 40: 3.5e-6 at ε = 2^-27, so it is
 * the ease, amplified, and the lift does not take it off).  With y_j of the
 * second path point alone the worst was 1.2e-6 at every ε; without the lift
 * 4.3e-6 at ε = 3e-8.
 *
 * The retry.  Late stages are degenerate by construction, and at the second
 * path point the reduced system lost positive definiteness in rounding on
 * 0.5–1.7 % of the family's draws at ε = 2^-27 (and on 1 of 25 instances with
 * identical types).  A stage whose solve ends in SW_IPM_BREAK or SW_IPM_CAP is
 * solved again with both the ease and μ₁ eight times larger, at most
 * SW_WFT_TRIES times (sw_wft_retry).  The call then sets SW_WFT_COARSE and
 * returns levels eased by the largest ease used.  Measured with the retry: no
 * refusal on 2,400 instances of 8 seeds at ε = 2^-27 nor on 1,800 of 6 seeds at
 * 2^-30, none on the 25 with identical types.
 *
 * Normalisation.  The rows' coefficients are the same at every stage (only κ
 * and β change), so one power of two serves all stages: the centred call's,
 * which brings the largest coefficient on a type with workers into [1, 2)
 * (sw_lp_shift on the host).  Every coefficient is then below 2 and every
 * SW_IPM_RSC is 1.0, and an instance with a single stage is the program of
 * sw_mmf_allocate_types_centred operation for operation: the same bits.  The
 * levels are held normalised and scaled back at the end.
 *
 * The bottleneck test.  An unfrozen job can still rise while the others keep
 * the level exactly when its value row has slack somewhere on the level LP's
 * optimal face, which is the same as slack at the face's analytic centre.  The
 * path converges to a strictly complementary pair (Goldman–Tucker): of the
 * slack u_j and the dual y_j (SW_IPM_SU) of an unfrozen row exactly one has a
 * positive limit.  At the second path point itself the two do not separate: a
 * bottleneck whose dual is small (it is held by other jobs' rows) has
 * u_j = μ₂/y_j as large as a free job's small slack, and (u_j/t)/y_j was 0.52
 * for a bottleneck on one seed and 0.51 for a free job on another.  So both
 * are extrapolated to μ = 0 from the two path points (SW_IPM_U1, SW_IPM_SU1),
 * which takes the part linear in μ off, and the statistic is
 *     r_j = (u*_j / t) / y*_j     (0 if u* ≤ 0, SW_WFT_HUGE if y* ≤ 0).
 * Measured on the twin over 8 seeds of tests/wftcases.py's family (2,400
 * instances, m 2…24, n 2…4) against the per-job LPs of tests/wf_types_ref.py
 * (HiGHS; gain ≤ 1e-9 bottleneck, ≥ 1e-6 free; smallest free gain 1.1e-5): the
 * largest r_j of a bottleneck was 4.32e-5 (SW_WFT_GAP_LO), the smallest of a
 * free job 0.119 (SW_WFT_GAP_HI), both on seed 3; on the other seeds the ends
 * were ≤ 1.1e-5 and ≥ 79.  SW_WFT_THRESH = 2.3e-3 is the geometric middle.  The
 * same jobs froze in the same stages on all 2,400.  tests/test_wf_types.py
 * holds a seed that was not among the eight to these ends.  A stage whose ends
 * come within SW_WFT_NEAR_BY of the threshold sets the flag SW_WFT_NEAR.  The
 * family has m ≤ 24; beyond it the statistic is not validated.
 *
 * Limits.  Every stage must freeze at least one job, so there are at most m
 * stages; a stage that freezes none ends the call with SW_WFT_STALL (the
 * caller's SW_ERR_CAPACITY), not a loop.  A type with 0 workers gets shares of
 * exactly 0.0.  A job with no positive coefficient on a type that has workers
 * is the caller's SW_ERR_INVALID: its normalised throughput is undefined.
 *
 * result[4] = last level, Newton steps of all stages, stages, flags.
 */
#ifndef SW_WF_TYPES_H
#define SW_WF_TYPES_H

#include "sw_arith.h"
#include "sw_mmf_ipm.h"

/* Both ends of the measured gap (see above) and its geometric middle. */
#define SW_WFT_GAP_LO 4.4e-5
#define SW_WFT_GAP_HI 0.119
#ifndef SW_WFT_THRESH
#define SW_WFT_THRESH 2.3e-3
#endif
#define SW_WFT_NEAR_BY 10.0
#ifndef SW_WFT_EASE
#define SW_WFT_EASE 9.313225746154785e-10 /* 2^-30 */
#endif

#define SW_WFT_HUGE 1.7976931348623157e308
#define SW_WFT_ONE 1  /* flags: a single stage froze every job */
#define SW_WFT_COARSE 4 /* flags: a stage's solve broke down and was done again at a larger μ */
#define SW_WFT_NEAR 2 /* flags: a statistic came within SW_WFT_NEAR_BY of the threshold */

#define SW_WFT_STALL (-6) /* a stage froze no job */

/* Two more fields per job after the engine's: the stage the job froze in
 * (1-based; 0.0 while it is unfrozen) and its level F_j (normalised). */
#define SW_WFT_FROZE SW_IPM_NSCAL
#define SW_WFT_F (SW_IPM_NSCAL + 1)
#define SW_WFT_XE(J, k) SW_IPM_Q(J, SW_IPM_NSCAL + 2 + (k)) /* the shares of the last stage at the ease ε */
#define SW_WFT_FIELDS(n) (SW_IPM_FIELDS(n) + 2 + (n))

/* The state of a call that is not the engine's (LDS in the kernel). */
typedef struct {
    double level, lo, hi; /* the last stage's level; the stage's largest bottleneck and smallest free statistic */
    double ease;          /* ε, 2ε in the repeat of the last stage */
    double theta;         /* how far the shares go from x(ε) towards 2·x(ε) − x(2ε) */
    double wE[SW_IPM_MAX_TYPES]; /* the capacity rows' slack at x(ε) */
    double elast, emax;   /* the ease of the last stage's solve; the largest ease of the call */
    double coarse, clast; /* 1, or the multiple of SW_IPM_MU_1 at which a stage is solved again; the last stage's */
    int32_t shift, stage, left, iters, flags, status, last, rep, tries, pad;
} sw_wft_glob;

SW_HD void sw_wft_begin(sw_wft_glob* q, int32_t m, int32_t shift) {
    q->level = 0.0;
    q->lo = 0.0;
    q->hi = 0.0;
    q->ease = SW_WFT_EASE;
    q->elast = SW_WFT_EASE;
    q->emax = SW_WFT_EASE;
    q->tries = 0;
    q->coarse = 1.0;
    q->clast = 1.0;
    q->theta = 0.0;
    q->last = 0;
    q->rep = 0;
    q->shift = shift;
    q->stage = 0;
    q->left = m;
    q->iters = 0;
    q->flags = 0;
    q->status = 0;
}

SW_HD void sw_wft_job_begin(sw_ipm_job* J) {
    SW_IPM_Q(J, SW_WFT_FROZE) = 0.0;
    SW_IPM_Q(J, SW_WFT_F) = 0.0;
}

/* Whether another stage is needed.  Every stage that does not stall takes at
 * least one job out of `left`, so there are at most m. */
SW_HD int sw_wft_next(const sw_wft_glob* q) { return q->status == 0 && q->left > 0; }

/* After sw_ipm_setup of a stage (one thread): the path points of its solve. */
SW_HD void sw_wft_setup(sw_ipm_glob* g, const sw_wft_glob* q) { g->mu1 = SW_IPM_MU_1 * q->coarse; }

/* Whether the job's row is a frozen one in the solve at hand: in the repeat
 * the jobs of the last stage are unfrozen once more. */
SW_HD int sw_wft_frozen(const sw_wft_glob* q, const sw_ipm_job* J) {
    const double fz = SW_IPM_Q(J, SW_WFT_FROZE);
    return fz != 0.0 && !(q->rep == 1 && fz == (double)(q->stage + 1));
}

/* A stage's solve ended in SW_IPM_CAP or SW_IPM_BREAK (one thread).  Late
 * stages are degenerate by construction (the frozen rows leave an interior of
 * the ease's width only), and with identical types or many more types than
 * jobs the reduced system came out singular in rounding on 0.5–1.7 % of the
 * fuzz family's draws.  The stage is then solved again at eight times the
 * ease, at most SW_WFT_TRIES times; the lift is taken off at whatever ease was
 * used, and the levels returned are eased by the largest ease of the call, so
 * that the shares meet every row at them.  Returns 1: solve the stage again;
 * 2: it was the repeat, which is given up (the shares stay x(ε)); 0: the
 * call fails with the engine's status. */
#define SW_WFT_TRIES 2
SW_HD int sw_wft_retry(const sw_ipm_glob* g, sw_wft_glob* q) {
    q->iters = q->iters + g->iters;
    if (q->rep == 1) {
        q->rep = 3;
        q->left = 0;
        q->stage = q->stage + 1;
        return 2;
    }
    if (q->stage == 0 || q->tries >= SW_WFT_TRIES) { /* the first stage has no eased row */
        q->status = g->status;
        return 0;
    }
    q->tries = q->tries + 1;
    q->coarse = 8.0 * q->coarse;
    q->flags = q->flags | SW_WFT_COARSE;
    q->ease = 8.0 * q->ease;
    q->emax = sw_max(q->emax, q->ease);
    return 1;
}

/* Init pass 1 of a stage (in place of sw_ipm_job_load): the job's normalised
 * row, κ and β.  Sums: [0] sf, [1] whether the job has a value row; max: [0]
 * −(largest coefficient) of an unfrozen job, −DBL_MAX of a frozen one. */
SW_HD void sw_wft_job_load(const sw_ipm_glob* g, const sw_wft_glob* q, sw_ipm_job* J, const double* coef,
                           double* sums, double* maxes) {
    const int frozen = sw_wft_frozen(q, J);
    double mx = 0.0;
    for (int32_t k = 0; k < J->na; ++k) {
        const double c = sw_lp_scale(coef[g->act[k]], q->shift);
        SW_IPM_C(J, k) = c;
        mx = sw_max(mx, c);
    }
    SW_IPM_Q(J, SW_IPM_HASV) = mx > 0.0 ? 1.0 : 0.0;
    SW_IPM_Q(J, SW_IPM_KAP) = frozen ? 0.0 : 1.0;
    SW_IPM_Q(J, SW_IPM_RSC) = 1.0;
    SW_IPM_Q(J, SW_IPM_BET) = frozen ? SW_IPM_Q(J, SW_WFT_F) * (1.0 - q->ease) : 0.0;
    sums[0] = J->sf;
    sums[1] = mx > 0.0 ? 1.0 : 0.0;
    maxes[0] = frozen ? -1.7976931348623157e308 : -mx;
}

/* The job's term of the eased rows' lift (one more sum of the final pass):
 * y_j·β_j of a frozen job, at the engine's second path point. */
SW_HD double sw_wft_job_lift(const sw_ipm_job* J) {
    if (SW_IPM_Q(J, SW_IPM_KAP) != 0.0 || SW_IPM_Q(J, SW_IPM_HASV) == 0.0) return 0.0;
    {
        const double y2 = SW_IPM_Q(J, SW_IPM_SU);
        const double y = y2 + (y2 - SW_IPM_Q(J, SW_IPM_SU1)) / (SW_IPM_MU_RATIO - 1.0);
        return sw_max(y, 0.0) * SW_IPM_Q(J, SW_IPM_BET);
    }
}

/* After a stage's final pass (one thread): its steps, and its level less what
 * the eased rows lifted it by, eased in its turn. */
SW_HD void sw_wft_glob_level(const sw_ipm_glob* g, sw_wft_glob* q, double lift) {
    if (!q->rep) q->level = sw_ipm_level(g, 0) - q->ease / (1.0 - q->ease) * lift;
    q->iters = q->iters + g->iters;
}

/* The statistic of an unfrozen job at the engine's second path point. */
SW_HD double sw_wft_stat(const sw_ipm_glob* g, const sw_ipm_job* J) {
    const double u2 = SW_IPM_Q(J, SW_IPM_U), y2 = SW_IPM_Q(J, SW_IPM_SU);
    const double u = u2 + (u2 - SW_IPM_Q(J, SW_IPM_U1)) / (SW_IPM_MU_RATIO - 1.0);
    const double y = y2 + (y2 - SW_IPM_Q(J, SW_IPM_SU1)) / (SW_IPM_MU_RATIO - 1.0);
    if (!(u > 0.0)) return 0.0;
    if (!(y > 0.0)) return SW_WFT_HUGE;
    return u / g->t / y;
}

/* The classifying pass.  Sums: [0] 1.0 if the job froze in this stage; max:
 * [0] its statistic if it did, [1] −(its statistic) if it stays free. */
SW_HD void sw_wft_job_classify(const sw_ipm_glob* g, const sw_wft_glob* q, sw_ipm_job* J, double* sums,
                               double* maxes) {
    sums[0] = 0.0;
    maxes[0] = -1.7976931348623157e308;
    maxes[1] = -1.7976931348623157e308;
    if (SW_IPM_Q(J, SW_WFT_FROZE) != 0.0) return;
    {
        const double r = sw_wft_stat(g, J);
        if (r < SW_WFT_THRESH) {
            SW_IPM_Q(J, SW_WFT_FROZE) = (double)(q->stage + 1);
            SW_IPM_Q(J, SW_WFT_F) = q->level;
            sums[0] = 1.0;
            maxes[0] = r;
        } else {
            maxes[1] = -r;
        }
    }
}

/* After the classifying pass (one thread): `froze` jobs froze (an exact sum of
 * ones), the ends of the stage's statistics. */
SW_HD void sw_wft_feed(sw_wft_glob* q, double froze, const double* maxes) {
    const int32_t cnt = (int32_t)froze;
    q->lo = maxes[0];
    q->hi = -maxes[1];
    if (cnt <= 0) {
        q->status = SW_WFT_STALL;
        return;
    }
    if (maxes[0] * SW_WFT_NEAR_BY > SW_WFT_THRESH) q->flags = q->flags | SW_WFT_NEAR;
    if (cnt < q->left && -maxes[1] < SW_WFT_THRESH * SW_WFT_NEAR_BY) q->flags = q->flags | SW_WFT_NEAR;
    q->left = q->left - cnt;
    q->last = cnt;
    q->stage = q->stage + 1;
    q->elast = q->ease;
    q->ease = SW_WFT_EASE;
    q->tries = 0;
    q->clast = q->coarse;
    q->coarse = 1.0;
}

/* The repeat.  The shares of the last stage are those of the eased program,
 * off the centre of the true face by what the ease moves them: up to 380 times
 * ε on the fuzz family (2.8e-6 at ε = 2^-27).  That is linear in ε to first
 * order, so the last stage is solved once more at 2ε and the shares returned
 * are x(ε) + θ·(x(ε) − x(2ε)), θ = 1 unless a row of the program at the
 * returned levels would be violated on the way (x(ε) meets them all); θ is
 * then the ratio test's, as at the engine's own extrapolation.  Measured: the
 * worst share error fell from 2.8e-6 to 3.2e-7 at ε = 2^-27; at 2^-30 it is
 * 9.7e-8.  A repeat whose solve breaks down is given up (x(ε) is returned); it
 * runs at the path points the last stage's solve got through with.  Only with more than one
 * stage: a single stage has no eased row.
 *   sw_wft_repeat (one thread, after the last stage): whether to; then
 * sw_wft_job_keep on every job (sums: [k] sf·x_k(ε)) and sw_wft_glob_keep, the
 * stage again, sw_wft_job_blend on every job (sums: [k] sf·e_k, e = x(ε) −
 * x(2ε); max: [0] the job's ratio) and sw_wft_glob_blend. */
SW_HD int sw_wft_repeat(sw_wft_glob* q) {
    if (q->rep || q->status != 0 || q->left > 0 || q->stage < 2) return 0;
    q->rep = 1;
    q->ease = 2.0 * q->elast;
    q->coarse = q->clast; /* the path points the last stage's solve got through with */
    q->left = q->last;
    q->stage = q->stage - 1;
    return 1;
}
SW_HD void sw_wft_job_keep(const sw_ipm_glob* g, const sw_wft_glob* q, sw_ipm_job* J, double* sums) {
    double row[SW_IPM_MAX_TYPES];
    sw_ipm_job_emit(g, J, row);
    for (int32_t k = 0; k < J->na; ++k) {
        SW_WFT_XE(J, k) = row[g->act[k]];
        sums[k] = J->sf * row[g->act[k]];
    }
    (void)q;
}
SW_HD void sw_wft_glob_keep(const sw_ipm_glob* g, sw_wft_glob* q, const double* sums) {
    for (int32_t k = 0; k < g->na; ++k) q->wE[k] = g->Wk[k] - sums[k];
}
SW_HD void sw_wft_job_blend(const sw_ipm_glob* g, const sw_wft_glob* q, sw_ipm_job* J, double* sums,
                            double* maxes) {
    double row[SW_IPM_MAX_TYPES];
    double se = 0.0, sce = 0.0, sx = 0.0, scx = 0.0, r = 0.0;
    sw_ipm_job_emit(g, J, row);
    for (int32_t k = 0; k < J->na; ++k) {
        const double xe = SW_WFT_XE(J, k), e = xe - row[g->act[k]];
        sums[k] = J->sf * e;
        se = se + e;
        sce = sce + SW_IPM_C(J, k) * e;
        sx = sx + xe;
        scx = scx + SW_IPM_C(J, k) * xe;
        if (e < 0.0) r = sw_max(r, xe > 0.0 ? -e / xe : SW_WFT_HUGE);
    }
    if (se > 0.0) r = sw_max(r, 1.0 - sx > 0.0 ? se / (1.0 - sx) : SW_WFT_HUGE);
    if (sce < 0.0) {
        const double us = scx - SW_IPM_Q(J, SW_WFT_F) * (1.0 - q->emax);
        r = sw_max(r, us > 0.0 ? -sce / us : SW_WFT_HUGE);
    }
    maxes[0] = r;
}
SW_HD void sw_wft_glob_blend(const sw_ipm_glob* g, sw_wft_glob* q, const double* sums, const double* maxes) {
    double r = maxes[0];
    for (int32_t k = 0; k < g->na; ++k)
        if (sums[k] > 0.0) r = sw_max(r, q->wE[k] > 0.0 ? sums[k] / q->wE[k] : SW_WFT_HUGE);
    q->theta = r > 1.0 ? 1.0 / r : 1.0;
    q->rep = 2;
    q->left = 0;
    q->stage = q->stage + 1;
}

/* The job's row of the allocation. */
SW_HD void sw_wft_job_emit(const sw_ipm_glob* g, const sw_wft_glob* q, const sw_ipm_job* J, double* xrow) {
    sw_ipm_job_emit(g, J, xrow);
    if (q->rep < 2) return;
    for (int32_t k = 0; k < J->na; ++k) {
        const double xe = SW_WFT_XE(J, k);
        xrow[g->act[k]] = q->rep == 3 ? xe : sw_max(0.0, xe + q->theta * (xe - xrow[g->act[k]]));
    }
}

/* The job's final level, scaled back. */
SW_HD double sw_wft_job_level(const sw_wft_glob* q, const sw_ipm_job* J) {
    return sw_lp_scale(SW_IPM_Q(J, SW_WFT_F) * (1.0 - q->emax), -q->shift);
}

/* result[4] */
SW_HD void sw_wft_result(const sw_wft_glob* q, double* out) {
    out[0] = sw_lp_scale(q->level * (1.0 - q->emax), -q->shift);
    out[1] = (double)q->iters;
    out[2] = (double)q->stage;
    out[3] = (double)(q->flags | (q->stage == 1 && q->left == 0 ? SW_WFT_ONE : 0));
}

#endif /* SW_WF_TYPES_H */
