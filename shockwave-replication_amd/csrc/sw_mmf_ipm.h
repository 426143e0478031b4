/*
 * sw_mmf_ipm.h — the heterogeneity-aware MaxMinFairness LP over several worker
 * types (the LP of sw_mmf_lp.h) solved by a primal–dual interior-point method
 * that ends at the ANALYTIC CENTRE of the optimal face, the point the
 * reference's ECOS converges to.  Shared by the HIP kernel (sw_mmf_ipm.hip,
 * one workgroup per instance, the whole iteration in one launch) and the CPU
 * twin (tests/twins/mmfc_twin.c).  Only IEEE +, −, ×, ÷ and comparisons
 * (-ffp-contract=off on both sides), every sum over jobs through the
 * deterministic tree (sw_block.h detsum, tests/twins/twin_detsum.h), so the two
 * return the same bits.
 *
 * The result.  The level t* of
 *     maximise t   s.t.  t ≤ Σ_k coef[j][k]·x[j][k]      (m value rows)
 *                        Σ_j sf_j·x[j][k] ≤ workers[k]    (n capacity rows)
 *                        Σ_k x[j][k] ≤ 1                  (m time rows)
 *                        x ≥ 0, t ≥ 0
 * and the maximiser of Σ log(slack) over the optimal face, the sum taken over
 * every inequality (x ≥ 0 and t ≥ 0 included) that is not tight on the whole
 * face: the limit of the LP's central path.  For one type it is the point
 * sw_mmf_allocate computes in closed form (sw_mmf.h).
 *
 * Standard form.  A slack per row: u_j (value), w_k (capacity), v_j (time);
 * every variable z_i ≥ 0 has a dual s_i ≥ 0, and the row duals are held through
 * the slacks' (y = −s of the row's slack, so the slack columns' dual residuals
 * are identically zero).  A Newton step towards z_i·s_i = τ solves
 *     M·D·Mᵀ·dy = r_p − M·h,   D = diag(z/s),  h = (τ − z·s − z·r_d)/s.
 * Among the value and time rows M·D·Mᵀ has only the 2×2 diagonal blocks
 *     B_j = [a b; b e],  a = Σ c²d + d_u,  b = −Σ c·d,  e = Σ d + d_v
 * apart from the rank-one term of the t column, so dt is kept as an unknown,
 * each job's block is eliminated on its own, and what remains is the
 * (n+1)×(n+1) system over the capacity rows bordered by t:
 *     S·dy_C − q·dt = r,     (1/d_t + Σ_j e_j/det_j)·dt + qᵀ·dy_C = r_t.
 * S is symmetric positive definite: it is factorised as L·D·Lᵀ, dt follows from
 * the scalar Schur complement (τ_t + qᵀS⁻¹q > 0), and the per-job
 * back-substitution is again independent.
 *   The eliminated quantities are formed without cancellation where the
 * closed form allows it: det_j = Σ_{l<i} d_i·d_l·(c_i − c_l)² + d_u·e + d_v·Σc²d
 * (never a·e − b²), and a job's part of S_kk is sf²·d_k·det_j(without k)/det_j,
 * the determinant of the job's block with type k left out (never
 * d_k − d_k²·…).  Near the end d spans eighteen decades; the textbook forms
 * lose the centre there.  The price is O(n³) per job and step instead of
 * O(n²), n ≤ 16.
 *
 * The path.  One loop: the target is τ = max(σ·μ, μ_end), steps go the fraction
 * SW_IPM_BACK of the way to the boundary (primal and dual apart), and a point
 * of the path is reached when every product is at μ_end,
 * max_i |z_i·s_i/μ_end − 1| ≤ SW_IPM_DEV, with both residuals ≤ SW_IPM_RES.
 * Once σ·μ ≤ μ_end the steps are pure centring steps at μ_end: without them
 * the end point lies somewhere in the face, not at its centre.
 *   Two points are taken, at μ₁ = SW_IPM_MU_1·min(1, t) = 2e-8·min(1, t) (t the
 * level of the normalised program: the duals are of the objective's size, so μ
 * is measured against it; with μ₁ fixed at 2e-8 a level of 1e-6 of the largest
 * coefficient came out wrong by its own size) and μ₂ = μ₁/4, and the
 * result is their extrapolation to μ = 0 (the LP's central path is analytic
 * there: z(μ) = z* + a·μ + O(μ²)), under a ratio test that keeps every slack
 * non-negative (sw_ipm_job_final).  Stopping is by this criterion, not as far
 * as the arithmetic allows: the reduced system's condition grows as 1/μ² and
 * at μ = 1e-9 its L·D·Lᵀ broke down on degenerate vertices (one instance in
 * about 150), while a single point at μ = 1e-9 lay up to 2e-6 from the centre
 * (the distance is a·μ; a reached 2,000).  The extrapolated point lay within
 * 3.4e-9 on the same instances.  SW_IPM_MAX_ITERS caps the
 * steps (status −3).
 *
 * Degenerate inputs.  A type with no workers is left out of the program; its
 * shares are exactly 0.0.  If a job has no positive coefficient on a type that
 * has workers the level is exactly 0.0, t is pinned and that job's value row is
 * tight on the whole face: the program then has no objective, the central path
 * is a single point, and the same Newton steps at μ = 1 find it (has_t = 0;
 * such a job has no value row, its block B_j is the 1×1 time row).
 *
 * Normalisation as in sw_mmf_lp.h: the coefficients are multiplied by the
 * power of two that brings the largest one on a type with workers into [1, 2)
 * (sw_lp_shift, sw_lp_scale), the level is scaled back at the end.
 */
#ifndef SW_MMF_IPM_H
#define SW_MMF_IPM_H

#include "sw_arith.h"
#include "sw_mmf_lp.h"

#define SW_IPM_MAX_TYPES 16
#define SW_IPM_MAX_JOBS 16384
#define SW_IPM_MAX_ITERS 200
#define SW_IPM_SIGMA 0.2
#define SW_IPM_BACK 0.995
#ifndef SW_IPM_MU_1
#define SW_IPM_MU_1 2e-8
#endif
#ifndef SW_IPM_MU_RATIO
#define SW_IPM_MU_RATIO 4.0
#endif
#define SW_IPM_DEV 1e-8
#define SW_IPM_RES 1e-10
#define SW_IPM_FAR 16.0 /* μ above this multiple of μ₁: μ₁ still follows the level */
/* sums of one reduction: a row of the reduced system is at most n + 4 values */
#define SW_IPM_NRED (SW_IPM_MAX_TYPES + 4)
#define SW_IPM_NMAX 3

#define SW_IPM_OK 0
#define SW_IPM_CAP (-3)   /* SW_IPM_MAX_ITERS steps without reaching the criterion */
#define SW_IPM_BREAK (-4) /* a pivot of the reduced system was not positive */

/* The state that is not per job (LDS in the kernel). */
typedef struct {
    int32_t m, n, na, has_t, iters, status, done, stage, save, pad;
    int32_t act[SW_IPM_MAX_TYPES]; /* the types that have workers */
    double Wk[SW_IPM_MAX_TYPES], theta[SW_IPM_MAX_TYPES];
    double sfsum, nv, npairs, mu_end, scale;
    double t, st, dt, dst, t1;
    double w[SW_IPM_MAX_TYPES], sw[SW_IPM_MAX_TYPES], dw[SW_IPM_MAX_TYPES], dsw[SW_IPM_MAX_TYPES];
    double dwd[SW_IPM_MAX_TYPES], hw[SW_IPM_MAX_TYPES], rpc[SW_IPM_MAX_TYPES];
    double mu, target, rdt, ap, ad;
    double S[SW_IPM_MAX_TYPES * SW_IPM_MAX_TYPES]; /* lower triangle: S, then L and D in place */
    double q[SW_IPM_MAX_TYPES], r[SW_IPM_MAX_TYPES], a[SW_IPM_MAX_TYPES], b[SW_IPM_MAX_TYPES];
    double dyc[SW_IPM_MAX_TYPES], tau, rhst;
    double mu1; /* μ₁ of the normalised program at level 1: SW_IPM_MU_1; sw_wf_types.h raises it for a stage it solves again */
} sw_ipm_glob;

/* The per-job workspace, structure of arrays: field f of job j at
 * ws[f·stride + j].  Fields: c, x, s, dx, ds, d, h per active type, then the
 * scalars below: 8·na + SW_IPM_NSCAL doubles per job.
 *   SW_IPM_KAP is κ_j, the coefficient of t in the job's value row
 * (κ_j·t ≤ Σ_k c·x): 1.0 for every job of the MaxMinFairness program, so that
 * each product with it is exact and that program's bits are what they were
 * before κ existed; 0.0 for a row that does not bound the level (a job without
 * remaining steps in sw_mtd_types.h).  SW_IPM_RSC is the power of two by which
 * the residuals of the job's value row and of its shares' dual equations are
 * multiplied before they are held against SW_IPM_RES: 1.0 here, where every
 * coefficient is below 2; 1/(the row's largest coefficient) where rows are
 * larger (sw_mtd_types.h), whose residuals' rounding grows with it.  With has_t = 0, g->t is a constant of
 * the rows: 0.0 here, the fixed level of sw_mtd_types.h's second phase.
 *   SW_IPM_BET is β_j, the constant of the job's value row
 * (κ_j·t + β_j ≤ Σ_k c·x): 0.0 for every program but the staged one of
 * sw_wf_types.h, so that each operation with it is exact and those programs'
 * bits are what they were before β existed; there a job frozen at the level
 * F_j has κ = 0 and β = F_j.  It enters the start (sw_ipm_job_start2) and the
 * primal residual (sw_ipm_rpv) and nothing else: a constant drops out of every
 * difference.
 *   The start x = θ need not meet such a row, so its slack starts at
 * max(Σ c·θ − κ·t − β, ½·Σ c·θ) and the row's residual is worked off by the
 * steps like any other; with β = 0 the first is never the smaller
 * (t ≤ ½·Σ c·θ), so nothing changes there.
 *   SW_IPM_SU1 and SW_IPM_U1 keep the value row's dual and slack at the first
 * path point, as X1 keeps the shares: sw_wf_types.h extrapolates both. */
enum { SW_IPM_U, SW_IPM_SU, SW_IPM_V, SW_IPM_SV, SW_IPM_DU, SW_IPM_DSU, SW_IPM_DV, SW_IPM_DSV,
       SW_IPM_DDU, SW_IPM_DDV, SW_IPM_HU, SW_IPM_HV, SW_IPM_RHOV, SW_IPM_RHOT, SW_IPM_DET, SW_IPM_HASV,
       SW_IPM_KAP, SW_IPM_RSC, SW_IPM_BET, SW_IPM_SU1, SW_IPM_U1, SW_IPM_NSCAL };
#define SW_IPM_FIELDS(n) (8 * (n) + SW_IPM_NSCAL)

typedef struct {
    double* ws;
    int64_t stride;
    int32_t j, na;
    double sf;
} sw_ipm_job;

#define SW_IPM_AT(J, f) ((J)->ws[(int64_t)(f) * (J)->stride + (J)->j])
#define SW_IPM_C(J, k) SW_IPM_AT(J, (k))
#define SW_IPM_X(J, k) SW_IPM_AT(J, (J)->na + (k))
#define SW_IPM_S(J, k) SW_IPM_AT(J, 2 * (J)->na + (k))
#define SW_IPM_DX(J, k) SW_IPM_AT(J, 3 * (J)->na + (k))
#define SW_IPM_DS(J, k) SW_IPM_AT(J, 4 * (J)->na + (k))
#define SW_IPM_D(J, k) SW_IPM_AT(J, 5 * (J)->na + (k))
#define SW_IPM_H(J, k) SW_IPM_AT(J, 6 * (J)->na + (k))
#define SW_IPM_X1(J, k) SW_IPM_AT(J, 7 * (J)->na + (k))
#define SW_IPM_Q(J, f) SW_IPM_AT(J, 8 * (J)->na + (f))

SW_HD double sw_ipm_abs(double x) { return x < 0.0 ? -x : x; }

/* The types that have workers (one thread). */
SW_HD void sw_ipm_setup(sw_ipm_glob* g, int32_t m, int32_t n, const int32_t* workers) {
    g->m = m;
    g->n = n;
    g->na = 0;
    g->iters = 0;
    g->status = SW_IPM_OK;
    g->done = 0;
    g->stage = 0;
    g->save = 0;
    g->mu1 = SW_IPM_MU_1;
    for (int32_t k = 0; k < n; ++k)
        if (workers[k] > 0) {
            g->act[g->na] = k;
            g->Wk[g->na] = (double)workers[k];
            g->na = g->na + 1;
        }
}

/* The largest coefficient of job row `coef` on a type with workers. */
SW_HD double sw_ipm_rowmax(const sw_ipm_glob* g, const double* coef) {
    double mx = 0.0;
    for (int32_t k = 0; k < g->na; ++k) mx = sw_max(mx, coef[g->act[k]]);
    return mx;
}

/* Init pass 1: the job's normalised coefficients into the workspace.  Sums:
 * [0] sf, [1] whether the job has a value row; max: [0] −(largest coefficient). */
SW_HD void sw_ipm_job_load(const sw_ipm_glob* g, sw_ipm_job* J, const double* coef, int32_t shift, double* sums,
                           double* maxes) {
    double mx = 0.0;
    for (int32_t k = 0; k < J->na; ++k) {
        const double c = sw_lp_scale(coef[g->act[k]], shift);
        SW_IPM_C(J, k) = c;
        mx = sw_max(mx, c);
    }
    SW_IPM_Q(J, SW_IPM_HASV) = mx > 0.0 ? 1.0 : 0.0;
    SW_IPM_Q(J, SW_IPM_KAP) = 1.0;
    SW_IPM_Q(J, SW_IPM_RSC) = 1.0;
    SW_IPM_Q(J, SW_IPM_BET) = 0.0;
    sums[0] = J->sf;
    sums[1] = mx > 0.0 ? 1.0 : 0.0;
    maxes[0] = -mx;
}

/* After pass 1 (one thread): whether t is a variable, the start shares θ_k. */
SW_HD void sw_ipm_glob_load(sw_ipm_glob* g, const double* sums, const double* maxes) {
    g->sfsum = sums[0];
    g->nv = sums[1];
    g->has_t = -maxes[0] > 0.0 ? 1 : 0;
    g->mu_end = g->has_t ? g->mu1 : 1.0;
    g->scale = 1.0;
    g->npairs = (double)g->m * (double)g->na + g->nv + (double)g->m + (double)g->na + (double)g->has_t;
    for (int32_t k = 0; k < g->na; ++k)
        g->theta[k] = sw_min(1.0 / (double)(2 * g->na), g->Wk[k] / (2.0 * g->sfsum));
}

/* Init pass 2: x = θ; max: [0] −(the job's value Σ c·x), −∞-free: a job without
 * a value row, or whose row does not hold t (κ = 0), gives −DBL_MAX so that it
 * never sets the minimum. */
SW_HD void sw_ipm_job_start(const sw_ipm_glob* g, sw_ipm_job* J, double* maxes) {
    double val = 0.0;
    for (int32_t k = 0; k < J->na; ++k) {
        SW_IPM_X(J, k) = g->theta[k];
        val = val + SW_IPM_C(J, k) * g->theta[k];
    }
    SW_IPM_Q(J, SW_IPM_U) = val;
    maxes[0] = SW_IPM_Q(J, SW_IPM_HASV) != 0.0 && SW_IPM_Q(J, SW_IPM_KAP) != 0.0 ? -val : -1.7976931348623157e308;
}

SW_HD void sw_ipm_glob_start(sw_ipm_glob* g, const double* maxes) {
    g->t = g->has_t ? 0.5 * -maxes[0] : 0.0;
    g->st = g->has_t ? 1.0 : 0.0;
    g->dt = 0.0;
    g->dst = 0.0;
    for (int32_t k = 0; k < g->na; ++k) {
        g->w[k] = g->Wk[k] - g->theta[k] * g->sfsum;
        g->sw[k] = 1.0;
    }
}

/* Init pass 3: the slacks and a dual-feasible start. */
SW_HD void sw_ipm_job_start2(const sw_ipm_glob* g, sw_ipm_job* J) {
    const int hasv = SW_IPM_Q(J, SW_IPM_HASV) != 0.0;
    const double su = !hasv ? 0.0 : (g->has_t ? 2.0 / (double)g->m : 1.0);
    double sx = 0.0, mx = 0.0;
    for (int32_t k = 0; k < J->na; ++k) {
        sx = sx + SW_IPM_X(J, k);
        mx = sw_max(mx, SW_IPM_C(J, k));
    }
    const double sv = 1.0 + mx * su;
    {
        const double val = SW_IPM_Q(J, SW_IPM_U);
        const double u = val - SW_IPM_Q(J, SW_IPM_KAP) * g->t - SW_IPM_Q(J, SW_IPM_BET);
        SW_IPM_Q(J, SW_IPM_U) = hasv ? sw_max(u, 0.5 * val) : 0.0;
    }
    SW_IPM_Q(J, SW_IPM_SU) = su;
    SW_IPM_Q(J, SW_IPM_V) = 1.0 - sx;
    SW_IPM_Q(J, SW_IPM_SV) = sv;
    for (int32_t k = 0; k < J->na; ++k) SW_IPM_S(J, k) = sv + J->sf * g->sw[k] - SW_IPM_C(J, k) * su;
}

/* the job's primal residuals and the dual residual of x[j][k] */
SW_HD double sw_ipm_rpv(const sw_ipm_glob* g, const sw_ipm_job* J) {
    double val = 0.0;
    if (SW_IPM_Q(J, SW_IPM_HASV) == 0.0) return 0.0;
    for (int32_t k = 0; k < J->na; ++k) val = val + SW_IPM_C(J, k) * SW_IPM_X(J, k);
    return val - SW_IPM_Q(J, SW_IPM_KAP) * g->t - SW_IPM_Q(J, SW_IPM_BET) - SW_IPM_Q(J, SW_IPM_U);
}
SW_HD double sw_ipm_rpt(const sw_ipm_job* J) {
    double sx = 0.0;
    for (int32_t k = 0; k < J->na; ++k) sx = sx + SW_IPM_X(J, k);
    return 1.0 - sx - SW_IPM_Q(J, SW_IPM_V);
}
SW_HD double sw_ipm_rd(const sw_ipm_glob* g, const sw_ipm_job* J, int32_t k) {
    return SW_IPM_Q(J, SW_IPM_SV) + J->sf * g->sw[k] - SW_IPM_C(J, k) * SW_IPM_Q(J, SW_IPM_SU) - SW_IPM_S(J, k);
}

/* Pass A.  Sums: [k] sf·x_k (k < na), [na] Σ z·s of the job, [na+1] κ·s_u.
 * Maxes: [0] primal residual, [1] dual residual, [2] |z·s/μ_end − 1|. */
SW_HD void sw_ipm_job_resid(const sw_ipm_glob* g, const sw_ipm_job* J, double* sums, double* maxes) {
    const int hasv = SW_IPM_Q(J, SW_IPM_HASV) != 0.0;
    const double ime = 1.0 / g->mu_end;
    double comp = 0.0, dinf = 0.0, dev = 0.0;
    for (int32_t k = 0; k < J->na; ++k) {
        const double p = SW_IPM_X(J, k) * SW_IPM_S(J, k);
        sums[k] = J->sf * SW_IPM_X(J, k);
        comp = comp + p;
        dev = sw_max(dev, sw_ipm_abs(p * ime - 1.0));
        dinf = sw_max(dinf, sw_ipm_abs(sw_ipm_rd(g, J, k)) * SW_IPM_Q(J, SW_IPM_RSC));
    }
    {
        const double p = SW_IPM_Q(J, SW_IPM_V) * SW_IPM_Q(J, SW_IPM_SV);
        comp = comp + p;
        dev = sw_max(dev, sw_ipm_abs(p * ime - 1.0));
    }
    if (hasv) {
        const double p = SW_IPM_Q(J, SW_IPM_U) * SW_IPM_Q(J, SW_IPM_SU);
        comp = comp + p;
        dev = sw_max(dev, sw_ipm_abs(p * ime - 1.0));
    }
    sums[J->na] = comp;
    sums[J->na + 1] = SW_IPM_Q(J, SW_IPM_KAP) * SW_IPM_Q(J, SW_IPM_SU);
    maxes[0] = sw_max(sw_ipm_abs(sw_ipm_rpv(g, J)) * SW_IPM_Q(J, SW_IPM_RSC), sw_ipm_abs(sw_ipm_rpt(J)));
    maxes[1] = dinf;
    maxes[2] = dev;
}

/* After pass A (one thread): μ, the residuals, the stop, the target. */
SW_HD void sw_ipm_glob_resid(sw_ipm_glob* g, const double* sums, const double* maxes) {
    const int32_t na = g->na;
    const double ime = 1.0 / g->mu_end;
    double comp = sums[na], pinf = maxes[0], dinf = maxes[1], dev = maxes[2];
    for (int32_t k = 0; k < na; ++k) {
        const double p = g->w[k] * g->sw[k];
        g->rpc[k] = g->Wk[k] - sums[k] - g->w[k];
        pinf = sw_max(pinf, sw_ipm_abs(g->rpc[k]));
        comp = comp + p;
        dev = sw_max(dev, sw_ipm_abs(p * ime - 1.0));
    }
    g->rdt = 0.0;
    if (g->has_t) {
        const double p = g->t * g->st;
        g->rdt = sums[na + 1] - 1.0 - g->st;
        dinf = sw_max(dinf, sw_ipm_abs(g->rdt));
        comp = comp + p;
        dev = sw_max(dev, sw_ipm_abs(p * ime - 1.0));
    }
    g->mu = comp / g->npairs;
    /* The objective's own scale.  The coefficients are normalised to [1, 2), the
     * level is not: with t far below 1 the duals are of its size, and μ₁ has to
     * be too (the path of max α·t at μ is that of max t at μ/α).  While the path
     * is still far from its first point, μ₁ follows min(1, t); then it is kept. */
    if (g->has_t && g->stage == 0 && g->mu > SW_IPM_FAR * g->mu_end) {
        g->scale = sw_min(1.0, g->t);
        g->mu_end = g->mu1 * g->scale;
    }
    if (dev <= SW_IPM_DEV && pinf <= SW_IPM_RES && dinf <= SW_IPM_RES * g->scale) {
        if (!g->has_t || g->stage == 1) {
            g->done = 1;
            return;
        }
        /* the first point of the path is reached: keep it (pass B), go on to the second */
        g->stage = 1;
        g->save = 1;
        g->t1 = g->t;
        g->mu_end = g->mu1 * g->scale / SW_IPM_MU_RATIO;
    }
    if (g->iters >= SW_IPM_MAX_ITERS) {
        g->status = SW_IPM_CAP;
        g->done = 1;
        return;
    }
    g->target = g->has_t ? sw_max(SW_IPM_SIGMA * g->mu, g->mu_end) : g->mu_end;
    for (int32_t k = 0; k < na; ++k) {
        g->dwd[k] = g->w[k] / g->sw[k];
        g->hw[k] = g->target / g->sw[k] - g->w[k];
    }
}

/* The determinant of the job's block over the types other than `skip` (−1:
 * all of them), every term positive.  Without a value row: the 1×1 time block. */
SW_HD double sw_ipm_det(const sw_ipm_job* J, int32_t skip) {
    const double du = SW_IPM_Q(J, SW_IPM_DDU), dv = SW_IPM_Q(J, SW_IPM_DDV);
    double sd = 0.0, scd = 0.0, pr = 0.0;
    for (int32_t i = 0; i < J->na; ++i) {
        if (i == skip) continue;
        const double di = SW_IPM_D(J, i), ci = SW_IPM_C(J, i);
        sd = sd + di;
        scd = scd + ci * ci * di;
        for (int32_t l = 0; l < i; ++l) {
            if (l == skip) continue;
            const double dc = ci - SW_IPM_C(J, l);
            pr = pr + di * SW_IPM_D(J, l) * (dc * dc);
        }
    }
    if (SW_IPM_Q(J, SW_IPM_HASV) == 0.0) return sd + dv;
    return pr + du * (sd + dv) + dv * scd;
}

/* Pass B: the scalings, the right-hand sides and the block's determinant. */
SW_HD void sw_ipm_job_prep(const sw_ipm_glob* g, sw_ipm_job* J) {
    const int hasv = SW_IPM_Q(J, SW_IPM_HASV) != 0.0;
    const double tg = g->target;
    double sch = 0.0, sh = 0.0;
    for (int32_t k = 0; k < J->na; ++k) {
        const double x = SW_IPM_X(J, k), s = SW_IPM_S(J, k), d = x / s;
        if (g->save) SW_IPM_X1(J, k) = x;
        const double h = tg / s - x - d * sw_ipm_rd(g, J, k);
        SW_IPM_D(J, k) = d;
        SW_IPM_H(J, k) = h;
        sch = sch + SW_IPM_C(J, k) * h;
        sh = sh + h;
    }
    {
        const double v = SW_IPM_Q(J, SW_IPM_V), sv = SW_IPM_Q(J, SW_IPM_SV), hv = tg / sv - v;
        SW_IPM_Q(J, SW_IPM_DDV) = v / sv;
        SW_IPM_Q(J, SW_IPM_HV) = hv;
        SW_IPM_Q(J, SW_IPM_RHOT) = sw_ipm_rpt(J) - sh - hv;
    }
    if (hasv) {
        const double u = SW_IPM_Q(J, SW_IPM_U), su = SW_IPM_Q(J, SW_IPM_SU), hu = tg / su - u;
        if (g->save) {
            SW_IPM_Q(J, SW_IPM_SU1) = su;
            SW_IPM_Q(J, SW_IPM_U1) = u;
        }
        SW_IPM_Q(J, SW_IPM_DDU) = u / su;
        SW_IPM_Q(J, SW_IPM_HU) = hu;
        /* row: κ·t − Σ c·x + u = 0, so r_p = Σ c·x − κ·t − u */
        SW_IPM_Q(J, SW_IPM_RHOV) = sw_ipm_rpv(g, J) + sch - hu;
    } else {
        SW_IPM_Q(J, SW_IPM_DDU) = 0.0;
        SW_IPM_Q(J, SW_IPM_HU) = 0.0;
        SW_IPM_Q(J, SW_IPM_RHOV) = 0.0;
    }
    SW_IPM_Q(J, SW_IPM_DET) = sw_ipm_det(J, -1);
}

/* What the values of row k share: B⁻¹·E_k = sf·d_k·(α, β)/det. */
typedef struct {
    double alpha, beta, e, b, det, dk, ck, kap;
    int32_t k, hasv;
} sw_ipm_rowctx;

SW_HD sw_ipm_rowctx sw_ipm_row_begin(const sw_ipm_job* J, int32_t k) {
    sw_ipm_rowctx r;
    r.k = k;
    r.hasv = SW_IPM_Q(J, SW_IPM_HASV) != 0.0;
    r.det = SW_IPM_Q(J, SW_IPM_DET);
    r.dk = SW_IPM_D(J, k);
    r.ck = SW_IPM_C(J, k);
    r.kap = SW_IPM_Q(J, SW_IPM_KAP);
    double sd = 0.0, scd = 0.0, al = 0.0, be = 0.0;
    for (int32_t i = 0; i < J->na; ++i) {
        const double di = SW_IPM_D(J, i), ci = SW_IPM_C(J, i);
        sd = sd + di;
        scd = scd + ci * di;
        al = al + di * (ci - r.ck);
        be = be + di * ci * (ci - r.ck);
    }
    r.e = sd + SW_IPM_Q(J, SW_IPM_DDV);
    r.b = -scd;
    r.alpha = r.hasv ? al - r.ck * SW_IPM_Q(J, SW_IPM_DDV) : 0.0;
    r.beta = r.hasv ? be + SW_IPM_Q(J, SW_IPM_DDU) : 1.0;
    return r;
}

/* γ_kl = (−c_k, 1)·adj(B)·(−c_l, 1)ᵀ = Σ_a d_a·(c_a − c_k)·(c_a − c_l) + c_k·c_l·d_v + d_u
 * (1 without a value row): d_k·d_l·γ_kl/det is the job's part of −S_kl. */
SW_HD double sw_ipm_gamma(const sw_ipm_job* J, const sw_ipm_rowctx* r, int32_t l) {
    const double cl = SW_IPM_C(J, l);
    double gm = 0.0;
    if (!r->hasv) return 1.0;
    for (int32_t a = 0; a < J->na; ++a) {
        const double ca = SW_IPM_C(J, a);
        gm = gm + SW_IPM_D(J, a) * ((ca - r->ck) * (ca - cl));
    }
    return gm + r->ck * cl * SW_IPM_Q(J, SW_IPM_DDV) + SW_IPM_Q(J, SW_IPM_DDU);
}

/* how many sums row k reduces: S_kk … S_k,na−1, q_k, r_k, and with row 0 the
 * t row's two */
SW_HD int32_t sw_ipm_row_count(int32_t na, int32_t k, int32_t has_t) {
    return na - k + 2 + (k == 0 && has_t ? 2 : 0);
}

/* Pass R_k: the job's part of value i of row k. */
SW_HD double sw_ipm_row_val(const sw_ipm_job* J, const sw_ipm_rowctx* r, int32_t i) {
    const int32_t na = J->na, k = r->k;
    const double sf = J->sf;
    if (i == 0) return sf * sf * r->dk * sw_ipm_det(J, k) / r->det;
    if (i < na - k) /* −S_kl, l = k + i */
        return sf * sf * r->dk * SW_IPM_D(J, k + i) * sw_ipm_gamma(J, r, k + i) / r->det;
    if (i == na - k) return r->hasv ? r->kap * (sf * r->dk * r->alpha / r->det) : 0.0;
    if (i == na - k + 1)
        return sf * SW_IPM_H(J, k) +
               sf * r->dk * (SW_IPM_Q(J, SW_IPM_RHOV) * r->alpha + SW_IPM_Q(J, SW_IPM_RHOT) * r->beta) / r->det;
    if (!r->hasv) return 0.0;
    if (i == na - k + 2) return r->kap * r->kap * (r->e / r->det);
    return r->kap * ((r->e * SW_IPM_Q(J, SW_IPM_RHOV) - r->b * SW_IPM_Q(J, SW_IPM_RHOT)) / r->det);
}

/* After pass R_k (one thread): row k of the reduced system. */
SW_HD void sw_ipm_glob_row(sw_ipm_glob* g, int32_t k, const double* sums) {
    const int32_t na = g->na;
    g->S[k * SW_IPM_MAX_TYPES + k] = g->dwd[k] + sums[0];
    for (int32_t i = 1; i < na - k; ++i) g->S[(k + i) * SW_IPM_MAX_TYPES + k] = -sums[i];
    g->q[k] = sums[na - k];
    g->r[k] = g->rpc[k] - g->hw[k] - sums[na - k + 1];
    if (k == 0) {
        g->tau = 0.0;
        g->rhst = 0.0;
        if (g->has_t) {
            g->tau = g->st / g->t + sums[na + 2];
            g->rhst = g->target / g->t - g->st - g->rdt + sums[na + 3];
        }
    }
}

/* S·y = v by the factors in g->S (unit lower L below the diagonal, D on it) */
SW_HD void sw_ipm_ldl_solve(const sw_ipm_glob* g, const double* v, double* y) {
    const int32_t na = g->na;
    for (int32_t i = 0; i < na; ++i) {
        double s = v[i];
        for (int32_t l = 0; l < i; ++l) s = s - g->S[i * SW_IPM_MAX_TYPES + l] * y[l];
        y[i] = s;
    }
    for (int32_t i = 0; i < na; ++i) y[i] = y[i] / g->S[i * SW_IPM_MAX_TYPES + i];
    for (int32_t i = na - 1; i >= 0; --i) {
        double s = y[i];
        for (int32_t l = i + 1; l < na; ++l) s = s - g->S[l * SW_IPM_MAX_TYPES + i] * y[l];
        y[i] = s;
    }
}

/* The reduced system (one thread): L·D·Lᵀ of S, then dt and dy_C, and the
 * steps of t and of the capacity slacks. */
SW_HD void sw_ipm_glob_solve(sw_ipm_glob* g) {
    const int32_t na = g->na, ld = SW_IPM_MAX_TYPES;
    for (int32_t c = 0; c < na; ++c) {
        double dg = g->S[c * ld + c];
        for (int32_t l = 0; l < c; ++l) dg = dg - g->S[c * ld + l] * g->S[c * ld + l] * g->S[l * ld + l];
        if (!(dg > 0.0)) {
            g->status = SW_IPM_BREAK;
            g->done = 1;
            return;
        }
        g->S[c * ld + c] = dg;
        for (int32_t i = c + 1; i < na; ++i) {
            double s = g->S[i * ld + c];
            for (int32_t l = 0; l < c; ++l) s = s - g->S[i * ld + l] * g->S[c * ld + l] * g->S[l * ld + l];
            g->S[i * ld + c] = s / dg;
        }
    }
    sw_ipm_ldl_solve(g, g->r, g->b);
    g->dt = 0.0;
    g->dst = 0.0;
    if (g->has_t) {
        double qa = 0.0, qb = 0.0;
        sw_ipm_ldl_solve(g, g->q, g->a);
        for (int32_t k = 0; k < na; ++k) {
            qa = qa + g->q[k] * g->a[k];
            qb = qb + g->q[k] * g->b[k];
        }
        g->dt = (g->rhst - qb) / (g->tau + qa);
        g->dst = (g->target - g->st * g->dt) / g->t - g->st;
    }
    for (int32_t k = 0; k < na; ++k) {
        g->dyc[k] = g->has_t ? g->b[k] + g->a[k] * g->dt : g->b[k];
        g->dw[k] = g->dwd[k] * g->dyc[k] + g->hw[k];
        g->dsw[k] = -g->dyc[k];
    }
}

/* Pass C: the job's step.  Maxes: [0] the largest −dz/z of its primal
 * variables, [1] the largest −ds/s of its duals.
 *   With y_k = sf·dy_C[k] and (ρ_V − dt, ρ_T) the block's right-hand side, the
 * step is written in the quantities of the rows above, never through
 * B⁻¹·(right-hand side with the d·y terms folded in):
 *     Mᵀdy at x_k = [ (ρ_V − dt)·α_k + ρ_T·β_k + y_k·det(without k) − Σ_{l≠k} y_l·d_l·γ_kl ] / det
 *     dy_V = [ Σ_k d_k·((ρ_V − dt) + c_k·ρ_T) + d_v·(ρ_V − dt) − Σ_k y_k·d_k·α_k ] / det
 *     dy_T = [ Σ_k d_k·c_k·((ρ_V − dt) + c_k·ρ_T) + d_u·ρ_T − Σ_k y_k·d_k·β_k ] / det
 * A variable far from its bound has d of 1/μ; folded in, the d·y terms of two
 * such variables cancel to an absolute error of d·ε in the step, here the error
 * stays relative to dy, which vanishes as the centring steps converge. */
SW_HD void sw_ipm_job_back(const sw_ipm_glob* g, sw_ipm_job* J, double* maxes) {
    const int hasv = SW_IPM_Q(J, SW_IPM_HASV) != 0.0;
    const double sf = J->sf, det = SW_IPM_Q(J, SW_IPM_DET);
    const double rv = SW_IPM_Q(J, SW_IPM_RHOV) - SW_IPM_Q(J, SW_IPM_KAP) * g->dt, rt = SW_IPM_Q(J, SW_IPM_RHOT);
    const double ddu = SW_IPM_Q(J, SW_IPM_DDU), ddv = SW_IPM_Q(J, SW_IPM_DDV);
    double nv = ddv * rv, nt = hasv ? ddu * rt : rt;
    double rp = 0.0, rd = 0.0;
    for (int32_t k = 0; k < J->na; ++k) {
        const sw_ipm_rowctx r = sw_ipm_row_begin(J, k);
        const double yk = sf * g->dyc[k];
        double num = rv * r.alpha + rt * r.beta + yk * sw_ipm_det(J, k);
        for (int32_t l = 0; l < J->na; ++l)
            if (l != k) num = num - sf * g->dyc[l] * SW_IPM_D(J, l) * sw_ipm_gamma(J, &r, l);
        {
            const double aty = num / det;
            const double dx = r.dk * aty + SW_IPM_H(J, k);
            const double ds = sw_ipm_rd(g, J, k) - aty;
            SW_IPM_DX(J, k) = dx;
            SW_IPM_DS(J, k) = ds;
            rp = sw_max(rp, -dx / SW_IPM_X(J, k));
            rd = sw_max(rd, -ds / SW_IPM_S(J, k));
        }
        if (hasv) {
            nv = nv + r.dk * (rv + r.ck * rt) - yk * r.dk * r.alpha;
            nt = nt + r.dk * r.ck * (rv + r.ck * rt) - yk * r.dk * r.beta;
        } else {
            nt = nt - yk * r.dk;
        }
    }
    {
        const double dyt = nt / det;
        const double dv = ddv * dyt + SW_IPM_Q(J, SW_IPM_HV);
        SW_IPM_Q(J, SW_IPM_DV) = dv;
        SW_IPM_Q(J, SW_IPM_DSV) = -dyt;
        rp = sw_max(rp, -dv / SW_IPM_Q(J, SW_IPM_V));
        rd = sw_max(rd, dyt / SW_IPM_Q(J, SW_IPM_SV));
    }
    if (hasv) {
        const double dyv = nv / det;
        const double du = ddu * dyv + SW_IPM_Q(J, SW_IPM_HU);
        SW_IPM_Q(J, SW_IPM_DU) = du;
        SW_IPM_Q(J, SW_IPM_DSU) = -dyv;
        rp = sw_max(rp, -du / SW_IPM_Q(J, SW_IPM_U));
        rd = sw_max(rd, dyv / SW_IPM_Q(J, SW_IPM_SU));
    }
    maxes[0] = rp;
    maxes[1] = rd;
}

/* After pass C (one thread): the step lengths, t and the capacity slacks moved. */
SW_HD void sw_ipm_glob_step(sw_ipm_glob* g, const double* maxes) {
    double rp = maxes[0], rd = maxes[1];
    for (int32_t k = 0; k < g->na; ++k) {
        rp = sw_max(rp, -g->dw[k] / g->w[k]);
        rd = sw_max(rd, -g->dsw[k] / g->sw[k]);
    }
    if (g->has_t) {
        rp = sw_max(rp, -g->dt / g->t);
        rd = sw_max(rd, -g->dst / g->st);
    }
    g->ap = rp * 1.0 > SW_IPM_BACK ? SW_IPM_BACK / rp : 1.0;
    g->ad = rd * 1.0 > SW_IPM_BACK ? SW_IPM_BACK / rd : 1.0;
    for (int32_t k = 0; k < g->na; ++k) {
        g->w[k] = g->w[k] + g->ap * g->dw[k];
        g->sw[k] = g->sw[k] + g->ad * g->dsw[k];
    }
    if (g->has_t) {
        g->t = g->t + g->ap * g->dt;
        g->st = g->st + g->ad * g->dst;
    }
    g->iters = g->iters + 1;
    g->save = 0;
}

/* Pass D: the job moved. */
SW_HD void sw_ipm_job_step(const sw_ipm_glob* g, sw_ipm_job* J) {
    for (int32_t k = 0; k < J->na; ++k) {
        SW_IPM_X(J, k) = SW_IPM_X(J, k) + g->ap * SW_IPM_DX(J, k);
        SW_IPM_S(J, k) = SW_IPM_S(J, k) + g->ad * SW_IPM_DS(J, k);
    }
    SW_IPM_Q(J, SW_IPM_V) = SW_IPM_Q(J, SW_IPM_V) + g->ap * SW_IPM_Q(J, SW_IPM_DV);
    SW_IPM_Q(J, SW_IPM_SV) = SW_IPM_Q(J, SW_IPM_SV) + g->ad * SW_IPM_Q(J, SW_IPM_DSV);
    if (SW_IPM_Q(J, SW_IPM_HASV) != 0.0) {
        SW_IPM_Q(J, SW_IPM_U) = SW_IPM_Q(J, SW_IPM_U) + g->ap * SW_IPM_Q(J, SW_IPM_DU);
        SW_IPM_Q(J, SW_IPM_SU) = SW_IPM_Q(J, SW_IPM_SU) + g->ad * SW_IPM_Q(J, SW_IPM_DSU);
    }
}

/* The end: the two points of the path, z1 at μ₁ and z2 at μ₂ = μ₁/R, are
 * extrapolated to μ = 0, z* = z2 + θ·e with e = (z2 − z1)/(R − 1) and θ = 1
 * unless a slack would turn negative on the way (the path's curvature can
 * leave z* beyond a tight constraint by O(μ²)); θ is then the ratio test's.
 * Final pass.  Sums: [k] sf·e_k (k < na); max: [0] the largest −e/z2 over the
 * job's shares and its two rows' slacks. */
SW_HD double sw_ipm_ext(const sw_ipm_job* J, int32_t k) {
    return (SW_IPM_X(J, k) - SW_IPM_X1(J, k)) / (SW_IPM_MU_RATIO - 1.0);
}
SW_HD void sw_ipm_job_final(const sw_ipm_glob* g, const sw_ipm_job* J, double* sums, double* maxes) {
    const double dte = (g->t - g->t1) / (SW_IPM_MU_RATIO - 1.0);
    double se = 0.0, sce = 0.0, r = 0.0;
    for (int32_t k = 0; k < J->na; ++k) {
        const double e = sw_ipm_ext(J, k);
        sums[k] = J->sf * e;
        se = se + e;
        sce = sce + SW_IPM_C(J, k) * e;
        r = sw_max(r, -e / SW_IPM_X(J, k));
    }
    r = sw_max(r, se / SW_IPM_Q(J, SW_IPM_V));
    if (SW_IPM_Q(J, SW_IPM_HASV) != 0.0) r = sw_max(r, (SW_IPM_Q(J, SW_IPM_KAP) * dte - sce) / SW_IPM_Q(J, SW_IPM_U));
    maxes[0] = r;
}

/* After the final pass (one thread): θ into g->ap. */
SW_HD void sw_ipm_glob_final(sw_ipm_glob* g, const double* sums, const double* maxes) {
    double r = maxes[0];
    for (int32_t k = 0; k < g->na; ++k) r = sw_max(r, sums[k] / g->w[k]);
    r = sw_max(r, -((g->t - g->t1) / (SW_IPM_MU_RATIO - 1.0)) / g->t);
    g->ap = r > 1.0 ? 1.0 / r : 1.0;
}

/* whether the end extrapolates: two points were reached */
SW_HD int sw_ipm_two_points(const sw_ipm_glob* g) {
    return g->has_t && g->status == SW_IPM_OK && g->stage == 1;
}

/* The job's row of the allocation: its shares on the types with workers, 0.0
 * on the others. */
SW_HD void sw_ipm_job_emit(const sw_ipm_glob* g, const sw_ipm_job* J, double* xrow) {
    const int two = sw_ipm_two_points(g);
    for (int32_t k = 0; k < g->n; ++k) xrow[k] = 0.0;
    for (int32_t k = 0; k < J->na; ++k) {
        double x = SW_IPM_X(J, k);
        if (two) x = sw_max(0.0, x + g->ap * sw_ipm_ext(J, k));
        xrow[g->act[k]] = x;
    }
}

SW_HD double sw_ipm_level(const sw_ipm_glob* g, int32_t shift) {
    if (!g->has_t) return 0.0;
    if (!sw_ipm_two_points(g)) return sw_lp_scale(g->t, -shift);
    return sw_lp_scale(g->t + g->ap * ((g->t - g->t1) / (SW_IPM_MU_RATIO - 1.0)), -shift);
}

#endif /* SW_MMF_IPM_H */
