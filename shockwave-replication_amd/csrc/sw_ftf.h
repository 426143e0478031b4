/*
 * sw_ftf.h — per-job arithmetic of the Gavel FinishTimeFairness (Themis)
 * allocation, shared by the HIP kernel (sw_ftf.hip) and its CPU twin
 * (tests/twins/ftf_twin.c).
 *
 * The reference baseline (policies/finish_time_fairness.py:55-140,
 * isolated.py:34-52) solves, with ECOS, for one worker type (or several with
 * identical throughputs, which FinishTimeFairnessPolicy enforces by copying
 * the v100 throughput, :35-43):
 *
 *     minimise  max_j (a_j + p_j / x_j) / E_j
 *     s.t.      Σ_j sf_j·x_j ≤ G,   0 ≤ x_j ≤ 1,
 *
 * p_j the time job j still needs at a full allocation (steps remaining /
 * throughput), a_j the time since its start, E_j its expected isolated
 * duration.  A level ρ is feasible exactly when, with d_j(ρ) = ρ·E_j − a_j,
 * d_j(ρ) ≥ p_j for every j and cap(ρ) = Σ_j sf_j·p_j/d_j(ρ) ≤ G; both are
 * monotone in ρ.  ρ_box = max_j (a_j + p_j)/E_j is the least level the bounds
 * x_j ≤ 1 admit.
 *   - cap(ρ_box) > G: capacity binds.  ρ* is the smallest double with
 *     cap(ρ) ≤ G, a bisection over the bit pattern of ρ from bits(ρ_box) to
 *     the largest finite double; x_j = p_j / d_j(ρ*) is the unique optimum.
 *     cap(ρ_box) = G exactly is the same case with ρ* = ρ_box: the optimal
 *     face is the single point x_j = p_j / d_j(ρ_box) (the barrier below has
 *     no interior there), so it is returned with μ = 0 as well.
 *   - cap(ρ_box) < G: ρ* = ρ_box.  Jobs with d_j ≤ p_j (in this arithmetic;
 *     sw_ftf_pinned) are pinned at x_j = 1; every other job is free in
 *     [p_j/d_j, 1] under the remaining capacity, and the kernel returns the
 *     analytic centre of that face with the barrier of sw_mmf.h: per free job
 *         1/x − 1/(1−x) + d_j/(d_j·x − p_j) = sf_j·μ,  μ·slack(μ) = 1,
 *     which is sw_mmf_x(c = d_j, sf_j, t = p_j, μ) unchanged.  Which optimal
 *     point ECOS would return here is unpinned: ECOS is absent, and its cone
 *     formulation of inv_pos is not the linear barrier used.
 *   - p_j = 0 (no steps left) is allowed: the job's ratio is the constant
 *     a_j/E_j, which enters ρ_box; it needs nothing, so it gets x_j = 0 when
 *     capacity binds and is a free job with lower bound 0 on the face
 *     (c = 1, t = 0: the barrier 2·log x + log(1 − x) does not depend on d_j).
 *
 * Only IEEE +, −, ×, ÷ and comparisons, with -ffp-contract=off on both sides,
 * and every job sum is sw_detsum: the GPU and the twin produce the same bits.
 */
#ifndef SW_FTF_H
#define SW_FTF_H

#include "sw_arith.h"
#include "sw_mmf.h"

#define SW_FTF_RHO_HI 0x7FEFFFFFFFFFFFFFull /* the largest finite double */
#define SW_FTF_ITERS 64

/* (a_j + p_j) / E_j: the job's ratio at a full allocation */
SW_HD double sw_ftf_box(double p, double a, double E) { return (a + p) / E; }

/* d_j(ρ) = ρ·E_j − a_j */
SW_HD double sw_ftf_d(double a, double E, double rho) { return rho * E - a; }

/* the least x_j that keeps the job's ratio ≤ ρ: p_j / d_j(ρ), 1 where the
 * level leaves no room, 0 for a job with nothing left to run */
SW_HD double sw_ftf_low(double p, double a, double E, double rho) {
    const double d = sw_ftf_d(a, E, rho);
    if (!(p > 0.0)) return 0.0;
    return d <= p ? 1.0 : p / d;
}

/* At ρ = ρ_box a job needs the whole of x_j = 1 when d_j ≤ p_j, or when its
 * own ratio is the maximum (the same condition in exact arithmetic; the
 * rounding of ρ·E_j − a_j can leave d_j a few ulps above p_j for the very job
 * that set ρ_box, which would make it a free job on an interval too narrow
 * for doubles to resolve).  Never a job with p_j = 0. */
SW_HD int sw_ftf_pinned(double p, double a, double E, double d, double rho_box) {
    return p > 0.0 && (d <= p || sw_ftf_box(p, a, E) >= rho_box);
}

/* sw_ftf_low at ρ_box, with the pinned jobs of the face */
SW_HD double sw_ftf_low_box(double p, double a, double E, double rho_box) {
    const double d = sw_ftf_d(a, E, rho_box);
    if (!(p > 0.0)) return 0.0;
    return sw_ftf_pinned(p, a, E, d, rho_box) ? 1.0 : p / d;
}

/* x_j at capacity multiplier μ on the optimal face of level ρ_box */
SW_HD double sw_ftf_x(double sf, double p, double a, double E, double rho_box, double mu) {
    const double d = sw_ftf_d(a, E, rho_box);
    if (!(p > 0.0)) return sw_mmf_x(1.0, sf, 0.0, mu);
    return sw_ftf_pinned(p, a, E, d, rho_box) ? 1.0 : sw_mmf_x(d, sf, p, mu);
}

#endif /* SW_FTF_H */
