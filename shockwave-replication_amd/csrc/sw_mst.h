/*
 * sw_mst.h — arithmetic of the Gavel max-sum-throughput allocation ("MST"),
 * shared by the HIP kernel (sw_mst.hip) and its CPU twin
 * (tests/twins/mst_twin.c).
 *
 * The reference baseline (policies/max_sum_throughput.py:39-96 with the base
 * constraints of policy.py:57-63) solves, with ECOS, for one worker type with
 * G workers, job j of scale factor sf_j, throughput tp_j, instance cost c > 0
 * and weight w_j = tp_j / c:
 *
 *     maximise  Σ_j w_j·x_j
 *     s.t.      0 ≤ x_j ≤ 1,   Σ_j sf_j·x_j ≤ G,
 *               tp_j·x_j ≥ steps_j / SLO_j      for the jobs that have an SLO,
 *
 * and again without the SLO rows when they make the LP infeasible (:91-94).
 * (`scale`, :60, is computed there and never used; it has no counterpart.)
 *
 * Floors.  With r_j = steps_j / SLO_j the SLO row is x_j ≥ l_j = r_j / tp_j
 * when r_j > 0 (+inf when tp_j = 0); a row with r_j ≤ 0 holds for every
 * x_j ≥ 0 and is dropped: l_j = 0, no barrier term.  The caller passes l_j.
 * The rows are infeasible exactly when some l_j > 1 or Σ_j sf_j·l_j > G; then
 * every floor becomes 0 and the instance is flagged slo_dropped.
 *
 * Threshold.  The LP is a fractional knapsack over the densities
 * d_j = w_j / sf_j (the rounded IEEE quotient; jobs of equal tp and sf tie
 * exactly, and ties are decided on that double).  With
 *     f(θ) = Σ_j sf_j·(d_j > θ ? 1 : l_j),
 * non-increasing in θ with f(max d) = Σ sf·l ≤ G: λ* = 0 when f(0) ≤ G,
 * otherwise λ* is the smallest double θ with f(θ) ≤ G, which is some job's
 * density.  Non-negative doubles order as their bit patterns, so λ* is found
 * by bisection over the bits of θ.  The bracket starts at
 * (pred(min d), max d], and every probe also returns the largest density ≤ θ
 * and the smallest density > θ: f is constant between neighbouring densities,
 * so a feasible probe moves the upper end down to the former and an infeasible
 * one moves the lower end up to just below the latter.  Each probe at least
 * halves the bracket's bit distance (< 2^63): SW_MST_THETA_ITERS = 64 bounds
 * the loop; with few distinct densities it ends after a few probes.
 * Jobs with d_j > λ* get x_j = 1, jobs with d_j < λ* get x_j = l_j, and the tie
 * class C = {d_j = λ*} shares the rest.
 *
 * Tie class.  Which point of a non-unique optimum ECOS returns is unpinned
 * (ECOS is absent), so, as for the other baselines, the kernel
 * returns the analytic centre of the optimal face under the log barrier of the
 * rows that are not tight on the whole face.  Per class job
 *     b_j(x) = log x + log(1 − x) + [l_j > 0]·log(x − l_j),
 *     h_j(x) = b_j'(x) = 1/x − 1/(1 − x) + [l_j > 0]·1/(x − l_j),
 * h_j strictly decreasing on (l_j, 1); x_j(m) = sw_mst_x(sf_j, l_j, m) is the
 * root of h_j(x) = sf_j·m by bisection to adjacent doubles (≤ 64 halvings of
 * an interval inside [0, 1] whose mid-points are doubles: SW_MST_X_ITERS).
 * A step compares without dividing: over the common denominator
 * den = x(1 − x)(x − l_j) > 0, h_j(x) > t ⇔ num > t·den with
 * num = (1 − x)(x − l_j) − x(x − l_j) + x(1 − x) (without the x − l_j factor
 * and term when l_j = 0).  Each term of num over den is one term of h_j, so
 * num/den carries a few ulps of 1/x + 1/(1 − x) + 1/(x − l_j), as the three
 * quotients would; a den that underflows to 0 still answers monotonically in t.
 *   λ* > 0: capacity is tight on the face.  Maximise Σ_C b_j s.t. Σ sf·x = G:
 *     the multiplier m = ν is signed.  ν is the smallest value, in the total
 *     order of doubles on [−2^64, 2^64], at which the sum over all jobs of
 *     sf_j·x_j is ≤ G; the bisection runs over sw_mst_key, an order-preserving
 *     integer key of the signed double.  The key distance of the ends is
 *     2·0x43F0000000000000 + 1 < 2^64 and a probe halves it:
 *     SW_MST_M_ITERS = 64.  (|h_j| ≤ 2^54 on doubles inside (l_j, 1) with
 *     sf_j ≥ 1, so at ν = ∓2^64 every class job sits at the double next to 1
 *     or to l_j.)
 *   λ* = 0: capacity is slack; the class is the zero-density jobs (w_j = 0),
 *     usually empty.  Maximise Σ_C b_j + log(G − Σ sf·x): m = μ > 0 is the
 *     smallest value with μ·slack(μ) ≥ 1, the bisection over the bits of μ in
 *     [2^-64, 2^64] of sw_mmf.h.  With an empty class μ = 0.
 *   Either: when the sum with the whole class at its floors is already ≥ G the
 *     face is the single point x_j = l_j and m = 0.
 *
 * Bounds.  The validator admits sf_j ∈ [1, 255], 0 ≤ w_j ≤ SW_MST_WEIGHT_MAX,
 * l_j ≥ 0 or +inf (not NaN), G ≥ 1 and N < 2^31.  SW_MST_WEIGHT_MAX = 1e30:
 * the objective Σ w·x ≤ 2^31·1e30 < 2.2e39 and every density are finite, so
 * no sum or bracket end is ever inf or NaN (sf·l with l = +inf is the only
 * infinite term, and it only ever sets slo_dropped); a throughput per unit
 * cost beyond 1e30 steps/s is not a measurement.  A weight so small that
 * w/sf rounds to 0 is a zero density, like w = 0.
 *
 * Only IEEE +, −, ×, ÷ and comparisons, with -ffp-contract=off on both sides,
 * every job sum is sw_detsum and every branch is taken on a block-reduced
 * value: the GPU and the twin produce the same bits.
 */
#ifndef SW_MST_H
#define SW_MST_H

#include "sw_arith.h"
#include "sw_mmf.h"

#define SW_MST_WEIGHT_MAX 1e30 /* the validator's bound on w_j */
#define SW_MST_THETA_ITERS 64
#define SW_MST_M_ITERS 64
#define SW_MST_X_ITERS 64
#define SW_MST_INF_BITS 0x7FF0000000000000ull
#define SW_MST_NU_LO_KEY 0x3C0FFFFFFFFFFFFFull /* sw_mst_key(−2^64) */
#define SW_MST_NU_HI_KEY 0xC3F0000000000000ull /* sw_mst_key(+2^64) */

/* Order-preserving key of a double (no NaN): a < b ⇔ key(a) < key(b), with
 * −0 just below +0. */
SW_HD uint64_t sw_mst_key(double v) {
    const uint64_t b = sw_bits(v);
    return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}
SW_HD double sw_mst_unkey(uint64_t k) {
    return sw_from_bits((k >> 63) ? (k & 0x7FFFFFFFFFFFFFFFull) : ~k);
}

/* d_j ≥ +0 (a weight of −0 is a zero density) */
SW_HD double sw_mst_density(double w, double sf) { return w > 0.0 ? w / sf : 0.0; }

/* the floor in force: 0 once the SLO rows were dropped */
SW_HD double sw_mst_floor(double l, int dropped) { return (!dropped && l > 0.0) ? l : 0.0; }

/* x_j(m): the root of h_j(x) = sf·m on (l, 1), by bisection to adjacent
 * doubles.  The upper one is returned, the least probed x with h_j(x) ≤ sf·m
 * (1 when there is none): it lies in (l, 1] for l < 1, and is non-increasing
 * in m because a larger m turns probe answers from "right" to "left" only
 * (target·den is non-decreasing in m for den ≥ 0).
 * l = 1 returns 1. */
SW_HD double sw_mst_x(double sf, double l, double m) {
    double lo = l, hi = 1.0;
    const double target = sf * m;
    for (int it = 0; it < SW_MST_X_ITERS; ++it) {
        const double mid = (lo + hi) * 0.5;
        if (!(mid > lo && mid < hi)) break;
        const double a = 1.0 - mid; /* > 0: mid < hi ≤ 1 */
        double num, den;           /* h_j(mid) = num / den, den ≥ 0 */
        if (l > 0.0) {
            const double b = mid - l; /* > 0: mid > lo ≥ l */
            num = a * b - mid * b + mid * a;
            den = mid * a * b;
        } else {
            num = a - mid;
            den = mid * a;
        }
        if (num > target * den) lo = mid; else hi = mid;
    }
    return hi;
}

/* x_j with the threshold λ and the class multiplier m; m = +inf stands for
 * the class at its floors (the face that is a single point) */
SW_HD double sw_mst_alloc(double d, double sf, double l, double lambda, double m) {
    if (d > lambda) return 1.0;
    if (d < lambda || sw_bits(m) == SW_MST_INF_BITS) return l;
    return sw_mst_x(sf, l, m);
}

#endif /* SW_MST_H */
