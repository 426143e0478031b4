/*
 * sw_mtd.h — arithmetic of the Gavel MinTotalDuration (makespan) allocation,
 * shared by the HIP kernel (sw_mtd.hip) and its CPU twin
 * (tests/twins/mtd_twin.c).
 *
 * The reference baseline (policies/min_total_duration.py:41-106) searches for
 * a small T at which this LP is feasible (:47-60, policy.py:57-63):
 *
 *     Σ_w x_jw ≤ 1,  Σ_j sf_j·x_jw ≤ G_w,  x ≥ 0,  Σ_w tp_jw·x_jw ≥ steps_j / T,
 *
 * and returns the x of the last feasible probe (the objective is a constant).
 * For one worker type (or several with identical throughputs, which
 * MinTotalDurationPolicy enforces by copying the v100 throughput, :25-31),
 * with p_j = steps_j / tp_j the time job j still needs at a full allocation,
 * the LP is feasible exactly when
 *
 *     max_j p_j ≤ T   and   cap(T) = Σ_j sf_j·(p_j / T) ≤ G,
 *
 * so a probe is one max (taken once) and one sum.
 *
 * The search (:82-101) is reproduced as written:
 *
 *     max_T = 1e6; min_T = 100; last_max_T = max_T; found = none
 *     while found is none:
 *         while 1.05·min_T < max_T:
 *             T = (min_T + max_T)/2
 *             feasible(T) ? (found = T, max_T = T) : (min_T = T)
 *         max_T = 10·last_max_T; min_T = last_max_T; last_max_T *= 10
 *
 * Round 0 searches [100, 1e6], round r ≥ 1 the decade [10^(5+r), 10^(6+r)].
 * Only midpoints are probed, so T never goes below 103.81…, and a least
 * feasible T in the top 5 % of a round's interval is found by the next round.
 * sw_mtd_next / sw_mtd_feed are the two loops as a state machine; the kernel
 * and the twin both drive it and differ only in how they evaluate cap(T).
 *
 * Both loops are bounded.
 *   Inner: a probe is the midpoint, so it halves max_T − min_T, and the loop
 *     runs while max_T − min_T > 0.05·min_T.  Round 0 starts at a width of
 *     9999·min_T and min_T only grows: at most ⌈log2(9999/0.05)⌉ = 18 probes.
 *     A decade round starts at 9·min_T: at most ⌈log2(9/0.05)⌉ = 8.
 *     SW_MTD_ROUND_PROBES = 32 is a guard above both that is never reached.
 *   Outer: the validator admits p_j ≤ SW_MTD_FULL_TIME_MAX = 1e15, sf_j ≤ 255,
 *     N < 2^31 and G ≥ 1, so cap(T)·T ≤ 255·2^31·1e15 < 5.48e26 in exact
 *     arithmetic.  The deterministic sum adds at most ⌈N/512⌉ ≤ 2^22 terms
 *     left to right and then nine tree levels, each term carrying two
 *     roundings: the computed cap(T) is within a factor 1 + 2^-29 of the exact
 *     one.  Every T ≥ 1e27 therefore passes both tests in this arithmetic.
 *     The first probe of round r ≥ 1 is 5.5·10^(5+r); at r = 22 it is 5.5e27,
 *     which is feasible, so the search has ended by round 22 on every admitted
 *     input: SW_MTD_ROUNDS = 23 rounds (0 … 22).  Should the cap ever be
 *     reached, sw_mtd_result returns the last interval's max_T (≥ 1e28,
 *     feasible by the same bound); no admitted input gets there.
 *
 * The feasible set at the found T is the face p_j/T ≤ x_j ≤ 1, Σ sf·x ≤ G.
 * Which of its points ECOS would return is unpinned (ECOS is absent; DESIGN.md
 * §15), so, as for MaxMinFairness and FinishTimeFairness, the kernel returns
 * the analytic centre of the face under the barrier of sw_mmf.h:
 *     x_j(μ) = sw_mmf_x(c = T, sf_j, t = p_j, μ),  μ the smallest value with
 *     μ·(G − Σ sf·x(μ)) ≥ 1  (a bisection over the bits of μ).
 *   - p_j/T = 1.0 only when p_j = T (p < T implies p/T ≤ 1 − 2^-52); then
 *     sw_mmf_x starts with lo = hi = 1 and returns 1.0: no pinning rule.
 *   - p_j = 0 (no steps left) is t = 0: a lower bound of 0.
 *   - cap(T) = G exactly: the face has no interior; x_j = p_j/T with μ = 0.
 *
 * Only IEEE +, −, ×, ÷ and comparisons, with -ffp-contract=off on both sides,
 * and every job sum is sw_detsum: the GPU and the twin produce the same bits.
 */
#ifndef SW_MTD_H
#define SW_MTD_H

#include "sw_arith.h"
#include "sw_mmf.h"

#define SW_MTD_FULL_TIME_MAX 1e15 /* seconds; the validator's bound on p_j */
#define SW_MTD_MIN_T 100.0
#define SW_MTD_MAX_T 1000000.0
#define SW_MTD_ROUNDS 23       /* round 0 and the decade rounds 1 … 22 */
#define SW_MTD_ROUND_PROBES 32 /* guard; a round takes at most 18 */
#define SW_MTD_MAX_PROBES (SW_MTD_ROUNDS * SW_MTD_ROUND_PROBES) /* the callers' loop bound */

typedef struct {
    double min_T, max_T, last_max_T;
    double found; /* the last feasible probe; valid when have */
    int32_t have;
    int32_t round;  /* the round in progress */
    int32_t in_round; /* probes taken in it */
    int32_t probes; /* probes taken in all */
} sw_mtd_search;

SW_HD void sw_mtd_begin(sw_mtd_search* s) {
    s->min_T = SW_MTD_MIN_T;
    s->max_T = SW_MTD_MAX_T;
    s->last_max_T = SW_MTD_MAX_T;
    s->found = 0.0;
    s->have = 0;
    s->round = 0;
    s->in_round = 0;
    s->probes = 0;
}

/* The next probe: 1 with *T set, 0 when the search has ended. */
SW_HD int sw_mtd_next(sw_mtd_search* s, double* T) {
    for (int32_t r = s->round; r < SW_MTD_ROUNDS; ++r) {
        if (1.05 * s->min_T < s->max_T && s->in_round < SW_MTD_ROUND_PROBES) {
            *T = (s->min_T + s->max_T) / 2.0;
            return 1;
        }
        if (s->have) return 0;
        if (r + 1 == SW_MTD_ROUNDS) return 0; /* keeps the last interval for sw_mtd_result */
        s->max_T = s->last_max_T * 10.0;
        s->min_T = s->last_max_T;
        s->last_max_T = s->last_max_T * 10.0;
        s->round = r + 1;
        s->in_round = 0;
    }
    return 0;
}

/* The answer to the probe sw_mtd_next returned. */
SW_HD void sw_mtd_feed(sw_mtd_search* s, double T, int feasible) {
    if (feasible) {
        s->found = T;
        s->have = 1;
        s->max_T = T;
    } else {
        s->min_T = T;
    }
    s->in_round = s->in_round + 1;
    s->probes = s->probes + 1;
}

SW_HD double sw_mtd_result(const sw_mtd_search* s) { return s->have ? s->found : s->max_T; }

/* the least x_j with which job j finishes within T */
SW_HD double sw_mtd_low(double p, double T) { return p / T; }

/* x_j at capacity multiplier μ on the feasible face of T */
SW_HD double sw_mtd_x(double sf, double p, double T, double mu) { return sw_mmf_x(T, sf, p, mu); }

#endif /* SW_MTD_H */
