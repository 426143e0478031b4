/*
 * sw_wf.h — per-job arithmetic of the Gavel water-filling MaxMinFairness
 * allocation, shared by the HIP kernel (sw_wf.hip) and its CPU twin
 * (tests/twins/wf_twin.c).
 *
 * The reference baseline (policies/max_min_fairness_water_filling.py:303-409)
 * runs stages: one ECOS LP raises every unfrozen job by a common amount
 * c / mult_j (mult_j = sf_j / w_j, :140-149, :363), one GLPK MILP finds the
 * jobs that cannot rise any more (:191-301: a job at x_j = 1, or every job
 * once capacity is full), those are frozen (:388-398), and the loop repeats.
 * For one worker type (or several identical ones) the proportional
 * throughput of a job is its own throughput (proportional.py:15-44), the
 * normalised effective throughput is x_j, and the loop's fixed point is the
 * lexicographic max-min allocation
 *
 *     x_j = min(1, L* / c_j),   c_j = sf_j / w_j,
 *     L*  the largest level with cap(L) = Σ_j sf_j·min(1, L/c_j) ≤ G.
 *
 *   - Σ_j sf_j ≤ G: every job gets 1 and L* = max_j c_j.  The test is exact:
 *     the deterministic sum of the integers sf_j is their sum (below 2^53).
 *   - otherwise: L* is the largest double in [0, max_j c_j) with cap(L) ≤ G,
 *     cap the sw_detsum of the terms sf_j·min(1, L/c_j).  A correctly rounded
 *     quotient, product and sum are each nondecreasing in a nondecreasing
 *     operand, so every term and the fixed-order sum are nondecreasing in L,
 *     and a bisection over the bit pattern of L from bits(0) to bits(max c)
 *     is well defined: cap(0) = 0 ≤ G < Σ sf = cap(max c) holds at the start
 *     and is kept by every step, which ends in at most 63 probes.
 *
 * The shares are determined to a few ulps of G in capacity.  The level itself
 * is only as well determined as cap is steep: where the exact level sits just
 * under some c_k and every job still rising beyond it has a coefficient many
 * orders of magnitude larger, cap in doubles is flat for a long way past c_k
 * and L* is the far end of that flat (the shares differ from the exact ones
 * by no more than the rounding of cap).
 *
 * Only IEEE +, ×, ÷ and comparisons, with -ffp-contract=off on both sides,
 * and every job sum is sw_detsum: the GPU and the twin produce the same bits.
 */
#ifndef SW_WF_H
#define SW_WF_H

#include "sw_arith.h"

#define SW_WF_ITERS 64

/* x_j at level L: min(1, L / c_j) */
SW_HD double sw_wf_x(double c, double L) {
    const double r = L / c;
    return r < 1.0 ? r : 1.0;
}

/* the job's term of cap(L): sf_j·x_j(L) */
SW_HD double sw_wf_term(double sf, double c, double L) { return sf * sw_wf_x(c, L); }

#endif /* SW_WF_H */
