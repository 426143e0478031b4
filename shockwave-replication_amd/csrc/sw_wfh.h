/*
 * sw_wfh.h — arithmetic of the hierarchical (entity) water-filling
 * MaxMinFairness allocation, shared by the HIP kernel (sw_wfh.hip) and its CPU
 * twin (tests/twins/wfh_twin.c).
 *
 * The reference (policies/max_min_fairness_water_filling.py:21-77, :303-409)
 * gives every entity e (a user or a team) a weight W_e and a mode, and before
 * each stage of its loop hands the entity's weight to its unfrozen jobs:
 * "fairness" in proportion to their priority weights, "fifo" all of it to the
 * unfrozen job with the smallest id.  For one worker type the loop's fixed
 * point is two nested water fillings, D_e = Σ_{j∈e} sf_j:
 *
 *   outer   g_e = D_e·min(1, C* / k_e),  k_e = D_e / W_e,
 *           C* the largest level with cap_out(C) = Σ_e D_e·min(1, C/k_e) ≤ G
 *           (Σ_e D_e ≤ G: every job gets 1, C* = max_e k_e over the entities
 *           that have jobs)
 *   inner   fairness: x_j = min(1, τ_e / c_j), τ_e the largest level with
 *                     cap_e(τ) = Σ_{j∈e} sf_j·min(1, τ/c_j) ≤ g_e
 *           fifo:     x_j = clamp((g_e − Σ_{k∈e, k<j} sf_k) / sf_j, 0, 1)
 *
 * An entity with g_e ≥ D_e is saturated: every job of it gets exactly 1.0 and
 * no search runs.  An entity of one job is filled by the fifo formula whatever
 * its mode (the two agree: sf·min(1, τ/c) = g has x = g/sf).
 *
 * The order of every floating-point sum, fixed once, here:
 *   - the entities and the jobs of an instance are kept in MEMBER ORDER: entity
 *     0's jobs in ascending job index, then entity 1's, …; position p of that
 *     order holds job mem[p];
 *   - cap_out(C), Σ_e D_e and the allocated capacity Σ_p sf_p·x_p are
 *     sw_detsum: the E entities (or the N positions) split into 512
 *     contiguous chunks, each summed left to right, then the halving tree over
 *     each wave's 64 partials and the halving tree over the 8 waves;
 *   - cap_e(τ) is a WAVE sum over the entity's n members: lane l adds its
 *     members l, l + 64, l + 128, … left to right, then the halving tree over
 *     the 64 lane partials (p[i] += p[i+h], h = 32 … 1).
 * D_e and the fifo prefixes are sums of integers, kept in int64: exact in any
 * order.  Every term is nondecreasing in its level under correctly rounded
 * ÷, × and +, so each fixed-order sum is, and both levels are found by a
 * bisection over the bit pattern of the level as in sw_wf.h.
 *
 * Only IEEE +, −, ×, ÷ and comparisons, with -ffp-contract=off on both sides:
 * the GPU and the twin produce the same bits.
 */
#ifndef SW_WFH_H
#define SW_WFH_H

#include "sw_wf.h"

#define SW_WFH_FAIRNESS 0
#define SW_WFH_FIFO 1

/* k_e = D_e / W_e (an entity without jobs: 0, and its terms are 0) */
SW_HD double sw_wfh_coef(int64_t D, double W) { return D > 0 ? (double)D / W : 0.0; }

/* the entity's term of cap_out(C): D_e·min(1, C / k_e) */
SW_HD double sw_wfh_outer_term(int64_t D, double k, double C) {
    return D > 0 ? sw_wf_term((double)D, k, C) : 0.0;
}

/* the fifo fill: pre = Σ_{k∈e, k<j} sf_k */
SW_HD double sw_wfh_fifo_x(double g, int64_t pre, int32_t sf) {
    const double r = (g - (double)pre) / (double)sf;
    return r < 0.0 ? 0.0 : (r < 1.0 ? r : 1.0);
}

#endif /* SW_WFH_H */
