/*
 * sw_mst_types.h — the Gavel max-sum-throughput allocation over worker types
 * that DIFFER, as a transportation problem solved by successive best paths:
 * the state of an instance and every step that one thread takes on it, shared
 * by the HIP kernel (sw_mst_types.hip) and its CPU twin
 * (tests/twins/mstt_twin.c).  Plain C99 + HIP qualifiers.
 *
 * The reference LP (policies/max_sum_throughput.py:39-96 without SLOs, with the
 * base constraints of policy.py:46-63), w_jk = throughput_jk / cost_k:
 *
 *     maximise  Σ_jk w_jk·x_jk
 *     s.t.      Σ_k x_jk ≤ 1,   Σ_j sf_j·x_jk ≤ W_k,   x ≥ 0.
 *
 * Substitution.  y_jk = sf_j·x_jk turns it into a transportation problem: job j
 * is a source of sf_j units, type k a sink of W_k units, one more sink (the
 * dummy, node n) of profit 0 and no bound takes what is not allocated, and a
 * unit of j on k earns d_jk = w_jk / sf_j (the rounded IEEE quotient; d_jn = 0).
 * Supplies and capacities are integers, so every y_jk stays an integer; doubles
 * appear in profit comparisons only.
 *
 * Successive best paths.  Jobs enter in index order.  The entering job j pushes
 * its units along the best path of the residual graph until all are placed (on
 * the dummy counts).  A path reaches a sink k at gain d_jk and may go on along
 * displacements k → l, in which a job i with y_ik > 0 moves units from k to l
 * at gain d_il − d_ik, to end at a sink with residual capacity (the dummy always
 * has some).  The flow before a push is optimal for the jobs entered so far
 * (the invariant), so the residual graph has no cycle of positive gain and
 * best paths exist; after the push along a best path the invariant holds again.
 * No displacement leaves the dummy: with an optimal flow, moving a unit from
 * the dummy to l and on to a free sink gains nothing, so a best path that ends
 * at the dummy is as good as any through it.
 *
 * Sink graph.  All that path finding needs of the jobs is, for every ordered
 * pair of a type k and a sink l ≠ k (the dummy included),
 *     g_kl = max over i with y_ik > 0 of (d_il − d_ik),    a_kl its job,
 * −inf without such a job: a graph on at most 17 nodes.  Equal gains go to the
 * lowest job index.  Bellman–Ford on it takes at most n rounds (a path has at
 * most n arcs); every round relaxes every sink from the distances of the round
 * before (sw_mstt_relax: one lane per sink on the GPU, a loop in the twin, the
 * same bits), strictly, the predecessors in ascending order, so that equal
 * gains go to the lowest type.  The end of the path is the sink with residual
 * capacity of the largest gain; the dummy wins ties (no unit is placed where it
 * earns nothing), then the lowest type.
 *
 * Push.  δ = min(supply left of j, residual of the end, y_ik of every displaced
 * arc on the path) ≥ 1.  An arc (i, l) that the push creates updates row l of g
 * in O(n) (sw_mstt_arc_add).  An arc (i, k) that it empties makes row k stale
 * only when i is a_kl for some l; then the row is recomputed from all jobs
 * (sw_mstt_better over the jobs with y_ik > 0: a lexicographic maximum, so its
 * result does not depend on the order of the reduction).  Every push places at
 * least one unit of the entering job, so an instance takes at most
 * Σ sf_j ≤ 255·m augmentations: SW_MSTT_CAP_MULT·(m + n) can only be exceeded
 * by a broken invariant (SW_MSTT_CAP).  Largest augmentations / jobs seen in
 * tests/test_mst_types.py and tests/test_gpu_mst_types.py: 2.0 (two and three
 * jobs on two types); 1.2–1.7 on the random instances of 24 to 4097 jobs.
 *
 * Duals.  After the last job q_k = the best gain of a displacement chain from k
 * to a sink with residual capacity (0 for such a sink and for the dummy) is ≤ 0
 * by the invariant, and price_k = −q_k ≥ 0 is the loss of freeing a unit of k.
 * With u_j = max(0, max_k (d_jk − price_k)),
 *     D = Σ_k W_k·price_k + Σ_j sf_j·u_j
 * equals the objective (complementary slackness along the arcs of the residual
 * graph): the certificate the tests recompute.  A type without workers has no
 * flow and no chain; its price is max_j d_jk, at which no job wants it.
 *
 * The returned point x_jk = y_jk / sf_j is a vertex of the LP (the flow of
 * successive best paths is a basic, forest-supported, solution); among several
 * optimal vertices it is the one the tie rules above pick.
 *
 * Rounding.  Gains are differences of doubles and distances rounded sums of
 * them, so a cycle of exact gain 0 (a job moved k → l and back) can gain an ulp
 * and "improve" a distance.  The rounds therefore keep the predecessor of every
 * sink per round (pr[r][l]: a walk back through the rounds always ends at the
 * source, after at most n arcs), and sw_mstt_push cuts such a cycle out of the
 * walk when it meets a sink a second time: what is left is a path of the graph
 * whose gain differs from the walk's by that rounding.
 */
#ifndef SW_MST_TYPES_H
#define SW_MST_TYPES_H

#include "sw_arith.h"

#define SW_MSTT_MAX_TYPES 16
#define SW_MSTT_NODES (SW_MSTT_MAX_TYPES + 1)
#define SW_MSTT_WEIGHT_MAX 1e30 /* the validator's bound on w_jk, as SW_MST_WEIGHT_MAX */
#define SW_MSTT_CAP_MULT 256    /* augmentations ≤ Σ sf ≤ 255·m < 256·(m + n) */
/* the flow y[m][n] (int32) is LDS-resident up to this many cells: 48 KB of the
 * 64 KB a launch gets without opting in (the rest holds sw_mstt_state and the
 * reduction slots).  The twin has one path; the tests take the limit from here. */
#define SW_MSTT_LDS_CELLS 12288
#define SW_MSTT_NEG_INF_BITS 0xFFF0000000000000ull
#define SW_MSTT_NO_JOB 0x7FFFFFFF

#define SW_MSTT_OK 0
#define SW_MSTT_CAP (-3)   /* the step cap (SW_IPM_CAP of the worker-type frame) */

#define SW_MSTT_UNPLACED 1 /* flags: some unit went to the dummy */
#define SW_MSTT_SLACK 2    /* no type with workers is saturated */

/* doubles of workspace per job: d[n], then y[n] as int32 (read only when the
 * flow is not LDS-resident) */
#define SW_MSTT_FIELDS(n) ((n) + ((n) + 1) / 2)

typedef struct {
    double g[SW_MSTT_MAX_TYPES][SW_MSTT_NODES];
    double dist[2][SW_MSTT_NODES];
    int32_t arg[SW_MSTT_MAX_TYPES][SW_MSTT_NODES];
    int32_t resid[SW_MSTT_MAX_TYPES];
    int32_t new_job[SW_MSTT_NODES], new_type[SW_MSTT_NODES];
    int8_t pr[SW_MSTT_MAX_TYPES][SW_MSTT_NODES]; /* per round: the predecessor, or −1 for "as the round before" */
    int32_t n, m;
    int32_t rem;    /* units of the entering job still to place */
    int32_t nnew;   /* arcs the last push created */
    int32_t dirty;  /* bit k: the last push made row k stale */
    int32_t status, flags;
    int64_t augs, cap, rows;
} sw_mstt_state;

SW_HD double sw_mstt_neg_inf(void) { return sw_from_bits(SW_MSTT_NEG_INF_BITS); }

/* d_jk ≥ +0 (a weight of −0 is a zero density) */
SW_HD double sw_mstt_density(double w, double sf) { return w > 0.0 ? w / sf : 0.0; }

/* the profit of a unit of job i at sink l of D[m][n]; 0 at the dummy */
SW_HD double sw_mstt_d(const double* D, int32_t n, int32_t i, int32_t l) {
    return l < n ? D[(int64_t)i * n + l] : 0.0;
}

/* is (c, i) a better displacement than (best, bi)?  larger gain, then lower job */
SW_HD int sw_mstt_better(double c, int32_t i, double best, int32_t bi) {
    return c > best || (c == best && i < bi);
}

SW_HD void sw_mstt_setup(sw_mstt_state* s, int32_t m, int32_t n, const int32_t* workers) {
    s->n = n;
    s->m = m;
    for (int32_t k = 0; k < n; ++k) {
        s->resid[k] = workers[k];
        for (int32_t l = 0; l <= n; ++l) {
            s->g[k][l] = sw_mstt_neg_inf();
            s->arg[k][l] = SW_MSTT_NO_JOB;
        }
    }
    s->rem = 0;
    s->nnew = 0;
    s->dirty = 0;
    s->status = SW_MSTT_OK;
    s->flags = 0;
    s->augs = 0;
    s->rows = 0;
    s->cap = (int64_t)SW_MSTT_CAP_MULT * ((int64_t)m + n);
}

/* sink l's distance before the first round of job j's path */
SW_HD void sw_mstt_start(sw_mstt_state* s, const double* D, int32_t j, int32_t l) {
    s->dist[0][l] = sw_mstt_d(D, s->n, j, l);
}

/* Round r of sink l (0..n): dist[from ^ 1][l] from dist[from][·]; returns
 * whether it improved. */
SW_HD int sw_mstt_relax(sw_mstt_state* s, int32_t l, int32_t r, int from) {
    const double* od = s->dist[from];
    double best = od[l];
    int32_t p = -1;
    for (int32_t k = 0; k < s->n; ++k) {
        if (k == l) continue;
        const double c = od[k] + s->g[k][l];
        if (c > best) { best = c; p = k; }
    }
    s->dist[from ^ 1][l] = best;
    s->pr[r][l] = (int8_t)p;
    return p >= 0;
}

/* The new arc (i, k) in row k, for sink l (0..n). */
SW_HD void sw_mstt_arc_add(sw_mstt_state* s, const double* D, int32_t i, int32_t k, int32_t l) {
    if (l == k) return;
    const double c = sw_mstt_d(D, s->n, i, l) - sw_mstt_d(D, s->n, i, k);
    if (sw_mstt_better(c, i, s->g[k][l], s->arg[k][l])) { s->g[k][l] = c; s->arg[k][l] = i; }
}

/* One thread, after `rounds` rounds left the distances in dist[buf]: the end of
 * the path, δ, the moves in y[m][n], the list of created arcs and the stale rows. */
SW_HD void sw_mstt_push(sw_mstt_state* s, int32_t* y, int32_t j, int32_t rounds, int buf) {
    const int32_t n = s->n;
    const double* dist = s->dist[buf];
    s->nnew = 0;
    s->dirty = 0;
    if (++s->augs > s->cap) { s->status = SW_MSTT_CAP; return; }
    int32_t e = n;
    double best = dist[n];
    for (int32_t l = 0; l < n; ++l)
        if (s->resid[l] > 0 && dist[l] > best) { best = dist[l]; e = l; }
    /* the path backwards from e through the rounds; node[0] = e.  A sink met
     * again closes a cycle of rounding: the walk since its first visit is dropped */
    int32_t node[SW_MSTT_NODES], pos[SW_MSTT_NODES];
    int32_t len = 0, seen = 0, v = e, r = rounds - 1;
    for (;;) {
        if ((seen >> v) & 1) {
            while (len > pos[v] + 1) seen &= ~(1 << node[--len]);
        } else {
            pos[v] = len;
            node[len++] = v;
            seen |= 1 << v;
        }
        while (r >= 0 && s->pr[r][v] < 0) --r;
        if (r < 0) break;
        v = s->pr[r][v];
        --r;
    }
    int32_t delta = s->rem;
    if (e < n && s->resid[e] < delta) delta = s->resid[e];
    for (int32_t a = len - 1; a > 0; --a) { /* the arc node[a] → node[a−1] */
        const int32_t k = node[a], i = s->arg[k][node[a - 1]];
        const int32_t have = y[(int64_t)i * n + k];
        if (have < delta) delta = have;
    }
    const int32_t first = node[len - 1];
    if (first < n) {
        int32_t* c = y + (int64_t)j * n + first;
        if (*c == 0) { s->new_job[s->nnew] = j; s->new_type[s->nnew] = first; ++s->nnew; }
        *c += delta;
    }
    for (int32_t a = len - 1; a > 0; --a) {
        const int32_t k = node[a], l = node[a - 1], i = s->arg[k][l];
        int32_t* from = y + (int64_t)i * n + k;
        *from -= delta;
        if (*from == 0)
            for (int32_t t = 0; t <= n; ++t)
                if (t != k && s->arg[k][t] == i) s->dirty |= 1 << k;
        if (l < n) {
            int32_t* to = y + (int64_t)i * n + l;
            if (*to == 0) { s->new_job[s->nnew] = i; s->new_type[s->nnew] = l; ++s->nnew; }
            *to += delta;
        }
    }
    if (e < n) s->resid[e] -= delta; else s->flags |= SW_MSTT_UNPLACED;
    s->rem -= delta;
}

/* the duals: q of sink l before the first round, and one round of type k
 * (q_k from the q of the round before); q is the gain of the best chain to a
 * sink with residual capacity, −inf without one */
SW_HD void sw_mstt_dual_start(sw_mstt_state* s, int32_t l) {
    s->dist[0][l] = (l == s->n || s->resid[l] > 0) ? 0.0 : sw_mstt_neg_inf();
}
SW_HD int sw_mstt_dual_relax(sw_mstt_state* s, int32_t k, int from) {
    const double* oq = s->dist[from];
    double best = oq[k];
    int changed = 0;
    if (k < s->n)
        for (int32_t l = 0; l <= s->n; ++l) {
            if (l == k) continue;
            const double c = s->g[k][l] + oq[l];
            if (c > best) { best = c; changed = 1; }
        }
    s->dist[from ^ 1][k] = best;
    return changed;
}
/* the price of type k from its q; colmax = max_j d_jk, read only when the type
 * has no chain (no workers, so no flow) */
SW_HD double sw_mstt_price(double q, double colmax) {
    if (sw_bits(q) == SW_MSTT_NEG_INF_BITS) return colmax;
    return q < 0.0 ? 0.0 - q : 0.0;
}

/* Σ_k w_jk·x_jk of one job, left to right, with x_jk = y_jk / sf_j written to x */
SW_HD double sw_mstt_emit(int32_t n, const int32_t* y, double sf, const double* w, double* x) {
    double v = 0.0;
    for (int32_t k = 0; k < n; ++k) {
        x[k] = (double)y[k] / sf;
        v = v + w[k] * x[k];
    }
    return v;
}

/* result[4] = the objective, augmentations, row recomputations, flags */
SW_HD void sw_mstt_result(sw_mstt_state* s, const int32_t* workers, double objective, double* out) {
    int slack = 1;
    for (int32_t k = 0; k < s->n; ++k)
        if (workers[k] > 0 && s->resid[k] == 0) slack = 0;
    if (slack) s->flags |= SW_MSTT_SLACK;
    out[0] = objective;
    out[1] = (double)s->augs;
    out[2] = (double)s->rows;
    out[3] = (double)s->flags;
}

#endif /* SW_MST_TYPES_H */
