/*
 * sw_allox.h — the AlloX assignment (policies/allox.py:71-118), its column
 * state and the step functions that decide results, shared by the HIP kernel
 * (sw_allox.hip) and its CPU twin (tests/twins/allox_twin.c).
 *
 * The reference (allox.py:71-103) places m jobs on n free workers by a
 * min-cost bipartite assignment: job i in column (worker j, position k),
 * k = 1..m, costs
 *     c(i, j, k) = k·p[i][type(j)] + d[i],
 * p the processing time (steps remaining / throughput, :77-82) and d the delay
 * (time since start, :93).  Position 1 runs last: the job at position k adds
 * its p to its own completion time and to those of the k − 1 jobs behind it,
 * hence the factor k (:83-87).  The reference builds the dense m × (m·n) matrix and
 * calls scipy.optimize.linear_sum_assignment (:103).
 *
 * Method.  The same shortest-augmenting-path scheme (Jonker–Volgenant, one
 * Dijkstra search per row, rows in job order) with the cost computed where it
 * is used, over a pruned column set:
 *   - a column that was never assigned has dual v = 0, and an assigned column
 *     stays assigned (an augmentation only ever adds the sink);
 *   - p ≥ 0, so c(i, j, k) does not decrease in k: among the never-assigned
 *     columns of worker j the lowest position has the smallest reduced cost
 *     for every row, and an unassigned column can only end a search (as its
 *     sink), never lie inside a path.  Only that one column per worker, its
 *     frontier, has to be looked at;
 *   - so worker j's assigned positions are 1..len_j without gaps, and the
 *     live set is the assigned columns plus n frontiers: at most m + n.
 * Slots.  Slot j < n is worker j's frontier (position len_j + 1, v = 0, no
 * owner).  Slot n + r is the column assigned by the r-th augmentation: the
 * sink of row r's search is copied there and the worker's frontier moves one
 * position up.  Row r's search therefore scans the slots [0, n + r).
 *
 * Tie rule.  A search step takes, among the unvisited slots, the smallest
 * tentative distance; among equal distances the LOWEST SLOT.  Frontiers hold
 * the lowest slots, so an unassigned column goes before an assigned one
 * (scipy's rule, which ends a search as early as it can), then the lower
 * worker index, then the column assigned earlier.  Distances are compared as
 * doubles with <, so −0 and +0 tie.  The order is total over the slots, so the
 * minimum does not depend on how a reduction groups them.
 *
 * Arithmetic.  Only IEEE +, −, × and comparisons in a fixed order
 * (-ffp-contract=off on both sides):
 *     cost     c = (double)k·p + d
 *     reduced  ((minv + c) − u[i]) − v[j]               (scipy's order)
 *     duals    δ = minv − sh[j];  u[row[j]] += δ;  v[j] −= δ   for every
 *              visited assigned column j;  u[r] = minv for the new row r.
 * The validator admits 0 ≤ p ≤ 1e30 and 0 ≤ d ≤ 1e15, m ≤ 1024: every cost
 * is finite (< 1.1e33), so is every dual and distance, and each search meets
 * a frontier after at most r + 1 steps.
 *
 * The optimum's cost is unique; the assignment is not, even for generic
 * costs: workers of one type are identical columns.
 */
#ifndef SW_ALLOX_H
#define SW_ALLOX_H

#include <stddef.h>

#include "sw_arith.h"

#define SW_ALLOX_MAX_TYPES 8
#define SW_ALLOX_MAX_JOBS 1024    /* rows; positions fit int16 */
#define SW_ALLOX_MAX_WORKERS 1024 /* worker index fits 10 bits */
#define SW_ALLOX_PROC_MAX 1e30
#define SW_ALLOX_DELAY_MAX 1e15
#define SW_ALLOX_INF_BITS 0x7FF0000000000000ull
#define SW_ALLOX_NO_SLOT 0x7FFFFFFF
#define SW_ALLOX_TYPE_SHIFT 10

/* Column state, one entry per slot (cap = m + n), and the row duals.  25
 * bytes a slot and 8 a row: 59,392 bytes at m = n = 1024. */
typedef struct {
    double* v;     /* [cap] column dual                                     */
    double* sh;    /* [cap] tentative distance of the running search        */
    double* u;     /* [m]   row dual; at the end the job's cost term        */
    int16_t* row;  /* [cap] owner row, −1 for a frontier                    */
    int16_t* from; /* [cap] the visited column whose row relaxed this one, −1: the new row */
    int16_t* pos;  /* [cap] position k ≥ 1                                  */
    int16_t* wt;   /* [cap] worker | type << 10                             */
    uint8_t* seen; /* [cap] visited by the running search                   */
} sw_allox_cols;

SW_HD size_t sw_allox_bytes(int32_t m, int32_t n) {
    const size_t cap = (size_t)m + (size_t)n;
    return (cap * 25 + (size_t)m * 8 + 7) & ~(size_t)7;
}

SW_HD sw_allox_cols sw_allox_layout(void* base, int32_t m, int32_t n) {
    const size_t cap = (size_t)m + (size_t)n;
    sw_allox_cols c;
    c.v = (double*)base;
    c.sh = c.v + cap;
    c.u = c.sh + cap;
    c.row = (int16_t*)(c.u + m);
    c.from = c.row + cap;
    c.pos = c.from + cap;
    c.wt = c.pos + cap;
    c.seen = (uint8_t*)(c.wt + cap);
    return c;
}

/* type of free worker j, type-major: the first free[0] workers are type 0 … */
SW_HD int32_t sw_allox_worker_type(const int32_t* free_workers, int32_t num_types, int32_t j) {
    int32_t t = 0, end = free_workers[0];
    while (t + 1 < num_types && j >= end) end += free_workers[++t];
    return t;
}

/* slot j < n at the start: position 1 of worker j */
SW_HD void sw_allox_init_frontier(const sw_allox_cols* c, int32_t j, int32_t type) {
    c->v[j] = 0.0;
    c->row[j] = -1;
    c->pos[j] = 1;
    c->wt[j] = (int16_t)(j | (type << SW_ALLOX_TYPE_SHIFT));
}

SW_HD double sw_allox_cost(int32_t k, double p, double d) { return (double)k * p + d; }

/* a before b in a search step: value, then the lower slot */
SW_HD int sw_allox_less(double va, int32_t sa, double vb, int32_t sb) {
    return va < vb || (va == vb && sa < sb);
}

/* Relax unvisited slot s from row i (duals ui, processing time p on the
 * slot's type, delay d), reached through visited column `via` at distance
 * minv; returns the slot's tentative distance. */
SW_HD double sw_allox_relax(const sw_allox_cols* c, int32_t s, double minv, double ui, double p,
                            double d, int32_t via) {
    const double r = ((minv + sw_allox_cost(c->pos[s], p, d)) - ui) - c->v[s];
    double sh = c->sh[s];
    if (r < sh) {
        sh = r;
        c->sh[s] = r;
        c->from[s] = (int16_t)via;
    }
    return sh;
}

/* the dual update of a visited assigned slot s after a search that ended at
 * distance minv */
SW_HD void sw_allox_dual(const sw_allox_cols* c, int32_t s, double minv) {
    const double delta = minv - c->sh[s];
    const int32_t i = c->row[s];
    c->u[i] = c->u[i] + delta;
    c->v[s] = c->v[s] - delta;
}

/* The augmentation of row r, whose search ended at frontier `sink` (< n): the
 * sink becomes slot n + r, the worker's frontier moves one position up, and
 * the owners shift back along the path (≤ r + 1 columns). */
SW_HD void sw_allox_augment(const sw_allox_cols* c, int32_t n, int32_t r, int32_t sink) {
    const int32_t s = n + r;
    c->v[s] = 0.0;
    c->pos[s] = c->pos[sink];
    c->wt[s] = c->wt[sink];
    c->pos[sink] = (int16_t)(c->pos[sink] + 1);
    int32_t j = s, f = c->from[sink];
    for (int32_t it = 0; f >= 0 && it <= r; ++it) {
        c->row[j] = c->row[f];
        j = f;
        f = c->from[j];
    }
    c->row[j] = (int16_t)r;
}

/* The result of assigned slot s (≥ n) once every row is placed: its job's
 * worker and position, the job's cost term into u, and worker_first when the
 * slot is the highest position of its worker (the frontier sits one above). */
SW_HD void sw_allox_emit(const sw_allox_cols* c, int32_t s, int32_t num_types, const double* p,
                         const double* d, int32_t* job_worker, int32_t* job_position,
                         int32_t* worker_first) {
    const int32_t i = c->row[s], k = c->pos[s];
    const int32_t w = c->wt[s] & ((1 << SW_ALLOX_TYPE_SHIFT) - 1), t = c->wt[s] >> SW_ALLOX_TYPE_SHIFT;
    job_worker[i] = w;
    job_position[i] = k;
    c->u[i] = sw_allox_cost(k, p[(size_t)i * (size_t)num_types + (size_t)t], d[i]);
    if (k + 1 == c->pos[w]) worker_first[w] = i;
}

#endif /* SW_ALLOX_H */
