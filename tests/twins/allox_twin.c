/*
 * tests/twins/allox_twin.c — TEST INFRASTRUCTURE: CPU bit-exact twin of the
 * AlloX assignment kernel (shockwave-replication_amd/csrc/sw_allox.hip).
 *
 * The same searches in the same order with the step functions of sw_allox.h
 * (-ffp-contract=off): where the kernel scans the slots in parallel and
 * reduces the arg-min, the twin scans them left to right — the order
 * (distance, slot) is total, so both find the same slot.  It is pinned
 * against scipy.optimize.linear_sum_assignment on the reference's dense
 * matrix by tests/test_allox.py (tests/allox_ref.py).  Never linked into the
 * product.
 */
#include <stdint.h>

#include "../../shockwave-replication_amd/csrc/sw_allox.h"

/* scratch: sw_allox_bytes(m, n) bytes, 8-aligned.  steps (optional) receives
 * the number of search steps.  Returns 0, 1 when the sizes exceed the
 * kernel's caps, 2 if a search found no column (non-finite costs). */
int allox_twin_assign(int32_t m, int32_t num_types, const int32_t* free_workers, const double* p,
                      const double* d, int32_t* job_worker, int32_t* job_position,
                      int32_t* worker_first, double* cost, void* scratch, int64_t* steps) {
    int64_t n64 = 0;
    for (int32_t t = 0; t < num_types; ++t) n64 += free_workers[t];
    if (steps) *steps = 0;
    if (cost) *cost = 0.0;
    if (m > SW_ALLOX_MAX_JOBS || n64 > SW_ALLOX_MAX_WORKERS) return 1;
    const int32_t n = (int32_t)n64;
    for (int32_t i = 0; i < m; ++i) { job_worker[i] = -1; job_position[i] = 0; }
    for (int32_t j = 0; j < n; ++j) worker_first[j] = -1;
    if (m <= 0 || n <= 0) return 0;

    const sw_allox_cols c = sw_allox_layout(scratch, m, n);
    const double inf = sw_from_bits(SW_ALLOX_INF_BITS);
    int64_t nsteps = 0;
    for (int32_t j = 0; j < n; ++j) sw_allox_init_frontier(&c, j, sw_allox_worker_type(free_workers, num_types, j));

    for (int32_t r = 0; r < m; ++r) {
        const int32_t ncol = n + r;
        for (int32_t s = 0; s < ncol; ++s) { c.sh[s] = inf; c.seen[s] = 0; }
        double minv = 0.0;
        int32_t i = r, via = -1, sink = -1;
        c.u[r] = 0.0;
        for (int32_t it = 0; it <= r && sink < 0; ++it) {
            const double ui = c.u[i], di = d[i];
            const double* pi = p + (size_t)i * (size_t)num_types;
            double bv = inf;
            int32_t bs = SW_ALLOX_NO_SLOT;
            for (int32_t s = 0; s < ncol; ++s) {
                if (c.seen[s]) continue;
                const double sh = sw_allox_relax(&c, s, minv, ui, pi[c.wt[s] >> SW_ALLOX_TYPE_SHIFT], di, via);
                if (sw_allox_less(sh, s, bv, bs)) { bv = sh; bs = s; }
            }
            ++nsteps;
            if (bs >= ncol) return 2;
            minv = bv;
            c.seen[bs] = 1;
            if (bs < n) sink = bs;
            else { i = c.row[bs]; via = bs; }
        }
        if (sink < 0) return 2;
        for (int32_t s = n; s < ncol; ++s)
            if (c.seen[s]) sw_allox_dual(&c, s, minv);
        c.u[r] = minv;
        sw_allox_augment(&c, n, r, sink);
    }

    for (int32_t s = n; s < n + m; ++s)
        sw_allox_emit(&c, s, num_types, p, d, job_worker, job_position, worker_first);
    double total = 0.0;
    for (int32_t i = 0; i < m; ++i) total = total + c.u[i];
    if (cost) *cost = total;
    if (steps) *steps = nsteps;
    return 0;
}
