/*
 * tests/twins/mstt_twin.c — TEST INFRASTRUCTURE: CPU bit-exact twin of the
 * max-sum-throughput kernel over worker types
 * (shockwave-replication_amd/csrc/sw_mst_types.hip, sw_mst_allocate_types).
 *
 * The same job order, the one-thread steps of sw_mst_types.h (the rounds of
 * every sink from the distances of the round before, the push, the O(n) row
 * update of a created arc), a stale row as a loop over the jobs with the
 * kernel's lexicographic maximum (its result does not depend on the order), and
 * the objective by the deterministic tree (twin_detsum.h), so it returns the
 * bits the GPU returns.  It is held to its own optimality certificate and to
 * HiGHS by tests/test_mst_types.py.  Never linked into the product.
 */
#include <stdint.h>
#include <stdlib.h>

#include "../../shockwave-replication_amd/csrc/sw_arith.h"
#include "../../shockwave-replication_amd/csrc/sw_mst_types.h"
#include "twin_detsum.h"

static void row(sw_mstt_state* s, const double* D, const int32_t* y, int32_t k) {
    const int32_t n = s->n;
    for (int32_t l = 0; l <= n; ++l) {
        if (l == k) continue;
        double best = sw_mstt_neg_inf();
        int32_t bi = SW_MSTT_NO_JOB;
        for (int32_t i = 0; i < s->m; ++i) {
            if (y[(size_t)i * n + k] <= 0) continue;
            const double c = sw_mstt_d(D, n, i, l) - sw_mstt_d(D, n, i, k);
            if (sw_mstt_better(c, i, best, bi)) { best = c; bi = i; }
        }
        s->g[k][l] = best;
        s->arg[k][l] = bi;
    }
    ++s->rows;
}

/* result[4] = objective, augmentations, row recomputations, flags; y (optional,
 * [m][n]) receives the integer flow; returns 0 or SW_MSTT_CAP */
int mstt_twin_allocate(int32_t m, int32_t n, const int32_t* workers, const int32_t* sf, const double* w, double* x,
                       double* prices, double* result, int32_t* flow) {
    sw_mstt_state S;
    sw_mstt_state* s = &S;
    for (int i = 0; i < 4; ++i) result[i] = 0.0;
    for (int32_t k = 0; k < n; ++k) prices[k] = 0.0;
    if (m <= 0) return 0;
    const size_t cells = (size_t)m * n;
    double* D = (double*)malloc(sizeof(double) * cells);
    int32_t* y = (int32_t*)calloc(cells, sizeof(int32_t));
    double* v = (double*)malloc(sizeof(double) * (size_t)m);
    if (!D || !y || !v) { free(D); free(y); free(v); return -1; }
    for (size_t c = 0; c < cells; ++c) D[c] = sw_mstt_density(w[c], (double)sf[c / n]);
    sw_mstt_setup(s, m, n, workers);

    for (int32_t j = 0; j < m && s->status == SW_MSTT_OK; ++j) {
        s->rem = sf[j];
        while (s->rem > 0) {
            for (int32_t l = 0; l <= n; ++l) sw_mstt_start(s, D, j, l);
            int buf = 0;
            int32_t r = 0;
            while (r < n) {
                int changed = 0;
                for (int32_t l = 0; l <= n; ++l) changed |= sw_mstt_relax(s, l, r, buf);
                buf ^= 1;
                ++r;
                if (!changed) break;
            }
            sw_mstt_push(s, y, j, r, buf);
            if (s->status != SW_MSTT_OK) break;
            for (int32_t a = 0; a < s->nnew; ++a)
                for (int32_t l = 0; l <= n; ++l) sw_mstt_arc_add(s, D, s->new_job[a], s->new_type[a], l);
            for (int32_t k = 0; k < n; ++k)
                if ((s->dirty >> k) & 1) row(s, D, y, k);
        }
    }

    if (s->status == SW_MSTT_OK) {
        for (int32_t l = 0; l <= n; ++l) sw_mstt_dual_start(s, l);
        int buf = 0;
        for (int32_t r = 0; r < n; ++r) {
            int changed = 0;
            for (int32_t k = 0; k <= n; ++k) changed |= sw_mstt_dual_relax(s, k, buf);
            buf ^= 1;
            if (!changed) break;
        }
        for (int32_t k = 0; k < n; ++k) {
            double cm = sw_mstt_neg_inf();
            for (int32_t i = 0; i < m; ++i)
                if (D[(size_t)i * n + k] > cm) cm = D[(size_t)i * n + k];
            prices[k] = sw_mstt_price(s->dist[buf][k], cm);
        }
    }
    for (int32_t i = 0; i < m; ++i)
        v[i] = sw_mstt_emit(n, y + (size_t)i * n, (double)sf[i], w + (size_t)i * n, x + (size_t)i * n);
    sw_mstt_result(s, workers, detsum(v, m), result);
    if (flow)
        for (size_t c = 0; c < cells; ++c) flow[c] = y[c];
    free(D);
    free(y);
    free(v);
    return s->status;
}

/* the header's constants, for the tests */
int32_t mstt_twin_cap_mult(void) { return SW_MSTT_CAP_MULT; }
int32_t mstt_twin_lds_cells(void) { return SW_MSTT_LDS_CELLS; }
int32_t mstt_twin_flag_unplaced(void) { return SW_MSTT_UNPLACED; }
int32_t mstt_twin_flag_slack(void) { return SW_MSTT_SLACK; }
