/*
 * tests/twins/mtdt_twin.c — TEST INFRASTRUCTURE: CPU bit-exact twin of the
 * MinTotalDuration kernel over worker types
 * (shockwave-replication_amd/csrc/sw_mtd_types.hip, sw_mtd_allocate_types).
 *
 * The same passes over the jobs in the same order, the per-job and the
 * one-thread arithmetic of sw_mtd_types.h and sw_mmf_ipm.h (-ffp-contract=off),
 * and every sum over the jobs by the deterministic tree (twin_detsum.h), so it
 * returns the bits the GPU returns.  It is pinned against an independent
 * computation (tests/mtd_types_ref.py: HiGHS, a Python replay of the search, a
 * null-space Newton centre) by tests/test_mtd_types.py.  Never linked into the
 * product.
 */
#include <stdint.h>
#include <stdlib.h>

#include "../../shockwave-replication_amd/csrc/sw_arith.h"
#include "../../shockwave-replication_amd/csrc/sw_mtd_types.h"
#include "twin_ipm.h"

/* the shift of the normalisation (the host does this for the kernel while it
 * validates) */
int32_t mtdt_twin_shift(int32_t m, int32_t n, const int32_t* workers, const double* thr, const double* steps) {
    double cmin = 0.0;
    for (int32_t j = 0; j < m; ++j)
        if (steps[j] > 0.0) cmin = sw_mtdt_shift_take(cmin, sw_mtdt_rowmax(n, workers, thr + (size_t)j * n, steps[j]));
    return sw_lp_shift(cmin);
}

/* result[4] = T, t*, Newton steps, flags; returns 0, SW_IPM_CAP or SW_IPM_BREAK */
int mtdt_twin_allocate(int32_t m, int32_t n, const int32_t* workers, const int32_t* sf, const double* thr,
                       const double* steps, double* x, double* result) {
    sw_ipm_glob G;
    sw_ipm_glob* g = &G;
    sw_mtdt_glob Q;
    sw_mtdt_glob* q = &Q;
    double sums[SW_IPM_NRED], mx[SW_IPM_NMAX];
    for (int i = 0; i < 4; ++i) result[i] = 0.0;
    if (m <= 0) return 0;
    sw_ipm_setup(g, m, n, workers);
    sw_mtdt_setup(q);
    const int32_t na = g->na;
    if (na == 0) {
        for (size_t i = 0; i < (size_t)m * n; ++i) x[i] = 0.0;
        q->flags = SW_MTDT_IDLE;
        sw_mtdt_search(q, 0.0, 1);
        sw_mtdt_result(g, q, result);
        return 0;
    }
    const int32_t shift = mtdt_twin_shift(m, n, workers, thr, steps);
    double* ws = (double*)malloc(sizeof(double) * (size_t)SW_IPM_FIELDS(na) * m);
    red R;
    R.m = m;
    R.val = (double*)malloc(sizeof(double) * (size_t)SW_IPM_NRED * m);
    if (!ws || !R.val) { free(ws); free(R.val); return -1; }
    sw_ipm_job J = {ws, m, 0, na, 0.0};

    red_begin(&R);
    EACH_JOB {
        sw_mtdt_job_load(g, &J, thr + (size_t)J.j * n, steps[J.j], shift, sums, mx);
        PUT(3);
        red_max(&R, mx, 1);
    }
    red_sums(&R, 3, sums);
    sw_mtdt_glob_load(g, q, sums, R.mx);

    twin_ipm_start_tail(g, R, J, sf, m);

    for (int phase = 0; phase < 2; ++phase) {
        twin_ipm_solve(g, R, J, sf, m);
        if (g->status != SW_IPM_OK || !g->has_t) break;
        red_begin(&R);
        EACH_JOB {
            sw_ipm_job_final(g, &J, sums, mx);
            PUT(na);
            red_max(&R, mx, 1);
        }
        red_sums(&R, na, sums);
        sw_ipm_glob_final(g, sums, R.mx);
        if (!sw_mtdt_glob_switch(g, q, shift)) break;
        EACH_JOB sw_mtdt_job_switch(g, &J);
    }
    EACH_JOB sw_ipm_job_emit(g, &J, x + (size_t)J.j * n);
    sw_mtdt_result(g, q, result);
    free(ws);
    free(R.val);
    return g->status;
}

/* the headers' constants, for the tests */
double mtdt_twin_thin(void) { return SW_MTDT_THIN; }
int32_t mtdt_twin_max_iters(void) { return SW_IPM_MAX_ITERS; }
int32_t mtdt_twin_max_jobs(void) { return SW_IPM_MAX_JOBS; }
int32_t mtdt_twin_max_types(void) { return SW_IPM_MAX_TYPES; }
double mtdt_twin_full_time_max(void) { return SW_MTD_FULL_TIME_MAX; }
int32_t mtdt_twin_flag_idle(void) { return SW_MTDT_IDLE; }
int32_t mtdt_twin_flag_thin(void) { return SW_MTDT_THIN_FLAG; }
