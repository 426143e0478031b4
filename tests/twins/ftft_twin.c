/*
 * tests/twins/ftft_twin.c — TEST INFRASTRUCTURE: CPU bit-exact twin of the
 * FinishTimeFairness kernel over worker types
 * (shockwave-replication_amd/csrc/sw_ftf_types.hip, sw_ftf_allocate_types).
 *
 * The same passes over the jobs in the same order, the per-job and the
 * one-thread arithmetic of sw_ftf_types.h and sw_mmf_ipm.h (-ffp-contract=off),
 * and every sum over the jobs by the deterministic tree (twin_detsum.h), so it
 * returns the bits the GPU returns.  It is pinned against an independent
 * computation (tests/ftf_types_ref.py: a bracketing search over ρ on HiGHS's
 * level, a null-space Newton centre) by tests/test_ftf_types.py.  Never linked into the
 * product.
 */
#include <stdint.h>
#include <stdlib.h>

#include "../../shockwave-replication_amd/csrc/sw_arith.h"
#include "../../shockwave-replication_amd/csrc/sw_ftf_types.h"
#include "twin_ipm.h"

/* result[5] = ρ*, t, Newton steps, level solves, flags; returns 0, SW_IPM_CAP,
 * SW_IPM_BREAK or SW_FTFT_CAP */
int ftft_twin_allocate(int32_t m, int32_t n, const int32_t* workers, const int32_t* sf, const double* thr,
                       const double* steps, const double* el, const double* ex, double* x, double* result) {
    sw_ipm_glob G;
    sw_ipm_glob* g = &G;
    sw_ftft_glob Q;
    sw_ftft_glob* q = &Q;
    double sums[SW_IPM_NRED], mx[SW_IPM_NMAX];
    for (int i = 0; i < 5; ++i) result[i] = 0.0;
    if (m <= 0) return 0;
    sw_ipm_setup(g, m, n, workers);
    const int32_t na = g->na;
    double* ws = (double*)malloc(sizeof(double) * (size_t)SW_IPM_FIELDS(na > 0 ? na : 1) * m);
    red R;
    R.m = m;
    R.val = (double*)malloc(sizeof(double) * (size_t)SW_IPM_NRED * m);
    if (!ws || !R.val) { free(ws); free(R.val); return -1; }
    sw_ipm_job J = {ws, m, 0, na, 0.0};
#define JOB_IN thr + (size_t)J.j * n, steps[J.j], el[J.j], ex[J.j]

    /* ρ_box and the aggregate start */
    red_begin(&R);
    EACH_JOB {
        sw_ftft_job_box(g, JOB_IN, sums, mx);
        PUT(1);
        red_max(&R, mx, 1);
    }
    red_sums(&R, 1, sums);
    sw_ftft_glob_box(g, q, sums, R.mx);
    if (na == 0) { /* no type has workers, so (validated) no job is live */
        for (size_t i = 0; i < (size_t)m * n; ++i) x[i] = 0.0;
        sw_ftft_result(q, result);
        free(ws);
        free(R.val);
        return 0;
    }
    while (sw_ftft_start_next(q)) {
        EACH_JOB R.val[J.j] = sw_ftft_job_cap(g, q, J.sf, JOB_IN);
        red_sums(&R, 1, sums);
        sw_ftft_start_feed(q, sums[0]);
    }

    for (;;) {
        if (q->centring) {
            EACH_JOB sw_mtdt_job_switch(g, &J);
        } else {
        if (!sw_ftft_next(&q->s, &q->rho)) break;
        sw_ipm_setup(g, m, n, workers);
        red_begin(&R);
        EACH_JOB {
            mx[0] = sw_ftft_job_rowmax(g, q, JOB_IN);
            red_max(&R, mx, 1);
        }
        sw_ftft_glob_shift(q, R.mx);

        red_begin(&R);
        EACH_JOB {
            sw_ftft_job_load(g, q, &J, JOB_IN, sums, mx);
            PUT(2);
            red_max(&R, mx, 1);
        }
        red_sums(&R, 2, sums);
        sw_ftft_glob_load(g, q, sums, R.mx);

        twin_ipm_start_tail(g, R, J, sf, m);
        }

        twin_ipm_solve(g, R, J, sf, m);
        if (g->status != SW_IPM_OK) break;
        if (!g->has_t) {
            sw_ftft_glob_free(g, q);
            break;
        }
        red_begin(&R);
        EACH_JOB {
            sw_ipm_job_final(g, &J, sums, mx);
            sums[na] = sw_ftft_job_slope(g, q, &J, JOB_IN);
            PUT(na + 1);
            red_max(&R, mx, 1);
        }
        red_sums(&R, na + 1, sums);
        sw_ipm_glob_final(g, sums, R.mx);
        sw_ftft_glob_feed(g, q, sums[na]);
        sw_ftft_glob_switch(g, q);
    }
    EACH_JOB sw_ipm_job_emit(g, &J, x + (size_t)J.j * n);
    sw_ftft_result(q, result);
    free(ws);
    free(R.val);
    return g->status != SW_IPM_OK ? g->status : q->s.status;
}

/* the headers' constants, for the tests */
double ftft_twin_tol(void) { return SW_FTFT_TOL; }
int32_t ftft_twin_max_solves(void) { return SW_FTFT_MAX_SOLVES; }
int32_t ftft_twin_max_jobs(void) { return SW_IPM_MAX_JOBS; }
int32_t ftft_twin_max_types(void) { return SW_IPM_MAX_TYPES; }
int32_t ftft_twin_flag_box(void) { return SW_FTFT_BOX; }
int32_t ftft_twin_flag_idle(void) { return SW_FTFT_IDLE; }
int32_t ftft_twin_flag_safe(void) { return SW_FTFT_SAFE; }
int32_t ftft_twin_status_cap(void) { return SW_FTFT_CAP; }
