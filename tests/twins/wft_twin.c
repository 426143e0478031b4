/*
 * tests/twins/wft_twin.c — TEST INFRASTRUCTURE: CPU bit-exact twin of the
 * water-filling MaxMinFairness kernel over worker types
 * (shockwave-replication_amd/csrc/sw_wf_types.hip, sw_wf_allocate_types).
 *
 * The same passes over the jobs in the same order, the per-job and the
 * one-thread arithmetic of sw_wf_types.h and sw_mmf_ipm.h (-ffp-contract=off),
 * and every sum over the jobs by the deterministic tree (twin_detsum.h), so it
 * returns the bits the GPU returns.  It is pinned against an independent
 * computation (tests/wf_types_ref.py: the stage loop on HiGHS, one LP per
 * unfrozen job for the bottleneck test) by tests/test_wf_types.py.  Never
 * linked into the product.
 */
#include <stdint.h>
#include <stdlib.h>

#include "../../shockwave-replication_amd/csrc/sw_arith.h"
#include "../../shockwave-replication_amd/csrc/sw_wf_types.h"
#include "twin_ipm.h"

/* the call's normalisation, as the library's host code finds it */
int32_t wft_twin_shift(int32_t m, int32_t n, const int32_t* workers, const double* coef) {
    double cmax = 0.0;
    for (int32_t j = 0; j < m; ++j)
        for (int32_t k = 0; k < n; ++k)
            if (workers[k] > 0 && coef[(size_t)j * n + k] > cmax) cmax = coef[(size_t)j * n + k];
    return sw_lp_shift(cmax);
}

/* result[4] = last level, Newton steps, stages, flags; levels[m] the jobs'
 * final levels; froze[m] (may be NULL) the 1-based stage each job froze in;
 * stats (may be NULL) receives, stage-major, the statistic of every job that
 * was unfrozen when stage s began (−1.0 for the others) for s < stat_stages.
 * Returns 0, SW_IPM_CAP, SW_IPM_BREAK or SW_WFT_STALL. */
int wft_twin_allocate_stats(int32_t m, int32_t n, const int32_t* workers, const int32_t* sf, const double* coef,
                            double* x, double* levels, double* result, int32_t* froze, double* stats,
                            int32_t stat_stages) {
    sw_ipm_glob G;
    sw_ipm_glob* g = &G;
    sw_wft_glob Q;
    sw_wft_glob* q = &Q;
    double sums[SW_IPM_NRED], mx[SW_IPM_NMAX];
    for (int i = 0; i < 4; ++i) result[i] = 0.0;
    if (m <= 0) return 0;
    sw_ipm_setup(g, m, n, workers);
    const int32_t na = g->na;
    if (na == 0) { /* no type has workers */
        for (size_t i = 0; i < (size_t)m * n; ++i) x[i] = 0.0;
        for (int32_t j = 0; j < m; ++j) levels[j] = 0.0;
        if (froze)
            for (int32_t j = 0; j < m; ++j) froze[j] = 0;
        return 0;
    }
    double* ws = (double*)malloc(sizeof(double) * (size_t)SW_WFT_FIELDS(na) * m);
    red R;
    R.m = m;
    R.val = (double*)malloc(sizeof(double) * (size_t)SW_IPM_NRED * m);
    if (!ws || !R.val) { free(ws); free(R.val); return -1; }
    sw_ipm_job J = {ws, m, 0, na, 0.0};

    sw_wft_begin(q, m, wft_twin_shift(m, n, workers, coef));
    EACH_JOB sw_wft_job_begin(&J);

    int kept = 0;
    while (sw_wft_next(q) || sw_wft_repeat(q)) {
        if (q->rep == 1 && !kept) {
            kept = 1;
            EACH_JOB {
                sw_wft_job_keep(g, q, &J, sums);
                PUT(na);
            }
            red_sums(&R, na, sums);
            sw_wft_glob_keep(g, q, sums);
        }
        sw_ipm_setup(g, m, n, workers);
        sw_wft_setup(g, q);
        red_begin(&R);
        EACH_JOB {
            sw_wft_job_load(g, q, &J, coef + (size_t)J.j * n, sums, mx);
            PUT(2);
            red_max(&R, mx, 1);
        }
        red_sums(&R, 2, sums);
        sw_ipm_glob_load(g, sums, R.mx);

        twin_ipm_start_tail(g, R, J, sf, m);

        twin_ipm_solve(g, R, J, sf, m);
        if (g->status != SW_IPM_OK) {
            if (sw_wft_retry(g, q) == 1) continue;
            break;
        }
        /* every job has a positive coefficient on a type with workers and a stage has an
         * unfrozen job, so the level is a variable and both path points were reached */
        red_begin(&R);
        EACH_JOB {
            sw_ipm_job_final(g, &J, sums, mx);
            sums[na] = sw_wft_job_lift(&J);
            PUT(na + 1);
            red_max(&R, mx, 1);
        }
        red_sums(&R, na + 1, sums);
        sw_ipm_glob_final(g, sums, R.mx);
        sw_wft_glob_level(g, q, sums[na]);

        if (q->rep == 1) {
            red_begin(&R);
            EACH_JOB {
                sw_wft_job_blend(g, q, &J, sums, mx);
                PUT(na);
                red_max(&R, mx, 1);
            }
            red_sums(&R, na, sums);
            sw_wft_glob_blend(g, q, sums, R.mx);
            break;
        }
        if (stats && q->stage < stat_stages)
            EACH_JOB stats[(size_t)q->stage * m + J.j] =
                SW_IPM_Q(&J, SW_WFT_FROZE) != 0.0 ? -1.0 : sw_wft_stat(g, &J);
        red_begin(&R);
        EACH_JOB {
            sw_wft_job_classify(g, q, &J, sums, mx);
            PUT(1);
            red_max(&R, mx, 2);
        }
        red_sums(&R, 1, sums);
        sw_wft_feed(q, sums[0], R.mx);
    }
    EACH_JOB {
        sw_wft_job_emit(g, q, &J, x + (size_t)J.j * n);
        levels[J.j] = sw_wft_job_level(q, &J);
        if (froze) froze[J.j] = (int32_t)SW_IPM_Q(&J, SW_WFT_FROZE);
    }
    sw_wft_result(q, result);
    free(ws);
    free(R.val);
    return q->status;
}

int wft_twin_allocate(int32_t m, int32_t n, const int32_t* workers, const int32_t* sf, const double* coef, double* x,
                      double* levels, double* result) {
    return wft_twin_allocate_stats(m, n, workers, sf, coef, x, levels, result, 0, 0, 0);
}

/* the headers' constants, for the tests */
double wft_twin_thresh(void) { return SW_WFT_THRESH; }
double wft_twin_gap_lo(void) { return SW_WFT_GAP_LO; }
double wft_twin_gap_hi(void) { return SW_WFT_GAP_HI; }
int32_t wft_twin_max_jobs(void) { return SW_IPM_MAX_JOBS; }
int32_t wft_twin_max_types(void) { return SW_IPM_MAX_TYPES; }
int32_t wft_twin_flag_one(void) { return SW_WFT_ONE; }
int32_t wft_twin_flag_near(void) { return SW_WFT_NEAR; }
int32_t wft_twin_flag_coarse(void) { return SW_WFT_COARSE; }
int32_t wft_twin_status_stall(void) { return SW_WFT_STALL; }
