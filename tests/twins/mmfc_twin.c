/*
 * tests/twins/mmfc_twin.c — TEST INFRASTRUCTURE: CPU bit-exact twin of the
 * centred MaxMinFairness kernel over worker types
 * (shockwave-replication_amd/csrc/sw_mmf_ipm.hip, sw_mmf_allocate_types_centred).
 *
 * The same passes over the jobs in the same order, the per-job and the
 * one-thread arithmetic of sw_mmf_ipm.h (-ffp-contract=off), and every sum over
 * the jobs by the deterministic tree (twin_detsum.h), so it returns the bits
 * the GPU returns.  It is pinned against an independent computation of the
 * face's analytic centre by tests/test_mmf_centre.py (tests/mmf_centre_ref.py).
 * Never linked into the product.
 */
#include <stdint.h>
#include <stdlib.h>

#include "../../shockwave-replication_amd/csrc/sw_arith.h"
#include "../../shockwave-replication_amd/csrc/sw_mmf_ipm.h"
#include "twin_ipm.h"

/* the shift of the normalisation: from the largest coefficient on a type with
 * workers (the host does this for the kernel while it validates) */
int32_t mmfc_twin_shift(int32_t m, int32_t n, const int32_t* workers, const double* coef) {
    double cmax = 0.0;
    for (int32_t j = 0; j < m; ++j)
        for (int32_t k = 0; k < n; ++k)
            if (workers[k] > 0 && coef[(size_t)j * n + k] > cmax) cmax = coef[(size_t)j * n + k];
    return sw_lp_shift(cmax);
}

/* level[0] = t*, level[1] = Newton steps; returns 0, SW_IPM_CAP or SW_IPM_BREAK */
int mmfc_twin_allocate(int32_t m, int32_t n, const int32_t* workers, const int32_t* sf, const double* coef,
                       double* x, double* level) {
    sw_ipm_glob G;
    sw_ipm_glob* g = &G;
    double sums[SW_IPM_NRED], mx[SW_IPM_NMAX];
    level[0] = 0.0;
    level[1] = 0.0;
    if (m <= 0) return 0;
    sw_ipm_setup(g, m, n, workers);
    const int32_t na = g->na;
    if (na == 0) {
        for (size_t i = 0; i < (size_t)m * n; ++i) x[i] = 0.0;
        return 0;
    }
    const int32_t shift = mmfc_twin_shift(m, n, workers, coef);
    double* ws = (double*)malloc(sizeof(double) * (size_t)SW_IPM_FIELDS(na) * m);
    red R;
    R.m = m;
    R.val = (double*)malloc(sizeof(double) * (size_t)SW_IPM_NRED * m);
    if (!ws || !R.val) { free(ws); free(R.val); return -1; }
    sw_ipm_job J = {ws, m, 0, na, 0.0};

    red_begin(&R);
    EACH_JOB {
        sw_ipm_job_load(g, &J, coef + (size_t)J.j * n, shift, sums, mx);
        PUT(2);
        red_max(&R, mx, 1);
    }
    red_sums(&R, 2, sums);
    sw_ipm_glob_load(g, sums, R.mx);

    twin_ipm_start_tail(g, R, J, sf, m);

    twin_ipm_solve(g, R, J, sf, m);
    if (sw_ipm_two_points(g)) {
        red_begin(&R);
        EACH_JOB {
            sw_ipm_job_final(g, &J, sums, mx);
            PUT(na);
            red_max(&R, mx, 1);
        }
        red_sums(&R, na, sums);
        sw_ipm_glob_final(g, sums, R.mx);
    }
    EACH_JOB sw_ipm_job_emit(g, &J, x + (size_t)J.j * n);
    level[0] = sw_ipm_level(g, shift);
    level[1] = (double)g->iters;
    free(ws);
    free(R.val);
    return g->status;
}

/* the header's constants, for the tests */
int32_t mmfc_twin_max_iters(void) { return SW_IPM_MAX_ITERS; }
int32_t mmfc_twin_max_jobs(void) { return SW_IPM_MAX_JOBS; }
