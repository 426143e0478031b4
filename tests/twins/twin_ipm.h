/*
 * tests/twins/twin_ipm.h — TEST INFRASTRUCTURE: what the CPU twins of the four
 * kernels of the interior-point engine (mmfc_twin.c, mtdt_twin.c, ftft_twin.c,
 * wft_twin.c) share: the reduction of a pass over the jobs, the engine's start
 * after a twin's own load pass, and the Newton loop, the counterparts of
 * ipm_start_tail and ipm_solve in csrc/sw_mmf_ipm_dev.h.  Include it after the
 * policy's arithmetic header.  Never linked into the product.
 */
#ifndef TWIN_IPM_H
#define TWIN_IPM_H

#include <stdint.h>
#include <stdlib.h>

#include "../../shockwave-replication_amd/csrc/sw_mmf_ipm.h"
#include "twin_detsum.h"

#define NEG_HUGE (-1.7976931348623157e308)

/* one pass's values: the jobs' summands, summed by the deterministic tree, and
 * the running maxima */
typedef struct {
    int32_t m;
    double* val; /* [SW_IPM_NRED][m] */
    double mx[SW_IPM_NMAX];
} red;

static void red_begin(red* r) {
    for (int i = 0; i < SW_IPM_NMAX; ++i) r->mx[i] = NEG_HUGE;
}
static void red_max(red* r, const double* v, int cnt) {
    for (int i = 0; i < cnt; ++i) r->mx[i] = v[i] > r->mx[i] ? v[i] : r->mx[i];
}
static void red_sums(const red* r, int cnt, double* out) {
    for (int i = 0; i < cnt; ++i) out[i] = detsum(r->val + (size_t)i * r->m, r->m);
}

/* With `sw_ipm_job J`, `red R`, `const int32_t* sf`, `int32_t m` and
 * `double sums[SW_IPM_NRED]` in scope: a pass over the jobs, and the job's
 * summands into the reduction.  The two functions below take R and J by value
 * for these: the summands R.val and the workspace J.ws are the caller's, R.mx,
 * J.j and J.sf are scratch that every pass sets before it reads them. */
#define EACH_JOB for (J.j = 0; J.j < m; ++J.j) if ((J.sf = (double)sf[J.j]), 1)
#define PUT(cnt) for (int i_ = 0; i_ < (cnt); ++i_) R.val[(size_t)i_ * m + J.j] = sums[i_]

/* x = θ and the level's start, then the slacks and a dual-feasible start */
static void twin_ipm_start_tail(sw_ipm_glob* g, red R, sw_ipm_job J, const int32_t* sf, int32_t m) {
    double mx[SW_IPM_NMAX];
    red_begin(&R);
    EACH_JOB {
        sw_ipm_job_start(g, &J, mx);
        red_max(&R, mx, 1);
    }
    sw_ipm_glob_start(g, R.mx);
    EACH_JOB sw_ipm_job_start2(g, &J);
}

/* the Newton loop: steps until g->done */
static void twin_ipm_solve(sw_ipm_glob* g, red R, sw_ipm_job J, const int32_t* sf, int32_t m) {
    const int32_t na = J.na;
    double sums[SW_IPM_NRED], mx[SW_IPM_NMAX];
    for (;;) {
        red_begin(&R);
        EACH_JOB {
            sw_ipm_job_resid(g, &J, sums, mx);
            PUT(na + 2);
            red_max(&R, mx, 3);
        }
        red_sums(&R, na + 2, sums);
        sw_ipm_glob_resid(g, sums, R.mx);
        if (g->done) break;
        EACH_JOB sw_ipm_job_prep(g, &J);
        for (int32_t k = 0; k < na; ++k) {
            const int32_t cnt = sw_ipm_row_count(na, k, g->has_t);
            EACH_JOB {
                const sw_ipm_rowctx rc = sw_ipm_row_begin(&J, k);
                for (int32_t i = 0; i < cnt; ++i) R.val[(size_t)i * m + J.j] = sw_ipm_row_val(&J, &rc, i);
            }
            red_sums(&R, cnt, sums);
            sw_ipm_glob_row(g, k, sums);
        }
        sw_ipm_glob_solve(g);
        if (g->done) break;
        red_begin(&R);
        EACH_JOB {
            sw_ipm_job_back(g, &J, mx);
            red_max(&R, mx, 2);
        }
        sw_ipm_glob_step(g, R.mx);
        EACH_JOB sw_ipm_job_step(g, &J);
    }
}

#endif /* TWIN_IPM_H */
