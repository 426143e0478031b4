/*
 * tests/native/wft_check.c — TEST INFRASTRUCTURE: csrc/sw_wf_types.h (with
 * sw_mmf_ipm.h) on the host as a stand-alone program, for
 * tests/test_wf_types_header.py, which builds it plainly under
 * -Wall -Wextra -Werror and under the address and undefined-behaviour
 * sanitizers.
 *
 * Part 1 drives the stage bookkeeping alone (sw_wft_begin / _next / _feed /
 * _repeat / _result) on synthetic classifications:
 *   one       every job freezes in the first stage: one stage, SW_WFT_ONE, no repeat
 *   ladder    one job per stage: m stages, then the repeat, which leaves the
 *             stage count and the level alone
 *   stall     a stage that freezes none: SW_WFT_STALL, no further stage
 *   near      statistics within a decade of the threshold set SW_WFT_NEAR
 * Part 2 runs the twin's arithmetic (tests/twins/wft_twin.c, included as
 * source) over a ladder of small instances — numbers of types 1 … 16, job
 * counts around the chunking of the deterministic sum, types without workers —
 * and checks on each that the call succeeds, that the result is finite, that
 * the levels rise with the stages and that every row of the program holds at
 * the returned levels.  Above 100 jobs the jobs come in three classes of
 * identical rows, so that the stages stay few.
 * Prints "ok <checks>".
 */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>

#include "../twins/wft_twin.c"

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static double rnd(void) { /* xorshift64*, in [0, 1) */
    rng_state ^= rng_state >> 12;
    rng_state ^= rng_state << 25;
    rng_state ^= rng_state >> 27;
    return (double)((rng_state * 0x2545F4914F6CDD1Dull) >> 11) / 9007199254740992.0;
}

static long checks = 0;
static int32_t m = 0, n = 0;
#define CHECK(c)                                                                  \
    do {                                                                          \
        ++checks;                                                                 \
        if (!(c)) {                                                               \
            printf("FAILED %s at line %d (m %d n %d)\n", #c, __LINE__, m, n);     \
            exit(1);                                                              \
        }                                                                         \
    } while (0)

#define TOL 1e-9

static void stage_checks(void) {
    sw_wft_glob q;
    double out[4];
    const double clear[2] = {SW_WFT_THRESH / 1e3, -SW_WFT_THRESH * 1e3};
    /* one */
    sw_wft_begin(&q, 5, 0);
    CHECK(sw_wft_next(&q));
    q.level = 0.75;
    sw_wft_feed(&q, 5.0, clear);
    CHECK(!sw_wft_next(&q) && !sw_wft_repeat(&q) && q.status == 0);
    sw_wft_result(&q, out);
    CHECK(out[2] == 1.0 && out[3] == (double)SW_WFT_ONE && out[0] == 0.75 * (1.0 - SW_WFT_EASE));
    /* ladder */
    sw_wft_begin(&q, 7, 0);
    for (int s = 0; s < 7; ++s) {
        CHECK(sw_wft_next(&q) && q.stage == s && q.left == 7 - s);
        q.level = 1.0 + s;
        sw_wft_feed(&q, 1.0, clear);
    }
    CHECK(!sw_wft_next(&q) && q.stage == 7 && q.left == 0);
    CHECK(sw_wft_repeat(&q) && q.rep == 1 && q.stage == 6 && q.left == 1 && q.ease == 2.0 * SW_WFT_EASE);
    CHECK(sw_wft_next(&q)); /* the repeat is a stage to the loop */
    {
        sw_ipm_glob g;
        const double none[1] = {0.0};
        g.na = 0;
        sw_wft_glob_blend(&g, &q, none, none);
    }
    CHECK(q.rep == 2 && q.theta == 1.0 && !sw_wft_next(&q) && !sw_wft_repeat(&q));
    sw_wft_result(&q, out);
    CHECK(out[2] == 7.0 && out[3] == 0.0 && out[0] == 7.0 * (1.0 - SW_WFT_EASE));
    /* stall */
    sw_wft_begin(&q, 3, 0);
    q.level = 1.0;
    sw_wft_feed(&q, 1.0, clear);
    sw_wft_feed(&q, 0.0, clear);
    CHECK(q.status == SW_WFT_STALL && !sw_wft_next(&q) && !sw_wft_repeat(&q) && q.stage == 1 && q.left == 2);
    /* near */
    {
        const double lo_near[2] = {SW_WFT_THRESH / 2.0, -SW_WFT_THRESH * 1e3};
        const double hi_near[2] = {SW_WFT_THRESH / 1e3, -SW_WFT_THRESH * 2.0};
        sw_wft_begin(&q, 3, 0);
        sw_wft_feed(&q, 1.0, clear);
        CHECK(q.flags == 0);
        sw_wft_feed(&q, 1.0, lo_near);
        CHECK(q.flags == SW_WFT_NEAR);
        sw_wft_begin(&q, 3, 0);
        sw_wft_feed(&q, 1.0, hi_near);
        CHECK(q.flags == SW_WFT_NEAR);
        sw_wft_begin(&q, 3, 0);
        sw_wft_feed(&q, 3.0, hi_near); /* every job froze: no free job's statistic to be near */
        CHECK(q.flags == 0);
    }
}

static void run(int zero_type) {
    int32_t* W = (int32_t*)malloc(sizeof(int32_t) * (size_t)n);
    int32_t* sf = (int32_t*)malloc(sizeof(int32_t) * (size_t)m);
    int32_t* froze = (int32_t*)malloc(sizeof(int32_t) * (size_t)m);
    double* c = (double*)malloc(sizeof(double) * (size_t)m * n);
    double* x = (double*)malloc(sizeof(double) * (size_t)m * n);
    double* F = (double*)malloc(sizeof(double) * (size_t)m);
    double res[4];
    const int32_t groups = m > 100 ? 3 : m;
    CHECK(W && sf && froze && c && x && F);
    for (int32_t k = 0; k < n; ++k) W[k] = 1 + (int32_t)(rnd() * (double)(m / (2 * n) + 1));
    if (zero_type && n > 1) W[n / 2] = 0;
    for (int32_t j = 0; j < m; ++j) {
        if (j >= groups) { /* a copy of its class's first job */
            sf[j] = sf[j % groups];
            for (int32_t k = 0; k < n; ++k) c[(size_t)j * n + k] = c[(size_t)(j % groups) * n + k];
            continue;
        }
        sf[j] = 1 << (int32_t)(rnd() * 3.0);
        for (int32_t k = 0; k < n; ++k) c[(size_t)j * n + k] = (0.2 + 4.8 * rnd()) * sf[j];
    }
    const int rc = wft_twin_allocate_stats(m, n, W, sf, c, x, F, res, froze, 0, 0);
    CHECK(rc == 0);
    for (int i = 0; i < 4; ++i) CHECK(isfinite(res[i]));
    CHECK(res[2] >= 1.0 && res[2] <= (double)m);
    for (int32_t j = 0; j < m; ++j) {
        double val = 0.0, sx = 0.0;
        CHECK(froze[j] >= 1 && froze[j] <= (int32_t)res[2] && F[j] > 0.0 && F[j] <= res[0]);
        if (froze[j] == (int32_t)res[2]) CHECK(F[j] == res[0]);
        for (int32_t i = 0; i < m; ++i) /* the levels rise with the stages */
            if (froze[i] < froze[j]) CHECK(F[i] < F[j]);
            else if (froze[i] == froze[j]) CHECK(F[i] == F[j]);
        for (int32_t k = 0; k < n; ++k) {
            const double xv = x[(size_t)j * n + k];
            CHECK(xv >= 0.0 && isfinite(xv));
            if (W[k] == 0) CHECK(xv == 0.0);
            val += c[(size_t)j * n + k] * xv;
            sx += xv;
        }
        CHECK(sx <= 1.0 + TOL);
        CHECK(val >= F[j] * (1.0 - TOL));
    }
    for (int32_t k = 0; k < n; ++k) {
        double load = 0.0;
        for (int32_t j = 0; j < m; ++j) load += sf[j] * x[(size_t)j * n + k];
        CHECK(load <= W[k] * (1.0 + TOL));
    }
    free(W); free(sf); free(froze); free(c); free(x); free(F);
}

int main(int argc, char** argv) {
    const int reps = argc > 1 ? atoi(argv[1]) : 1;
    static const int32_t ms[] = {1, 2, 3, 7, 33, 511, 512, 513, 1025};
    stage_checks();
    for (int r = 0; r < reps; ++r)
        for (size_t i = 0; i < sizeof(ms) / sizeof(ms[0]); ++i)
            for (n = 1; n <= SW_IPM_MAX_TYPES; n += (ms[i] > 100 ? 5 : 1)) {
                m = ms[i];
                run(0);
                run(1);
            }
    printf("ok %ld\n", checks);
    return 0;
}
