/*
 * tests/native/mtdt_check.c — TEST INFRASTRUCTURE: csrc/sw_mtd_types.h (with
 * sw_mmf_ipm.h and sw_mtd.h) on the host as a stand-alone program, for
 * tests/test_mtd_types_header.py, which builds it plainly under
 * -Wall -Wextra -Werror and under the address and undefined-behaviour
 * sanitizers.  It runs the twin's arithmetic (tests/twins/mtdt_twin.c, included
 * as source) over a ladder of small instances — every number of types 1 … 16,
 * job counts around the chunking of the deterministic sum, dead jobs, types
 * without workers, steps from 1e1 to 1e9, the thin case — and checks on each
 * that the call succeeds, that the result is finite and that every row of the
 * LP holds at the returned T.  Prints "ok <checks>".
 */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>

#include "../twins/mtdt_twin.c"

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static double rnd(void) { /* xorshift64*, in [0, 1) */
    rng_state ^= rng_state >> 12;
    rng_state ^= rng_state << 25;
    rng_state ^= rng_state >> 27;
    return (double)((rng_state * 0x2545F4914F6CDD1Dull) >> 11) / 9007199254740992.0;
}

static long checks = 0;
#define CHECK(c)                                                                  \
    do {                                                                          \
        ++checks;                                                                 \
        if (!(c)) {                                                               \
            printf("FAILED %s at line %d (m %d n %d)\n", #c, __LINE__, m, n);     \
            exit(1);                                                              \
        }                                                                         \
    } while (0)

static void run(int32_t m, int32_t n, double lo, double hi, double dead, int zero_type) {
    int32_t* W = (int32_t*)malloc(sizeof(int32_t) * (size_t)n);
    int32_t* sf = (int32_t*)malloc(sizeof(int32_t) * (size_t)m);
    double* thr = (double*)malloc(sizeof(double) * (size_t)m * n);
    double* steps = (double*)malloc(sizeof(double) * (size_t)m);
    double* x = (double*)malloc(sizeof(double) * (size_t)m * n);
    double res[4];
    CHECK(W && sf && thr && steps && x);
    for (int32_t k = 0; k < n; ++k) W[k] = 1 + (int32_t)(rnd() * (m / 2 + 2));
    if (zero_type && n > 1) W[n - 1] = 0;
    for (int32_t j = 0; j < m; ++j) {
        sf[j] = 1 << (int)(rnd() * 3.0);
        for (int32_t k = 0; k < n; ++k) thr[(size_t)j * n + k] = rnd() < 0.15 ? 0.0 : (0.2 + 3.8 * rnd()) * sf[j];
        thr[(size_t)j * n] = (0.2 + 3.8 * rnd()) * sf[j]; /* type 0 always has workers */
        steps[j] = rnd() < dead ? 0.0 : pow(10.0, lo + (hi - lo) * rnd());
    }
    const int rc = mtdt_twin_allocate(m, n, W, sf, thr, steps, x, res);
    CHECK(rc == 0);
    const double T = res[0];
    CHECK(isfinite(T) && T > 100.0 && isfinite(res[1]) && res[1] >= 0.0);
    CHECK(res[2] >= 1.0 && res[2] <= 2.0 * SW_IPM_MAX_ITERS);
    for (int32_t j = 0; j < m; ++j) {
        double val = 0.0, sx = 0.0;
        for (int32_t k = 0; k < n; ++k) {
            const double v = x[(size_t)j * n + k];
            CHECK(v >= 0.0 && v <= 1.0 + 1e-9);
            if (W[k] == 0) CHECK(v == 0.0);
            val += thr[(size_t)j * n + k] * v;
            sx += v;
        }
        CHECK(sx <= 1.0 + 1e-9);
        CHECK(val >= steps[j] / T * (1.0 - 1e-9));
    }
    for (int32_t k = 0; k < n; ++k) {
        double cap = 0.0;
        for (int32_t j = 0; j < m; ++j) cap += sf[j] * x[(size_t)j * n + k];
        CHECK(cap <= W[k] * (1.0 + 1e-9));
    }
    free(W); free(sf); free(thr); free(steps); free(x);
}

int main(int argc, char** argv) {
    const int reps = argc > 1 ? atoi(argv[1]) : 2;
    static const int32_t ms[] = {1, 2, 3, 7, 31, 64, 65, 511, 512, 513, 1025};
    for (int r = 0; r < reps; ++r) {
        for (int32_t n = 1; n <= SW_IPM_MAX_TYPES; ++n)
            for (size_t i = 0; i < sizeof(ms) / sizeof(ms[0]); ++i) {
                if (ms[i] > 100 && n > 3 && n != SW_IPM_MAX_TYPES) continue;
                if (ms[i] > 600 && n > 3) continue;
                run(ms[i], n, 4.0, 6.0, 0.1, (int)(i & 1));
                if (ms[i] <= 65) {
                    run(ms[i], n, 1.0, 7.5, 0.1, (int)(i & 1));
                    run(ms[i], n, 8.0, 9.0, 0.0, 0);  /* the decade rounds */
                    run(ms[i], n, 4.0, 6.0, 1.0, 0);  /* no live job */
                }
            }
    }
    { /* the thin case */
        const int32_t m = 1, n = 1, W = 1, sf = 1;
        const double thr = 1.0, steps = 500050.0 * (1.0 - SW_MTDT_THIN / 4.0);
        double x, res[4];
        CHECK(mtdt_twin_allocate(1, 1, &W, &sf, &thr, &steps, &x, res) == 0);
        CHECK(res[0] == 500050.0 && ((int)res[3] & SW_MTDT_THIN_FLAG) && x >= steps / res[0] * (1.0 - 1e-9) && x <= 1.0);
    }
    printf("ok %ld\n", checks);
    return 0;
}
