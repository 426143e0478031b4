/*
 * tests/native/ftft_check.c — TEST INFRASTRUCTURE: csrc/sw_ftf_types.h (with
 * sw_mmf_ipm.h and sw_ftf.h) on the host as a stand-alone program, for
 * tests/test_ftf_types_header.py, which builds it plainly under
 * -Wall -Wextra -Werror and under the address and undefined-behaviour
 * sanitizers.
 *
 * Part 1 drives the outer iteration alone (sw_ftft_begin / _next / _feed) on
 * synthetic level functions t(ρ) with root 4:
 *   linear    t = ρ/4: one Newton step from the start
 *   concave   t = √(ρ/4), 1/t convex: the t-step stays left of the root,
 *             the probes increase, no SAFE
 *   convex    t = (ρ/4)², 1/t convex: the t-step from 1 lands at 8.5; SAFE, then
 *             φ-steps from the left only, increasing, up to the root
 *   flat      t = 1/2 with slope 1: never converges, the solve cap's status
 *   box       t(ρ_box) > 1 at the start: ends at once, `wide`
 * Part 2 runs the twin's arithmetic (tests/twins/ftft_twin.c, included as
 * source) over a ladder of small instances — numbers of types 1 … 16, job
 * counts around the chunking of the deterministic sum, dead jobs, types without
 * workers — and checks on each that the call succeeds, that the result is finite
 * and that every row of the program holds at the returned ρ.
 * Prints "ok <checks>".
 */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>

#include "../twins/ftft_twin.c"

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
#define ROOT 4.0

static double t_linear(double r, double* tp) { *tp = 0.25; return r / 4.0; }
static double t_concave(double r, double* tp) { const double t = sqrt(r / 4.0); *tp = 0.125 / t; return t; }
static double t_convex(double r, double* tp) { *tp = r / 8.0; return r * r / 16.0; }
static double t_flat(double r, double* tp) { (void)r; *tp = 1.0; return 0.5; }

/* runs the iteration; checks what holds for every level function with 1/t convex */
static void drive(double (*f)(double, double*), double start, sw_ftft_search* s, double* first_hi) {
    double rho = 0.0, last_left = 0.0;
    *first_hi = 0.0;
    sw_ftft_begin(s, 0.5, start, TOL);
    while (sw_ftft_next(s, &rho)) {
        double tp = 0.0;
        const double t = f(rho, &tp);
        CHECK(rho >= 0.5);
        if (s->safe) { /* after an overshoot: from the left only, and increasing */
            CHECK(rho <= ROOT * (1.0 + 1e-8));
            CHECK(rho > last_left);
        }
        if (t < 1.0) {
            CHECK(rho > last_left);
            last_left = rho;
        } else if (t > 1.0 + TOL && *first_hi == 0.0) {
            *first_hi = rho;
        }
        sw_ftft_feed(s, rho, t, tp);
        CHECK(s->solves <= SW_FTFT_MAX_SOLVES);
    }
}

static void search_checks(void) {
    sw_ftft_search s;
    double hi;
    drive(t_linear, 1.0, &s, &hi);
    CHECK(s.status == 0 && s.done && s.solves == 2 && s.rho == ROOT && !s.safe && hi == 0.0);
    drive(t_concave, 1.0, &s, &hi);
    CHECK(s.status == 0 && s.done && !s.safe && hi == 0.0);
    CHECK(fabs(s.rho - ROOT) <= 4.0 * TOL * ROOT && s.solves <= 8);
    drive(t_convex, 1.0, &s, &hi);
    CHECK(s.status == 0 && s.done && s.safe && hi == 8.5 && s.have_hi && s.hi == 8.5);
    CHECK(fabs(s.rho - ROOT) <= TOL * ROOT && s.rho <= ROOT * (1.0 + 1e-9));
    CHECK(sw_ftft_flags(&s) & SW_FTFT_SAFE);
    drive(t_flat, 1.0, &s, &hi);
    CHECK(s.status == SW_FTFT_CAP && !s.done && s.solves == SW_FTFT_MAX_SOLVES);
    /* the first probe above 1 + tol at ρ_box itself: nothing lower is admitted */
    sw_ftft_begin(&s, 8.0, 8.0, TOL);
    {
        double rho = 0.0, tp = 0.0;
        CHECK(sw_ftft_next(&s, &rho) && rho == 8.0);
        sw_ftft_feed(&s, rho, t_convex(rho, &tp), tp);
        CHECK(s.done && s.wide && !s.safe && s.solves == 1 && !sw_ftft_next(&s, &rho));
        CHECK(sw_ftft_flags(&s) == SW_FTFT_BOX);
    }
    /* above 1 + tol at a start that is not ρ_box (a start that was no lower bound): back to ρ_box */
    sw_ftft_begin(&s, 1.0, 8.0, TOL);
    {
        double rho = 0.0, tp = 0.0;
        int32_t k = 0;
        while (sw_ftft_next(&s, &rho)) {
            CHECK(k != 1 || rho == 1.0);
            sw_ftft_feed(&s, rho, t_convex(rho, &tp), tp);
            ++k;
        }
        CHECK(s.done && s.safe && fabs(s.rho - ROOT) <= TOL * ROOT);
    }
}

static void run(double dead, int zero_type) {
    int32_t* W = (int32_t*)malloc(sizeof(int32_t) * (size_t)n);
    int32_t* sf = (int32_t*)malloc(sizeof(int32_t) * (size_t)m);
    double* thr = (double*)malloc(sizeof(double) * (size_t)m * n);
    double* st = (double*)malloc(sizeof(double) * (size_t)m);
    double* a = (double*)malloc(sizeof(double) * (size_t)m);
    double* E = (double*)malloc(sizeof(double) * (size_t)m);
    double* x = (double*)malloc(sizeof(double) * (size_t)m * n);
    double res[5];
    CHECK(W && sf && thr && st && a && E && x);
    for (int32_t k = 0; k < n; ++k) W[k] = 1 + (int32_t)(rnd() * (double)(m / 4 + 1));
    if (zero_type && n > 1) W[n / 2] = 0;
    for (int32_t j = 0; j < m; ++j) {
        const double total = pow(10.0, 4.0 + 2.0 * rnd()), done = rnd() < 0.2 ? 0.0 : 0.9 * rnd();
        double iso = 0.0;
        sf[j] = 1 << (int32_t)(rnd() * 4.0);
        for (int32_t k = 0; k < n; ++k) {
            thr[(size_t)j * n + k] = rnd() < 0.15 ? 0.0 : (0.2 + 3.8 * rnd()) * sf[j];
            if (W[k] > 0) iso += thr[(size_t)j * n + k];
        }
        if (!(iso > 0.0)) { /* a positive throughput on a type with workers */
            const int32_t k = W[0] > 0 ? 0 : n - 1;
            thr[(size_t)j * n + k] = 1.0 + rnd();
            iso = thr[(size_t)j * n + k];
        }
        iso = iso / (double)(n * sf[j] * 4);
        st[j] = rnd() < dead ? 0.0 : total * (1.0 - done);
        E[j] = total / iso;
        a[j] = (total - st[j]) / iso * (0.3 + 0.5 * rnd());
    }
    const int rc = ftft_twin_allocate(m, n, W, sf, thr, st, a, E, x, res);
    CHECK(rc == 0);
    for (int i = 0; i < 5; ++i) CHECK(isfinite(res[i]));
    CHECK(res[3] >= 1.0 && res[3] <= (double)(SW_FTFT_MAX_SOLVES / 4));
    for (int32_t j = 0; j < m; ++j) {
        double val = 0.0, sx = 0.0;
        for (int32_t k = 0; k < n; ++k) {
            const double xv = x[(size_t)j * n + k];
            CHECK(xv >= 0.0 && isfinite(xv));
            if (W[k] == 0) CHECK(xv == 0.0);
            val += thr[(size_t)j * n + k] * xv;
            sx += xv;
        }
        CHECK(sx <= 1.0 + 1e-9);
        CHECK(a[j] / E[j] <= res[0]);
        if (st[j] > 0.0) CHECK(val * (res[0] * E[j] - a[j]) / st[j] >= 1.0 - 1e-9);
    }
    for (int32_t k = 0; k < n; ++k) {
        double load = 0.0;
        for (int32_t j = 0; j < m; ++j) load += sf[j] * x[(size_t)j * n + k];
        CHECK(load <= W[k] * (1.0 + 1e-9));
    }
    free(W); free(sf); free(thr); free(st); free(a); free(E); free(x);
}

int main(int argc, char** argv) {
    const int reps = argc > 1 ? atoi(argv[1]) : 1;
    static const int32_t ms[] = {1, 2, 3, 7, 33, 511, 512, 513, 1025};
    search_checks();
    for (int r = 0; r < reps; ++r)
        for (size_t i = 0; i < sizeof(ms) / sizeof(ms[0]); ++i)
            for (n = 1; n <= SW_IPM_MAX_TYPES; n += (ms[i] > 100 ? 5 : 1)) {
                m = ms[i];
                run(0.0, 0);
                run(0.15, 1);
                if (m < 40) run(1.0, 0); /* no live job */
            }
    printf("ok %ld\n", checks);
    return 0;
}
