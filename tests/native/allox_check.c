/*
 * allox_check.c — host check of the AlloX twin (tests/twins/allox_twin.c over
 * csrc/sw_allox.h): the lazy column bookkeeping under the sanitizers.
 * Stand-alone: built and run by tests/test_allox_header.py, once plain and
 * once with -fsanitize=address,undefined.  Exit status 0 and a line
 * "ok <checks>" when every property holds.
 *
 * Every instance gets a scratch block of exactly sw_allox_bytes(m, n) bytes
 * and output arrays of exactly m and n entries from malloc, so an index past
 * a slot, a row or a worker is an error the address sanitizer reports.
 *
 *   fixed     m = 1; m < n; m = n + 1; the three-job tie; two types; a type
 *             with no free worker; all p equal; rows with p = 0; no free
 *             worker; no job
 *   boundary  m + n at 63, 64, 65, 255, 256, 257, 511, 512, 513, 1–3 types,
 *             and the caps m = n = 1024; seeded random costs, integers with
 *             heavy ties and reals
 *   checked   each job has one (worker, position), positions on a worker are
 *             1..len, worker_first is the job at the highest position, the
 *             cost is the in-order sum, the search steps lie in
 *             [m, m(m+1)/2]; integer costs on one type equal the known
 *             optimum (shortest job last: sorted p dealt round-robin)
 */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../twins/allox_twin.c"

static uint64_t checks = 0;
static int failures = 0;

static void expect(int ok, const char* what, long a, long b) {
    ++checks;
    if (!ok && ++failures <= 10) fprintf(stderr, "FAIL %s: %ld %ld\n", what, a, b);
}

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint64_t rnd(void) { /* splitmix64 */
    uint64_t z = (rng_state += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

static int cmp_double(const void* a, const void* b) {
    const double x = *(const double*)a, y = *(const double*)b;
    return (x > y) - (x < y);
}

/* runs one instance and checks its structure; returns the cost */
static double run(int32_t m, int32_t T, const int32_t* free_workers, const double* p, const double* d) {
    int32_t n = 0;
    for (int32_t t = 0; t < T; ++t) n += free_workers[t];
    int32_t* jw = (int32_t*)malloc(sizeof(int32_t) * (size_t)(m > 0 ? m : 1));
    int32_t* jp = (int32_t*)malloc(sizeof(int32_t) * (size_t)(m > 0 ? m : 1));
    int32_t* wf = (int32_t*)malloc(sizeof(int32_t) * (size_t)(n > 0 ? n : 1));
    int32_t* len = (int32_t*)calloc((size_t)(n > 0 ? n : 1), sizeof(int32_t));
    int32_t* top = (int32_t*)calloc((size_t)(n > 0 ? n : 1), sizeof(int32_t));
    const size_t bytes = sw_allox_bytes(m, n);
    void* scratch = malloc(bytes ? bytes : 8);
    double cost = -1.0;
    int64_t steps = -1;
    const int rc = allox_twin_assign(m, T, free_workers, p, d, jw, jp, wf, &cost, scratch, &steps);
    expect(rc == 0, "return code", rc, 0);
    if (m == 0 || n == 0) {
        for (int32_t i = 0; i < m; ++i) expect(jw[i] == -1 && jp[i] == 0, "unassigned job", jw[i], jp[i]);
        for (int32_t j = 0; j < n; ++j) expect(wf[j] == -1, "idle worker", wf[j], j);
        expect(cost == 0.0 && steps == 0, "no-op cost", (long)cost, (long)steps);
    } else {
        double total = 0.0;
        for (int32_t i = 0; i < m; ++i) {
            expect(jw[i] >= 0 && jw[i] < n && jp[i] >= 1 && jp[i] <= m, "job range", jw[i], jp[i]);
            if (jw[i] < 0 || jw[i] >= n) continue;
            len[jw[i]] += 1;
            if (jp[i] > top[jw[i]]) top[jw[i]] = jp[i];
            total = total + ((double)jp[i] * p[(size_t)i * (size_t)T + (size_t)sw_allox_worker_type(free_workers, T, jw[i])] + d[i]);
        }
        /* m jobs, every position within 1..len, the highest equal to len: 1..len without gaps
         * once no two jobs share a (worker, position), which worker_first's owner shows for the top */
        for (int32_t j = 0; j < n; ++j) {
            expect(top[j] == len[j], "positions 1..len", top[j], len[j]);
            if (len[j] == 0) expect(wf[j] == -1, "idle worker", wf[j], j);
            else expect(wf[j] >= 0 && wf[j] < m && jw[wf[j]] == j && jp[wf[j]] == len[j], "worker_first", wf[j], j);
        }
        for (int32_t i = 0; i < m; ++i)
            for (int32_t k = i + 1; k < m && m <= 128; ++k)
                expect(jw[i] != jw[k] || jp[i] != jp[k], "shared column", i, k);
        expect(cost == total, "in-order cost", (long)cost, (long)total);
        expect(steps >= m && steps <= (int64_t)m * (m + 1) / 2, "search steps", (long)steps, m);
    }
    free(jw); free(jp); free(wf); free(len); free(top); free(scratch);
    return cost;
}

/* one type, integer p, d = 0: the optimum is the sorted p dealt round-robin,
 * the largest n at position 1, the next n at position 2, … */
static void known_optimum(int32_t m, int32_t n, int hi) {
    double* p = (double*)malloc(sizeof(double) * (size_t)m);
    double* d = (double*)calloc((size_t)m, sizeof(double));
    for (int32_t i = 0; i < m; ++i) p[i] = (double)(rnd() % (uint64_t)hi);
    const double got = run(m, 1, &n, p, d);
    qsort(p, (size_t)m, sizeof(double), cmp_double);
    double want = 0.0;
    for (int32_t r = 0; r < m; ++r) want += (double)(r / n + 1) * p[m - 1 - r];
    expect(got == want, "known optimum", (long)got, (long)want);
    free(p); free(d);
}

static void random_instance(int32_t m, int32_t n, int32_t T, int integer) {
    int32_t fw[SW_ALLOX_MAX_TYPES] = {0};
    for (int32_t j = 0; j < n; ++j) fw[rnd() % (uint64_t)T] += 1;
    double* p = (double*)malloc(sizeof(double) * (size_t)m * (size_t)T);
    double* d = (double*)malloc(sizeof(double) * (size_t)m);
    for (int32_t i = 0; i < m; ++i) {
        d[i] = integer ? (double)(rnd() % 5) : (double)(rnd() % 40000000) / 1000.0;
        for (int32_t t = 0; t < T; ++t)
            p[(size_t)i * (size_t)T + (size_t)t] = integer ? (double)(rnd() % 4) : 20.0 + (double)(rnd() % 1000000000) / 500.0;
    }
    run(m, T, fw, p, d);
    free(p); free(d);
}

int main(void) {
    { const int32_t f[1] = {2}; const double p[1] = {5.0}, d[1] = {3.0};
      expect(run(1, 1, f, p, d) == 8.0, "m = 1", 0, 0); }
    { const int32_t f[1] = {5}; const double p[3] = {4.0, 2.0, 9.0}, d[3] = {1.0, 2.0, 3.0};
      expect(run(3, 1, f, p, d) == 21.0, "m < n", 0, 0); }
    { const int32_t f[1] = {3}; const double p[4] = {7.0, 3.0, 9.0, 5.0}, d[4] = {0.0, 0.0, 0.0, 0.0};
      expect(run(4, 1, f, p, d) == 27.0, "m = n + 1", 0, 0); }
    { const int32_t f[1] = {2}; const double p[3] = {1.0, 2.0, 3.0}, d[3] = {0.0, 0.0, 0.0};
      expect(run(3, 1, f, p, d) == 7.0, "tie example", 0, 0); }
    { const int32_t f[2] = {1, 1}; const double p[4] = {10.0, 40.0, 500.0, 60.0}, d[2] = {5.0, 7.0};
      expect(run(2, 2, f, p, d) == 82.0, "two types", 0, 0); }
    { const int32_t f[3] = {1, 0, 2};
      const double p[12] = {3.0, 1.0, 6.0, 4.0, 1.0, 2.0, 8.0, 1.0, 8.0, 2.0, 1.0, 5.0}, d[4] = {0.0, 10.0, 20.0, 30.0};
      run(4, 3, f, p, d); }
    { const int32_t f[2] = {2, 1}; double p[14], d[7];
      for (int i = 0; i < 14; ++i) p[i] = 6.0;
      for (int i = 0; i < 7; ++i) d[i] = (double)i;
      expect(run(7, 2, f, p, d) == 93.0, "all p equal", 0, 0); }
    { const int32_t f[1] = {2}; const double p[5] = {0.0, 4.0, 0.0, 1.0, 0.0}, d[5] = {1.0, 0.0, 2.0, 0.0, 3.0};
      expect(run(5, 1, f, p, d) == 11.0, "p = 0 rows", 0, 0); }
    { const int32_t f[2] = {0, 0}; const double p[4] = {1.0, 2.0, 3.0, 4.0}, d[2] = {0.0, 1.0};
      expect(run(2, 2, f, p, d) == 0.0, "no free worker", 0, 0); }
    { const int32_t f[1] = {3}; const double p[1] = {0.0}, d[1] = {0.0};
      expect(run(0, 1, f, p, d) == 0.0, "no job", 0, 0); }

    static const int32_t sizes[][2] = {{40, 23}, {41, 23}, {41, 24}, {60, 195}, {60, 196}, {60, 197},
                                       {447, 64}, {448, 64}, {449, 64}, {91, 420}, {92, 420}, {90, 423},
                                       {1024, 1024}, {1, 1024}};
    for (size_t k = 0; k < sizeof(sizes) / sizeof(sizes[0]); ++k) {
        random_instance(sizes[k][0], sizes[k][1], 1 + (int32_t)(k % 3), 1);
        random_instance(sizes[k][0], sizes[k][1], 1 + (int32_t)((k + 1) % 3), 0);
    }
    random_instance(1024, 1, 1, 0); /* one chain of 1,024 positions: m(m+1)/2 search steps */
    known_optimum(30, 4, 1000);
    known_optimum(64, 7, 3);
    known_optimum(200, 32, 1 << 20);
    known_optimum(511, 2, 1000);
    for (int k = 0; k < 60; ++k)
        random_instance(1 + (int32_t)(rnd() % 60), 1 + (int32_t)(rnd() % 16), 1 + (int32_t)(rnd() % 8), k & 1);

    if (failures) { fprintf(stderr, "%d failures\n", failures); return 1; }
    printf("ok %llu\n", (unsigned long long)checks);
    return 0;
}
