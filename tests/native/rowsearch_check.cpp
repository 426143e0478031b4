/*
 * rowsearch_check.cpp — host check of csrc/sw_rowsearch.h against plain
 * linear scans (the loops the on-chip path of Ctx ran before the searches).
 * Stand-alone: built and run by tests/test_rowsearch.py, once plain and once
 * with -fsanitize=address,undefined.  Exit status 0 and a line "ok <checks>"
 * when every result is identical.
 */
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "sw_rowsearch.h"

namespace {

constexpr int KT = 32;
typedef float Row[KT];

uint64_t checks = 0;
int failures = 0;

template <bool GE>
int ref_count(const Row& row, uint32_t rho) {
    int c = 0;
    for (int n = 0; n < KT; ++n) {
        const uint32_t b = sw_fbits_of(row[n]);
        c += (GE ? (b >= rho) : (b > rho)) ? 1 : 0;
    }
    return c;
}

int ref_snap(const Row& row, uint32_t mid, uint32_t& lo_k, uint32_t& hi_k) {
    int c = 0;
    lo_k = 0x7FFFFFFFu;
    hi_k = sw_fbits_of(row[0]);
    for (int n = 0; n < KT; ++n) {
        const uint32_t b = sw_fbits_of(row[n]);
        const uint32_t nx = n + 1 < KT ? sw_fbits_of(row[n + 1]) : 0u;
        const bool gt = b > mid;
        c += gt ? 1 : 0;
        lo_k = gt ? b : lo_k;
        hi_k = gt ? nx : hi_k;
    }
    return c;
}

uint32_t ref_extract(const Row& row, int n) {
    uint32_t v = 0;
    for (int i = 0; i < KT; ++i) v = (i == n) ? sw_fbits_of(row[i]) : v;
    return v;
}

void fail(const char* what, const Row& row, uint32_t rho, long got, long want) {
    if (++failures > 10) return;
    std::fprintf(stderr, "%s: rho %08x got %ld want %ld; row:", what, rho, got, want);
    for (int n = 0; n < KT; ++n) std::fprintf(stderr, " %08x", sw_fbits_of(row[n]));
    std::fprintf(stderr, "\n");
}

void check_threshold(const Row& row, uint32_t rho) {
    const int c = sw_rs_count<false, KT>(row, rho), cr = ref_count<false>(row, rho);
    if (c != cr) fail("count", row, rho, c, cr);
    const int g = sw_rs_count<true, KT>(row, rho), gr = ref_count<true>(row, rho);
    if (g != gr) fail("count GE", row, rho, g, gr);
    uint32_t lo, hi, lor, hir;
    const int s = sw_rs_count_snap<KT>(row, rho, lo, hi), sr = ref_snap(row, rho, lor, hir);
    if (s != sr) fail("snap count", row, rho, s, sr);
    if (lo != lor) fail("snap lo_k", row, rho, lo, lor);
    if (hi != hir) fail("snap hi_k", row, rho, hi, hir);
    checks += 5;
}

/* thresholds 0, every key value and its two neighbours, +inf */
void check_row(const Row& row) {
    check_threshold(row, 0u);
    check_threshold(row, SW_KEY_INF_BITS);
    uint32_t prev = 0xFFFFFFFFu;
    for (int n = 0; n < KT; ++n) {
        const uint32_t b = sw_fbits_of(row[n]);
        if (b == prev) continue;
        prev = b;
        check_threshold(row, b);
        check_threshold(row, b + 1u);
        if (b > 0u) check_threshold(row, b - 1u);
    }
    for (int n = -2; n <= KT + 1; ++n) {
        const uint32_t v = sw_rs_extract<KT>(row, n), vr = ref_extract(row, n);
        if (v != vr) fail("extract", row, (uint32_t)n, v, vr);
        ++checks;
    }
}

struct Rng { /* splitmix64 */
    uint64_t s;
    uint64_t next() {
        uint64_t z = (s += 0x9E3779B97F4A7C15ull);
        z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
        z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
        return z ^ (z >> 31);
    }
    uint32_t below(uint32_t n) { return (uint32_t)(next() % n); }
};

/* every row of at most three distinct values a > b > c: [0,i) a, [i,j) b, [j,KT) c */
void three_value_rows() {
    const uint32_t sets[][3] = {
        {0x3F800000u, 0x3F000000u, 0u},          /* 1, 0.5, 0 */
        {0x3F800001u, 0x3F800000u, 0x3F7FFFFFu}, /* adjacent bit patterns */
        {0x7F7FFFFFu, 0x00800000u, 0u},          /* FLT_MAX, FLT_MIN, 0 */
        {0x40400000u, 0x40000000u, 0x00800000u},
    };
    for (const auto& v : sets)
        for (int i = 0; i <= KT; ++i)
            for (int j = i; j <= KT; ++j) {
                Row row;
                for (int n = 0; n < KT; ++n) row[n] = sw_float_of(n < i ? v[0] : (n < j ? v[1] : v[2]));
                check_row(row);
            }
}

/* T live keys (strictly decreasing, or all equal) then zeros; T = 0 … KT */
void live_prefix_rows(Rng& rng) {
    for (int T = 0; T <= KT; ++T)
        for (int rep = 0; rep < 8; ++rep) {
            Row row;
            uint32_t b = 0x3F800000u + rng.below(1u << 20);
            for (int n = 0; n < KT; ++n) {
                row[n] = n < T ? sw_float_of(b) : 0.0f;
                if (rep & 1) b -= 1u + rng.below(rep < 4 ? 3u : 1u << 18);
            }
            check_row(row);
        }
}

void all_equal_rows() {
    const uint32_t vals[] = {0u, 0x00800000u, 0x3F800000u, 0x7F7FFFFFu};
    for (uint32_t v : vals) {
        Row row;
        for (int n = 0; n < KT; ++n) row[n] = sw_float_of(v);
        check_row(row);
    }
}

/* nonincreasing rows with runs of ties, a zero tail of random length, and
 * steps from one bit pattern to many octaves */
void random_rows(Rng& rng, int count) {
    for (int r = 0; r < count; ++r) {
        Row row;
        const int T = (int)rng.below(KT + 1);
        const int tie_pct = (int)rng.below(100);
        const int shift = 1 + (int)rng.below(27);
        uint32_t b = 0x00800000u + rng.below(0x7F7FFFFFu - 0x00800000u);
        for (int n = 0; n < KT; ++n) {
            row[n] = n < T ? sw_float_of(b) : 0.0f;
            if ((int)rng.below(100) >= tie_pct) {
                const uint32_t step = 1u + rng.below(1u << shift);
                b = b > 0x00800000u + step ? b - step : (b > 0x00800000u ? 0x00800000u : 0u);
            }
        }
        if (r & 1) {
            check_row(row);
        } else { /* thresholds unrelated to the keys */
            for (int q = 0; q < 4; ++q) check_threshold(row, rng.below(0x7F800001u));
            const int n = (int)rng.below(KT);
            if (sw_rs_extract<KT>(row, n) != ref_extract(row, n)) fail("extract", row, (uint32_t)n, 0, 0);
            ++checks;
        }
    }
}

} // namespace

int main(int argc, char** argv) {
    const int count = argc > 1 ? std::atoi(argv[1]) : 300000;
    Rng rng{0x5EEDull};
    three_value_rows();
    live_prefix_rows(rng);
    all_equal_rows();
    random_rows(rng, count);
    if (failures) {
        std::fprintf(stderr, "%d mismatches in %llu checks\n", failures, (unsigned long long)checks);
        return 1;
    }
    std::printf("ok %llu\n", (unsigned long long)checks);
    return 0;
}
