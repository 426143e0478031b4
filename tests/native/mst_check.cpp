/*
 * mst_check.cpp — host check of csrc/sw_mst.h: the ordered key of signed
 * doubles and the per-job root x_j(m).  Stand-alone: built and run by
 * tests/test_mst_header.py, once plain and once with
 * -fsanitize=address,undefined.  Exit status 0 and a line "ok <checks>" when
 * every property holds.
 *
 *   key    monotone (a < b ⇔ key(a) < key(b), −0 just below +0) and
 *          round-trips bit for bit, over ±0, denormals, ±2^64, the ends of the
 *          ν search and seeded random doubles of every exponent
 *   x      sw_mst_x(sf, l, m) ∈ (l, 1] for l < 1 (1 for l = 1) and
 *          non-increasing in m, over a ladder of m from −2^64 to 2^64
 *   alloc  1 above λ, l below, l on the class at m = +inf
 */
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "sw_mst.h"

namespace {

uint64_t checks = 0;
int failures = 0;

void expect(bool ok, const char* what, double a, double b) {
    ++checks;
    if (!ok && ++failures <= 10) fprintf(stderr, "FAIL %s: %.17g %.17g\n", what, a, b);
}

uint64_t rng_state = 0x9E3779B97F4A7C15ull;
uint64_t rnd() { /* splitmix64 */
    uint64_t z = (rng_state += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

double rnd_double() { /* any finite double, either sign */
    for (;;) {
        const uint64_t b = rnd();
        if (((b >> 52) & 0x7FF) != 0x7FF) return sw_from_bits(b);
    }
}

void check_key(int n_random) {
    const double two64 = 18446744073709551616.0;
    std::vector<double> v = {0.0, -0.0, 4.9406564584124654e-324, -4.9406564584124654e-324,
                             2.2250738585072009e-308, -2.2250738585072009e-308, 2.2250738585072014e-308,
                             1.0, -1.0, two64, -two64, 1.7976931348623157e308, -1.7976931348623157e308};
    for (int i = 0; i < n_random; ++i) v.push_back(rnd_double());
    expect(sw_mst_key(-two64) == SW_MST_NU_LO_KEY, "key(-2^64)", -two64, 0);
    expect(sw_mst_key(two64) == SW_MST_NU_HI_KEY, "key(2^64)", two64, 0);
    expect(sw_mst_key(-0.0) + 1 == sw_mst_key(0.0), "key(-0) + 1 = key(+0)", 0, 0);
    for (size_t i = 0; i < v.size(); ++i) {
        const double a = v[i];
        expect(sw_bits(sw_mst_unkey(sw_mst_key(a))) == sw_bits(a), "round trip", a, sw_mst_unkey(sw_mst_key(a)));
        const double b = v[(i * 7 + 3) % v.size()];
        const uint64_t ka = sw_mst_key(a), kb = sw_mst_key(b);
        if (a < b) expect(ka < kb, "monotone <", a, b);
        if (a > b) expect(ka > kb, "monotone >", a, b);
        if (sw_bits(a) == sw_bits(b)) expect(ka == kb, "equal", a, b);
        /* the neighbour in key order is the neighbour in value order */
        if (ka > 0 && ka != 0x8000000000000000ull) {
            const double p = sw_mst_unkey(ka - 1);
            expect(p < a, "predecessor", p, a);
        }
    }
}

void check_x(int n_random) {
    std::vector<double> ms;
    for (int e = 64; e >= -64; e -= 4) ms.push_back(-sw_from_bits((uint64_t)(1023 + e) << 52));
    ms.push_back(-0.0);
    ms.push_back(0.0);
    for (int e = -64; e <= 64; e += 4) ms.push_back(sw_from_bits((uint64_t)(1023 + e) << 52));
    std::vector<double> ls = {0.0, 4.9406564584124654e-324, 1e-300, 1e-9, 0.25, 0.5, 0.75, 1.0 - 1e-9,
                              0.99999999999999989, 1.0};
    for (int i = 0; i < n_random; ++i) ls.push_back((double)(rnd() >> 11) / 9007199254740992.0);
    const double sfs[] = {1.0, 2.0, 8.0, 255.0};
    for (double l : ls)
        for (double sf : sfs) {
            double prev = 2.0;
            for (double m : ms) {
                const double x = sw_mst_x(sf, l, m);
                if (l < 1.0) expect(x > l && x <= 1.0, "x in (l, 1]", l, x);
                else expect(x == 1.0, "x = 1 at l = 1", l, x);
                expect(x <= prev, "x non-increasing in m", m, x);
                prev = x;
            }
            expect(sw_mst_x(sf, l, ms.front()) == 1.0, "x(-2^64) = 1", l, sf);
            expect(sw_mst_alloc(3.0, sf, l, 2.0, 0.5) == 1.0, "alloc above", l, sf);
            expect(sw_mst_alloc(1.0, sf, l, 2.0, 0.5) == l, "alloc below", l, sf);
            expect(sw_mst_alloc(2.0, sf, l, 2.0, sw_from_bits(SW_MST_INF_BITS)) == l, "alloc at floors", l, sf);
            expect(sw_mst_alloc(2.0, sf, l, 2.0, 0.5) == sw_mst_x(sf, l, 0.5), "alloc on the class", l, sf);
        }
    expect(sw_mst_density(-0.0, 2.0) == 0.0 && sw_bits(sw_mst_density(-0.0, 2.0)) == 0, "density of -0", 0, 0);
    expect(sw_mst_floor(0.5, 1) == 0.0 && sw_mst_floor(0.5, 0) == 0.5 && sw_bits(sw_mst_floor(-0.0, 0)) == 0,
           "floor", 0, 0);
}

}  // namespace

int main(int argc, char** argv) {
    const int n = argc > 1 ? atoi(argv[1]) : 1000;
    check_key(n * 100);
    check_x(n);
    if (failures) {
        fprintf(stderr, "%d failures in %llu checks\n", failures, (unsigned long long)checks);
        return 1;
    }
    printf("ok %llu\n", (unsigned long long)checks);
    return 0;
}
