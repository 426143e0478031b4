/*
 * key_arith_check.cpp — host check of csrc/sw_keyarith.h: the one-instruction
 * forms that Ctx::setup uses for its key rows (sw_e_nf, sw_min_nf, sw_key_nf)
 * against the text of sw_arith.h that the CPU twin compiles (sw_e, sw_min as
 * setup uses it on the running marginal, sw_key), bit for bit.
 * Stand-alone: built and run by tests/test_key_arith.py, once plain and once
 * with -fsanitize=address,undefined.  Exit status 0 and a line "ok <checks>"
 * when every result is identical.
 *
 * Inputs: ±0, the smallest and the largest denormal, DBL_MIN, FLT_MIN and
 * FLT_MAX as doubles with their two neighbours, DBL_MAX, +inf, equal
 * operands, cap = 0, the product 0·∞ that an overflowed key scale makes of a
 * zero marginal (a NaN key in both forms), and seeded random finite values.
 *
 * Left out, because no input that sw_validate.h admits produces it:
 *   - a NaN rate or cap (Δ and d are finite and positive, E − F an integer);
 *     a NaN product rate·n (rate = +inf at n = 0) is in;
 *   - a NaN operand of the running minimum: both come out of sw_pos;
 *   - +0 against −0 in a minimum, where fmin may hand back either: rate, n
 *     and cap are ≥ +0 and sw_pos returns +0, so only +0 meets +0.  −0 is in
 *     wherever the other operand is not a zero.
 * sw_key_nf is compared with sw_key on everything, NaN and negative included.
 */
#include <cfloat>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <vector>

#include "sw_keyarith.h"

namespace {

uint64_t checks = 0;
int failures = 0;

void fail(const char* what, double a, double b, uint64_t got, uint64_t want) {
    if (++failures > 10) return;
    std::fprintf(stderr, "%s(%a [%016llx], %a [%016llx]): got %016llx want %016llx\n", what, a,
                 (unsigned long long)sw_bits(a), b, (unsigned long long)sw_bits(b),
                 (unsigned long long)got, (unsigned long long)want);
}

bool is_zero(double x) { return x == 0.0; }
bool mixed_zeros(double a, double b) { return is_zero(a) && is_zero(b) && sw_bits(a) != sw_bits(b); }

void check_min(double a, double b) {
    if (a != a || b != b || mixed_zeros(a, b)) return;
    const uint64_t got = sw_bits(sw_min_nf(a, b)), want = sw_bits(sw_min(a, b));
    if (got != want) fail("min", a, b, got, want);
    ++checks;
}

void check_e(double rate, double cap, int32_t n) {
    if (rate != rate || cap != cap) return;
    sw_jobc c = sw_make_jobc(1, 1, 1.0, 1, 1.0, 0, 1, 0.0, 0.0);
    c.rate = rate;
    c.cap = cap;
    if (mixed_zeros(rate * (double)n, cap)) return;
    const uint64_t got = sw_bits(sw_e_nf(&c, n)), want = sw_bits(sw_e(&c, n));
    if (got != want) fail("e", rate, cap, got, want);
    ++checks;
}

void check_key(double vm, double scale) {
    const uint32_t got = sw_fbits_of(sw_key_nf(vm, scale)), want = sw_fbits_of(sw_key(vm, scale));
    if (got != want) fail("key", vm, scale, got, want);
    ++checks;
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
    double unit() { return (double)(next() >> 11) * 0x1p-53; }
    /* a finite double ≥ +0 of any exponent, denormals included */
    double finite_pos() {
        uint64_t u = next() & 0x7FFFFFFFFFFFFFFFull;
        if ((u >> 52) == 0x7FF) u &= 0x7FEFFFFFFFFFFFFFull;
        return sw_from_bits(u);
    }
};

std::vector<double> special_values() {
    const double inf = std::numeric_limits<double>::infinity();
    std::vector<double> v = {0.0, -0.0, 1.0, 0.5, 3.0, inf, DBL_MAX, DBL_MIN,
                             std::numeric_limits<double>::denorm_min(),
                             std::nextafter(DBL_MIN, 0.0), /* the largest denormal */
                             std::nextafter(DBL_MIN, 1.0), std::nextafter(DBL_MAX, 0.0)};
    for (double x : {SW_FLT_MIN, SW_FLT_MAX, (double)FLT_TRUE_MIN, 1.0}) {
        v.push_back(x);
        v.push_back(std::nextafter(x, 0.0));
        v.push_back(std::nextafter(x, inf));
    }
    /* where the conversion to fp32 changes its result around FLT_MAX: the
     * midpoint between FLT_MAX and 2^128 rounds to +inf, below it to FLT_MAX */
    const double mid = 0x1.ffffffp127;
    v.push_back(mid);
    v.push_back(std::nextafter(mid, 0.0));
    v.push_back(std::nextafter(mid, inf));
    v.push_back(0x1p128);
    /* … and around FLT_MIN: the largest double that still rounds below it */
    v.push_back(0x1.fffffefffffffp-127);
    return v;
}

void special_cases() {
    const std::vector<double> sv = special_values();
    const double inf = std::numeric_limits<double>::infinity();
    for (double a : sv)
        for (double b : sv) {
            check_min(a, b);
            check_key(a, b);
            check_key(-a, b);
            for (int32_t n : {0, 1, 2, 3, 31, 32, 33, 64}) check_e(a, b, n);
        }
    /* cap as the validator makes it: E − F, an integer ≥ 0 (0 when F == E) */
    for (double cap : {0.0, 1.0, 5.0, 200.0, 2147483647.0})
        for (double rate : sv)
            for (int32_t n = 0; n <= 64; ++n) check_e(rate, cap, n);
    /* The trap: A = max p/(N·T) so small that 1/(w·A) overflows; a zero
     * marginal then gives 0·∞, a NaN that sw_key converts as it is. */
    for (double A : {std::numeric_limits<double>::denorm_min(), 1e-310, 0x1p-1030})
        for (int32_t w : {1, 2, 8}) {
            const double scale = sw_key_scale(w, A);
            if (!(scale == inf)) {
                std::fprintf(stderr, "scale of A = %a, w = %d did not overflow\n", A, w);
                ++failures;
            }
            const float k0 = sw_key_nf(0.0, scale), k1 = sw_key(0.0, scale);
            if (k0 == k0 || k1 == k1) { /* both must be a NaN */
                std::fprintf(stderr, "0 * inf gave %a / %a, not a NaN\n", (double)k0, (double)k1);
                ++failures;
            }
            for (double vm : sv) check_key(vm, scale);
            ++checks;
        }
    check_key(std::numeric_limits<double>::quiet_NaN(), 1.0);
    check_key(1.0, std::numeric_limits<double>::quiet_NaN());
}

void random_cases(Rng& rng, int count) {
    for (int r = 0; r < count; ++r) {
        const double a = rng.finite_pos(), b = rng.finite_pos();
        check_min(a, b);
        check_min(a, a);
        check_e(a, b, (int32_t)rng.below(65));
        check_e(a, (double)rng.below(1000), (int32_t)rng.below(65));
        check_key(a, b);
        /* products near the two clamps and near 1 */
        const double j = 1.0 + (rng.unit() - 0.5) * 0x1p-20;
        check_key(SW_FLT_MAX * j, 1.0);
        check_key(SW_FLT_MIN * j, 1.0);
        check_key(a, SW_FLT_MAX / a * j);
        check_key(a, SW_FLT_MIN / a * j);
        check_key(rng.unit(), 1.0 / (double)(1 + rng.below(8)));
    }
}

/* a key row as setup builds it: v_n ≥ +0 from sw_pos, the running minimum,
 * the scaled key — both forms side by side */
void random_rows(Rng& rng, int count) {
    for (int r = 0; r < count; ++r) {
        const double scale = (r & 3) == 0 ? rng.finite_pos() : sw_key_scale(1 + (int32_t)rng.below(8), rng.unit());
        const double top = (r & 1) ? rng.finite_pos() : rng.unit();
        double vm0 = 0.0, vm1 = 0.0;
        for (int n = 0; n < 32; ++n) {
            const double v = sw_pos(rng.below(8) == 0 ? -rng.unit() : top * rng.unit());
            vm0 = n == 0 ? v : sw_min(vm0, v);
            vm1 = n == 0 ? v : sw_min_nf(vm1, v);
            if (sw_bits(vm0) != sw_bits(vm1)) fail("row min", v, scale, sw_bits(vm1), sw_bits(vm0));
            const uint32_t k0 = sw_fbits_of(sw_key(vm0, scale)), k1 = sw_fbits_of(sw_key_nf(vm1, scale));
            if (k0 != k1) fail("row key", vm0, scale, k1, k0);
            checks += 2;
        }
    }
}

} // namespace

int main(int argc, char** argv) {
    const int count = argc > 1 ? std::atoi(argv[1]) : 1000000;
    Rng rng{0x5EEDull};
    special_cases();
    random_cases(rng, count);
    random_rows(rng, count / 16);
    if (failures) {
        std::fprintf(stderr, "%d mismatches in %llu checks\n", failures, (unsigned long long)checks);
        return 1;
    }
    std::printf("ok %llu\n", (unsigned long long)checks);
    return 0;
}
