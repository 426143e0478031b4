/*
 * alloc_layout_check.cpp — host check of csrc/sw_alloc_layout.h, the arithmetic
 * of the allocation frame.  Stand-alone: built and run by
 * tests/test_alloc_layout.py, once plain and once with
 * -fsanitize=address,undefined.  Exit status 0 and a line "ok <checks>" when
 * every property holds.
 *
 *   layout  for the column sets of the four policies (ftf: 3 doubles, wf and
 *           mtd: 1, mst: 2 with the second absent; levels of 2 and 4): every
 *           view is aligned to its element size, the views tile in_bytes and
 *           out_bytes, and both equal the policy's formula written out here
 *   pack    packing a host block of exactly in_bytes reproduces every column,
 *           an absent column reads as zeros; unpacking a block of exactly
 *           out_bytes reproduces x and the levels
 *   maxq    ⌈n/512⌉ of the largest instance of at most LDS_JOBS jobs, 0 above,
 *           0 when the environment switch begins with '0'
 *   scan    the rejections, their texts and their order
 */
#include <climits>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "sw_alloc_layout.h"

namespace {

uint64_t checks = 0;
int failures = 0;

void expect(bool ok, const char* what, long long a, long long b) {
    ++checks;
    if (!ok && ++failures <= 10) fprintf(stderr, "FAIL %s: %lld %lld\n", what, a, b);
}

uint64_t rng_state = 0x9E3779B97F4A7C15ull;
uint64_t rnd() { /* splitmix64 */
    uint64_t z = (rng_state += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

const char* const ENV = "SW_ALLOC_LAYOUT_CHECK_LDS";
const char* const RULE = "worker counts must be > 0";

struct Policy {
    const char* name;
    int doubles;  /* 8-byte columns, before the one 4-byte column */
    int absent;   /* index of the column passed as null, or -1 */
    int W;
    size_t (*in_bytes)(size_t C, size_t T);
    size_t (*out_bytes)(size_t C, size_t T);
};

/* the formulas of sw_ftf.hip, sw_wf.hip, sw_mtd.hip and sw_mst.hip, written out */
const Policy POLICIES[] = {
    {"ftf", 3, -1, 2, [](size_t C, size_t T) { return (C + 1) * 8 + T * 8 + T * 8 + T * 8 + T * 4 + C * 4; },
     [](size_t C, size_t T) { return T * 8 + C * 16; }},
    {"wf", 1, -1, 2, [](size_t C, size_t T) { return (C + 1) * 8 + T * 8 + T * 4 + C * 4; },
     [](size_t C, size_t T) { return T * 8 + C * 16; }},
    {"mtd", 1, -1, 2, [](size_t C, size_t T) { return (C + 1) * 8 + T * 8 + T * 4 + C * 4; },
     [](size_t C, size_t T) { return T * 8 + C * 16; }},
    {"mst", 2, 1, 4, [](size_t C, size_t T) { return (C + 1) * 8 + T * 8 + T * 8 + T * 4 + C * 4; },
     [](size_t C, size_t T) { return T * 8 + C * 32; }},
};

void check_layout(const Policy& P, const std::vector<int64_t>& sizes) {
    const int32_t count = (int32_t)sizes.size();
    std::vector<int64_t> off(sizes.size() + 1, 0);
    for (size_t i = 0; i < sizes.size(); ++i) off[i + 1] = off[i] + sizes[i];
    if (off.back() < 0 || off.back() > (1 << 20)) abort(); /* the shapes below are small */
    const size_t T = (size_t)off.back(), C = sizes.size();
    std::vector<int32_t> workers(C);
    for (auto& g : workers) g = 1 + (int32_t)(rnd() % 1000);

    /* the columns' data: element j of column k is recognisable */
    const int ncols = P.doubles + 1;
    std::vector<std::vector<unsigned char>> data(ncols);
    sw_alloc_col cols[SW_ALLOC_MAX_COLS];
    for (int k = 0; k < ncols; ++k) {
        const size_t size = k < P.doubles ? 8 : 4;
        data[k].resize(T * size + 1);
        for (auto& b : data[k]) b = (unsigned char)rnd();
        cols[k] = sw_alloc_col{k == P.absent ? nullptr : (const void*)data[k].data(), size, k == P.absent};
    }

    const sw_alloc_layout L = sw_alloc_plan(cols, ncols, count, (int64_t)T, P.W);
    expect(L.in_bytes == P.in_bytes(C, T), "in_bytes formula", (long long)L.in_bytes, (long long)P.in_bytes(C, T));
    expect(L.out_bytes == P.out_bytes(C, T), "out_bytes formula", (long long)L.out_bytes,
           (long long)P.out_bytes(C, T));
    /* the views tile the input block in order, each aligned to its element */
    size_t at = (C + 1) * 8;
    for (int k = 0; k < ncols; ++k) {
        expect(L.col[k] == at, "column follows its predecessor", (long long)L.col[k], (long long)at);
        expect(L.col[k] % cols[k].size == 0, "column aligned", (long long)L.col[k], (long long)cols[k].size);
        at += T * cols[k].size;
    }
    expect(L.workers == at, "workers follow the columns", (long long)L.workers, (long long)at);
    expect(L.workers % 4 == 0, "workers aligned", (long long)L.workers, 4);
    expect(L.in_bytes == at + C * 4, "workers end the input block", (long long)L.in_bytes, (long long)(at + C * 4));
    expect(L.levels == T * 8 && L.levels % 8 == 0, "levels follow x", (long long)L.levels, (long long)(T * 8));
    expect(L.out_bytes == L.levels + C * (size_t)P.W * 8, "levels end the output block", (long long)L.out_bytes, 0);

    /* pack into exactly in_bytes of a stale block */
    std::vector<unsigned char> in(L.in_bytes, 0xA5);
    sw_alloc_pack(L, cols, off.data(), workers.data(), in.data());
    expect(memcmp(in.data(), off.data(), (C + 1) * 8) == 0, "offsets packed", 0, 0);
    for (int k = 0; k < ncols; ++k) {
        const size_t n = T * cols[k].size;
        if (k == P.absent) {
            size_t nz = 0;
            for (size_t i = 0; i < n; ++i) nz += in[L.col[k] + i] != 0;
            expect(nz == 0, "absent column reads as zeros", (long long)nz, k);
        } else {
            expect(n == 0 || memcmp(in.data() + L.col[k], data[k].data(), n) == 0, "column packed", k, 0);
        }
    }
    expect(C == 0 || memcmp(in.data() + L.workers, workers.data(), C * 4) == 0, "workers packed", 0, 0);

    /* unpack from exactly out_bytes */
    std::vector<unsigned char> out(L.out_bytes);
    for (auto& b : out) b = (unsigned char)rnd();
    std::vector<double> x(T + 1, -1.0), lv(C * (size_t)P.W + 1, -1.0);
    sw_alloc_unpack(L, out.data(), x.data(), lv.data());
    expect(T == 0 || memcmp(x.data(), out.data(), T * 8) == 0, "x unpacked", 0, 0);
    expect(memcmp(lv.data(), out.data() + L.levels, C * (size_t)P.W * 8) == 0, "levels unpacked", 0, 0);
    expect(x[T] == -1.0 && lv[C * (size_t)P.W] == -1.0, "nothing written past x and levels", 0, 0);
    std::vector<double> x2(T + 1, -1.0);
    sw_alloc_unpack(L, out.data(), x2.data(), nullptr); /* levels may be null */
    expect(T == 0 || memcmp(x2.data(), out.data(), T * 8) == 0, "x unpacked without levels", 0, 0);
}

int32_t maxq_of(const std::vector<int64_t>& sizes, int32_t lds_jobs) {
    std::vector<int64_t> off(sizes.size() + 1, 0);
    for (size_t i = 0; i < sizes.size(); ++i) off[i + 1] = off[i] + sizes[i];
    std::vector<int32_t> workers(sizes.size(), 3);
    int32_t maxq = -1;
    const char* e = sw_alloc_scan((int32_t)sizes.size(), off.data(), workers.data(), RULE, lds_jobs, ENV, &maxq);
    expect(e == nullptr, "valid call accepted", 0, 0);
    return maxq;
}

void check_maxq(int32_t J) {
    unsetenv(ENV);
    const int64_t ns[] = {0, 1, 511, 512, 513, J, J + 1};
    for (int64_t n : ns) {
        const int32_t want = n <= J ? (int32_t)((n + 511) / 512) : 0;
        const int32_t got = maxq_of({n}, J);
        expect(got == want, "maxq of one instance", got, want);
    }
    expect(maxq_of({J}, J) == J / 512, "an instance of LDS_JOBS is staged", maxq_of({J}, J), J / 512);
    expect(maxq_of({J + 1}, J) == 0, "one job more is not", maxq_of({J + 1}, J), 0);
    expect(maxq_of({J + 1, J, 0}, J) == J / 512, "a batch mixing the two", maxq_of({J + 1, J, 0}, J), J / 512);
    expect(maxq_of({513, J + 1, 1}, J) == 2, "a batch mixing the two (small)", maxq_of({513, J + 1, 1}, J), 2);
    setenv(ENV, "0", 1);
    expect(maxq_of({J}, J) == 0, "the switch forces 0", maxq_of({J}, J), 0);
    expect(maxq_of({513, J + 1, 1}, J) == 0, "the switch forces 0 (batch)", maxq_of({513, J + 1, 1}, J), 0);
    setenv(ENV, "1", 1);
    expect(maxq_of({513}, J) == 2, "the switch at 1 stages", maxq_of({513}, J), 2);
    unsetenv(ENV);
}

void expect_error(const char* what, std::vector<int64_t> off, std::vector<int32_t> workers, const char* rule,
                  const char* want) {
    int32_t maxq = -1;
    const char* e = sw_alloc_scan((int32_t)workers.size(), off.data(), workers.data(), rule, 2048, ENV, &maxq);
    ++checks;
    const bool ok = want ? (e && strcmp(e, want) == 0) : e == nullptr;
    if (!ok && ++failures <= 10) fprintf(stderr, "FAIL %s: got \"%s\", want \"%s\"\n", what, e ? e : "(null)", want ? want : "(null)");
    if (want) expect(maxq == 0, "maxq is 0 on a rejected call", maxq, 0);
}

void check_scan() {
    const int64_t big = (int64_t)INT32_MAX - 512;
    const char* const start = "offsets must start at 0";
    const char* const decr = "offsets must not decrease";
    const char* const rule1 = "worker counts must be >= 1";
    expect_error("start", {1, 5}, {2}, RULE, start);
    expect_error("decreasing", {0, 5, 3}, {2, 2}, RULE, decr);
    expect_error("largest instance accepted", {0, big}, {2}, RULE, nullptr);
    expect_error("oversized instance", {0, big + 1}, {2}, RULE, decr);
    expect_error("worker count 0", {0, 5}, {0}, RULE, RULE);
    expect_error("worker count 0, the other wording", {0, 5}, {0}, rule1, rule1);
    expect_error("negative worker count", {0, 5}, {-3}, RULE, RULE);
    /* two faults at once: the start, then instance by instance the offsets before the workers */
    expect_error("start before decreasing", {1, 0}, {2}, RULE, start);
    expect_error("start before workers", {1, 5}, {0}, RULE, start);
    expect_error("decreasing before workers, one instance", {0, -1}, {0}, RULE, decr);
    expect_error("oversized before workers, one instance", {0, big + 1}, {0}, RULE, decr);
    expect_error("workers of instance 0 before offsets of instance 1", {0, 5, 3}, {0, 2}, RULE, RULE);
    expect_error("offsets of instance 0 before workers of instance 1", {0, -2, 3}, {2, 0}, RULE, decr);
}

}  // namespace

int main() {
    const std::vector<std::vector<int64_t>> shapes = {
        {0}, {1}, {511}, {512}, {513}, {3073}, {0, 0}, {5, 0, 513}, {1, 2, 3, 4, 5, 6, 7}, {2049, 1, 0, 4097}};
    for (const Policy& P : POLICIES)
        for (const auto& s : shapes) check_layout(P, s);
    const int32_t lds_jobs[] = {2048, 3072, 4096};
    for (int32_t J : lds_jobs) check_maxq(J);
    check_scan();
    if (failures) {
        fprintf(stderr, "%d failures in %llu checks\n", failures, (unsigned long long)checks);
        return 1;
    }
    printf("ok %llu\n", (unsigned long long)checks);
    return 0;
}
