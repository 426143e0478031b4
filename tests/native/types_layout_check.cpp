/*
 * types_layout_check.cpp — host check of csrc/sw_types_layout.h, the arithmetic
 * of the worker-type frame.  Stand-alone: built and run by
 * tests/test_types_layout.py, once plain and once with
 * -fsanitize=address,undefined.  Exit status 0 and a line "ok <checks>" when
 * every property holds.
 *
 *   layout  for the column sets of the four policies (centred mmf: one [T·n]
 *           column, shifts, 2 results; mtd: [T·n] and [T], shifts, 4; ftf:
 *           [T·n] and three [T], no shifts, 5; wf: one [T·n], shifts, levels,
 *           4): every view is aligned to its element size, the views tile
 *           in_bytes and out_bytes, every offset equals the formula that the
 *           policy's *_run function held before the frame, written out here,
 *           and in_bytes is that formula's end rounded up to 8
 *   pack    packing a host block of exactly in_bytes reproduces every view;
 *           unpacking a block of exactly out_bytes reproduces x, the levels and
 *           the first W of every W + 1 result words, and the status word
 *   check   the common rejections, their texts and their order
 */
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "sw_types_layout.h"

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

size_t align8(size_t o) { return (o + 7) & ~(size_t)7; }

/* the offsets of one call as its *_run function wrote them by hand */
struct Want {
    size_t col[SW_TYPES_MAX_COLS], workers, shifts, sf, in_bytes, levels, results, out_bytes;
};

struct Policy {
    const char* name;
    int ncols;
    bool per_type[SW_TYPES_MAX_COLS];
    bool shifts, levels;
    int W;
    Want (*want)(size_t C, size_t T, size_t N);
};

const Policy POLICIES[] = {
    {"mmf", 1, {true}, true, false, 2,
     [](size_t C, size_t T, size_t N) {
         const size_t o_coef = (C + 1) * 8, o_w = o_coef + T * N * 8, o_sh = o_w + C * N * 4, o_sf = o_sh + C * 4;
         const size_t in_bytes = align8(o_sf + T * 4);
         const size_t o_lv = T * N * 8, out_bytes = o_lv + C * 3 * 8;
         return Want{{o_coef}, o_w, o_sh, o_sf, in_bytes, o_lv, o_lv, out_bytes};
     }},
    {"mtd", 2, {true, false}, true, false, 4,
     [](size_t C, size_t T, size_t N) {
         const size_t o_thr = (C + 1) * 8, o_st = o_thr + T * N * 8, o_w = o_st + T * 8, o_sh = o_w + C * N * 4,
                      o_sf = o_sh + C * 4;
         const size_t in_bytes = align8(o_sf + T * 4);
         const size_t o_rs = T * N * 8, out_bytes = o_rs + C * 5 * 8;
         return Want{{o_thr, o_st}, o_w, o_sh, o_sf, in_bytes, o_rs, o_rs, out_bytes};
     }},
    {"ftf", 4, {true, false, false, false}, false, false, 5,
     [](size_t C, size_t T, size_t N) {
         const size_t o_thr = (C + 1) * 8, o_st = o_thr + T * N * 8, o_el = o_st + T * 8, o_ex = o_el + T * 8,
                      o_w = o_ex + T * 8, o_sf = o_w + C * N * 4;
         const size_t in_bytes = align8(o_sf + T * 4);
         const size_t o_rs = T * N * 8, out_bytes = o_rs + C * 6 * 8;
         return Want{{o_thr, o_st, o_el, o_ex}, o_w, o_sf, o_sf, in_bytes, o_rs, o_rs, out_bytes};
     }},
    {"wf", 1, {true}, true, true, 4,
     [](size_t C, size_t T, size_t N) {
         const size_t o_coef = (C + 1) * 8, o_w = o_coef + T * N * 8, o_sh = o_w + C * N * 4, o_sf = o_sh + C * 4;
         const size_t in_bytes = align8(o_sf + T * 4);
         const size_t o_lv = T * N * 8, o_rs = o_lv + T * 8, out_bytes = o_rs + C * 5 * 8;
         return Want{{o_coef}, o_w, o_sh, o_sf, in_bytes, o_lv, o_rs, out_bytes};
     }},
};

void check_layout(const Policy& P, const std::vector<int64_t>& sizes, int32_t n) {
    const int32_t count = (int32_t)sizes.size();
    std::vector<int64_t> off(sizes.size() + 1, 0);
    for (size_t i = 0; i < sizes.size(); ++i) off[i + 1] = off[i] + sizes[i];
    const size_t T = (size_t)off.back(), C = sizes.size(), N = (size_t)n;
    expect(sw_types_check(count, n, off.data(), std::vector<int32_t>(C * N + 1, 0).data()) == nullptr,
           "valid call accepted", 0, 0);

    /* every array of exactly its length, so that the sanitizer sees a read past it */
    std::vector<int32_t> workers(C * N), shifts(C), sf(T);
    for (auto& v : workers) v = (int32_t)(rnd() % 1000);
    for (auto& v : shifts) v = (int32_t)(rnd() % 64) - 32;
    for (auto& v : sf) v = 1 + (int32_t)(rnd() % 255);
    std::vector<std::vector<double>> data(P.ncols);
    sw_types_shape S{};
    S.ncols = P.ncols;
    S.shifts = P.shifts;
    S.levels = P.levels;
    S.W = P.W;
    for (int k = 0; k < P.ncols; ++k) {
        data[k].resize(T * (P.per_type[k] ? N : 1));
        for (auto& v : data[k]) v = (double)(rnd() % 100000) / 7.0;
        S.cols[k] = sw_types_col{data[k].data(), P.per_type[k]};
    }

    const sw_types_layout L = sw_types_plan(S, count, n, (int64_t)T);
    const Want w = P.want(C, T, N);
    for (int k = 0; k < P.ncols; ++k) {
        expect(L.col[k] == w.col[k], "column offset formula", (long long)L.col[k], (long long)w.col[k]);
        expect(L.col[k] % 8 == 0, "column aligned", (long long)L.col[k], 8);
        expect(L.col_bytes[k] == data[k].size() * 8, "column length", (long long)L.col_bytes[k], k);
    }
    expect(L.workers == w.workers, "workers offset formula", (long long)L.workers, (long long)w.workers);
    expect(L.shifts == w.shifts, "shifts offset formula", (long long)L.shifts, (long long)w.shifts);
    expect(L.sf == w.sf, "sf offset formula", (long long)L.sf, (long long)w.sf);
    expect(L.in_bytes == w.in_bytes, "in_bytes formula", (long long)L.in_bytes, (long long)w.in_bytes);
    expect(L.levels == w.levels, "levels offset formula", (long long)L.levels, (long long)w.levels);
    expect(L.results == w.results, "results offset formula", (long long)L.results, (long long)w.results);
    expect(L.out_bytes == w.out_bytes, "out_bytes formula", (long long)L.out_bytes, (long long)w.out_bytes);
    /* the views tile the blocks in order, each aligned to its element */
    size_t at = (C + 1) * 8;
    for (int k = 0; k < P.ncols; ++k) {
        expect(L.col[k] == at, "column follows its predecessor", (long long)L.col[k], (long long)at);
        at += L.col_bytes[k];
    }
    expect(L.workers == at && at % 4 == 0, "workers follow the columns", (long long)L.workers, (long long)at);
    at += C * N * 4;
    expect(L.shifts == at && at % 4 == 0, "shifts follow the workers", (long long)L.shifts, (long long)at);
    at += P.shifts ? C * 4 : 0;
    expect(L.sf == at && at % 4 == 0, "sf follows", (long long)L.sf, (long long)at);
    at += T * 4;
    expect(L.in_bytes >= at && L.in_bytes - at < 8 && L.in_bytes % 8 == 0, "sf ends the input block, padded to 8",
           (long long)L.in_bytes, (long long)at);
    expect(L.levels == T * N * 8, "levels follow x", (long long)L.levels, (long long)(T * N * 8));
    expect(L.results == L.levels + (P.levels ? T * 8 : 0), "results follow the levels", (long long)L.results, 0);
    expect(L.out_bytes == L.results + C * (size_t)(P.W + 1) * 8, "results end the output block",
           (long long)L.out_bytes, 0);

    if (T == 0) return; /* the frame leaves a call without jobs before it packs */

    /* pack into exactly in_bytes of a stale block */
    std::vector<unsigned char> in(L.in_bytes, 0xA5);
    sw_types_pack(L, S, off.data(), workers.data(), P.shifts ? shifts.data() : nullptr, sf.data(), in.data());
    expect(memcmp(in.data(), off.data(), (C + 1) * 8) == 0, "offsets packed", 0, 0);
    for (int k = 0; k < P.ncols; ++k)
        expect(L.col_bytes[k] == 0 || memcmp(in.data() + L.col[k], data[k].data(), L.col_bytes[k]) == 0,
               "column packed", k, 0);
    expect(C * N == 0 || memcmp(in.data() + L.workers, workers.data(), C * N * 4) == 0, "workers packed", 0, 0);
    if (P.shifts) expect(memcmp(in.data() + L.shifts, shifts.data(), C * 4) == 0, "shifts packed", 0, 0);
    expect(T == 0 || memcmp(in.data() + L.sf, sf.data(), T * 4) == 0, "sf packed", 0, 0);
    for (size_t i = L.sf + T * 4; i < L.in_bytes; ++i) expect(in[i] == 0xA5, "the padding is left alone", (long long)i, 0);

    /* unpack from exactly out_bytes */
    std::vector<unsigned char> out(L.out_bytes);
    std::vector<double> od(L.out_bytes / 8);
    for (auto& v : od) v = (double)(int)(rnd() % 2001) - 1000.0;
    memcpy(out.data(), od.data(), L.out_bytes);
    const size_t W = (size_t)P.W;
    std::vector<double> x(T * N + 1, -1.0), lv(T + 1, -1.0), rs(C * W + 1, -1.0);
    sw_types_unpack(L, out.data(), x.data(), P.levels ? lv.data() : nullptr, rs.data());
    expect(T * N == 0 || memcmp(x.data(), out.data(), T * N * 8) == 0, "x unpacked", 0, 0);
    if (P.levels) expect(T == 0 || memcmp(lv.data(), out.data() + L.levels, T * 8) == 0, "levels unpacked", 0, 0);
    for (size_t i = 0; i < C; ++i) {
        for (size_t c = 0; c < W; ++c)
            expect(rs[W * i + c] == od[L.results / 8 + (W + 1) * i + c], "result word unpacked", (long long)i, (long long)c);
        expect(sw_types_status(L, out.data(), i) == (int)od[L.results / 8 + (W + 1) * i + W], "status word", (long long)i, 0);
    }
    expect(x[T * N] == -1.0 && lv[P.levels ? T : 0] == -1.0 && rs[C * W] == -1.0, "nothing written past the arrays", 0, 0);
    std::vector<double> x2(T * N + 1, -1.0);
    sw_types_unpack(L, out.data(), x2.data(), P.levels ? lv.data() : nullptr, nullptr); /* results may be null */
    expect(T * N == 0 || memcmp(x2.data(), out.data(), T * N * 8) == 0, "x unpacked without results", 0, 0);
}

void expect_error(const char* what, int32_t n, std::vector<int64_t> off, std::vector<int32_t> workers,
                  const char* want, bool null_offsets = false, bool null_workers = false) {
    const int32_t count = (int32_t)off.size() - 1;
    const char* e = sw_types_check(count, n, null_offsets ? nullptr : off.data(), null_workers ? nullptr : workers.data());
    ++checks;
    const bool ok = want ? (e && strcmp(e, want) == 0) : e == nullptr;
    if (!ok && ++failures <= 10)
        fprintf(stderr, "FAIL %s: got \"%s\", want \"%s\"\n", what, e ? e : "(null)", want ? want : "(null)");
}

void check_rejections() {
    const char* const sizes = "bad sizes or null pointers";
    const char* const start = "offsets must start at 0";
    const char* const decr = "offsets must not decrease";
    const char* const many = "more than 16384 jobs in an instance";
    const char* const neg = "worker counts must be >= 0";
    expect_error("no types", 0, {0, 5}, {}, sizes);
    expect_error("17 types", 17, {0, 5}, std::vector<int32_t>(17, 1), sizes);
    expect_error("16 types accepted", 16, {0, 5}, std::vector<int32_t>(16, 1), nullptr);
    expect_error("null offsets", 2, {0, 5}, {1, 1}, sizes, true, false);
    expect_error("null workers", 2, {0, 5}, {1, 1}, sizes, false, true);
    expect_error("start", 2, {1, 5}, {1, 1}, start);
    expect_error("decreasing", 1, {0, 5, 3}, {2, 2}, decr);
    expect_error("largest instance accepted", 1, {0, 16384}, {2}, nullptr);
    expect_error("oversized instance", 1, {0, 16385}, {2}, many);
    expect_error("worker count 0 accepted", 2, {0, 5}, {0, 0}, nullptr);
    expect_error("negative worker count", 2, {0, 5}, {3, -1}, neg);
    /* two faults at once: the sizes, the start, then instance by instance the offsets before the workers */
    expect_error("sizes before start", 17, {1, 5}, std::vector<int32_t>(17, -1), sizes);
    expect_error("start before decreasing", 1, {1, 0}, {2}, start);
    expect_error("start before workers", 1, {1, 5}, {-1}, start);
    expect_error("decreasing before workers, one instance", 1, {0, -1}, {-1}, decr);
    expect_error("oversized before workers, one instance", 1, {0, 16385}, {-1}, many);
    expect_error("workers of instance 0 before offsets of instance 1", 2, {0, 5, 3}, {1, -1, 2, 2}, neg);
    expect_error("offsets of instance 0 before workers of instance 1", 2, {0, -2, 3}, {2, 2, -1, 0}, decr);
    expect_error("oversized instance 0 before decreasing instance 1", 1, {0, 16385, 3}, {2, 2}, many);
}

}  // namespace

int main() {
    /* odd C, odd T: the int32 tail ends off a multiple of 8 and needs its padding */
    const std::vector<std::vector<int64_t>> shapes = {
        {0}, {1}, {5}, {513}, {0, 0, 0}, {5, 0, 513}, {1, 2, 3, 4, 5, 6, 7}, {1100, 1, 0, 40, 33}, {2, 2}, {3, 4}};
    const int32_t types[] = {1, 3, 16};
    for (const Policy& P : POLICIES)
        for (const auto& s : shapes)
            for (int32_t n : types) check_layout(P, s, n);
    check_rejections();
    if (failures) {
        fprintf(stderr, "%d failures in %llu checks\n", failures, (unsigned long long)checks);
        return 1;
    }
    printf("ok %llu\n", (unsigned long long)checks);
    return 0;
}
