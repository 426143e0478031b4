/*
 * tests/native/wfh_layout_check.cpp — TEST INFRASTRUCTURE: the host arithmetic
 * of a hierarchical water-filling call (csrc/sw_wfh_layout.h) as a stand-alone
 * host program: the views of the two blocks are aligned and tile them, the
 * packed input block is the member order (a stable sort of every instance's
 * jobs by entity, with ebeg and D_e), and a bad call is rejected with its text
 * in the documented order.  Prints "ok <checks>".  Built plain and under the
 * address and undefined-behaviour sanitizers by tests/test_wfh_layout.py.
 */
#include <stdio.h>
#include <stdlib.h>

#include <algorithm>
#include <string>
#include <vector>

#include "sw_wfh_layout.h"

static long checks = 0;
#define CHECK(cond)                                                        \
    do {                                                                   \
        ++checks;                                                          \
        if (!(cond)) {                                                     \
            printf("FAILED line %d: %s\n", __LINE__, #cond);               \
            exit(1);                                                       \
        }                                                                  \
    } while (0)

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint32_t rnd(uint32_t n) {
    rng_state = rng_state * 6364136223846793005ull + 1442695040888963407ull;
    return (uint32_t)(rng_state >> 33) % n;
}

struct Call {
    std::vector<int64_t> off, eoff;
    std::vector<int32_t> workers, sf, ent, modes;
    std::vector<double> c, W, x;
    int32_t count() const { return (int32_t)workers.size(); }
    const char* check() const {
        return sw_wfh_check(count(), off.data(), eoff.data(), sf.data(), c.data(), ent.data(), W.data(),
                            modes.data(), x.data());
    }
};

/* sizes[i] jobs and ents[i] entities in instance i */
static Call make(const std::vector<int>& sizes, const std::vector<int>& ents) {
    Call k;
    k.off.push_back(0);
    k.eoff.push_back(0);
    for (size_t i = 0; i < sizes.size(); ++i) {
        k.off.push_back(k.off.back() + sizes[i]);
        k.eoff.push_back(k.eoff.back() + ents[i]);
        k.workers.push_back(1 + (int32_t)rnd(64));
        for (int j = 0; j < sizes[i]; ++j) {
            k.sf.push_back(1 + (int32_t)rnd(255));
            k.c.push_back(0.25 + rnd(1000) / 7.0);
            k.ent.push_back(ents[i] > 0 ? (int32_t)rnd((uint32_t)ents[i]) : 0);
        }
        for (int e = 0; e < ents[i]; ++e) {
            k.W.push_back(0.5 + rnd(10));
            k.modes.push_back((int32_t)rnd(2));
        }
    }
    k.x.assign(k.sf.size() + 1, 0.0);
    return k;
}

static void check_layout_and_pack(const Call& k) {
    const int32_t C = k.count();
    const int64_t T = k.off[C], Et = k.eoff[C];
    CHECK(k.check() == nullptr);
    const sw_wfh_layout L = sw_wfh_plan(C, T, Et);
    /* the views tile the blocks in this order, each aligned to its element */
    const size_t in_views[][2] = {{0, 8}, {L.eoffs, 8}, {L.ebeg, 8}, {L.D, 8}, {L.c, 8}, {L.W, 8},
                                  {L.sf, 4}, {L.mem, 4}, {L.mode, 4}, {L.workers, 4}};
    const size_t in_len[] = {(size_t)C + 1, (size_t)C + 1, (size_t)Et + 1, (size_t)Et, (size_t)T, (size_t)Et,
                             (size_t)T, (size_t)T, (size_t)Et, (size_t)C};
    size_t o = 0;
    for (int v = 0; v < 10; ++v) {
        CHECK(in_views[v][0] == o);
        CHECK(o % in_views[v][1] == 0);
        o += in_len[v] * in_views[v][1];
    }
    CHECK(L.in_bytes == o);
    CHECK(L.g == (size_t)T * 8 && L.levels == L.g + (size_t)Et * 8);
    CHECK(L.back_bytes == L.levels + (size_t)C * 16 && L.K == L.back_bytes && L.out_bytes == L.K + (size_t)Et * 8);

    /* guard bytes on both sides of the packed block */
    std::vector<unsigned char> buf(L.in_bytes + 32, 0xA5);
    unsigned char* in = buf.data() + 16;
    sw_wfh_pack(L, k.off.data(), k.eoff.data(), k.workers.data(), k.sf.data(), k.c.data(), k.ent.data(),
                k.W.data(), k.modes.data(), in);
    for (int b = 0; b < 16; ++b) CHECK(buf[b] == 0xA5 && buf[16 + L.in_bytes + b] == 0xA5);
    const int64_t* off = (const int64_t*)in;
    const int64_t* eoff = (const int64_t*)(in + L.eoffs);
    const int64_t* ebeg = (const int64_t*)(in + L.ebeg);
    const int64_t* D = (const int64_t*)(in + L.D);
    const double* c = (const double*)(in + L.c);
    const double* W = (const double*)(in + L.W);
    const int32_t* sf = (const int32_t*)(in + L.sf);
    const int32_t* mem = (const int32_t*)(in + L.mem);
    const int32_t* mode = (const int32_t*)(in + L.mode);
    const int32_t* wk = (const int32_t*)(in + L.workers);
    for (int32_t i = 0; i <= C; ++i) CHECK(off[i] == k.off[i] && eoff[i] == k.eoff[i]);
    for (int32_t i = 0; i < C; ++i) CHECK(wk[i] == k.workers[i]);
    for (int64_t e = 0; e < Et; ++e) CHECK(W[e] == k.W[e] && mode[e] == k.modes[e]);
    CHECK(ebeg[Et] == T);
    for (int32_t i = 0; i < C; ++i) {
        const int64_t j0 = k.off[i], j1 = k.off[i + 1], e0 = k.eoff[i], e1 = k.eoff[i + 1];
        /* the reference order: a stable sort of the instance's jobs by entity */
        std::vector<int32_t> order;
        for (int64_t j = j0; j < j1; ++j) order.push_back((int32_t)(j - j0));
        std::stable_sort(order.begin(), order.end(),
                         [&](int32_t a, int32_t b) { return k.ent[j0 + a] < k.ent[j0 + b]; });
        for (int64_t p = j0; p < j1; ++p) {
            const int32_t j = order[(size_t)(p - j0)];
            CHECK(mem[p] == j && sf[p] == k.sf[j0 + j] && c[p] == k.c[j0 + j]);
        }
        int64_t p = j0;
        for (int64_t e = e0; e < e1; ++e) {
            CHECK(ebeg[e] == p);
            int64_t d = 0;
            while (p < j1 && k.ent[j0 + mem[p]] == e - e0) d += sf[p++];
            CHECK(D[e] == d);
        }
        CHECK(p == j1);
        if (e1 > e0) CHECK(ebeg[e0] == j0);
    }
}

static void expect(const Call& k, const char* text) {
    const char* e = k.check();
    CHECK(e != nullptr && std::string(e) == text);
}

int main() {
    check_layout_and_pack(make({1}, {1}));
    check_layout_and_pack(make({5}, {3}));
    check_layout_and_pack(make({0}, {2}));
    check_layout_and_pack(make({0, 7, 0}, {0, 4, 1}));
    check_layout_and_pack(make({513, 64, 1, 0, 65}, {9, 64, 1, 0, 200}));
    for (int r = 0; r < 40; ++r) {
        std::vector<int> sizes, ents;
        const int C = 1 + (int)rnd(6);
        for (int i = 0; i < C; ++i) {
            sizes.push_back((int)rnd(70));
            ents.push_back(sizes.back() ? 1 + (int)rnd(12) : (int)rnd(3));
        }
        check_layout_and_pack(make(sizes, ents));
    }

    /* rejections, and their order: entity offsets, null pointers, jobs, entities, entity indices */
    const Call ok = make({4, 3}, {2, 3});
    CHECK(ok.check() == nullptr);
    { Call k = ok; k.eoff[0] = 1; expect(k, "entity offsets must start at 0"); }
    { Call k = ok; k.eoff[1] = 6; expect(k, "entity offsets must not decrease"); }
    { Call k = ok; k.eoff[0] = 1; k.sf[0] = 0; expect(k, "entity offsets must start at 0"); }
    {
        const Call& k = ok;
        const char* e = sw_wfh_check(k.count(), k.off.data(), k.eoff.data(), nullptr, k.c.data(), k.ent.data(),
                                     k.W.data(), k.modes.data(), k.x.data());
        CHECK(e && std::string(e) == "null pointers");
        e = sw_wfh_check(k.count(), k.off.data(), k.eoff.data(), k.sf.data(), k.c.data(), k.ent.data(), nullptr,
                         k.modes.data(), k.x.data());
        CHECK(e && std::string(e) == "null pointers");
        e = sw_wfh_check(k.count(), k.off.data(), k.eoff.data(), k.sf.data(), k.c.data(), k.ent.data(), k.W.data(),
                         k.modes.data(), nullptr);
        CHECK(e && std::string(e) == "null pointers");
    }
    const char* job_rule = "scale factors must be in [1,255], coefficients finite and > 0";
    { Call k = ok; k.sf[2] = 0; expect(k, job_rule); }
    { Call k = ok; k.sf[6] = 256; expect(k, job_rule); }
    { Call k = ok; k.c[1] = 0.0; expect(k, job_rule); }
    { Call k = ok; k.c[1] = -1.0; expect(k, job_rule); }
    { Call k = ok; k.c[5] = NAN; expect(k, job_rule); }
    { Call k = ok; k.c[5] = INFINITY; expect(k, job_rule); }
    { Call k = ok; k.W[0] = 0.0; expect(k, "entity weights must be finite and > 0"); }
    { Call k = ok; k.W[4] = -2.0; expect(k, "entity weights must be finite and > 0"); }
    { Call k = ok; k.W[4] = NAN; expect(k, "entity weights must be finite and > 0"); }
    { Call k = ok; k.W[1] = INFINITY; expect(k, "entity weights must be finite and > 0"); }
    { Call k = ok; k.modes[3] = 2; expect(k, "entity modes must be 0 (fairness) or 1 (fifo)"); }
    { Call k = ok; k.modes[0] = -1; expect(k, "entity modes must be 0 (fairness) or 1 (fifo)"); }
    { Call k = ok; k.ent[0] = 2; expect(k, "entity_of_job must be in [0, num_entities)"); } /* instance 0 has 2 */
    { Call k = ok; k.ent[5] = 3; expect(k, "entity_of_job must be in [0, num_entities)"); }
    { Call k = ok; k.ent[5] = -1; expect(k, "entity_of_job must be in [0, num_entities)"); }
    { Call k = ok; k.ent[5] = 2; CHECK(k.check() == nullptr); }                            /* instance 1 has 3 */
    { Call k = ok; k.sf[0] = 0; k.W[0] = 0.0; k.ent[0] = 9; expect(k, job_rule); }
    { Call k = ok; k.W[0] = 0.0; k.ent[0] = 9; expect(k, "entity weights must be finite and > 0"); }
    { Call k = make({3}, {0}); expect(k, "entity_of_job must be in [0, num_entities)"); }  /* jobs, no entity */
    printf("ok %ld\n", checks);
    return 0;
}
