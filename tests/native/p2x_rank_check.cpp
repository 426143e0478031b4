/*
 * tests/native/p2x_rank_check.cpp — TEST INFRASTRUCTURE, NOT PRODUCT CODE.
 *
 * csrc/sw_p2x_rank.h on the host: the rank order taken from a candidate order
 * (stable partition by class, then a strict check of neighbours) against
 * std::sort on the exchange key (class asc, sw_p2x_ckey(c) desc, job asc).
 * For every case the program states what must happen — the candidate is
 * accepted exactly when its partition by class is the sorted order — and
 * checks both directions; where it is accepted the staged sequence must be
 * the sorted one.  Prints "ok <checks>"; any mismatch prints the case and
 * exits 1.  Built and run by tests/test_p2x_rank.py, plain and under the
 * address and undefined-behaviour sanitizers.
 */
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>

#include "sw_p2x.h"
#include "sw_p2x_rank.h"

namespace {

struct Job {
    int32_t job, w;
    double c;
};

long g_checks = 0;

[[noreturn]] void fail(const char* what, const char* name, int a, int b) {
    std::printf("FAIL %s: %s (%d, %d)\n", name, what, a, b);
    std::exit(1);
}

double from_bits(uint64_t u) {
    double d;
    std::memcpy(&d, &u, 8);
    return d;
}
uint64_t bits_of(double d) {
    uint64_t u;
    std::memcpy(&u, &d, 8);
    return u;
}

/* One instance: the active jobs and a candidate (indices into jobs, any
 * length, repeats allowed). */
void check(const char* name, const std::vector<Job>& jobs, const std::vector<int>& cand, int want /* -1: derive */) {
    const int A = (int)jobs.size();
    /* classes ascending */
    std::vector<int32_t> wc;
    for (const Job& j : jobs) wc.push_back(j.w);
    std::sort(wc.begin(), wc.end());
    wc.erase(std::unique(wc.begin(), wc.end()), wc.end());
    const int K = (int)wc.size();
    if (K < 1 || K > SW_P2X_KMAX) fail("bad case: class count", name, K, 0);
    auto cls = [&](int32_t w) { return (int32_t)(std::lower_bound(wc.begin(), wc.end(), w) - wc.begin()); };
    std::vector<int32_t> off(K + 1, 0);
    for (const Job& j : jobs) off[cls(j.w) + 1]++;
    for (int k = 0; k < K; ++k) off[k + 1] += off[k];
    /* the reference: std::sort on the exchange key */
    std::vector<int> ref(A);
    for (int i = 0; i < A; ++i) ref[i] = i;
    std::sort(ref.begin(), ref.end(), [&](int x, int y) {
        const int kx = cls(jobs[x].w), ky = cls(jobs[y].w);
        if (kx != ky) return kx < ky;
        const uint64_t cx = sw_p2x_ckey(jobs[x].c), cy = sw_p2x_ckey(jobs[y].c);
        if (cx != cy) return cx > cy;
        return jobs[x].job < jobs[y].job;
    });
    /* what must happen: the candidate's stable partition by class is ref */
    std::vector<int> part;
    for (int k = 0; k < K; ++k)
        for (int i : cand)
            if (cls(jobs[i].w) == k) part.push_back(i);
    const int expect = (int)cand.size() == A && part == ref;
    if (want >= 0 && want != expect) fail("bad case: the stated expectation is not the derived one", name, want, expect);
    /* the header under test */
    const int n = (int)cand.size();
    std::vector<int32_t> k_(n), job_(n), dst(n, -7), sjob(A > 0 ? A : 1, -1);
    std::vector<uint64_t> key_(n), skey(A > 0 ? A : 1, 0);
    for (int q = 0; q < n; ++q) {
        k_[q] = cls(jobs[cand[q]].w);
        key_[q] = sw_p2x_ckey(jobs[cand[q]].c);
        job_[q] = jobs[cand[q]].job;
    }
    const int got = sw_p2x_rank_place(n, A, K, off.data(), k_.data(), key_.data(), job_.data(), dst.data(),
                                      skey.data(), sjob.data());
    ++g_checks;
    if (got != expect) fail(expect ? "a sorted candidate was refused" : "an unsorted candidate was accepted", name, got, expect);
    if (got) {
        for (int p = 0; p < A; ++p) {
            ++g_checks;
            if (sjob[p] != jobs[ref[p]].job || skey[p] != sw_p2x_ckey(jobs[ref[p]].c))
                fail("accepted, but the staged sequence is not the sorted one", name, p, sjob[p]);
        }
        for (int q = 0; q < n; ++q) {
            ++g_checks;
            if (dst[q] < 0 || dst[q] >= A || ref[dst[q]] != cand[q]) fail("accepted, but a destination is wrong", name, q, dst[q]);
        }
    }
}

/* the candidates of one instance: the order by (ckey desc, job asc) without
 * the class (a density-like order: accepted), and its damaged forms */
void check_all(const char* name, const std::vector<Job>& jobs, std::mt19937_64& rng) {
    const int A = (int)jobs.size();
    std::vector<int> good(A);
    for (int i = 0; i < A; ++i) good[i] = i;
    std::sort(good.begin(), good.end(), [&](int x, int y) {
        const uint64_t cx = sw_p2x_ckey(jobs[x].c), cy = sw_p2x_ckey(jobs[y].c);
        if (cx != cy) return cx > cy;
        return jobs[x].job < jobs[y].job;
    });
    check(name, jobs, good, 1);
    /* classes one after another is the sorted order itself */
    std::vector<int> byclass = good;
    std::stable_sort(byclass.begin(), byclass.end(), [&](int x, int y) { return jobs[x].w < jobs[y].w; });
    check(name, jobs, byclass, 1);
    /* classes in descending order, each sorted: the partition restores it */
    std::vector<int> rev_classes = good;
    std::stable_sort(rev_classes.begin(), rev_classes.end(), [&](int x, int y) { return jobs[x].w > jobs[y].w; });
    check(name, jobs, rev_classes, 1);
    if (A >= 2) {
        std::vector<int> rev(good.rbegin(), good.rend());
        /* reversed: refused unless every class has one member */
        check(name, jobs, rev, -1);
        /* two neighbours of one class swapped, at every place (few) or at random places */
        for (int rep = 0; rep < (A <= 70 ? A - 1 : 24); ++rep) {
            const int q = A <= 70 ? rep : (int)(rng() % (uint64_t)(A - 1));
            std::vector<int> sw = good;
            std::swap(sw[q], sw[q + 1]);
            check(name, jobs, sw, jobs[good[q]].w == jobs[good[q + 1]].w ? 0 : 1);
        }
        /* a job repeated in place of another */
        std::vector<int> dup = good;
        dup[A - 1] = dup[0];
        check(name, jobs, dup, 0);
        dup = good;
        dup[0] = dup[A / 2];
        check(name, jobs, dup, A / 2 == 0 ? 1 : 0);
        /* a random permutation */
        std::vector<int> perm = good;
        std::shuffle(perm.begin(), perm.end(), rng);
        check(name, jobs, perm, -1);
    }
    /* one position short, one too many */
    std::vector<int> shrt(good.begin(), good.end() - 1);
    check(name, jobs, shrt, 0);
    std::vector<int> lng = good;
    lng.push_back(good[0]);
    check(name, jobs, lng, 0);
}

std::vector<Job> random_jobs(std::mt19937_64& rng, int A, const std::vector<int>& widths, int cmode) {
    std::vector<Job> v(A);
    std::uniform_real_distribution<double> U(0.05, 10.0);
    const double few[4] = {0.25, 0.5, 1.0, 1.5};
    for (int i = 0; i < A; ++i) {
        v[i].job = 3 * i + 1;
        v[i].w = widths[rng() % widths.size()];
        v[i].c = cmode == 0 ? U(rng) : cmode == 1 ? few[rng() % 4] : (double)(1 + rng() % 8) / (double)(1 + rng() % 32);
    }
    /* every width present, so K is the list's */
    for (size_t k = 0; k < widths.size() && (int)k < A; ++k) v[k].w = widths[k];
    return v;
}

} // namespace

int main(int argc, char** argv) {
    const int nrandom = argc > 1 ? std::atoi(argv[1]) : 200;
    std::mt19937_64 rng(20240611);
    const std::vector<std::vector<int>> wsets = {{1}, {1, 2, 4, 8}, {1, 2, 3, 5, 6, 7, 12}, {3, 5, 6, 7},
                                                 {1, 2, 3, 4, 5, 6, 8, 12}};
    /* sizes: the wave edges and the block's */
    for (int A : {1, 2, 63, 64, 65, 511, 512})
        for (size_t s = 0; s < wsets.size(); ++s)
            for (int cmode = 0; cmode < 3; ++cmode) {
                char name[64];
                std::snprintf(name, sizeof name, "A%d_wset%zu_c%d", A, s, cmode);
                check_all(name, random_jobs(rng, A, wsets[s], cmode), rng);
            }
    /* all-equal c: the order falls to the job */
    for (int A : {2, 64, 65, 200}) {
        std::vector<Job> v = random_jobs(rng, A, wsets[1], 0);
        for (Job& j : v) j.c = 0.75;
        check_all("equal_c", v, rng);
    }
    /* classes of 64 and 65 members; K = 1 and K = 8 */
    for (int M : {64, 65}) {
        std::vector<Job> v;
        for (int i = 0; i < M; ++i) v.push_back({2 * i, 1, 0.0});
        for (int i = 0; i < M; ++i) v.push_back({2 * i + 1, 2, 0.0});
        std::uniform_real_distribution<double> U(0.05, 10.0);
        for (Job& j : v) j.c = U(rng);
        check_all(M == 64 ? "class64" : "class65", v, rng);
        std::vector<Job> one(v.begin(), v.begin() + M);
        check_all(M == 64 ? "K1_M64" : "K1_M65", one, rng);
    }
    check_all("K8", random_jobs(rng, 300, wsets[4], 0), rng);
    /* near ties: pairs equal in the leading 42 mantissa bits (and above) and
     * different below, the later job the larger — the density key (the bits
     * above the lowest 11) ties and puts the earlier job first, the exchange
     * key (above the lowest 3) puts the later one first: such a candidate
     * must be refused */
    for (int A : {2, 64, 130}) {
        std::vector<Job> v = random_jobs(rng, A, wsets[0], 0);
        for (int i = 0; i + 1 < A; i += 2) {
            const uint64_t b = bits_of(v[i].c) & ~0x3FFull;
            v[i].c = from_bits(b);
            v[i + 1].c = from_bits(b | (8ull << (rng() % 7))); /* a bit in 3 … 9 */
        }
        std::vector<int> dens(A);
        for (int i = 0; i < A; ++i) dens[i] = i;
        std::sort(dens.begin(), dens.end(), [&](int x, int y) {
            const uint64_t kx = bits_of(v[x].c) >> 11, ky = bits_of(v[y].c) >> 11;
            if (kx != ky) return kx > ky;
            return v[x].job < v[y].job;
        });
        check("near_tie_density_order", v, dens, 0);
        check_all("near_tie", v, rng);
        /* ties below the exchange key's own cut (the lowest 3 bits): equal keys, job order holds */
        for (int i = 0; i + 1 < A; i += 2) v[i + 1].c = from_bits(bits_of(v[i].c) | (1ull + rng() % 7));
        std::sort(dens.begin(), dens.end(), [&](int x, int y) {
            const uint64_t kx = bits_of(v[x].c) >> 11, ky = bits_of(v[y].c) >> 11;
            if (kx != ky) return kx > ky;
            return v[x].job < v[y].job;
        });
        check("tie_below_key_density_order", v, dens, 1);
    }
    /* random instances */
    for (int i = 0; i < nrandom; ++i) {
        const int A = 1 + (int)(rng() % 512);
        check_all("random", random_jobs(rng, A, wsets[rng() % wsets.size()], (int)(rng() % 3)), rng);
    }
    std::printf("ok %ld\n", g_checks);
    return 0;
}
