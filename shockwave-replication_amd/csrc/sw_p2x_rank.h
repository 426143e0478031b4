/*
 * sw_p2x_rank.h — the P2 exchange step's rank order taken from a candidate
 * order instead of a sort (sw_p2x_dev.h).  Plain C99 + HIP
 * qualifiers: the index arithmetic and the check, shared by the device set-up
 * and the host program tests/native/p2x_rank_check.cpp.
 *
 * The rank order is (class asc, sw_p2x_ckey(c) desc, job asc).  A candidate
 * is the active jobs as a sequence of positions q = 0 … A − 1 (the density
 * pack's order, which agrees with the rank order inside a class unless two
 * keys tie in their leading bits).  Position q of class k goes to
 *     dst = off[k] + (number of earlier positions of class k)
 * — a stable partition by class — and the partitioned sequence is accepted
 * exactly when, inside every class, each entry strictly follows its
 * predecessor in (ckey desc, job asc).  Jobs are distinct, so the keys are,
 * and a sequence that ascends strictly inside each class with the classes in
 * off order is the one sorted sequence; any other candidate (a repeated job
 * included: equal neighbours are not strictly ordered) is refused and the
 * caller sorts.
 */
#ifndef SW_P2X_RANK_H
#define SW_P2X_RANK_H

#include <stddef.h>
#include <stdint.h>

#include "sw_arith.h"

/* (ka, ja) strictly before (kb, jb): key descending, then job ascending */
SW_HD int sw_p2x_rank_before(uint64_t ka, int32_t ja, uint64_t kb, int32_t jb) {
    return ka > kb || (ka == kb && ja < jb);
}

/* A position's rank among its wave's 64: same = the lanes of its class
 * (a ballot), lane its own. */
SW_HD int32_t sw_p2x_rank_lane(uint64_t same, int32_t lane) {
    return (int32_t)__builtin_popcountll(same & ((1ull << (lane & 63)) - 1ull));
}

/* Destination of the r-th position (from 0) of class k, −1 when the class
 * has no room for it (more candidates of a class than it has members: the
 * candidate is not a permutation of the active jobs). */
SW_HD int32_t sw_p2x_rank_dst(const int32_t* off, int32_t k, int32_t r) {
    const int32_t d = off[k] + r;
    return d < off[k + 1] ? d : -1;
}

/* The check of the staged entry at dst (class k): the first of its class, or
 * strictly after its predecessor. */
SW_HD int sw_p2x_rank_ok(const uint64_t* skey, const int32_t* sjob, const int32_t* off, int32_t k,
                         int32_t dst) {
    return dst == off[k] || sw_p2x_rank_before(skey[dst - 1], sjob[dst - 1], skey[dst], sjob[dst]);
}

/* Bytes of the staging area for A positions and a job → active index table of
 * njobs 16-bit entries: keys, jobs, table (16-byte aligned parts). */
SW_HD size_t sw_p2x_rank_bytes(int32_t A, int32_t njobs) {
    return (((size_t)A * 8 + 15) & ~(size_t)15) + (((size_t)A * 4 + 15) & ~(size_t)15) +
           (((size_t)njobs * 2 + 15) & ~(size_t)15);
}

/* The whole placement, sequentially, in the device's order of operations
 * (ranks per 64-position wave from ballots, then the waves' counts added):
 * positions q < n with class cls[q] (< K), key ckey[q] and job job[q] against
 * the classes' offsets off[0 … K] (off[K] = A).  Fills dst[q] and the staging
 * arrays (A entries each) and returns 1 when the candidate is accepted: then
 * skey / sjob in dst order are the sorted sequence.  n ≠ A is refused. */
SW_HD int sw_p2x_rank_place(int32_t n, int32_t A, int32_t K, const int32_t* off, const int32_t* cls,
                            const uint64_t* ckey, const int32_t* job, int32_t* dst, uint64_t* skey,
                            int32_t* sjob) {
    int32_t cnt[8]; /* SW_P2X_KMAX */
    int ok = 1;
    if (n != A || K < 1 || K > 8) return 0;
    for (int32_t k = 0; k < K; ++k) cnt[k] = 0;
    for (int32_t q0 = 0; q0 < n; q0 += 64) {
        const int32_t m = n - q0 < 64 ? n - q0 : 64;
        for (int32_t k = 0; k < K; ++k) {
            uint64_t same = 0;
            for (int32_t l = 0; l < m; ++l) same |= (uint64_t)(cls[q0 + l] == k) << l;
            for (int32_t l = 0; l < m; ++l)
                if (cls[q0 + l] == k) dst[q0 + l] = sw_p2x_rank_dst(off, k, cnt[k] + sw_p2x_rank_lane(same, l));
            cnt[k] += (int32_t)__builtin_popcountll(same);
        }
    }
    for (int32_t q = 0; q < n; ++q) {
        if (dst[q] < 0) {
            ok = 0;
            continue;
        }
        skey[dst[q]] = ckey[q];
        sjob[dst[q]] = job[q];
    }
    if (!ok) return 0;
    for (int32_t q = 0; q < n; ++q) ok &= sw_p2x_rank_ok(skey, sjob, off, cls[q], dst[q]);
    return ok;
}

#endif /* SW_P2X_RANK_H */
