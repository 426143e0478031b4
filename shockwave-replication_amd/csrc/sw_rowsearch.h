/*
 * sw_rowsearch.h — searches over one job's key row held as a fixed array
 * (registers on the device).  Plain C++17 + HIP qualifiers, usable on the
 * host: tests/native/rowsearch_check.cpp checks it against linear scans.
 *
 * A row is KT fp32 keys, KT a power of two, all ≥ +0 (so the bit patterns
 * order like the values, sw_arith.h) and nonincreasing in n:
 * vm(n) = min(vm(n − 1), ·) scaled by a positive constant, rounded to fp32,
 * zero past T_j.  The keys above a threshold therefore form a prefix
 * [0, c0) and c0 is found by a binary search of log2(KT) compares plus one
 * for the last key.
 *
 * Registers cannot be indexed per lane, so the search is a select tree: the
 * pivot of level L is one of 2^(L−1) fixed array elements, chosen by the
 * outcomes of the earlier compares (KT = 32: row[15]; row[7] or row[23];
 * one of row[3], row[11], row[19], row[27]; …).  That is 1 + 3 + 7 + 15
 * selects and 6 compares for 32 keys where a scan takes 32 compares and 32
 * adds.  Every array index below is a template constant: nothing here may
 * make the compiler index the row dynamically (that puts the row in
 * scratch).  The selections are written depth first — one sub-tree is
 * reduced to a single value before its sibling is started — so few
 * temporaries are live at a time.
 */
#ifndef SW_ROWSEARCH_H
#define SW_ROWSEARCH_H

#include "sw_arith.h"

#if defined(__HIPCC__) || defined(__HIP__)
#define SW_RS_HD __host__ __device__ static __forceinline__
#else
#define SW_RS_HD static inline
#endif

template <int V>
struct sw_rs_log2 {
    static_assert(V > 0 && (V & (V - 1)) == 0, "row length must be a power of two");
    static constexpr int value = 1 + sw_rs_log2<V / 2>::value;
};
template <>
struct sw_rs_log2<1> {
    static constexpr int value = 0;
};

/* row[FIRST + STRIDE · i], i = the number whose binary digits are the
 * arguments after the row, most significant first */
template <int KT, int FIRST, int STRIDE>
SW_RS_HD uint32_t sw_rs_sel(const float (&row)[KT]) {
    static_assert(FIRST >= 0 && FIRST < KT, "row index out of range");
    return sw_fbits_of(row[FIRST]);
}
template <int KT, int FIRST, int STRIDE, class... B>
SW_RS_HD uint32_t sw_rs_sel(const float (&row)[KT], bool p, B... rest) {
    constexpr int HALF = STRIDE << sizeof...(rest);
    const uint32_t up = sw_rs_sel<KT, FIRST + HALF, STRIDE>(row, rest...);
    const uint32_t dn = sw_rs_sel<KT, FIRST, STRIDE>(row, rest...);
    return p ? up : dn;
}

template <bool GE>
SW_RS_HD bool sw_rs_above(uint32_t b, uint32_t rho) {
    return GE ? (b >= rho) : (b > rho);
}

/* L levels left of the search over row[0 .. KT − 2]; p... are the outcomes so
 * far, first level first.  SNAP: lo_k / hi_k follow the last pivot that
 * compared above / not above, which in a sorted row are row[c0 − 1] and
 * row[c0]. */
template <bool GE, bool SNAP, int KT, int L, class... B>
SW_RS_HD int sw_rs_levels(const float (&row)[KT], uint32_t rho, uint32_t& lo_k, uint32_t& hi_k,
                          B... p) {
    if constexpr (L == 0) {
        (void)row; (void)rho; (void)lo_k; (void)hi_k;
        return 0;
    } else {
        const uint32_t piv = sw_rs_sel<KT, (1 << (L - 1)) - 1, 1 << L>(row, p...);
        const bool t = sw_rs_above<GE>(piv, rho);
        if constexpr (SNAP) {
            lo_k = t ? piv : lo_k;
            hi_k = t ? hi_k : piv;
        }
        return (t ? (1 << (L - 1)) : 0) +
               sw_rs_levels<GE, SNAP, KT, L - 1>(row, rho, lo_k, hi_k, p..., t);
    }
}

/* #{n < KT : row[n] > rho} (GE: ≥ rho) of a nonincreasing row */
template <bool GE, int KT>
SW_RS_HD int sw_rs_count(const float (&row)[KT], uint32_t rho) {
    uint32_t lo_k = 0, hi_k = 0;
    const int c = sw_rs_levels<GE, false, KT, sw_rs_log2<KT>::value>(row, rho, lo_k, hi_k);
    /* c ≤ KT − 1 counts row[0 .. KT − 2]; the last key is above only when
     * all of those are */
    return c + (sw_rs_above<GE>(sw_fbits_of(row[KT - 1]), rho) ? 1 : 0);
}

/* c0 = #{n < KT : row[n] > rho} with the keys either side of the split:
 * lo_k = row[c0 − 1] (0x7FFFFFFF when c0 = 0), hi_k = row[c0] (0 when
 * c0 = KT) */
template <int KT>
SW_RS_HD int sw_rs_count_snap(const float (&row)[KT], uint32_t rho, uint32_t& lo_k,
                              uint32_t& hi_k) {
    const uint32_t last = sw_fbits_of(row[KT - 1]);
    lo_k = 0x7FFFFFFFu;
    hi_k = last; /* what row[c0] is when every pivot compares above */
    const int c = sw_rs_levels<false, true, KT, sw_rs_log2<KT>::value>(row, rho, lo_k, hi_k);
    const bool t = last > rho;
    lo_k = t ? last : lo_k;
    hi_k = t ? 0u : hi_k;
    return c + (t ? 1 : 0);
}

/* L digits of n left, least significant first: row[FIRST + STRIDE · (n mod 2^L)] */
template <int KT, int FIRST, int STRIDE, int L>
SW_RS_HD uint32_t sw_rs_digit(const float (&row)[KT], int n) {
    if constexpr (L == 0) {
        (void)n;
        static_assert(FIRST >= 0 && FIRST < KT, "row index out of range");
        return sw_fbits_of(row[FIRST]);
    } else {
        const uint32_t up = sw_rs_digit<KT, FIRST + STRIDE, 2 * STRIDE, L - 1>(row, n);
        const uint32_t dn = sw_rs_digit<KT, FIRST, 2 * STRIDE, L - 1>(row, n);
        return (n & STRIDE) ? up : dn;
    }
}

/* the bits of row[n] for a per-lane n; 0 outside [0, KT) */
template <int KT>
SW_RS_HD uint32_t sw_rs_extract(const float (&row)[KT], int n) {
    const uint32_t v = sw_rs_digit<KT, 0, 1, sw_rs_log2<KT>::value>(row, n);
    return (uint32_t)n < (uint32_t)KT ? v : 0u;
}

#endif
