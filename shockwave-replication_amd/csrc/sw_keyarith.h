/*
 * sw_keyarith.h — the key-row arithmetic of Ctx::setup (sw_kernels.hip) in
 * forms that compile to one min / max instruction each.
 *
 * sw_arith.h writes its minima as `a < b ? a : b`, which is what the CPU twin
 * compiles and which stays the specification.  On gfx950 that text costs a
 * compare and two v_cndmask per fp64 minimum, because it has to hand back b
 * when a is a NaN.  The on-chip key rows evaluate three such minima per key,
 * 64 keys per thread, on operands that are never a NaN where it matters, so
 * the forms below give the same bits for every input the validator admits
 * (sw_validate.h: finite values, priorities ≥ 0, F ≤ E) — checked on the
 * host by tests/native/key_arith_check.cpp.  Device code only; the twin does
 * not include this header.
 */
#ifndef SW_KEYARITH_H
#define SW_KEYARITH_H

#include "sw_arith.h"

/* sw_e: min(rate·n, cap).  cap is a finite integer ≥ +0 and never a NaN;
 * rate·n is ≥ +0, +inf, or a NaN (rate = +inf at n = 0), and fmin hands back
 * cap for a NaN as the comparison does.  +0 only ever meets +0. */
SW_HD double sw_e_nf(const sw_jobc* c, int32_t n) { return __builtin_fmin(c->rate * (double)n, c->cap); }

/* sw_min of the running marginal and the next one: both come out of sw_pos,
 * so both lie in [+0, +inf] — no NaN, no −0. */
SW_HD double sw_min_nf(double a, double b) { return __builtin_fmin(a, b); }

/* sw_key with the upper clamp after the conversion: a k above FLT_MAX
 * converts to FLT_MAX or to +inf, and the fp32 comparison brings +inf back to
 * FLT_MAX; a NaN k (a zero marginal times an overflowed scale 1/(w·A), 0·∞)
 * fails both comparisons and converts as in sw_key — fmin(k, FLT_MAX) would
 * have turned it into FLT_MAX.  The flush below FLT_MIN stays an fp64
 * comparison: a k just below FLT_MIN would round up to it. */
SW_HD float sw_key_nf(double vm, double scale) {
    const double k = vm * scale;
    if (k < SW_FLT_MIN) return 0.0f;
    const float f = (float)k;
    return f > 3.4028234663852886e+38f ? 3.4028234663852886e+38f : f;
}

#endif /* SW_KEYARITH_H */
