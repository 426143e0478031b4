"""csrc/sw_keyarith.h on the host: the one-instruction minima and the key clamp
that Ctx::setup builds its key rows with, bit for bit against sw_e, sw_min (on
the running marginal) and sw_key of sw_arith.h, which the CPU twin compiles
(tests/native/key_arith_check.cpp).

The program covers ±0, the smallest and largest denormals, DBL_MIN, FLT_MIN and
FLT_MAX as doubles with their neighbours, the fp32 rounding boundaries beside
the two clamps, DBL_MAX, +inf, equal operands, cap = 0, the 0·∞ product of a
zero marginal and an overflowed key scale (a NaN key in both forms), and
seeded random finite values, singly and as 32-key rows.  A NaN rate or cap
cannot pass the validator and is left out; the program's header lists what
else is and why.  It is built twice — plain, and with the address and
undefined-behaviour sanitizers — as a stand-alone host program.
"""
from nativecheck import CSRC, SANITIZE, build_and_run

SRC = "key_arith_check.cpp"  # in tests/native/
# the twin's floating-point flags: no contraction, no fast-math
FLAGS = ["-ffp-contract=off", "-fno-fast-math", "-I", CSRC]


def test_key_forms_match_twin_text(tmp_path):
    # 10 checks per random case and 4 per key of a row: a few million random values
    checks = build_and_run(tmp_path, SRC, "key_arith_check", "c++", FLAGS, [1_000_000])
    assert checks > 10_000_000


def test_key_forms_under_sanitizers(tmp_path):
    checks = build_and_run(tmp_path, SRC, "key_arith_check_san", "c++", FLAGS + SANITIZE, [200_000])
    assert checks > 2_000_000
