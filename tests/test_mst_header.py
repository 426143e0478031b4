"""csrc/sw_mst.h on the host: the ordered key of signed doubles and the per-job
root x_j(m) (tests/native/mst_check.cpp).

The program checks that the key is monotone and round-trips over signed
doubles (±0, denormals, ±2^64, seeded random doubles of every exponent) and
that sw_mst_x stays inside (l, 1] and is non-increasing in m over a ladder of
multipliers from −2^64 to 2^64, for floors from 0 to 1.  It is built twice —
plain, and with the address and undefined-behaviour sanitizers — as a
stand-alone host program.
"""
from nativecheck import CSRC, SANITIZE, build_and_run

SRC = "mst_check.cpp"  # in tests/native/
FLAGS = ["-ffp-contract=off", "-I", CSRC]


def test_mst_header_properties(tmp_path):
    checks = build_and_run(tmp_path, SRC, "mst_check", "c++", FLAGS, [400])
    assert checks > 300_000


def test_mst_header_under_sanitizers(tmp_path):
    checks = build_and_run(tmp_path, SRC, "mst_check_san", "c++", FLAGS + SANITIZE, [100])
    assert checks > 80_000
