"""csrc/sw_rowsearch.h on the host: the select-tree searches over a key row
against plain linear scans (tests/native/rowsearch_check.cpp).

The program checks count (strict and GE), count-with-neighbours and extract for
KT = 32 on every row of up to three distinct values, rows of T live keys then
zeros for T = 0 … 32, all-equal rows and seeded random nonincreasing rows, at
the thresholds 0, every key value and its two neighbours, and +inf.  It is
built twice — plain, and with the address and undefined-behaviour sanitizers —
as a stand-alone host program.
"""
from nativecheck import CSRC, SANITIZE, build_and_run

SRC = "rowsearch_check.cpp"  # in tests/native/
FLAGS = ["-ffp-contract=off", "-I", CSRC]


def test_rowsearch_matches_linear_scan(tmp_path):
    checks = build_and_run(tmp_path, SRC, "rowsearch_check", "c++", FLAGS, [300000])
    assert checks > 5_000_000


def test_rowsearch_under_sanitizers(tmp_path):
    checks = build_and_run(tmp_path, SRC, "rowsearch_check_san", "c++", FLAGS + SANITIZE, [100000])
    assert checks > 2_000_000
