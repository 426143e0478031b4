"""csrc/sw_allox.h on the host: the twin's lazy column bookkeeping
(tests/native/allox_check.c).

The program runs tests/twins/allox_twin.c over the fixed cases, the boundary
sizes (m + n at 63 … 513, the caps m = n = 1024) and seeded random instances,
with scratch and output arrays of exactly the documented sizes, and checks
the structure of every assignment, the in-order cost, the bound on the search
steps and, for one worker type, the known optimum.  It is built twice —
plain, and with the address and undefined-behaviour sanitizers — as a
stand-alone host program.
"""
from nativecheck import SANITIZE, build_and_run

SRC = "allox_check.c"  # in tests/native/
FLAGS = ["-ffp-contract=off"]


def test_allox_twin_properties(tmp_path):
    assert build_and_run(tmp_path, SRC, "allox_check", "c", FLAGS) > 50_000


def test_allox_twin_under_sanitizers(tmp_path):
    checks = build_and_run(tmp_path, SRC, "allox_check_san", "c", FLAGS + SANITIZE)
    assert checks > 50_000
