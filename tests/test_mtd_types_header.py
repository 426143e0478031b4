"""csrc/sw_mtd_types.h (with sw_mmf_ipm.h and sw_mtd.h) on the host
(tests/native/mtdt_check.c).

The program runs the twin's arithmetic over a ladder of small instances —
every number of types, job counts around the chunks of the deterministic sum,
dead jobs, types without workers, steps from 1e1 to 1e9, the thin case — and
checks that every call succeeds and every row of the LP holds at the returned
T.  It is built twice — plain, and with the address and undefined-behaviour
sanitizers — as a stand-alone host program.
"""
from nativecheck import SANITIZE, build_and_run

SRC = "mtdt_check.c"  # in tests/native/
FLAGS = ["-ffp-contract=off", "-fno-fast-math"]


def test_mtd_types_header_ladder(tmp_path):
    checks = build_and_run(tmp_path, SRC, "mtdt_check", "c", FLAGS, [2], timeout=300)
    assert checks > 100_000


def test_mtd_types_header_under_sanitizers(tmp_path):
    checks = build_and_run(tmp_path, SRC, "mtdt_check_san", "c", FLAGS + SANITIZE, [1], timeout=300)
    assert checks > 50_000
