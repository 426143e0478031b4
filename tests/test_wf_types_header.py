"""csrc/sw_wf_types.h (with sw_mmf_ipm.h) on the host
(tests/native/wft_check.c).

The program first drives the stage bookkeeping alone (sw_wft_begin / _next /
_feed / _repeat / _result) on synthetic classifications: every job in one
stage, one job per stage and the repeat after it, a stage that freezes none
(the stall's status), statistics near the threshold.  Then it runs the twin's
arithmetic over a ladder of small instances — numbers of types 1 … 16, job
counts around the chunks of the deterministic sum, types without workers — and
checks that every call succeeds, that the levels rise with the stages and that
every row of the program holds at the returned levels.  It is built twice —
plain, and with the address and undefined-behaviour sanitizers — as a
stand-alone host program.
"""
from nativecheck import SANITIZE, build_and_run

SRC = "wft_check.c"  # in tests/native/
FLAGS = ["-ffp-contract=off", "-fno-fast-math"]


def test_wf_types_header_ladder(tmp_path):
    checks = build_and_run(tmp_path, SRC, "wft_check", "c", FLAGS, [2], timeout=300)
    assert checks > 100_000


def test_wf_types_header_under_sanitizers(tmp_path):
    checks = build_and_run(tmp_path, SRC, "wft_check_san", "c", FLAGS + SANITIZE, [1], timeout=300)
    assert checks > 50_000
