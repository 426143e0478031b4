"""csrc/sw_ftf_types.h (with sw_mmf_ipm.h and sw_ftf.h) on the host
(tests/native/ftft_check.c).

The program first drives the outer iteration alone (sw_ftft_begin / _next /
_feed) on synthetic level functions: a linear one (one step), a concave one
with convex 1/t (monotone from the left, no overshoot), a convex one built to
make the Newton step on t overshoot (the SAFE path, which still converges from
the left), a flat one that never converges (the solve cap's status), and the
first probe above 1 at ρ_box.  Then it runs the twin's arithmetic over a ladder
of small instances — numbers of types 1 … 16, job counts around the chunks of
the deterministic sum, dead jobs, types without workers — and checks that every
call succeeds and every row of the program holds at the returned ρ.  It is
built twice — plain, and with the address and undefined-behaviour sanitizers —
as a stand-alone host program.
"""
from nativecheck import SANITIZE, build_and_run

SRC = "ftft_check.c"  # in tests/native/
FLAGS = ["-ffp-contract=off", "-fno-fast-math"]


def test_ftf_types_header_ladder(tmp_path):
    checks = build_and_run(tmp_path, SRC, "ftft_check", "c", FLAGS, [2], timeout=300)
    assert checks > 100_000


def test_ftf_types_header_under_sanitizers(tmp_path):
    checks = build_and_run(tmp_path, SRC, "ftft_check_san", "c", FLAGS + SANITIZE, [1], timeout=300)
    assert checks > 50_000
