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
import os
import shutil
import subprocess


ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "native", "ftft_check.c")


def _build_and_run(tmp_path, name, extra, reps):
    cc = shutil.which("gcc")
    assert cc, "no host C compiler (gcc)"
    exe = str(tmp_path / name)
    subprocess.check_call([cc, "-std=c99", "-O2", "-Wall", "-Wextra", "-Werror", "-Wno-unused-function",
                           "-ffp-contract=off", "-fno-fast-math", *extra, "-o", exe, SRC, "-lm"])
    r = subprocess.run([exe, str(reps)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.startswith("ok "), r.stdout + r.stderr
    return int(r.stdout.split()[1])


def test_ftf_types_header_ladder(tmp_path):
    checks = _build_and_run(tmp_path, "ftft_check", [], 2)
    assert checks > 100_000


def test_ftf_types_header_under_sanitizers(tmp_path):
    checks = _build_and_run(tmp_path, "ftft_check_san",
                            ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                             # the runtimes inside the program: it must start whatever else the
                             # environment loads into it first
                             "-static-libasan", "-static-libubsan"], 1)
    assert checks > 50_000
