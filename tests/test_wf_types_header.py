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
import os
import shutil
import subprocess


ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "native", "wft_check.c")


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


def test_wf_types_header_ladder(tmp_path):
    checks = _build_and_run(tmp_path, "wft_check", [], 2)
    assert checks > 100_000


def test_wf_types_header_under_sanitizers(tmp_path):
    checks = _build_and_run(tmp_path, "wft_check_san",
                            ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                             # the runtimes inside the program: it must start whatever else the
                             # environment loads into it first
                             "-static-libasan", "-static-libubsan"], 1)
    assert checks > 50_000
