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
import os
import shutil
import subprocess


ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "native", "allox_check.c")


def _build_and_run(tmp_path, name, extra):
    cc = shutil.which("gcc")
    assert cc, "no host C compiler (gcc)"
    exe = str(tmp_path / name)
    subprocess.check_call([cc, "-std=c99", "-O2", "-Wall", "-Wextra", "-Werror", "-Wno-unused-function",
                           "-ffp-contract=off", *extra, "-o", exe, SRC, "-lm"])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.startswith("ok "), r.stdout + r.stderr
    return int(r.stdout.split()[1])


def test_allox_twin_properties(tmp_path):
    assert _build_and_run(tmp_path, "allox_check", []) > 50_000


def test_allox_twin_under_sanitizers(tmp_path):
    checks = _build_and_run(tmp_path, "allox_check_san",
                            ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                             # the runtimes inside the program: it must start whatever else the
                             # environment loads into it first
                             "-static-libasan", "-static-libubsan"])
    assert checks > 50_000
