"""csrc/sw_rowsearch.h on the host: the select-tree searches over a key row
against plain linear scans (tests/native/rowsearch_check.cpp).

The program checks count (strict and GE), count-with-neighbours and extract for
KT = 32 on every row of up to three distinct values, rows of T live keys then
zeros for T = 0 … 32, all-equal rows and seeded random nonincreasing rows, at
the thresholds 0, every key value and its two neighbours, and +inf.  It is
built twice — plain, and with the address and undefined-behaviour sanitizers —
as a stand-alone host program.
"""
import os
import shutil
import subprocess


ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "native", "rowsearch_check.cpp")
CSRC = os.path.join(ROOT, "shockwave-replication_amd", "csrc")


def _build_and_run(tmp_path, name, extra, rows):
    cxx = shutil.which("g++")
    assert cxx, "no host C++ compiler (g++)"
    exe = str(tmp_path / name)
    subprocess.check_call([cxx, "-std=c++17", "-O2", "-Wall", "-Wextra", "-Werror", "-ffp-contract=off",
                           "-I", CSRC, *extra, "-o", exe, SRC])
    r = subprocess.run([exe, str(rows)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.startswith("ok "), r.stdout + r.stderr
    return int(r.stdout.split()[1])


def test_rowsearch_matches_linear_scan(tmp_path):
    checks = _build_and_run(tmp_path, "rowsearch_check", [], 300000)
    assert checks > 5_000_000


def test_rowsearch_under_sanitizers(tmp_path):
    checks = _build_and_run(tmp_path, "rowsearch_check_san",
                            ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                             # the runtimes inside the program: it must start whatever else the
                             # environment loads into it first
                             "-static-libasan", "-static-libubsan"], 100000)
    assert checks > 2_000_000
