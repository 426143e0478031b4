"""csrc/sw_mst.h on the host: the ordered key of signed doubles and the per-job
root x_j(m) (tests/native/mst_check.cpp).

The program checks that the key is monotone and round-trips over signed
doubles (±0, denormals, ±2^64, seeded random doubles of every exponent) and
that sw_mst_x stays inside (l, 1] and is non-increasing in m over a ladder of
multipliers from −2^64 to 2^64, for floors from 0 to 1.  It is built twice —
plain, and with the address and undefined-behaviour sanitizers — as a
stand-alone host program.
"""
import os
import shutil
import subprocess


ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "native", "mst_check.cpp")
CSRC = os.path.join(ROOT, "shockwave-replication_amd", "csrc")


def _build_and_run(tmp_path, name, extra, n):
    cxx = shutil.which("g++")
    assert cxx, "no host C++ compiler (g++)"
    exe = str(tmp_path / name)
    subprocess.check_call([cxx, "-std=c++17", "-O2", "-Wall", "-Wextra", "-Werror", "-ffp-contract=off",
                           "-I", CSRC, *extra, "-o", exe, SRC])
    r = subprocess.run([exe, str(n)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.startswith("ok "), r.stdout + r.stderr
    return int(r.stdout.split()[1])


def test_mst_header_properties(tmp_path):
    checks = _build_and_run(tmp_path, "mst_check", [], 400)
    assert checks > 300_000


def test_mst_header_under_sanitizers(tmp_path):
    checks = _build_and_run(tmp_path, "mst_check_san",
                            ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                             # the runtimes inside the program: it must start whatever else the
                             # environment loads into it first
                             "-static-libasan", "-static-libubsan"], 100)
    assert checks > 80_000
