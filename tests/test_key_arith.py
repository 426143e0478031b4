"""csrc/sw_keyarith.h on the host: the one-instruction minima and the key clamp
that Ctx::setup builds its key rows with, bit for bit against sw_e, sw_min (on
the running marginal) and sw_key of sw_arith.h, which the CPU twin compiles
(tests/native/key_arith_check.cpp).

The program covers ±0, the smallest and largest denormals, DBL_MIN, FLT_MIN and
FLT_MAX as doubles with their neighbours, the fp32 rounding boundaries beside
the two clamps, DBL_MAX, +inf, equal operands, cap = 0, the 0·∞ product of a
zero marginal and an overflowed key scale (a NaN key in both forms), and
seeded random finite values, singly and as 32-key rows.  A NaN rate or cap
cannot pass the validator and is left out; the program's header lists what
else is and why.  It is built twice — plain, and with the address and
undefined-behaviour sanitizers — as a stand-alone host program.
"""
import os
import shutil
import subprocess


ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "native", "key_arith_check.cpp")
CSRC = os.path.join(ROOT, "shockwave-replication_amd", "csrc")


def _build_and_run(tmp_path, name, extra, count):
    cxx = shutil.which("g++")
    assert cxx, "no host C++ compiler (g++)"
    exe = str(tmp_path / name)
    # the twin's floating-point flags: no contraction, no fast-math
    subprocess.check_call([cxx, "-std=c++17", "-O2", "-Wall", "-Wextra", "-Werror", "-ffp-contract=off",
                           "-fno-fast-math", "-I", CSRC, *extra, "-o", exe, SRC])
    r = subprocess.run([exe, str(count)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.startswith("ok "), r.stdout + r.stderr
    return int(r.stdout.split()[1])


def test_key_forms_match_twin_text(tmp_path):
    # 10 checks per random case and 4 per key of a row: a few million random values
    checks = _build_and_run(tmp_path, "key_arith_check", [], 1_000_000)
    assert checks > 10_000_000


def test_key_forms_under_sanitizers(tmp_path):
    checks = _build_and_run(tmp_path, "key_arith_check_san",
                            ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                             # the runtimes inside the program: it must start whatever else the
                             # environment loads into it first
                             "-static-libasan", "-static-libubsan"], 200_000)
    assert checks > 2_000_000
