"""csrc/sw_types_layout.h on the host: the arithmetic of the worker-type frame
(tests/native/types_layout_check.cpp).

The program checks, for the column sets of the four worker-type policies, that
the views of the input and output blocks are aligned and tile them, that every
offset equals the formula the policy's call held before the frame and the
padded input size that formula's end rounded up to 8, that packing and
unpacking reproduce the arrays (the results without their status word), and
the common rejections with their texts and order.  It is built twice — plain,
and with the address and undefined-behaviour sanitizers — as a stand-alone host
program that includes that header only.
"""
import os
import shutil
import subprocess


ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "native", "types_layout_check.cpp")
CSRC = os.path.join(ROOT, "shockwave-replication_amd", "csrc")


def _build_and_run(tmp_path, name, extra):
    cxx = shutil.which("g++")
    assert cxx, "no host C++ compiler (g++)"
    exe = str(tmp_path / name)
    subprocess.check_call([cxx, "-std=c++17", "-O2", "-Wall", "-Wextra", "-Werror", "-I", CSRC, *extra,
                           "-o", exe, SRC])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.startswith("ok "), r.stdout + r.stderr
    return int(r.stdout.split()[1])


def test_types_layout_properties(tmp_path):
    assert _build_and_run(tmp_path, "types_layout_check", []) > 3000


def test_types_layout_under_sanitizers(tmp_path):
    checks = _build_and_run(tmp_path, "types_layout_check_san",
                            ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                             # the runtimes inside the program: it must start whatever else the
                             # environment loads into it first
                             "-static-libasan", "-static-libubsan"])
    assert checks > 3000
