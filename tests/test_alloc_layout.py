"""csrc/sw_alloc_layout.h on the host: the arithmetic of the allocation frame
(tests/native/alloc_layout_check.cpp).

The program checks, for column sets shaped like those of the four per-job
policies, that the views of the input and output blocks are aligned and tile
them, that the block sizes equal each policy's formula, that packing and
unpacking reproduce the columns (an absent one as zeros), the LDS staging
bound maxq around 512 and LDS_JOBS with its environment switch, and the
rejections of bad offsets and worker counts with their texts and order.  It is
built twice — plain, and with the address and undefined-behaviour sanitizers —
as a stand-alone host program that includes that header only.
"""
import os
import shutil
import subprocess


ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "native", "alloc_layout_check.cpp")
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


def test_alloc_layout_properties(tmp_path):
    assert _build_and_run(tmp_path, "alloc_layout_check", []) > 700


def test_alloc_layout_under_sanitizers(tmp_path):
    checks = _build_and_run(tmp_path, "alloc_layout_check_san",
                            ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                             # the runtimes inside the program: it must start whatever else the
                             # environment loads into it first
                             "-static-libasan", "-static-libubsan"])
    assert checks > 700
