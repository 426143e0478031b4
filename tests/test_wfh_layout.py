"""csrc/sw_wfh_layout.h on the host: the checks, the block layout and the
member-order packing of a hierarchical water-filling call
(tests/native/wfh_layout_check.cpp), built twice — plain, and with the address
and undefined-behaviour sanitizers — as a stand-alone host program that
includes that header only."""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "native", "wfh_layout_check.cpp")
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


def test_wfh_layout_properties(tmp_path):
    assert _build_and_run(tmp_path, "wfh_layout_check", []) > 5000


def test_wfh_layout_under_sanitizers(tmp_path):
    checks = _build_and_run(tmp_path, "wfh_layout_check_san",
                            ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                             # the runtimes inside the program: it must start whatever else the
                             # environment loads into it first
                             "-static-libasan", "-static-libubsan"])
    assert checks > 5000
