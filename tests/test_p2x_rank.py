"""csrc/sw_p2x_rank.h on the host, and the premise it rests on.

  * tests/native/p2x_rank_check.cpp: the rank order taken from a candidate
    (stable partition by class, strict check of neighbours) against std::sort
    on the exchange key — random instances, all-equal c, pairs equal in their
    leading mantissa bits and different below with the later job the larger,
    widths 3, 5, 6 and 7, A = 1, 2, 63, 64, 65, 511, 512, classes of 64 and 65
    members, K = 1 and 8; every candidate is accepted exactly when its
    partition is the sorted order.  Built twice — plain, and with the address
    and undefined-behaviour sanitizers — as a stand-alone host program.
  * the premise: on the headline instances, with the twin's own counts, the
    density pack's order partitioned by class is the exchange step's rank
    order.
"""
import os
import shutil
import subprocess

import numpy as np

import p2x_rank_ref as rr
import sw_synth as ss

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "native", "p2x_rank_check.cpp")
CSRC = os.path.join(ROOT, "shockwave-replication_amd", "csrc")


def _build_and_run(tmp_path, name, extra, nrandom):
    cxx = shutil.which("g++")
    assert cxx, "no host C++ compiler (g++)"
    exe = str(tmp_path / name)
    subprocess.check_call([cxx, "-std=c++17", "-O2", "-Wall", "-Wextra", "-Werror", "-ffp-contract=off",
                           "-I", CSRC, *extra, "-o", exe, SRC])
    r = subprocess.run([exe, str(nrandom)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.startswith("ok "), r.stdout + r.stderr
    return int(r.stdout.split()[1])


def test_rank_from_candidate_matches_sort(tmp_path):
    checks = _build_and_run(tmp_path, "p2x_rank_check", [], 200)
    assert checks > 2_000_000


def test_rank_from_candidate_under_sanitizers(tmp_path):
    checks = _build_and_run(tmp_path, "p2x_rank_check_san",
                            ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                             # the runtimes inside the program: it must start whatever else the
                             # environment loads into it first
                             "-static-libasan", "-static-libubsan"], 60)
    assert checks > 1_000_000


def test_density_order_is_rank_order_on_c3_with_twin_counts(twin):
    for seed in range(64):
        a = ss.c3_problem(seed)
        n = twin.solve(a)["planned_rounds"]
        act = np.nonzero(n > 0)[0]
        assert 0 < len(act) <= 512, seed
        P = dict(job=[int(j) for j in act], w=[int(a.w[j]) for j in act],
                 c=[np.float64(a.p[j]) / np.float64(n[j]) for j in act])
        # the pack's key operand: p / (double)(n·w)
        ratio = [np.float64(a.p[j]) / np.float64(int(n[j]) * int(a.w[j])) for j in act]
        assert rr.partition(P, rr.density_order(P, ratio)) == rr.rank_order(P), seed
