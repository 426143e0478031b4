"""The exchange step's rank order from the density pack's positions
(csrc/sw_p2x_rank.h) in the product: sw_place_kernel (the pack stage as three
kernels) and the fused sw_pack_kernel against the CPU twin, every field bit
for bit.

A dozen instances of 120 jobs × 30 rounds at G = 32 (tests/place_rank_worker.py):
plain, repaired and exchanged ones, one the pack stage leaves to the full
kernel, and a near-tie instance — pairs of jobs whose density keys tie and
whose exchange keys do not, so the positions are not the rank order and the
set-up has to notice and sort.  The thresholds are read once per process, so
each form runs in a child process; one set of twin solves serves all tests.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

import loop_split_worker as lw
import p2x_rank_ref as rr
import place_rank_worker as pw
import sw_native as sn
from helpers import assert_same_result, check_plan_valid

pytestmark = pytest.mark.gpu

NOT_DENSITY = (sn.SW_STATUS_P1_REPACKED | sn.SW_STATUS_P2_WEIGHT_ORDER | sn.SW_STATUS_P2_CLASSWISE |
               sn.SW_STATUS_P2_FALLBACK)
FORMS = {"split": "1", "fused": "1000000"}  # SW_LOOP_MIN


@pytest.fixture(scope="module")
def want(twin):
    batch = pw.batch()
    return batch, [twin.solve(a) for a in batch]


@pytest.fixture(scope="module")
def child(tmp_path_factory):
    out = tmp_path_factory.mktemp("place_rank")
    worker = os.path.join(os.path.dirname(os.path.abspath(__file__)), "place_rank_worker.py")
    for name, loop_min in FORMS.items():
        env = dict(os.environ, SW_SPLIT_MIN="1", SW_LOOP_MIN=loop_min)
        p = subprocess.run([sys.executable, worker, str(out), name], env=env, capture_output=True, text=True,
                           timeout=120)
        assert p.returncode == 0, p.stdout + p.stderr
    return str(out)


def positions_are_rank_order(a, w):
    """By the twin's counts: the density order of the placed jobs, partitioned
    by class, is the exchange step's rank order."""
    n = w["planned_rounds"]
    act = np.nonzero(n > 0)[0]
    P = dict(job=[int(j) for j in act], w=[int(a.w[j]) for j in act],
             c=[np.float64(a.p[j]) / np.float64(n[j]) for j in act])
    ratio = [np.float64(a.p[j]) / np.float64(int(n[j]) * int(a.w[j])) for j in act]
    return rr.partition(P, rr.density_order(P, ratio)) == rr.rank_order(P)


def test_batch_covers_the_cases(want):
    batch, res = want
    assert len(batch) == 12 and all((a.N, a.T, a.G) == (120, 30, 32) for a in batch)
    clean = [not (w["status"] & NOT_DENSITY) for w in res]
    same = [positions_are_rank_order(a, w) for a, w in zip(batch, res)]
    # the ordinary case: the positions are the rank order, and the step cancels cycles on them
    assert any(c and s and w["status"] & sn.SW_STATUS_P2_EXCHANGED for c, s, w in zip(clean, same, res))
    # the repair ran and the positions are still the placed jobs
    assert any(c and s and w["status"] & sn.SW_STATUS_P2_REPAIRED for c, s, w in zip(clean, same, res))
    # the near-tie instance is placed by the density order, and its positions are not the rank order
    assert clean[-1] and not same[-1] and res[-1]["status"] & sn.SW_STATUS_P2_EXCHANGED
    assert any(not c for c in clean)  # left to the full kernel


@pytest.mark.parametrize("form", sorted(FORMS))
def test_place_matches_twin(child, want, form):
    batch, res = want
    path = os.path.join(child, form + ".npz")
    for i, (a, w) in enumerate(zip(batch, res)):
        r = lw.load(path, i, True)
        what = f"{form} case {i}"
        check_plan_valid(a, r)
        assert_same_result(r, w, what)
        bits = (r["plan_masks"][:, None] >> np.arange(a.T, dtype=np.uint64)[None, :]) & np.uint64(1)
        assert np.array_equal(bits.astype(np.uint8), w["plan"]), f"{what}: plan_masks differ"
