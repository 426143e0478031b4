"""The pack stage as three kernels — sw_sort_kernel, sw_rounds_kernel (the round
loop, one wave per instance), sw_place_kernel — against the CPU twin, bit for
bit (csrc/sw_kernels.hip, selected by loop_min_count() in csrc/sw_api.hip).

The thresholds are read once per process, so the solves run in a child process
(tests/loop_split_worker.py) started with SW_LOOP_MIN=1 and SW_SPLIT_MIN=1; it
writes every result field to .npz files, compared here with the twin.  One
child run and one set of twin solves serve all tests of the module.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

import loop_split_worker as lw
import sw_native as sn
from helpers import assert_same_result, check_plan_valid

pytestmark = pytest.mark.gpu

# the twin took another path than density order + repair somewhere: its first
# density pack and the repair left rounds unplaced (oracle/plan_twin.c: dens = 0)
NOT_DENSITY = (sn.SW_STATUS_P1_REPACKED | sn.SW_STATUS_P2_WEIGHT_ORDER | sn.SW_STATUS_P2_CLASSWISE |
               sn.SW_STATUS_P2_FALLBACK)


@pytest.fixture(scope="module")
def child(tmp_path_factory):
    out = tmp_path_factory.mktemp("loop_split")
    env = dict(os.environ, SW_LOOP_MIN="1", SW_SPLIT_MIN="1")
    worker = os.path.join(os.path.dirname(os.path.abspath(__file__)), "loop_split_worker.py")
    p = subprocess.run([sys.executable, worker, str(out)], env=env, capture_output=True, text=True,
                       timeout=300)
    assert p.returncode == 0, p.stdout + p.stderr
    return str(out)


@pytest.fixture(scope="module")
def main_case(twin):
    batch = lw.main_batch()
    return batch, [twin.solve(a) for a in batch]


def compare(path, batch, want, masks):
    for i, (a, w) in enumerate(zip(batch, want)):
        r = lw.load(path, i, masks)
        what = f"{os.path.basename(path)} case {i} N={a.N} G={a.G} T={a.T}"
        check_plan_valid(a, r)
        assert_same_result(r, w, what)
        if masks:
            bits = (r["plan_masks"][:, None] >> np.arange(a.T, dtype=np.uint64)[None, :]) & np.uint64(1)
            assert np.array_equal(bits.astype(np.uint8), w["plan"]), f"{what}: plan_masks differ"


def test_batch_covers_every_path(main_case):
    """The batch holds what the three kernels treat differently (by the twin:
    positions = jobs with planned rounds, which are the level search's counts
    unless P1 was re-solved): every positions-per-lane range of the loop
    kernel, more than 512 positions (marked by the sort kernel), a repaired
    density pack (the in-workgroup class loops after the workspace back half),
    an instance of at most 512 jobs that density order and repair do not place
    (the place kernel's mark), a cancelled exchange cycle, T < 30, T = 32,
    N = 1 and N = 1,024."""
    batch, want = main_case
    assert len(batch) <= 100
    act = [int((w["planned_rounds"] > 0).sum()) for w in want]
    clean = [not (w["status"] & NOT_DENSITY) for w in want]
    for lo, hi in ((1, 128), (129, 256), (257, 384), (385, 512)):
        assert any(lo <= x <= hi and c for x, c in zip(act, clean)), (lo, hi)
    assert any(x > 512 for x in act)
    assert any(w["status"] & sn.SW_STATUS_P2_REPAIRED and c for w, c in zip(want, clean))
    assert any(w["status"] & NOT_DENSITY and a.N <= 512 for a, w in zip(batch, want))
    assert any(w["status"] & sn.SW_STATUS_P2_EXCHANGED and c for w, c in zip(want, clean))
    assert any(a.T < 30 for a in batch) and any(a.T == 32 for a in batch)
    assert any(a.N == 1 for a in batch) and any(a.N == 1024 for a in batch)
    offs = np.cumsum([a.N for a in batch])
    assert np.any(offs % 4 != 0)  # unaligned job offsets


def test_loop_split_matches_twin(child, main_case):
    batch, want = main_case
    compare(os.path.join(child, "keep0.npz"), batch, want, masks=False)


def test_loop_split_masks_match_twin(child, main_case):
    batch, want = main_case
    compare(os.path.join(child, "keep1.npz"), batch, want, masks=True)


def test_loop_split_stale_workspace(child, twin):
    """A batch of few-position instances after one of many-position instances
    on the same handle: the workspace past each instance's positions still
    holds the first batch's words and masks, and none may be read."""
    large, small = lw.stale_batches()
    wl, ws = [twin.solve(a) for a in large], [twin.solve(a) for a in small]
    assert min(int((w["planned_rounds"] > 0).sum()) for w in wl) > 256
    assert max(int((w["planned_rounds"] > 0).sum()) for w in ws) <= 128
    compare(os.path.join(child, "stale_large.npz"), large, wl, masks=False)
    compare(os.path.join(child, "stale_small.npz"), small, ws, masks=False)
