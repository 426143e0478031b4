"""The bit-packed plan of the sharded solve (sw_result.plan_masks on
sw_dist_plan_solve / sw_dist_plan_solve_dev, csrc/sw_shard.hip k_emit_plan).

The reference is the byte plan of the same engine with masks off, packed in
numpy, and the plan_masks of sw_plan_solve on the whole instance (each is one
share); every comparison is exact.  Capacity binds, so the last round's bit
is in use; one job in eight is wider than the cluster.
"""
import ctypes as C

import numpy as np
import pytest

import shardcases as sc
import sw_native as sn

pytestmark = pytest.mark.gpu

SCALARS = ("rc", "objective", "utility", "makespan", "p2_objective", "bound", "iters", "status")


@pytest.fixture(scope="module")
def rccl_solver():
    s = sn.Solver(device=0)
    s.dist_init(sn.unique_id(), 0, 1)
    yield s
    s.close()


def pack(plan):
    return (plan.astype(np.uint64) << np.arange(plan.shape[1], dtype=np.uint64)).sum(axis=1, dtype=np.uint64)


def single_masks(solver, a):
    m = np.zeros(a.N, dtype=np.uint64)
    pr, res = a.c_problem(), a.c_result()
    res.plan_masks = m.ctypes.data_as(C.POINTER(C.c_uint64))
    assert solver.lib.sw_plan_solve(solver.h, C.byref(pr), C.byref(res)) >= 0
    return m


def check(a, rccl_solver, gpu_solver, what):
    import torch
    ref = rccl_solver.dist_solve(a, 0, a.N)
    want = pack(ref["plan"])
    both = rccl_solver.dist_solve(a, 0, a.N, masks=True)
    assert np.array_equal(both["plan_masks"], want), what
    assert np.array_equal(both["plan"], ref["plan"]), what
    a.plan[:] = 0xAA
    only = rccl_solver.dist_solve(a, 0, a.N, masks=True, plan=False)
    assert np.array_equal(only["plan_masks"], want), what
    assert (a.plan == 0xAA).all(), f"{what}: plan=False wrote the byte plan"
    assert np.array_equal(only["planned_rounds"], ref["planned_rounds"]), what
    for key in SCALARS:
        assert np.float64(only[key]).tobytes() == np.float64(ref[key]).tobytes(), (what, key)
    shard = sn.DeviceShard(a, "cuda:0", masks=True)
    torch.cuda.synchronize()
    rccl_solver.dist_solve_dev(shard, 0, a.N, plan=False)
    assert np.array_equal(shard.masks.cpu().numpy().view(np.uint64), want), what
    assert not shard.plan.any().item(), f"{what}: plan=False wrote the byte plan"
    rccl_solver.dist_solve_dev(shard, 0, a.N)
    assert np.array_equal(shard.plan.cpu().numpy(), ref["plan"]), what
    assert np.array_equal(single_masks(gpu_solver, a), want), what
    assert not (want[a.w > a.G]).any(), f"{what}: a job wider than the cluster has rounds"
    assert a.T == 64 or not (want >> np.uint64(a.T)).any(), f"{what}: bits at or above T"
    return want


@pytest.mark.parametrize("T", [1, 30, 64])
@pytest.mark.parametrize("N", [1, 63, 64, 65, 513, 4097])
def test_gpu_shard_masks(N, T, rccl_solver, gpu_solver):
    a = sc.short_problem(1, N, G=max(1, N // 40), T=T, k=1e5, idle=N // 8)
    want = check(a, rccl_solver, gpu_solver, f"N{N} T{T}")
    assert (want >> np.uint64(T - 1)).any(), "the instance leaves the last round empty"


def test_gpu_shard_masks_gathered_path(rccl_solver, gpu_solver):
    """A share placement that strands rounds: the host-driven controller's final step."""
    check(sc.build(sc.CASES[sc.CASE_IDS.index("gath_N400")]), rccl_solver, gpu_solver, "gath_N400")
