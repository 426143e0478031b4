"""Every size-selected launch form of the sharded GPU engine against the CPU
shard engine.

csrc/sw_shard.hip picks the kernels of a placement by the entries per
workgroup and by the active entries; tests/shardcases.py holds one instance
per branch (tests/test_shard_ladder.py asserts the list covers them all).
Each case is one solve per world — world 1 through RCCL (the device
controller and its escape to the host controller), world 2 through host
collectives on threads (the host controller's ops), world 8 on threads where
the instance takes eight shares — and must equal oracle/shard_twin.c at that
world bit for bit: rc, status, collective steps, counts, plan rows and the
bits of every scalar.
"""
import numpy as np
import pytest

import shardcases as sc
import sw_native as sn
import sw_synth as ss
from helpers import check_plan_valid
from test_gpu_shard import gpu_shard_threads
from test_shard import CASES as SMALL_CASES
from test_shard import SCALARS, assert_same_as_single, run_threads, shard_lib  # noqa: F401
from test_shard_ladder import reference

pytestmark = pytest.mark.gpu

V8_CASES = [c for c in sc.CASES if c[0].startswith("v8_")]


@pytest.fixture(scope="module")
def rccl_solver():
    s = sn.Solver(device=0)
    s.dist_init(sn.unique_id(), 0, 1)
    yield s
    s.close()


def assert_same_solve(r, ref, what):
    assert_same_as_single(r, ref, what)
    assert r["iters"] == ref["iters"], (what, r["iters"], ref["iters"])


@pytest.mark.parametrize("case", sc.CASES, ids=sc.CASE_IDS)
def test_gpu_ladder_rccl_world1(case, rccl_solver, shard_lib):
    a, ref, _, _ = reference(shard_lib, case, 1)
    r = rccl_solver.dist_solve(a, 0, a.N)
    check_plan_valid(a, r)
    assert_same_solve(r, ref, f"rccl W=1 {case[0]}")


@pytest.mark.parametrize("case", sc.CASES, ids=sc.CASE_IDS)
def test_gpu_ladder_host_comm_world2(case, shard_lib):
    a, ref, _, _ = reference(shard_lib, case, 2)
    r = gpu_shard_threads(a, 2)
    check_plan_valid(a, r)
    assert_same_solve(r, ref, f"W=2 {case[0]}")


@pytest.mark.parametrize("case", V8_CASES, ids=[c[0] for c in V8_CASES])
def test_gpu_ladder_host_comm_world8(case, shard_lib):
    a, ref, _, _ = reference(shard_lib, case, 8)
    r = gpu_shard_threads(a, 8)
    check_plan_valid(a, r)
    assert_same_solve(r, ref, f"W=8 {case[0]}")


@pytest.mark.parametrize("case", sc.RR_CASES, ids=[c[0] for c in sc.RR_CASES])
def test_gpu_ladder_plan_kernel_reround(case, gpu_solver, twin):
    """The same re-optimisation knapsacks (two and more take-bit words,
    capacity ≥ 512, the three refusals) in the plan kernel's workspace form:
    sw_plan_solve against the twin."""
    a = sc.build(case)
    rt = twin.solve(a)
    assert rt["status"] & sn.SW_STATUS_P1_REPACKED
    r = gpu_solver.solve(a)
    check_plan_valid(a, r)
    assert_same_solve(r, rt, f"sw_plan_solve {case[0]}")


@pytest.mark.parametrize("name", ["v8_N40000", "edge_N32768"])
def test_gpu_ladder_device_resident(name, rccl_solver, shard_lib):
    """sw_dist_plan_solve_dev above 32,768 jobs in eight shares and on the
    widest one-share form: plan and counts in HBM equal the CPU engine's."""
    import torch
    case = sc.CASES[sc.CASE_IDS.index(name)]
    a, ref, _, _ = reference(shard_lib, case, 1)
    shard = sn.DeviceShard(a, "cuda:0")
    torch.cuda.synchronize()
    rd = rccl_solver.dist_solve_dev(shard, 0, a.N)
    assert np.array_equal(shard.plan.cpu().numpy(), ref["plan"])
    assert np.array_equal(shard.planned.cpu().numpy(), ref["planned_rounds"])
    for key in SCALARS + ("iters", "status", "rc"):
        assert np.float64(rd[key]).tobytes() == np.float64(ref[key]).tobytes(), (name, key, rd[key], ref[key])


def test_gpu_ladder_peer_transport_world2(shard_lib):
    """A two-launch share form (16,384 entries per rank: k_pack_rounds_sel and
    k_pack_rounds<32>) with every step's collective on the peer transport,
    ranks as threads."""
    case = sc.CASES[sc.CASE_IDS.index("edge_N32768")]
    a, ref, _, forms = reference(shard_lib, case, 2)
    assert "S3/rounds32" in forms
    r = gpu_shard_threads(a, 2, peer=True)
    check_plan_valid(a, r)
    assert_same_solve(r, ref, "peer W=2 edge_N32768")


@pytest.mark.parametrize("refusal", sc.REFUSALS, ids=[r[0] for r in sc.REFUSALS])
def test_gpu_ladder_refusals(refusal, rccl_solver, twin):
    """The engine's size limits are clean error returns: the code, the
    message, and the same handle then solves a small instance equal to the
    twin."""
    name, case, world, message = refusal
    assert world == 1
    a = sc.build(case)
    with pytest.raises(sn.NativeError) as e:
        rccl_solver.dist_solve(a, 0, a.N)
    assert e.value.code == sn.SW_ERR_CAPACITY, (name, e.value.code)
    assert message in str(e.value), (name, str(e.value))
    seed, N, G, T, k, lam = SMALL_CASES[1]
    b = ss.synth_problem(seed, N, G, T, 120.0, k, lam)
    r = rccl_solver.dist_solve(b, 0, b.N)
    check_plan_valid(b, r)
    assert_same_as_single(r, twin.solve(b), f"after the refusal {name}")
