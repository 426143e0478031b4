"""MinTotalDuration on the GPU: the HIP kernel (sw_mtd_allocate and
sw_mtd_allocate_batch) against its CPU twin bit for bit, on the LDS path and
the L2 path, bad input, and the policy mirror and the simulator on the HIP
engine against the twin engine."""
import numpy as np
import pytest

import mtd_ref
import mtdcases as mc
import sw_native as sn


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(mc.FIXED))
def test_gpu_fixed_list_bit_exact_vs_twin(gpu_solver, name):
    inst = mc.FIXED[name]
    g = gpu_solver.mtd_allocate(*inst)
    assert mc.same_bits(g, mtd_ref.twin_allocate(*inst)), (g[1], g[2])
    mc.check_allocation(inst, *g)


@pytest.fixture(scope="module")
def fuzz():
    """About 300 random instances with N ≤ 1500 and three above the staged
    size, with the twin's results (computed once)."""
    insts = mc.random_instances(300, seed=11, max_n=1500) + mc.above_staged()
    return insts, [mtd_ref.twin_allocate(*inst) for inst in insts]


@pytest.mark.gpu
def test_gpu_fuzz_single_calls_bit_exact_vs_twin(gpu_solver, fuzz):
    insts, want = fuzz
    assert sum(len(i[0]) > mc.LDS_JOBS for i in insts) == 3
    for i, (inst, w) in enumerate(zip(insts, want)):
        assert mc.same_bits(gpu_solver.mtd_allocate(*inst), w), (i, len(inst[0]), inst[2])


@pytest.mark.gpu
def test_gpu_fuzz_one_batch_bit_exact_vs_twin(gpu_solver, fuzz):
    insts, want = fuzz
    got = gpu_solver.mtd_allocate_batch(insts)
    assert len(got) == len(insts)
    for i, (g, w) in enumerate(zip(got, want)):
        assert mc.same_bits(g, w), (i, len(insts[i][0]), insts[i][2])


def batches():
    small = mc.random_instances(300, seed=17, max_n=40, max_g=64)
    empty = (np.zeros(0, dtype=np.int32), np.zeros(0, dtype=np.float64), 4)
    return {
        "one": [mc.FIXED["sf_above_G"]],
        "empty_middle": [mc.FIXED["p0_mixed"], empty, mc.FIXED["n513_G96"]],
        "many_small": small,  # more workgroups than CUs
        "mixed_paths": (small[:5] + [mc.FIXED[f"n{mc.LDS_JOBS + 1}_G8192"]] + small[5:9]
                        + [mc.FIXED["n1025_G8"], mc.FIXED["decade"]]),
    }


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["one", "empty_middle", "many_small", "mixed_paths"])
def test_gpu_batch_equals_single_calls(gpu_solver, name):
    batch = batches()[name]
    got = gpu_solver.mtd_allocate_batch(batch)
    assert len(got) == len(batch)
    for i, (inst, g) in enumerate(zip(batch, got)):
        if len(inst[0]) == 0:
            assert len(g[0]) == 0 and g[1] == 0.0 and g[2] == 0.0
        else:
            assert mc.same_bits(g, gpu_solver.mtd_allocate(*inst)), (name, i)


@pytest.mark.gpu
def test_gpu_batch_rejects_decreasing_offsets_and_empty_batch_is_a_noop(gpu_solver):
    batch = [mc.FIXED["p0_mixed"], mc.FIXED["sf_above_G"]]
    with pytest.raises(sn.NativeError) as e:
        gpu_solver.mtd_allocate_batch(batch, offsets=[0, 8, 4])
    assert e.value.code == sn.SW_ERR_INVALID
    assert gpu_solver.mtd_allocate_batch([]) == []
    assert mc.same_bits(gpu_solver.mtd_allocate_batch(batch)[1], gpu_solver.mtd_allocate(*batch[1]))


@pytest.mark.gpu
def test_gpu_rejects_bad_input_and_keeps_working(gpu_solver):
    ok = ([1, 2], [100.0, 200.0], 2)
    bad = [
        ([1, 0], ok[1], 2),                     # sf = 0
        (ok[0], [100.0, float("nan")], 2),      # a NaN
        (ok[0], [100.0, -1.0], 2),              # p < 0
        (ok[0], [100.0, 1.0000001e15], 2),      # p above SW_MTD_FULL_TIME_MAX
        (ok[0], [100.0, float("inf")], 2),      # not finite
        (ok[0], ok[1], 0),                      # G = 0
    ]
    for inst in bad:
        with pytest.raises(sn.NativeError) as e:
            gpu_solver.mtd_allocate(*inst)
        assert e.value.code == sn.SW_ERR_INVALID
        assert mc.same_bits(gpu_solver.mtd_allocate(*ok), mtd_ref.twin_allocate(*ok))
    # the bound itself is admitted
    edge = ([1], [1e15], 1)
    assert mc.same_bits(gpu_solver.mtd_allocate(*edge), mtd_ref.twin_allocate(*edge))
    x, T, mu = gpu_solver.mtd_allocate([], [], 4)
    assert len(x) == 0 and T == 0.0 and mu == 0.0


@pytest.mark.gpu
def test_gpu_policy_sequence_equals_twin_engine(gpu_solver):
    _, g, pg = mc.policy_sequence(gpu_solver)
    _, c, pc = mc.policy_sequence(mtd_ref.TwinEngine())
    assert g == c
    assert pg.last_level == pc.last_level


@pytest.mark.gpu
def test_gpu_simulation_equals_twin_simulation(gpu_solver):
    rg, rc = {"workers": [], "allocations": []}, {"workers": [], "allocations": []}
    g = mc.simulate_30(gpu_solver, rg)
    c = mc.simulate_30(mtd_ref.TwinEngine(), rc)
    assert rg == rc
    for s in (g, c):
        s.pop("solve_seconds")
    assert g == c
