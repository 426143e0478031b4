"""Max sum throughput on the GPU: the HIP kernel (sw_mst_allocate and
sw_mst_allocate_batch) against its CPU twin bit for bit, on the LDS path and
the global path, bad input, and the policy mirror and the simulator on the HIP
engine against the twin engine."""
import numpy as np
import pytest

import mst_ref
import mstcases as mc
import sw_native as sn


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(mc.FIXED))
def test_gpu_fixed_list_bit_exact_vs_twin(gpu_solver, name):
    inst = mc.FIXED[name]
    g = gpu_solver.mst_allocate(*inst)
    assert mc.same_bits(g, mst_ref.twin_allocate(*inst)), g[1:]
    mst_ref.check_allocation(inst, *g, cap_excess=mc.CAP_BAR)


@pytest.fixture(scope="module")
def fuzz():
    """About 300 random instances with N ≤ 1500 and three above the staged
    size, with the twin's results (computed once)."""
    insts = mc.random_instances(300, seed=11, max_n=1500) + mc.above_staged()
    return insts, [mst_ref.twin_allocate(*inst) for inst in insts]


@pytest.mark.gpu
def test_gpu_fuzz_single_calls_bit_exact_vs_twin(gpu_solver, fuzz):
    insts, want = fuzz
    assert sum(len(i[0]) > mc.LDS_JOBS for i in insts) == 3
    for i, (inst, w) in enumerate(zip(insts, want)):
        assert mc.same_bits(gpu_solver.mst_allocate(*inst), w), (i, len(inst[0]), inst[3])


@pytest.mark.gpu
def test_gpu_fuzz_one_batch_bit_exact_vs_twin(gpu_solver, fuzz):
    insts, want = fuzz
    got = gpu_solver.mst_allocate_batch(insts)
    assert len(got) == len(insts)
    for i, (g, w) in enumerate(zip(got, want)):
        assert mc.same_bits(g, w), (i, len(insts[i][0]), insts[i][3])


def batches():
    small = mc.random_instances(300, seed=17, max_n=40)
    empty = (np.zeros(0, dtype=np.int32), np.zeros(0, dtype=np.float64), None, 4)
    return {
        "one": [mc.FIXED["sf_above_G"]],
        "empty_middle": [mc.FIXED["floors_on_class"], empty, mc.FIXED["n513"]],
        "many_small": small,  # more workgroups than CUs
        "mixed_paths": (small[:5] + [mc.FIXED[f"n{mc.LDS_JOBS + 1}"]] + small[5:9]
                        + [mc.FIXED["n1025"], mc.FIXED["floor_inf"]]),
        "all_null_floors": [mc.FIXED["all_tied"], mc.FIXED["slack_zero_tp"], mc.FIXED["boundary"]],
    }


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["one", "empty_middle", "many_small", "mixed_paths", "all_null_floors"])
def test_gpu_batch_equals_single_calls(gpu_solver, name):
    batch = batches()[name]
    got = gpu_solver.mst_allocate_batch(batch)
    assert len(got) == len(batch)
    for i, (inst, g) in enumerate(zip(batch, got)):
        if len(inst[0]) == 0:
            assert len(g[0]) == 0 and g[1:] == (0.0, 0.0, 0.0, False)
        else:
            assert mc.same_bits(g, gpu_solver.mst_allocate(*inst)), (name, i)


@pytest.mark.gpu
def test_gpu_batch_rejects_decreasing_offsets_and_empty_batch_is_a_noop(gpu_solver):
    batch = [mc.FIXED["floors_on_class"], mc.FIXED["sf_above_G"]]
    for offsets in ([0, 6, 4], [1, 4, 7]):
        with pytest.raises(sn.NativeError) as e:
            gpu_solver.mst_allocate_batch(batch, offsets=offsets)
        assert e.value.code == sn.SW_ERR_INVALID and "offsets" in str(e.value)
    assert gpu_solver.mst_allocate_batch([]) == []
    assert mc.same_bits(gpu_solver.mst_allocate_batch(batch)[1], gpu_solver.mst_allocate(*batch[1]))


@pytest.mark.gpu
def test_gpu_rejects_bad_input_and_keeps_working(gpu_solver):
    ok = ([1, 2], [3.0, 4.0], [0.0, 0.25], 2)
    nan, inf = float("nan"), float("inf")
    bad = [
        (([1, 0], ok[1], ok[2], 2), "scale factors"),        # sf = 0
        (([1, 256], ok[1], ok[2], 2), "scale factors"),      # sf above 255
        ((ok[0], [3.0, nan], ok[2], 2), "weights"),          # a NaN weight
        ((ok[0], [3.0, -1.0], ok[2], 2), "weights"),         # w < 0
        ((ok[0], [3.0, 1.0000001e30], ok[2], 2), "weights"),  # w above SW_MST_WEIGHT_MAX
        ((ok[0], [3.0, inf], ok[2], 2), "weights"),          # not finite
        ((ok[0], ok[1], [0.0, nan], 2), "floors"),           # a NaN floor
        ((ok[0], ok[1], [0.0, -0.5], 2), "floors"),          # l < 0
        ((ok[0], ok[1], ok[2], 0), "worker"),                # G = 0
    ]
    for inst, rule in bad:
        with pytest.raises(sn.NativeError) as e:
            gpu_solver.mst_allocate(*inst)
        assert e.value.code == sn.SW_ERR_INVALID and rule in str(e.value), str(e.value)
        assert mc.same_bits(gpu_solver.mst_allocate(*ok), mst_ref.twin_allocate(*ok))
    # the bounds themselves are admitted, and so is a floor of +inf
    for edge in [([1], [1e30], None, 1), ([255], [0.0], [inf], 1)]:
        assert mc.same_bits(gpu_solver.mst_allocate(*edge), mst_ref.twin_allocate(*edge))
    x, lam, m, obj, dropped = gpu_solver.mst_allocate([], [], None, 4)
    assert len(x) == 0 and (lam, m, obj, dropped) == (0.0, 0.0, 0.0, False)


@pytest.mark.gpu
def test_gpu_policy_sequence_equals_twin_engine(gpu_solver):
    _, g, pg = mc.policy_sequence(gpu_solver)
    _, c, pc = mc.policy_sequence(mst_ref.TwinEngine())
    assert g == c
    assert pg.last_level == pc.last_level


@pytest.mark.gpu
def test_gpu_simulation_equals_twin_simulation(gpu_solver):
    rg, rc = {"workers": [], "allocations": []}, {"workers": [], "allocations": []}
    g = mc.simulate_30(gpu_solver, rg)
    c = mc.simulate_30(mst_ref.TwinEngine(), rc)
    assert rg == rc
    for s in (g, c):
        s.pop("solve_seconds")
    assert g == c
