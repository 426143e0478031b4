"""FinishTimeFairness on the GPU: the HIP kernel (sw_ftf_allocate and
sw_ftf_allocate_batch) against its CPU twin bit for bit, on the LDS path and
the L2 path, the exact certificate on the GPU's own level, bad input, and the
policy mirror and the simulator on the HIP engine against the twin engine."""
import numpy as np
import pytest

import ftf_ref
import ftfcases as fc
import sw_native as sn


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(fc.FIXED))
def test_gpu_fixed_list_bit_exact_vs_twin(gpu_solver, name):
    inst = fc.FIXED[name]
    g = gpu_solver.ftf_allocate(*inst)
    assert fc.same_bits(g, ftf_ref.twin_allocate(*inst))
    sf, p, a, E, G = inst
    assert ftf_ref.certified(sf, p, a, E, G, g[1], 1e-9)
    fc.check_allocation(inst, *g)


@pytest.mark.gpu
def test_gpu_fuzz_bit_exact_vs_twin(gpu_solver):
    for i, inst in enumerate(fc.random_instances(300, seed=11, max_n=5000)):
        g = gpu_solver.ftf_allocate(*inst)
        assert fc.same_bits(g, ftf_ref.twin_allocate(*inst)), (i, len(inst[0]), inst[4])
        if i % 3 == 0:
            sf, p, a, E, G = inst
            assert ftf_ref.certified(sf, p, a, E, G, g[1], 1e-9), (i, len(sf), G)


def batches():
    small = fc.random_instances(300, seed=17, max_n=40, max_g=64)
    empty = tuple(np.zeros(0, dtype=t) for t in (np.int32, np.float64, np.float64, np.float64)) + (4,)
    return {
        "one": [fc.FIXED["no_unit_width"]],
        "empty_middle": [fc.FIXED["p0_free"], empty, fc.FIXED["n513_G96"]],
        "many_small": small,  # more workgroups than CUs
        "mixed_paths": small[:5] + [fc.FIXED["n2500_G256"]] + small[5:9] + [fc.FIXED["n1025_G2048"]],
    }


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["one", "empty_middle", "many_small", "mixed_paths"])
def test_gpu_batch_equals_single_calls(gpu_solver, name):
    batch = batches()[name]
    got = gpu_solver.ftf_allocate_batch(batch)
    assert len(got) == len(batch)
    for i, (inst, g) in enumerate(zip(batch, got)):
        if len(inst[0]) == 0:
            assert len(g[0]) == 0 and g[1] == 0.0 and g[2] == 0.0
        else:
            assert fc.same_bits(g, gpu_solver.ftf_allocate(*inst)), (name, i)


@pytest.mark.gpu
def test_gpu_batch_rejects_decreasing_offsets_and_empty_batch_is_a_noop(gpu_solver):
    batch = [fc.FIXED["p0_free"], fc.FIXED["no_unit_width"]]
    with pytest.raises(sn.NativeError):
        gpu_solver.ftf_allocate_batch(batch, offsets=[0, 8, 4])
    assert gpu_solver.ftf_allocate_batch([]) == []
    assert fc.same_bits(gpu_solver.ftf_allocate_batch(batch)[1], gpu_solver.ftf_allocate(*batch[1]))


@pytest.mark.gpu
def test_gpu_rejects_bad_input_and_keeps_working(gpu_solver):
    ok = ([1, 2], [100.0, 200.0], [0.0, 5.0], [150.0, 300.0], 2)
    bad = [
        ([1, 0], ok[1], ok[2], ok[3], 2),              # sf = 0
        (ok[0], [100.0, -1.0], ok[2], ok[3], 2),       # p < 0
        (ok[0], ok[1], ok[2], [150.0, 0.0], 2),        # E = 0
        (ok[0], ok[1], [0.0, float("nan")], ok[3], 2),  # a NaN
        (ok[0], ok[1], ok[2], ok[3], 0),               # G = 0
    ]
    for inst in bad:
        with pytest.raises(sn.NativeError):
            gpu_solver.ftf_allocate(*inst)
        assert fc.same_bits(gpu_solver.ftf_allocate(*ok), ftf_ref.twin_allocate(*ok))
    x, rho, mu = gpu_solver.ftf_allocate([], [], [], [], 4)
    assert len(x) == 0 and rho == 0.0 and mu == 0.0


@pytest.mark.gpu
def test_gpu_policy_sequence_equals_twin_engine(gpu_solver):
    _, g, pg = fc.policy_sequence(gpu_solver)
    _, c, pc = fc.policy_sequence(ftf_ref.TwinEngine())
    assert g == c
    assert pg.last_level == pc.last_level
    assert pg._cumulative_isolated_time == pc._cumulative_isolated_time


@pytest.mark.gpu
def test_gpu_simulation_equals_twin_simulation(gpu_solver):
    rg, rc = {"workers": [], "allocations": []}, {"workers": [], "allocations": []}
    g = fc.simulate_30(gpu_solver, rg)
    c = fc.simulate_30(ftf_ref.TwinEngine(), rc)
    assert rg == rc
    for s in (g, c):
        s.pop("solve_seconds")
    assert g == c
