"""Water-filling MaxMinFairness on the GPU: the HIP kernel (sw_wf_allocate and
sw_wf_allocate_batch) against its CPU twin bit for bit, on the LDS path and
the L2 path, the exact certificate on the GPU's own level, bad input, and the
policy mirror and the simulator on the HIP engine against the twin engine."""
import numpy as np
import pytest

import sw_native as sn
import wf_ref
import wfcases as wc


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(wc.FIXED))
def test_gpu_fixed_list_bit_exact_vs_twin(gpu_solver, name):
    inst = wc.FIXED[name]
    g = gpu_solver.wf_allocate(*inst)
    assert wc.same_bits(g, wf_ref.twin_allocate(*inst))
    wc.check_allocation(inst, *g)


BOUNDARY = {n: next(k for k, v in wc.FIXED.items() if len(v[0]) == n) for n in (511, 512, 513, 1025, 2048, 2049)}


@pytest.mark.gpu
@pytest.mark.parametrize("n", sorted(BOUNDARY))
def test_gpu_chunk_and_path_boundaries(gpu_solver, n):
    """q = ⌈N/512⌉ steps at 513 and 1025; 2048 is the last size staged in LDS,
    2049 the first read from L2.  Each size at a binding and at an ample
    cluster, against the twin."""
    sf, c, G = wc.FIXED[BOUNDARY[n]]
    assert len(sf) == n
    for g_workers in (G, 7, int(sf.sum()) - 1, int(sf.sum())):
        g = gpu_solver.wf_allocate(sf, c, g_workers)
        assert wc.same_bits(g, wf_ref.twin_allocate(sf, c, g_workers)), (n, g_workers)
        assert g[2] <= g_workers


@pytest.mark.gpu
def test_gpu_fuzz_bit_exact_vs_twin(gpu_solver):
    for i, inst in enumerate(wc.random_instances(300, seed=11, max_n=5000)):
        g = gpu_solver.wf_allocate(*inst)
        assert wc.same_bits(g, wf_ref.twin_allocate(*inst)), (i, len(inst[0]), inst[2])
        sf, c, G = inst
        if int(sf.sum()) > G:
            assert wf_ref.certified(sf, c, G, g[1], 1e-9), (i, len(sf), G)
        else:
            assert np.all(g[0] == 1.0) and g[1] == c.max()


def batches():
    small = wc.random_instances(300, seed=17, max_n=40, max_g=64)
    empty = (np.zeros(0, dtype=np.int32), np.zeros(0, dtype=np.float64), 4)
    l2 = next(k for k, v in wc.FIXED.items() if len(v[0]) == 2500)
    return {
        "one": [wc.FIXED["no_unit_width"]],
        "empty_middle": [wc.FIXED["spread"], empty, wc.FIXED[BOUNDARY[513]]],
        "many_small": small,  # more workgroups than CUs
        "mixed_paths": small[:5] + [wc.FIXED[l2]] + small[5:9] + [wc.FIXED[BOUNDARY[1025]], wc.FIXED[BOUNDARY[2049]]],
    }


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["one", "empty_middle", "many_small", "mixed_paths"])
def test_gpu_batch_equals_single_calls(gpu_solver, name):
    batch = batches()[name]
    got = gpu_solver.wf_allocate_batch(batch)
    assert len(got) == len(batch)
    for i, (inst, g) in enumerate(zip(batch, got)):
        if len(inst[0]) == 0:
            assert len(g[0]) == 0 and g[1] == 0.0 and g[2] == 0.0
        else:
            assert wc.same_bits(g, gpu_solver.wf_allocate(*inst)), (name, i)


@pytest.mark.gpu
def test_gpu_batch_rejects_bad_offsets_and_empty_batch_is_a_noop(gpu_solver):
    batch = [wc.FIXED["spread"], wc.FIXED["no_unit_width"]]
    for off in ([0, 9, 5], [1, 5, 9]):
        with pytest.raises(sn.NativeError) as e:
            gpu_solver.wf_allocate_batch(batch, offsets=off)
        assert e.value.code == sn.SW_ERR_INVALID
    with pytest.raises(sn.NativeError) as e:
        gpu_solver.wf_allocate_batch([batch[0], batch[1][:2] + (0,)])
    assert e.value.code == sn.SW_ERR_INVALID
    assert gpu_solver.wf_allocate_batch([]) == []
    assert wc.same_bits(gpu_solver.wf_allocate_batch(batch)[1], gpu_solver.wf_allocate(*batch[1]))


@pytest.mark.gpu
def test_gpu_rejects_bad_input_and_keeps_working(gpu_solver):
    ok = ([1, 2], [1.0, 4.0], 2)
    bad = [
        ([1, 0], ok[1], 2),                    # sf = 0
        ([1, 256], ok[1], 2),                  # sf > 255
        (ok[0], [1.0, 0.0], 2),                # c = 0
        (ok[0], [1.0, -2.0], 2),               # c < 0
        (ok[0], [float("nan"), 4.0], 2),       # c NaN
        (ok[0], [1.0, float("inf")], 2),       # c infinite
        (ok[0], ok[1], 0),                     # G = 0
        (ok[0], ok[1], -3),                    # G < 0
    ]
    for inst in bad:
        with pytest.raises(sn.NativeError) as e:
            gpu_solver.wf_allocate(*inst)
        assert e.value.code == sn.SW_ERR_INVALID
        assert wc.same_bits(gpu_solver.wf_allocate(*ok), wf_ref.twin_allocate(*ok))
    # null pointers with jobs present, straight at the C-ABI
    assert gpu_solver.lib.sw_wf_allocate(gpu_solver.h, 2, 2, None, None, None, None) == sn.SW_ERR_INVALID
    assert wc.same_bits(gpu_solver.wf_allocate(*ok), wf_ref.twin_allocate(*ok))
    x, level, used = gpu_solver.wf_allocate([], [], 4)
    assert len(x) == 0 and level == 0.0 and used == 0.0


@pytest.mark.gpu
def test_gpu_policy_sequence_equals_twin_engine(gpu_solver):
    _, g, pg = wc.policy_sequence(gpu_solver)
    _, c, pc = wc.policy_sequence(wf_ref.TwinEngine())
    assert g == c
    assert pg.last_level == pc.last_level


@pytest.mark.gpu
def test_gpu_simulation_equals_twin_simulation(gpu_solver):
    rg, rc = {"workers": [], "allocations": []}, {"workers": [], "allocations": []}
    g = wc.simulate_30("max_min_fairness_water_filling", rg, wf_allocator=sn.WfAllocator(solver=gpu_solver))
    c = wc.simulate_30("max_min_fairness_water_filling", rc, wf_allocator=wf_ref.twin_allocator)
    assert rg == rc
    for s in (g, c):
        s.pop("solve_seconds")
    assert g == c
