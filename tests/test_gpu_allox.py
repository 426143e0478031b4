"""AlloX on the GPU: the HIP kernel (sw_allox_assign and sw_allox_assign_batch)
against its CPU twin bit for bit — job_worker, job_position, worker_first and
the bits of the cost — on the one-wave and the 512-thread path, the caps, bad
input, and the policy mirror and the simulator on the HIP engine against the
twin engine."""
import numpy as np
import pytest

import allox_ref
import alloxcases as ac
import sw_native as sn


def slots(inst):
    return len(inst[2]) + int(inst[0].sum())


@pytest.fixture(scope="module")
def sets():
    """name → (instances, the twin's results), computed once."""
    groups = {"fixed": [ac.FIXED[k] for k in sorted(ac.FIXED)], "fuzz": ac.gpu_instances(),
              "boundary": ac.boundary_instances(), "tall": ac.tall_instances()}
    return {k: (v, [allox_ref.twin_assign(*i) for i in v]) for k, v in groups.items()}


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["fixed", "fuzz", "boundary", "tall"])
def test_gpu_single_calls_bit_exact_vs_twin(gpu_solver, sets, name):
    insts, want = sets[name]
    if name == "fuzz":
        assert len(insts) >= 200 and max(len(i[2]) for i in insts) <= 60
    if name == "boundary":
        assert sorted({slots(i) for i in insts}) == [63, 64, 65, 255, 256, 257, 511, 512, 513]
    if name == "tall":  # p and d in LDS, and (the 1,024-job instance) left in global memory
        assert {ac.staged(i) for i in insts} == {True, False}
    for k, (inst, w) in enumerate(zip(insts, want)):
        g = gpu_solver.allox_assign(*inst)
        assert ac.same_bits(g, w), (name, k, len(inst[2]), inst[0], g[3], w[3])
        allox_ref.check_structure(*inst, *g)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["fixed", "fuzz", "boundary", "tall"])
def test_gpu_one_batch_bit_exact_vs_twin(gpu_solver, sets, name):
    """All instances of a set in one launch: "fixed" and "fuzz" run one wave
    per instance, "boundary" and "tall" 512 threads (their largest has more
    than 256 slots), so the small boundary sizes run on both paths."""
    insts, want = sets[name]
    assert (max(slots(i) for i in insts) <= ac.WAVE_SLOTS) == (name in ("fixed", "fuzz"))
    got = gpu_solver.allox_assign_batch(insts)
    assert len(got) == len(insts)
    for k, (g, w) in enumerate(zip(got, want)):
        assert ac.same_bits(g, w), (name, k, len(insts[k][2]), insts[k][0], g[3], w[3])


@pytest.mark.gpu
def test_gpu_caps_and_bad_input_keep_the_handle_usable(gpu_solver):
    ok = ac.FIXED["two_types"]
    want = allox_ref.twin_assign(*ok)
    nan, inf = float("nan"), float("inf")
    one = lambda m: (np.ones((m, 1)), np.zeros(m))
    cases = [
        (([1], *one(1025)), sn.SW_ERR_CAPACITY, "1024"),                 # jobs above the cap
        (([1025], *one(2)), sn.SW_ERR_CAPACITY, "1024"),                 # workers above the cap
        (([600, 425], np.ones((2, 2)), np.zeros(2)), sn.SW_ERR_CAPACITY, "1024"),
        (([1, 1], [[1.0, nan], [1.0, 1.0]], [0.0, 0.0]), sn.SW_ERR_INVALID, "processing times"),
        (([1, 1], [[1.0, -1.0], [1.0, 1.0]], [0.0, 0.0]), sn.SW_ERR_INVALID, "processing times"),
        (([1, 1], [[1.0, inf], [1.0, 1.0]], [0.0, 0.0]), sn.SW_ERR_INVALID, "processing times"),
        (([1, 1], [[1.0, 1.0000001e30], [1.0, 1.0]], [0.0, 0.0]), sn.SW_ERR_INVALID, "processing times"),
        (([1, 1], np.ones((2, 2)), [0.0, nan]), sn.SW_ERR_INVALID, "delays"),
        (([1, 1], np.ones((2, 2)), [0.0, -1.0]), sn.SW_ERR_INVALID, "delays"),
        (([1, 1], np.ones((2, 2)), [0.0, 1.0000001e15]), sn.SW_ERR_INVALID, "delays"),
        (([1, -1], np.ones((2, 2)), [0.0, 0.0]), sn.SW_ERR_INVALID, "worker counts"),
        (([1] * 9, np.ones((2, 9)), [0.0, 0.0]), sn.SW_ERR_INVALID, "num_types"),
        (([], np.ones((2, 0)), [0.0, 0.0]), sn.SW_ERR_INVALID, "num_types"),
    ]
    for inst, code, rule in cases:
        with pytest.raises(sn.NativeError) as e:
            gpu_solver.allox_assign(*inst)
        assert e.value.code == code and rule in str(e.value), str(e.value)
        assert ac.same_bits(gpu_solver.allox_assign(*ok), want)
    # a batch with one bad instance is rejected whole; the next batch succeeds
    with pytest.raises(sn.NativeError) as e:
        gpu_solver.allox_assign_batch([ok, cases[3][0], ok])
    assert e.value.code == sn.SW_ERR_INVALID
    got = gpu_solver.allox_assign_batch([ok, ac.FIXED["no_free_worker"], ac.FIXED["no_jobs"], ok])
    assert ac.same_bits(got[0], want) and ac.same_bits(got[3], want)
    for g, name in ((got[1], "no_free_worker"), (got[2], "no_jobs")):
        assert np.all(g[0] == -1) and np.all(g[1] == 0) and np.all(g[2] == -1) and g[3] == 0.0
        assert len(g[0]) == len(ac.FIXED[name][2]) and len(g[2]) == int(ac.FIXED[name][0].sum())
    assert gpu_solver.allox_assign_batch([]) == []


@pytest.mark.gpu
def test_gpu_policy_sequence_equals_twin_engine(gpu_solver):
    _, g, pg = ac.policy_sequence(gpu_solver)
    _, c, pc = ac.policy_sequence(allox_ref.TwinEngine())
    assert g == c
    assert pg.last_cost == pc.last_cost and pg._prev_allocation == pc._prev_allocation


@pytest.mark.gpu
def test_gpu_simulation_equals_twin_simulation(gpu_solver):
    rg, rc = {"workers": [], "allocations": []}, {"workers": [], "allocations": []}
    g = ac.simulate_30(gpu_solver, rg)
    c = ac.simulate_30(allox_ref.TwinEngine(), rc)
    assert rg == rc
    for s in (g, c):
        s.pop("solve_seconds")
    assert g == c
