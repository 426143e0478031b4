"""Max sum throughput over worker types that differ on the GPU
(sw_mst_allocate_types / _batch, csrc/sw_mst_types.hip): allocation, prices and
all four results bit for bit those of the CPU twin at every shape of
tests/msttcases.py (the flow in LDS up to lds_limit, in the workspace beyond),
single and batched, and the kernel's own certificate."""
import numpy as np
import pytest

import msttcases as tc

pytestmark = pytest.mark.gpu


def _same(got, want):
    assert got[2:] == want[2:] and float(got[2]).hex() == float(want[2]).hex(), (got[2:], want[2:])
    for a, b in zip(got[:2], want[:2]):
        assert np.array_equal(np.ascontiguousarray(a).view(np.uint64), np.ascontiguousarray(b).view(np.uint64))


@pytest.mark.parametrize("name", list(tc.cases()))
def test_gpu_bit_exact_vs_twin(gpu_solver, name):
    W, sf, w = tc.cases()[name]
    got = gpu_solver.mst_allocate_types(W, sf, w)
    print(f"{name}: gpu objective {got[2]!r} augmentations {got[3]} rows {got[4]} flags {got[5]}")
    _same(got, tc.twin_of(name))
    assert tc.certificate(W, sf, w, got) <= 4 * w.size * tc.EPS


def test_gpu_batch_equals_single_calls_and_twin(gpu_solver):
    """Uneven instances over three types in one launch, one of them empty."""
    names = ["zero_type", "m513", "wide", "roomy", "m511"]
    insts = [tc.cases()[n] for n in names]
    insts.insert(2, (np.array([1, 2, 3], dtype=np.int32), np.zeros(0, dtype=np.int32), np.zeros((0, 3))))
    outs = gpu_solver.mst_allocate_types_batch(insts)
    empty = outs.pop(2)
    assert empty[0].shape == (0, 3) and (empty[1] == 0.0).all() and empty[2:] == (0.0, 0, 0, 0)
    for name, got in zip(names, outs):
        _same(got, tc.twin_of(name))


def test_gpu_refusals_each_followed_by_a_good_call(gpu_solver):
    import sw_native as sn

    W, sf, w = tc.cases()["n2_m3"]
    bad_w = w.copy()
    bad_w[1, 0] = np.inf
    for args, text in (((W, [1, 0, 2], w), "scale factors"), ((W, sf, -w), "weights"), ((W, sf, bad_w), "weights"),
                       (([1, -1], sf, w), "worker counts")):
        with pytest.raises(sn.NativeError, match=text) as e:
            gpu_solver.mst_allocate_types(*args)
        assert e.value.code == -1
        _same(gpu_solver.mst_allocate_types(W, sf, w), tc.twin_of("n2_m3"))
    assert gpu_solver.mst_allocate_types([3, 1], [], np.zeros((0, 2)))[2:] == (0.0, 0, 0, 0)
