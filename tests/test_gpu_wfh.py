"""Hierarchical (entity) water filling on the GPU: the HIP kernel
(sw_wfh_allocate and sw_wfh_allocate_batch) against its CPU twin bit for bit in
the shares, the entity capacities and the level; the batch against the single
calls; bad input; the policy mirror on the HIP engine against the twin engine."""
import ctypes as C

import numpy as np
import pytest

import sw_native as sn
import wfh_ref
import wfhcases as wc

SIZES = (1, 2, 63, 64, 65, 511, 512, 513, 1025, 2049)


def workers_of(inst):
    t = wc.total(inst)
    return sorted({g for g in (1, t - 1, t, t + 1, t // 2) if g >= 1})


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["fairness", "fifo", "mixed"])
@pytest.mark.parametrize("lay", wc.LAYOUTS)
def test_gpu_bit_exact_vs_twin(gpu_solver, lay, kind):
    """Every size, layout and kind of modes at G in {1, Σsf − 1, Σsf, Σsf + 1,
    ≈ Σsf/2}.  The sizes step the job chunk (513, 1025, 2049), the entity chunk
    (singletons: 513 entities and more), the 64-member tile of the fifo prefix
    and the lanes' strides (one entity of 63, 64, 65 jobs), and the entity of
    one job, which takes the fifo formula, next to entities of two and more."""
    rng = np.random.default_rng(1000 + 10 * wc.LAYOUTS.index(lay) + len(kind))
    for n in SIZES:
        inst = wc.draw(rng, n, lay, kind, continuous=n % 2 == 1)
        for G in workers_of(inst):
            one = wc.with_G(inst, G)
            g = gpu_solver.wfh_allocate(*one)
            assert wc.same_bits(g, wfh_ref.twin_allocate(*one)), (n, G)
            assert g[3] <= G * (1 + 1e-12)


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(wc.FIXED))
def test_gpu_fixed_list_bit_exact_vs_twin(gpu_solver, name):
    inst = wc.FIXED[name]
    g = gpu_solver.wfh_allocate(*inst)
    assert wc.same_bits(g, wfh_ref.twin_allocate(*inst))
    wc.check_properties(inst, *g)


@pytest.mark.gpu
def test_gpu_entities_of_one_and_two_jobs_side_by_side(gpu_solver):
    """The smallest shape on each side of the one path boundary: an entity of
    one job is filled by the fifo formula, an entity of two by its mode's."""
    sf, c = wc.i32(4, 2, 2, 8, 1), wc.f64(4.0, 1.0, 4.0, 2.0, 3.0)
    for modes in ([0, 0, 0], [1, 1, 1], [0, 1, 0]):
        for G in (3, 9, 16):
            inst = (sf, c, wc.i32(0, 1, 1, 2, 2), wc.f64(1.0, 2.0, 0.5), np.array(modes, dtype=np.int32), G)
            assert wc.same_bits(gpu_solver.wfh_allocate(*inst), wfh_ref.twin_allocate(*inst)), (modes, G)


def batch_of_64():
    rng = np.random.default_rng(77)
    empty = (wc.i32(), wc.f64(), wc.i32(), wc.f64(1.0, 2.0), wc.i32(0, 1), 4)
    out = []
    for i in range(64):
        if i in (0, 31, 63):
            out.append(empty)
        else:
            n = (1, 7, 40, 64, 65, 130, 600)[i % 7]
            out.append(wc.draw(rng, n, wc.LAYOUTS[i % 5], ("fairness", "fifo", "mixed")[i % 3], continuous=i % 2 == 0))
    return out


@pytest.mark.gpu
def test_gpu_batch_of_64_equals_single_calls(gpu_solver):
    batch = batch_of_64()
    got = gpu_solver.wfh_allocate_batch(batch)
    assert len(got) == 64
    for i, (inst, g) in enumerate(zip(batch, got)):
        if len(inst[0]) == 0:
            assert len(g[0]) == 0 and list(g[1]) == [0.0, 0.0] and g[2] == 0.0 and g[3] == 0.0, i
        else:
            assert wc.same_bits(g, gpu_solver.wfh_allocate(*inst)), i
            assert wc.same_bits(g, wfh_ref.twin_allocate(*inst)), i
    assert gpu_solver.wfh_allocate_batch([]) == []
    x, g, level, used = gpu_solver.wfh_allocate([], [], [], [1.0], [0], 4)
    assert len(x) == 0 and list(g) == [0.0] and level == 0.0 and used == 0.0


@pytest.mark.gpu
def test_gpu_rejects_bad_input_names_the_entry_point_and_keeps_working(gpu_solver):
    ok = ([1, 2, 1], [1.0, 4.0, 2.0], [0, 1, 0], [1.0, 2.0], [0, 1], 2)

    def bad_single(**kw):
        keys = ("sf", "c", "ent", "W", "modes", "G")
        inst = tuple(kw.get(k, v) for k, v in zip(keys, ok))
        with pytest.raises(sn.NativeError) as e:
            gpu_solver.wfh_allocate(*inst)
        assert e.value.code == sn.SW_ERR_INVALID
        assert gpu_solver.error().startswith("sw_wfh_allocate:"), gpu_solver.error()
        assert wc.same_bits(gpu_solver.wfh_allocate(*ok), wfh_ref.twin_allocate(*ok))

    bad_single(sf=[1, 0, 1])                      # sf = 0
    bad_single(sf=[1, 256, 1])                    # sf > 255
    bad_single(c=[1.0, 0.0, 2.0])                 # c = 0
    bad_single(c=[1.0, -2.0, 2.0])                # c < 0
    bad_single(c=[float("nan"), 4.0, 2.0])        # c NaN
    bad_single(c=[1.0, float("inf"), 2.0])        # c infinite
    bad_single(ent=[0, 2, 0])                     # entity index past the end
    bad_single(ent=[0, -1, 0])                    # entity index < 0
    bad_single(W=[1.0, 0.0])                      # weight = 0
    bad_single(W=[-1.0, 2.0])                     # weight < 0
    bad_single(W=[float("inf"), 2.0])             # weight infinite
    bad_single(W=[1.0, float("nan")])             # weight NaN
    bad_single(modes=[0, 2])                      # mode past 1
    bad_single(modes=[-1, 1])                     # mode < 0
    bad_single(G=0)                               # no workers
    bad_single(G=-3)
    # null pointers with jobs present, and negative counts, straight at the C-ABI
    lib, h = gpu_solver.lib, gpu_solver.h
    assert lib.sw_wfh_allocate(h, 2, 1, 2, None, None, None, None, None, None, None, None) == sn.SW_ERR_INVALID
    assert gpu_solver.error().startswith("sw_wfh_allocate:")
    assert lib.sw_wfh_allocate(h, -1, 1, 2, None, None, None, None, None, None, None, None) == sn.SW_ERR_INVALID
    assert gpu_solver.error().startswith("sw_wfh_allocate:")

    batch = [ok, (ok[0][:2], ok[1][:2], [0, 0], [3.0], [0], 5)]
    for kw in (dict(job_offsets=[0, 4, 3]), dict(job_offsets=[1, 3, 5]), dict(entity_offsets=[0, 3, 2]),
               dict(entity_offsets=[1, 2, 3])):
        with pytest.raises(sn.NativeError) as e:
            gpu_solver.wfh_allocate_batch(batch, **kw)
        assert e.value.code == sn.SW_ERR_INVALID
        assert gpu_solver.error().startswith("sw_wfh_allocate_batch:"), gpu_solver.error()
    for broken in ([ok, batch[1][:5] + (0,)],                                  # no workers
                   [ok, (ok[0][:2], ok[1][:2], [0, 1], [3.0], [0], 5)],        # the instance's own entity range
                   [ok, (ok[0][:2], ok[1][:2], [0, 0], [3.0], [7], 5)]):       # mode
        with pytest.raises(sn.NativeError) as e:
            gpu_solver.wfh_allocate_batch(broken)
        assert e.value.code == sn.SW_ERR_INVALID
        assert gpu_solver.error().startswith("sw_wfh_allocate_batch:"), gpu_solver.error()
    lp = C.POINTER(C.c_int64)
    assert lib.sw_wfh_allocate_batch(h, 1, lp(), lp(), None, None, None, None, None, None, None, None,
                                     None) == sn.SW_ERR_INVALID
    assert gpu_solver.error().startswith("sw_wfh_allocate_batch:")
    assert lib.sw_wfh_allocate_batch(h, -1, lp(), lp(), None, None, None, None, None, None, None, None,
                                     None) == sn.SW_ERR_INVALID
    got = gpu_solver.wfh_allocate_batch(batch)
    assert all(wc.same_bits(g, wfh_ref.twin_allocate(*inst)) for g, inst in zip(got, batch))


@pytest.mark.gpu
def test_gpu_policy_mirror_equals_twin_engine(gpu_solver):
    g, pg = wc.policy_run(gpu_solver)
    c, pc = wc.policy_run(wfh_ref.TwinEngine())
    assert g == c
    assert pg.last_level == pc.last_level and pg.last_entity_capacity == pc.last_entity_capacity
