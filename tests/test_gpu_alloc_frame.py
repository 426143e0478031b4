"""The allocation frame on the GPU (csrc/sw_alloc.h): the four per-job policies
and AlloX share one input block and one output block per handle, so a call
after a larger one runs over that call's bytes.  One handle makes the calls
below in this order, each compared bit for bit with its CPU twin: a view at a
wrong offset, or a zero-fill that did not happen (the absent floors of mst),
would read a stale byte of an earlier, larger block."""
import numpy as np
import pytest

import allox_ref
import alloxcases as ac
import ftf_ref
import ftfcases as fc
import mst_ref
import mstcases as mc
import mtd_ref
import mtdcases as dc
import wf_ref
import wfcases as wc


@pytest.mark.gpu
def test_gpu_policies_share_one_buffer_set_bit_exact_vs_twins(gpu_solver):
    s = gpu_solver
    rng = np.random.default_rng(23)

    # 1. mst above its staged size: the global path, and the largest block of the sequence
    big = mc.draw(rng, mc.LDS_JOBS + 1, floors="ok", fill=0.5)
    assert len(big[0]) == 3073 and big[2] is not None and np.count_nonzero(big[2]) > 0
    assert mc.same_bits(s.mst_allocate(*big), mst_ref.twin_allocate(*big))

    # 2. wf at N = 1: the smallest block
    one = wc.draw(rng, 1, 4)
    assert wc.same_bits(s.wf_allocate(*one), wf_ref.twin_allocate(*one))

    # 3. ftf at N = 513: two jobs per thread, four columns
    ftf = fc.draw(rng, 513, 300)
    assert fc.same_bits(s.ftf_allocate(*ftf), ftf_ref.twin_allocate(*ftf))

    # 4. mtd one job above its staged size
    mtd = dc.draw(rng, dc.LDS_JOBS + 1, 2000, zero_job=True)
    assert len(mtd[0]) == 4097
    assert dc.same_bits(s.mtd_allocate(*mtd), mtd_ref.twin_allocate(*mtd))

    # 5. an mst batch without floors: the floors column is absent and must read as zeros
    a, b = mc.draw(rng, 5, fill=0.5), mc.draw(rng, 513, fill=0.4)
    assert a[2] is None and b[2] is None
    empty = (np.zeros(0, dtype=np.int32), np.zeros(0, dtype=np.float64), None, 4)
    got = s.mst_allocate_batch([a, empty, b])
    assert mc.same_bits(got[0], mst_ref.twin_allocate(*a))
    assert len(got[1][0]) == 0 and got[1][1:] == (0.0, 0.0, 0.0, False)
    assert mc.same_bits(got[2], mst_ref.twin_allocate(*b))

    # 6. the same batch with floors in the middle instance only: the column is present
    got = s.mst_allocate_batch([a, empty[:2] + (np.zeros(0, dtype=np.float64), 4), b])
    assert mc.same_bits(got[0], mst_ref.twin_allocate(*a))
    assert len(got[1][0]) == 0 and got[1][1:] == (0.0, 0.0, 0.0, False)
    assert mc.same_bits(got[2], mst_ref.twin_allocate(*b))

    # 7. AlloX on the same blocks
    inst = ac.FIXED["empty_type"]
    assert ac.same_bits(s.allox_assign(*inst), allox_ref.twin_assign(*inst))

    # 8. the smallest block again
    assert wc.same_bits(s.wf_allocate(*one), wf_ref.twin_allocate(*one))
