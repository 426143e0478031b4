"""The AlloX assignment without a GPU: the CPU twin of the kernel
(tests/twins/allox_twin.c, the step functions of csrc/sw_allox.h) against
scipy.optimize.linear_sum_assignment on the reference's dense matrix
(allox.py:71-103), the structure of every assignment, and the fixed cases
whose answers are known by hand.  tests/test_gpu_allox.py holds the kernel to
the twin bit for bit.

The assignment itself is not compared with scipy's: workers of one type are
identical columns, so the optimum is not unique (the tie example below) and
the tie rule here is the one stated in csrc/sw_allox.h, not scipy's.
"""
import numpy as np
import pytest

import allox_ref
import alloxcases as ac


def solve(inst):
    assert allox_ref.dense_entries(inst[0], inst[2]) <= allox_ref.DENSE_CAP
    r = allox_ref.twin_assign(*inst)
    allox_ref.check_structure(*inst, *r)
    return r, allox_ref.dense_optimum(*inst)


def real_bar(m):
    """8 × the recorded worst gap; the rounding of the sum itself, 4·m·2^-53,
    if the record is 0."""
    return ac.GAP_FACTOR * ac.WORST_REAL_GAP if ac.WORST_REAL_GAP > 0 else 4 * m * ac.EPS


@pytest.fixture(scope="module")
def real_gaps():
    out = []
    for inst in ac.real_gap_instances():
        r, opt = solve(inst)
        out.append((len(inst[2]), abs(r[3] - opt) / opt))
    return out


def test_integer_costs_equal_scipy_exactly():
    """p and d integers below 2^20: every product, sum and dual is exact in
    double, so the twin's cost is scipy's to the bit."""
    insts = ac.integer_instances() + ac.boundary_instances()[0::2]
    assert len(insts) >= 200
    for k, inst in enumerate(insts):
        assert np.all(inst[1] == np.floor(inst[1])) and inst[1].max(initial=0) < 2 ** 20
        r, opt = solve(inst)
        assert r[3] == opt, (k, len(inst[2]), inst[0], r[3], opt)


def test_real_costs_within_the_bar(real_gaps):
    for k, (m, gap) in enumerate(real_gaps):
        print(k, m, gap)
        assert gap <= real_bar(m), (k, m, gap)


def test_recorded_gap_is_what_the_sets_give(real_gaps):
    assert max(g for _, g in real_gaps) == ac.WORST_REAL_GAP
    assert ac.GAP_FACTOR * ac.WORST_REAL_GAP <= 1e-14


def test_sets_cover_the_boundary_sizes_and_types():
    sizes = sorted({len(i[2]) + int(i[0].sum()) for i in ac.boundary_instances()})
    assert sizes == [63, 64, 65, 255, 256, 257, 511, 512, 513]
    assert {len(i[0]) for i in ac.boundary_instances()} == {1, 2, 3}
    assert {len(i[0]) for i in ac.integer_instances()} == {1, 2, 3}
    for inst in ac.boundary_instances():
        if len(inst[2]) + int(inst[0].sum()) == 513:
            assert int(inst[0].sum()) >= 400


def test_structure_beyond_the_dense_cap():
    """Long chains and the caps themselves (1024 jobs, 1024 workers): the
    twin alone, its structure and the bound on the search steps."""
    for inst in ac.tall_instances():
        steps = []
        r = allox_ref.twin_assign(*inst, steps=steps)
        allox_ref.check_structure(*inst, *r)
        m = len(inst[2])
        assert m <= steps[0] <= m * (m + 1) // 2


@pytest.mark.parametrize("name", sorted(ac.FIXED))
def test_fixed_cases_cost_and_structure(name):
    inst = ac.FIXED[name]
    r, opt = solve(inst)
    if name == "bounds":  # 1·1e30 + 1e15 + 0: not integers below 2^20, one rounding each
        assert abs(r[3] - opt) <= 4 * 2 * ac.EPS * opt
    else:
        assert r[3] == opt


def test_fixed_answers_known_by_hand():
    t = lambda name: allox_ref.twin_assign(*ac.FIXED[name])
    jw, jp, wf, cost = t("m1")
    assert (list(jw), list(jp), list(wf), cost) == ([0], [1], [0, -1], 8.0)
    # m < n: every job at position 1 on a worker of its own; the others idle
    jw, jp, wf, cost = t("m_lt_n")
    assert list(jp) == [1, 1, 1] and len(set(jw)) == 3 and cost == 4 + 2 + 9 + 1 + 2 + 3
    assert sorted(wf) == [-1, -1, 0, 1, 2]
    # m = n + 1: the smallest p (job 1, p = 3) at position 2, first on its worker
    jw, jp, wf, cost = t("m_eq_n_plus_1")
    assert list(jp) == [1, 2, 1, 1] and wf[jw[1]] == 1 and cost == 7 + 2 * 3 + 9 + 5
    # the tie example: p = 1 runs first on one worker, behind it either other job
    jw, jp, wf, cost = t("tie_three")
    assert cost == 7.0 and jp[0] == 2 and wf[jw[0]] == 0 and sorted(jp[1:]) == [1, 1] and jw[1] != jw[2]
    # two types: the slow job on the type where it is least slow
    jw, jp, wf, cost = t("two_types")
    assert (list(jw), list(jp), list(wf), cost) == ([0, 1], [1, 1], [0, 1], 10 + 5 + 60 + 7.0)
    # a type with no free workers is never used: workers are 0 (type 0), 1 and 2 (type 2)
    jw, jp, wf, cost = t("empty_type")
    assert set(jw) <= {0, 1, 2} and cost == allox_ref.dense_optimum(*ac.FIXED["empty_type"])
    # all p equal: 7 jobs on 3 workers, chains of 3, 2, 2
    jw, jp, wf, cost = t("all_p_equal")
    assert sorted(np.bincount(jw, minlength=3)) == [2, 2, 3] and cost == 6 * (3 * 1 + 3 * 2 + 3) + 21
    # rows with p = 0 cost their delay wherever they sit
    jw, jp, wf, cost = t("p_zero_rows")
    assert cost == 6.0 + 4 + 1 and jp[1] == 1 and jp[3] == 1 and jw[1] != jw[3]
    jw, jp, wf, cost = t("all_zero")
    assert cost == 0.0
    for name in ("no_free_worker", "no_jobs"):
        jw, jp, wf, cost = t(name)
        assert np.all(jw == -1) and np.all(jp == 0) and np.all(wf == -1) and cost == 0.0


def test_tie_rule_prefers_the_lowest_slot():
    """csrc/sw_allox.h: equal distances go to the lowest slot — an unassigned
    column before an assigned one, then the lower worker."""
    jw, jp, wf, _ = allox_ref.twin_assign([3], [[5.0], [5.0]], [0.0, 0.0])
    assert list(jw) == [0, 1] and list(jp) == [1, 1] and list(wf) == [0, 1, -1]
    # two equal jobs, one worker: the later row takes the free position 2 rather than displacing
    jw, jp, wf, _ = allox_ref.twin_assign([1], [[0.0], [0.0]], [0.0, 0.0])
    assert list(jw) == [0, 0] and list(jp) == [1, 2] and list(wf) == [1]


def test_twin_refuses_sizes_beyond_the_caps():
    import ctypes as C
    lib = allox_ref._lib()
    dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int32)
    for m, n in ((allox_ref.MAX_JOBS + 1, 1), (1, allox_ref.MAX_WORKERS + 1)):
        free = np.array([n], dtype=np.int32)
        p, d = np.ones((m, 1)), np.zeros(m)
        jw, jp, wf = np.zeros(m, dtype=np.int32), np.zeros(m, dtype=np.int32), np.zeros(n, dtype=np.int32)
        rc = lib.allox_twin_assign(m, 1, free.ctypes.data_as(ip), p.ctypes.data_as(dp), d.ctypes.data_as(dp),
                                   jw.ctypes.data_as(ip), jp.ctypes.data_as(ip), wf.ctypes.data_as(ip), None,
                                   None, None)
        assert rc == 1
