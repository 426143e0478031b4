"""MinTotalDuration allocation (Gavel's makespan baseline, sw_mtd_allocate):
the CPU twin of the HIP kernel (tests/twins/mtd_twin.c) against the
reference's search (policies/min_total_duration.py:82-101) written out twice
in tests/mtd_ref.py — over the closed-form predicate in exact rationals, and
over the reference's LP through HiGHS — and the conditions of its allocation.
The HIP kernel against the twin, bit for bit: tests/test_gpu_mtd.py."""
import numpy as np
import pytest

import mtd_ref
import mtdcases as mc


def check(inst):
    sf, p, G = inst
    probes = []
    x, T, mu = mtd_ref.twin_allocate(sf, p, G, probes)
    Tx, px, _ = mtd_ref.exact_search(sf, p, G)
    assert np.float64(T).tobytes() == np.float64(Tx).tobytes(), (T, Tx)
    assert probes[0] == len(px)
    mc.check_allocation(inst, x, T, mu)
    return x, T, mu


@pytest.mark.parametrize("name", sorted(mc.FIXED))
def test_twin_matches_the_exact_search_and_allocation_holds(name):
    check(mc.FIXED[name])


def test_fixed_list_reaches_every_path():
    r, n = {}, {}
    for k, v in mc.FIXED.items():
        probes = []
        r[k] = mtd_ref.twin_allocate(*v, probes)
        n[k] = probes[0]
    for k, (T, count) in mc.KNOWN.items():
        assert r[k][1] == T and n[k] == count, (k, r[k][1], n[k])
    assert r["n1"][2] > 0.0
    # max p sets T: the long job's share is within 5 % of 1
    assert 8e4 <= r["box_sets_T"][1] <= 8e4 * 1.05 and r["box_sets_T"][0][0] >= 1 / 1.05
    # capacity sets T: max p is far below it
    sf, p, G = mc.FIXED["cap_sets_T"]
    assert r["cap_sets_T"][1] > 10 * p.max()
    assert np.all(r["all_zero"][0] > 0.0) and r["all_zero"][2] > 0.0
    x = r["p0_mixed"][0]
    assert np.all(x[[0, 2]] > 0.0) and np.all(x > 0.0)
    x, T, mu = r["exact_cap_pinned"]
    assert x[0] == 1.0 and mu == 0.0
    assert r["sf_above_G"][0][0] < 4 / 8
    big = [k for k in mc.FIXED if len(mc.FIXED[k][0]) > 500]
    assert sorted(len(mc.FIXED[k][0]) for k in big) == [511, 512, 513, 1025, mc.LDS_JOBS, mc.LDS_JOBS + 1]
    # some of them are set by max p, some by the capacity row
    kinds = set()
    for k in big:
        sf, p, G = mc.FIXED[k]
        kinds.add(bool(p.max() * G >= float(np.dot(sf, p))))
    assert kinds == {True, False}


def test_twin_random_instances():
    rounds = 0
    for inst in mc.random_instances(200, seed=5, max_n=300):
        rounds += check(inst)[1] > 1e6
    assert 5 <= rounds <= 195  # both round 0 and the decade rounds are reached


def test_twin_matches_the_lp_search_through_highs():
    """The twin's T equals the T of the reference's search over the
    reference's LP (HiGHS) on 300 seeded instances; none is left out."""
    insts = mc.lp_instances()
    assert len(insts) == 300
    rejected = sum(not adm for *_, adm, _ in insts)
    closest = min(gap for *_, gap in insts)
    two = sum(len(w) == 2 for _, _, _, w, _, _, _ in insts)
    print(f"lp: {rejected} rejected, closest probe {closest:.3g} from T*, {two} on two types")
    assert rejected == 0
    assert two >= 100
    for tp, sf, steps, workers, p, _, _ in insts:
        _, T, _ = mtd_ref.twin_allocate(sf, p, sum(workers))
        Tl, _, _ = mtd_ref.lp_search(tp, sf, steps, workers)
        assert T == Tl, (T, Tl, len(sf), workers)


def test_twin_empty_and_deterministic():
    x, T, mu = mtd_ref.twin_allocate([], [], 8)
    assert len(x) == 0 and T == 0.0 and mu == 0.0
    for name in ("n513_G96", f"n{mc.LDS_JOBS + 1}_G8192", "p0_mixed"):
        inst = mc.FIXED[name]
        assert mc.same_bits(mtd_ref.twin_allocate(*inst), mtd_ref.twin_allocate(*inst))


def test_checker_rejects_a_wrong_T_and_a_shifted_x():
    inst = mc.FIXED["sf_above_G"]
    x, T, mu = mtd_ref.twin_allocate(*inst)
    mc.check_allocation(inst, x, T, mu)
    for wrong in (T * 1.05, T / 1.05, np.nextafter(T, np.inf)):
        with pytest.raises(AssertionError):
            mc.check_allocation(inst, x, wrong, mu)
    shifted = x.copy()
    shifted[1] += 1e-6
    with pytest.raises(AssertionError):
        mc.check_allocation(inst, shifted, T, mu)
    below = x.copy()
    below[0] = inst[1][0] / T * (1 - 1e-9)
    with pytest.raises(AssertionError):
        mc.check_allocation(inst, below, T, mu)
