"""FinishTimeFairness allocation (Gavel / Themis baseline, sw_ftf_allocate):
the CPU twin of the HIP kernel (tests/twins/ftf_twin.c) against an exact
rational certificate of its level, the optimality conditions of its
allocation, and scipy's SLSQP on the reference's program as written
(policies/finish_time_fairness.py:55-140).  The HIP kernel against the twin,
bit for bit: tests/test_gpu_ftf.py."""
import numpy as np
import pytest

import ftf_ref
import ftfcases as fc


def check(inst):
    sf, p, a, E, G = inst
    x, rho, mu = ftf_ref.twin_allocate(sf, p, a, E, G)
    assert ftf_ref.certified(sf, p, a, E, G, rho, 1e-9), rho
    fc.check_allocation(inst, x, rho, mu)
    return x, rho, mu


@pytest.mark.parametrize("name", sorted(fc.FIXED))
def test_twin_level_certified_and_allocation_optimal(name):
    check(fc.FIXED[name])


def test_fixed_list_covers_both_cases_and_their_edges():
    r = {k: ftf_ref.twin_allocate(*v) for k, v in fc.FIXED.items()}
    assert r["n1"][2] > 0.0 and r["n1_binds"][2] == 0.0
    assert r["p0_binds"][2] == 0.0 and r["p0_binds"][0][0] == 0.0
    assert r["p0_free"][2] > 0.0 and 0.0 < r["p0_free"][0][0] < 1.0
    # a finished job sets the level: ρ* = a/E of that job, and capacity is free
    assert r["p0_is_box"][1] == 9e3 / 3e3 and r["p0_is_box"][2] > 0.0
    # the jobs that tie at ρ_box are pinned, the others are not
    x = r["tie_at_box"][0]
    assert np.all(x[:3] == 1.0) and np.all(x[3:] < 1.0) and r["tie_at_box"][1] == 1000.0 / 800.0
    # cap(ρ_box) = G exactly: the face is the single point x = 1
    x, rho, mu = r["cap_equals_G"]
    assert np.all(x == 1.0) and rho == 1.0 and mu == 0.0
    big = [k for k in fc.FIXED if k.startswith("n") and k[1:2].isdigit() and len(fc.FIXED[k][0]) > 500]
    assert len(big) == 6
    assert {r[k][2] == 0.0 for k in big} == {True, False}  # some bind, some do not


def test_twin_random_instances():
    binds = 0
    for inst in fc.random_instances(200, seed=5, max_n=300):
        binds += check(inst)[2] == 0.0
    assert 20 <= binds <= 180


@pytest.mark.filterwarnings("ignore:Values in x were outside bounds")
def test_level_matches_slsqp_on_the_reference_program():
    """|ρ_slsqp − ρ*| ≤ 1e-9·ρ* on 60 seeded instances; the ones where scipy
    reports failure are left out, at most 10 % of them."""
    insts = fc.slsqp_instances()
    failed, binds, worst = 0, 0, 0.0
    for sf, p, a, E, G in insts:
        _, rho, mu = ftf_ref.twin_allocate(sf, p, a, E, G)
        binds += mu == 0.0
        r, ok = ftf_ref.slsqp_level(sf, p, a, E, G)
        if not ok:
            failed += 1
            continue
        worst = max(worst, abs(r - rho) / rho)
        assert abs(r - rho) <= 1e-9 * rho, (r, rho, len(sf), G)
    print(f"slsqp: {failed} of {len(insts)} failed, {binds} bind, worst relative difference {worst:.3g}")
    assert failed <= len(insts) // 10
    assert binds >= 10 and len(insts) - binds >= 10


def test_twin_empty_and_deterministic():
    x, rho, mu = ftf_ref.twin_allocate([], [], [], [], 8)
    assert len(x) == 0 and rho == 0.0 and mu == 0.0
    for name in ("n513_G96", "n2500_G256", "p0_free"):
        inst = fc.FIXED[name]
        assert fc.same_bits(ftf_ref.twin_allocate(*inst), ftf_ref.twin_allocate(*inst))


def test_certificate_rejects_a_wrong_level():
    sf, p, a, E, G = inst = fc.FIXED["no_unit_width"]
    _, rho, _ = ftf_ref.twin_allocate(*inst)
    assert ftf_ref.certified(sf, p, a, E, G, rho, 1e-9)
    assert not ftf_ref.certified(sf, p, a, E, G, rho * (1 + 1e-6), 1e-9)
    assert not ftf_ref.certified(sf, p, a, E, G, rho * (1 - 1e-6), 1e-9)
