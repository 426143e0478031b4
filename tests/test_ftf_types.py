"""FinishTimeFairness over worker types that differ (sw_ftf_allocate_types,
csrc/sw_ftf_types.h) without a GPU: the CPU twin of the kernel against an
independent computation (tests/ftf_types_ref.py: a bracketing search over ρ on
HiGHS's level, a null-space Newton centre), against the one-type twin and the
centred MaxMinFairness twin.

Bars.  ρ: RHO_BAR relative, a decade above the worst gap measured on the two
families (the docstring of test_level_fuzz_rho_and_rows), no looser than 1e-6.  Shares: 1e-6.  Rows: 1e-9.

The figures measured with these seeds (twin vs reference) are in the tests'
docstrings; each test prints its own.
"""
import numpy as np
import pytest

import ftf_ref
import ftf_types_ref as ref
import ftftcases as tc
import mmfccases
import mtd_types_ref

RHO_BAR = 1e-6
SHARE_BAR = 1e-6


@pytest.mark.parametrize("family", tc.FAMILIES)
def test_level_fuzz_rho_and_rows(family):
    """Measured at the built tolerance: the worst relative gap of ρ is 8.9e-8
    (narrow) and 7.5e-8 (wide), so RHO_BAR = 1e-6; the engine's level at the
    probed ρ is within 2.0e-9 (narrow) and 7.7e-9 (wide) of HiGHS's on the same
    rows, so SW_FTFT_TOL = 1e-7; 1–5 level solves on both, 15–114 and 15–96
    Newton steps; SW_FTFT_SAFE on none, capacity binds on 63 and 77 of 150."""
    cases, refs = tc.level_fuzz(family), tc.level_refs(family)
    assert len(cases) == 150
    gap = lvl = 0.0
    solves, steps, safe, binds = [], [], 0, 0
    for i, (inst, (rho_ref, box_ref)) in enumerate(zip(cases, refs)):
        x, rho, t, its, sol, flags = tc.twin_allocate(*inst)
        tc.check_rows(*inst, x, rho)
        gap = max(gap, abs(rho - rho_ref) / rho_ref)
        if (inst[3] > 0.0).any():
            probed = rho * t if t < 1.0 - 1e-12 else rho  # the call returns the probed level divided by t < 1
            lvl = max(lvl, abs(t - ref.level_at(*inst, probed)) / t)
            assert t >= 1.0 - tc.const("tol")
        solves.append(sol)
        steps.append(its)
        safe += bool(flags & tc.const("flag_safe"))
        binds += not flags & (tc.const("flag_box") | tc.const("flag_idle"))
        assert sol <= tc.const("max_solves") // 4, (family, i, sol)
    print(f"{family}: worst rho gap {gap:.2e}, worst level gap at the returned rho {lvl:.2e}, solves "
          f"{min(solves)}-{max(solves)}, Newton steps {min(steps)}-{max(steps)} (median {int(np.median(steps))}), "
          f"SAFE on {safe}, capacity binds on {binds}")
    assert gap <= RHO_BAR <= 1e-6
    assert 10.0 * lvl <= tc.const("tol")


def test_centre_fuzz_shares_within_1e_6_of_the_reference():
    """Measured: 0 of 60 instances left out; the worst share error is 7.5e-8
    (narrow) and 1.0e-8 (wide)."""
    cases = tc.centre_fuzz()
    assert len(cases) == 60
    worst = {f: 0.0 for f in tc.FAMILIES}
    for i, (fam, inst) in enumerate(cases):
        xr, rho_ref, box_ref = tc.centre_ref(i)
        x, rho, t, its, sol, flags = tc.twin_allocate(*inst)
        tc.check_rows(*inst, x, rho)
        assert abs(rho - rho_ref) <= RHO_BAR * rho_ref, (i, rho, rho_ref)
        worst[fam] = max(worst[fam], float(np.abs(x - xr).max()))
    print(f"centre: worst max|x - x_ref| {worst}; 0 of {len(cases)} left out")
    assert max(worst.values()) <= SHARE_BAR


def _one_type_instances():
    rng = np.random.default_rng(733)
    out = []
    for _ in range(40):
        m = int(rng.integers(1, 40))
        G = int(rng.integers(m // 2 + 1, 3 * m + 3))
        sf = rng.choice([1, 2, 4, 8], size=m).astype(np.int32)
        thr = rng.uniform(0.2, 4.0, size=(m, 1)) * sf[:, None]
        steps = 10.0 ** rng.uniform(4.0, 6.0, size=m)
        steps[rng.random(size=m) < 0.1] = 0.0
        left, a, E = tc.history(rng, [G], sf, thr, steps)
        out.append(([G], sf, thr, left, a, E))
    return out


def test_one_type_agrees_with_the_one_type_call():
    """Measured: ρ equal on 40 of 40; shares compared on 34 (the others are
    single points: capacity binds, the one-type call returns μ = 0), worst
    1.5e-10."""
    compared, gap, worst = 0, 0.0, 0.0
    for W, sf, thr, left, a, E in _one_type_instances():
        x1, rho1, mu = ftf_ref.twin_allocate(sf, left / thr[:, 0], a, E, W[0])
        x, rho, t, _, sol, flags = tc.twin_allocate(W, sf, thr, left, a, E)
        gap = max(gap, abs(rho - rho1) / rho1)
        assert abs(rho - rho1) <= RHO_BAR * rho1
        assert sol == 1  # the aggregate start is the one-type program itself
        if mu == 0.0:  # a single point
            continue
        compared += 1
        worst = max(worst, float(np.abs(x[:, 0] - x1).max()))
    print(f"one type: worst rho gap {gap:.2e}, shares compared on {compared} of 40, worst {worst:.2e}")
    assert compared >= 30
    assert worst <= SHARE_BAR


def test_no_elapsed_time_is_the_centred_max_min_fairness_program():
    """Every a_j = 0: c(ρ) = ρ·thr·E/s, so ρ* = 1/t*(thr·E/s), reached in at
    most two solves, at the same shares.  Measured on 40 instances: |ρ·t* − 1|
    ≤ 3.5e-8, shares within 2.4e-9; 1–2 solves."""
    rng = np.random.default_rng(744)
    gap = worst = 0.0
    solves = set()
    for i in range(40):
        W, sf, thr, steps = tc.mt.draw(rng, i, 30, 5, "narrow")
        W = (W + 7) // 8
        steps = np.where(steps > 0.0, steps, 1e5)
        E = steps / tc.isolated(W, sf, thr) * rng.uniform(0.5, 2.0, size=len(sf))
        x, rho, t, _, sol, flags = tc.twin_allocate(W, sf, thr, steps, np.zeros(len(sf)), E)
        xc, tstar, _ = mmfccases.twin_allocate(W, sf, thr * (E / steps)[:, None])
        solves.add(sol)
        assert sol <= 2
        gap = max(gap, abs(rho * tstar - 1.0))
        if flags & tc.const("flag_box") and tstar * rho > 1.0 + 1e-6:
            continue  # never with a = 0: ρ_box is then a live job's
        worst = max(worst, float(np.abs(x - xc).max()))
    print(f"no elapsed time: worst |rho t* - 1| {gap:.2e}, worst share gap {worst:.2e}, solves {sorted(solves)}")
    assert gap <= RHO_BAR
    assert worst <= SHARE_BAR


def _named(name):
    inst = tc.NAMED[name]()
    return inst, tc.twin_allocate(*inst)


def test_named_box():
    inst, (x, rho, t, _, sol, flags) = _named("box")
    assert flags == tc.const("flag_box") and sol == 1
    assert rho == ref.rho_box(inst[0], *inst[2:])
    tc.check_rows(*inst, x, rho)
    assert np.abs(x - ref.centre(*inst, rho)).max() <= SHARE_BAR


def test_named_all_dead_is_the_centre_of_the_plain_polytope():
    inst, (x, rho, t, _, sol, flags) = _named("all_dead")
    assert flags == tc.const("flag_idle") and t == 0.0 and sol == 1
    assert rho == float((inst[4] / inst[5]).max())
    tc.check_rows(*inst, x, rho)
    assert np.abs(x - mtd_types_ref.centre(inst[0], inst[1], inst[2], inst[3], 1.0)).max() <= SHARE_BAR


def test_named_dead_among_live_and_a_dead_job_that_sets_the_level():
    inst, (x, rho, t, _, sol, flags) = _named("dead_among_live")
    tc.check_rows(*inst, x, rho)
    xr, rho_ref, _ = ref.allocate(*inst)
    assert abs(rho - rho_ref) <= RHO_BAR * rho_ref and np.abs(x - xr).max() <= SHARE_BAR
    # a dead job's ratio above every live one's: ρ* is that ratio, the live rows have room
    W, sf, thr, left, a, E = inst
    a = a.copy()
    a[2] = 3.0 * E[2]
    x, rho, t, _, sol, flags = tc.twin_allocate(W, sf, thr, left, a, E)
    assert rho == 3.0 and flags == tc.const("flag_box") and t > 1.0 + 1e-3 and sol == 1
    tc.check_rows(W, sf, thr, left, a, E, x, rho)
    assert np.abs(x - ref.centre(W, sf, thr, left, a, E, rho)).max() <= SHARE_BAR


def test_named_zero_worker_gets_exact_zeros():
    inst, (x, rho, t, _, sol, flags) = _named("zero_worker")
    assert (x[:, 1] == 0.0).all() and (x[:, [0, 2]] > 0.0).any()
    tc.check_rows(*inst, x, rho)
    xr, rho_ref, _ = ref.allocate(*inst)
    assert abs(rho - rho_ref) <= RHO_BAR * rho_ref and np.abs(x - xr).max() <= SHARE_BAR


def test_named_tight():
    inst, (x, rho, t, _, sol, flags) = _named("tight")
    assert rho > 10.0 * ref.rho_box(inst[0], *inst[2:]) and not flags & tc.const("flag_box")
    tc.check_rows(*inst, x, rho)
    assert abs(ref.level_at(*inst, rho) - 1.0) <= 2.0 * tc.const("tol")  # the stop's tolerance and the level's own error


def test_named_no_elapsed_takes_two_solves():
    inst, (x, rho, t, _, sol, flags) = _named("no_elapsed")
    assert sol == 2 and flags == 0
    tc.check_rows(*inst, x, rho)


def test_constants():
    assert tc.const("tol") == 1e-7 and tc.const("max_solves") == 32
    assert (tc.const("flag_box"), tc.const("flag_idle"), tc.const("flag_safe")) == (1, 2, 4)
