"""Water-filling MaxMinFairness over worker types that differ
(sw_wf_allocate_types, csrc/sw_wf_types.h) without a GPU: the CPU twin of the
kernel against an independent computation (tests/wf_types_ref.py: the stage
loop on HiGHS, one LP per unfrozen job for the bottleneck test, a null-space
Newton centre), against the one-type twin and the centred MaxMinFairness twin.

Bars.  Levels: LEVEL_BAR = 1e-6 relative, the issue's cap (the docstring of
test_fuzz_levels_stages_and_frozen_sets says why it is the cap).  Shares: 1e-6.  Rows: 1e-9.

The figures measured with these seeds (twin vs reference) are in the tests'
docstrings; each test prints its own.
"""
import numpy as np
import pytest

import mmfccases
import wf_ref
import wf_types_ref as ref
import wftcases as tc

LEVEL_BAR = 1e-6
SHARE_BAR = 1e-6


@pytest.mark.parametrize("seed", list(tc.SEEDS))
def test_the_reference_leaves_out_at_most_two_percent(seed):
    """Measured: seed 6100: 0 of 300 instances ambiguous (0 of 8,827 job tests),
    smallest relative gain of a free job 1.35e-3, 1–9 stages, mean 2.5; seed 11:
    0 of 150, smallest gain 3.7e-3, 1–7 stages, mean 2.45."""
    refs = tc.fuzz_refs(seed)
    assert len(refs) == tc.SEEDS[seed]
    out = sum(r[0] is None for r in refs)
    stages = [r[2] for r in refs if r[0] is not None]
    print(f"reference, seed {seed}: {out} of {len(refs)} instances ambiguous ({sum(r[3] for r in refs)} of "
          f"{sum(r[4] for r in refs)} job tests), smallest free gain {min(r[5] for r in refs):.3e}, stages "
          f"{min(stages)}-{max(stages)} (mean {np.mean(stages):.2f})")
    assert out <= tc.AMBIGUOUS_CAP * len(refs)


@pytest.mark.parametrize("seed", list(tc.SEEDS))
def test_fuzz_levels_stages_and_frozen_sets(seed):
    """Seed 6100 is one of the eight on which SW_WFT_THRESH, SW_WFT_EASE and the
    retry were chosen; seed 11 took no part in any of it.  No call may be
    refused on either.  Measured: the same jobs freeze in the same stages on 300
    of 300 and 150 of 150; worst relative gap of a level 4.8e-8 and 3.5e-7; the
    statistic of a bottleneck at most 6.3e-9 and 3.7e-9, of a free job at least
    2.9e3 and 1.3e5 (the ends over the eight seeds, 4.32e-5 and 0.119, are
    SW_WFT_GAP_LO / _HI; the threshold is 2.3e-3); SW_WFT_NEAR on none, a
    retried stage (SW_WFT_COARSE) on 3 and on 2.
      The bar.  The issue asks for a decade above the worst measured and not
    above 1e-6.  The worst over 1,950 instances of seven seeds is 8.6e-7
    (test_named_hard_level), so the cap binds: LEVEL_BAR = 1e-6, and it is not a
    decade above the worst, only above all but three instances."""
    cases, refs = tc.fuzz(seed), tc.fuzz_refs(seed)
    gap, lo, hi, steps, near, coarse, done = 0.0, 0.0, np.inf, [], 0, 0, 0
    for i, (inst, r) in enumerate(zip(cases, refs)):
        if r[0] is None:
            continue
        F_ref, froze_ref, stages_ref = r[:3]
        x, F, level, its, stages, flags, froze, rc, st = tc.twin_allocate_rc(*inst, stats=True)
        assert rc == 0, (i, rc)
        assert stages == stages_ref, (i, stages, stages_ref)
        assert (froze == froze_ref).all(), (i, froze, froze_ref)
        assert level == F[froze == stages][0]
        tc.check_rows(*inst, x, F)
        gap = max(gap, float((np.abs(F - F_ref) / F_ref).max()))
        for s in range(stages):
            live = st[s] >= 0.0
            lo = max(lo, float(st[s][live & (froze_ref == s + 1)].max()))
            if (live & (froze_ref > s + 1)).any():
                hi = min(hi, float(st[s][live & (froze_ref > s + 1)].min()))
        steps.append(its)
        near += bool(flags & tc.const("flag_near"))
        coarse += bool(flags & tc.const("flag_coarse"))
        done += 1
    print(f"fuzz, seed {seed}: {done} instances, worst level gap {gap:.2e}, statistic of a bottleneck <= {lo:.3e}, "
          f"of a free job >= {hi:.3e}, Newton steps {min(steps)}-{max(steps)} (median {int(np.median(steps))}), "
          f"NEAR on {near}, COARSE on {coarse}")
    assert done >= (1.0 - tc.AMBIGUOUS_CAP) * len(cases)
    assert gap <= LEVEL_BAR <= 1e-6
    assert lo <= tc.const("gap_lo") < tc.const("thresh") < tc.const("gap_hi") <= hi
    assert abs(tc.const("thresh") / np.sqrt(tc.const("gap_lo") * tc.const("gap_hi")) - 1.0) < 0.01


def test_named_hard_level():
    """The largest level error met: 8.6e-7 (3.5e-6 at an ease of 2^-27: the
    ease, amplified 470 times, where the lift's dual is not unique)."""
    inst = tc.hard_level_case()
    F_ref, froze_ref, stages_ref, *_ = ref.allocate(*inst)
    x, F, level, its, stages, flags, froze = tc.twin_allocate(*inst)
    tc.check_rows(*inst, x, F)
    gap = float((np.abs(F - F_ref) / F_ref).max())
    print(f"hard level: gap {gap:.2e}")
    assert stages == stages_ref and (froze == froze_ref).all() and gap <= LEVEL_BAR


def _small():
    return [i for i, inst in enumerate(tc.fuzz()) if inst[2].size <= 40 and tc.fuzz_refs()[i][0] is not None][:40]


def test_shares_within_1e_6_of_the_centre_of_the_last_face():
    """The instances with m·n ≤ 40 (the first 40 of them)."""
    worst = 0.0
    picked = _small()
    assert len(picked) == 40
    for i in picked:
        inst, r = tc.fuzz()[i], tc.fuzz_refs()[i]
        x = tc.twin_allocate(*inst)[0]
        xr = ref.centre(*inst, r[0], r[1])
        worst = max(worst, float(np.abs(x - xr).max()))
    print(f"centre: worst max|x - x_ref| {worst:.2e} on {len(picked)} instances")
    assert worst <= SHARE_BAR


def test_identical_types_reduce_to_the_one_type_call():
    """Σ_k x_jk = min(1, L*/c_j) of sw_wf_allocate on Σ workers, on every one of
    25 instances (m 2…12, n 2…4, 1–4 stages).  One of them is solved with a
    retry (SW_WFT_COARSE): with identical types and capacity tight the reduced
    system came out exactly singular at the second path point of a late
    stage."""
    rng = np.random.default_rng(6170)
    worst, coarse = 0.0, 0
    for _ in range(25):
        m, n = int(rng.integers(2, 13)), int(rng.integers(2, 5))
        W = rng.integers(1, 5, size=n).astype(np.int32)
        sf = rng.choice([1, 2, 4], size=m).astype(np.int32)
        mult = (1.0 / rng.choice([0.5, 1.0, 2.0, 4.0], size=m)) * sf
        x1, level, used = wf_ref.twin_allocate(sf, mult, int(W.sum()))
        x, F, _, _, _, flags, _ = tc.twin_allocate(W, sf, np.tile(mult[:, None], (1, n)))
        tc.check_rows(W, sf, np.tile(mult[:, None], (1, n)), x, F)
        worst = max(worst, float(np.abs(x.sum(axis=1) - np.asarray(x1)).max()))
        coarse += bool(flags & tc.const("flag_coarse"))
    print(f"identical types: worst |sum_k x - x_one_type| {worst:.2e}, retried {coarse} of 25")
    assert worst <= LEVEL_BAR


def test_one_stage_is_the_centred_call_bit_for_bit():
    inst = tc.one_stage_case()
    x, F, level, its, stages, flags, froze = tc.twin_allocate(*inst)
    xc, tstar, itc = mmfccases.twin_allocate(*inst)
    assert stages == 1 and flags & tc.const("flag_one") and (froze == 1).all()
    assert np.array_equal(x.view(np.uint64), xc.view(np.uint64))
    assert its == itc and (F == level).all() and abs(level - tstar) <= 1e-8 * tstar


def test_named_zero_worker_gets_exact_zeros():
    inst = tc.zero_worker_case()
    x, F, *_ = tc.twin_allocate(*inst)
    assert (x[:, [1, 3]] == 0.0).all() and (x[:, [0, 2]] > 0.0).any()
    tc.check_rows(*inst, x, F)
    F_ref, froze_ref, *_ = ref.allocate(*inst)
    assert (np.abs(F - F_ref) <= LEVEL_BAR * F_ref).all()


def test_named_all_capped_ends_every_job_at_a_full_share():
    inst = tc.all_capped_case()
    x, F, level, its, stages, flags, froze = tc.twin_allocate(*inst)
    tc.check_rows(*inst, x, F)
    assert np.abs(x.sum(axis=1) - 1.0).max() <= SHARE_BAR
    assert (np.abs(F - inst[2].max(axis=1)) <= LEVEL_BAR * F).all()
    assert stages == len(set(np.round(inst[2].max(axis=1), 9)))


def test_named_last_job_alone():
    inst = tc.last_job_alone_case()
    x, F, level, its, stages, flags, froze = tc.twin_allocate(*inst)
    tc.check_rows(*inst, x, F)
    assert stages == 2 and (froze == [1, 1, 1, 1, 1, 2]).all()
    assert abs(F[5] - 1.0) <= LEVEL_BAR and abs(x[5, 2] - 1.0) <= SHARE_BAR


def test_named_many_stages():
    inst = tc.many_stages_case()
    x, F, level, its, stages, flags, froze = tc.twin_allocate(*inst)
    assert stages >= 8 and sorted(set(froze)) == list(range(1, stages + 1))
    assert (np.diff([F[froze == s][0] for s in range(1, stages + 1)]) > 0.0).all()


def test_constants():
    assert (tc.const("flag_one"), tc.const("flag_near"), tc.const("flag_coarse"), tc.const("status_stall")) == (1, 2, 4, -6)
    assert tc.const("thresh") == 2.3e-3 and tc.const("max_types") == 16 and tc.const("max_jobs") == 16384
