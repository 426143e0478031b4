"""MinTotalDuration over worker types that differ (sw_mtd_allocate_types,
csrc/sw_mtd_types.h) without a GPU: the CPU twin of the kernel against an
independent computation (tests/mtd_types_ref.py: HiGHS, a Python replay of the
reference's search, a null-space Newton centre), the policy mirror over the
twin, and the bit record that holds the centred MaxMinFairness twin to what it
was before csrc/sw_mmf_ipm.h was generalised.

Measured with these seeds (twin vs reference): T equal on all 300 level
instances and all 105 centre instances, none excluded by the near-probe rule
(the nearest probe is further than 1e-5 relative from 1/t* everywhere); every
centre instance has a margin ≥ 1e-3 (the smallest 1.57e-3), none excluded; the
worst share error is 1.8e-10 (narrow) and 8.9e-11 (wide).
"""
import json
import os

import numpy as np
import pytest

import min_total_duration as mtd
import mmfccases
import mtd_ref
import mtd_types_ref as ref
import mtdtcases as tc

NEAR = 1e-5
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "mmfc_bits.json")


@pytest.mark.parametrize("family", tc.FAMILIES)
def test_level_fuzz_T_equals_the_replay_and_rows_hold(family):
    excluded = 0
    cases = tc.level_fuzz(family)
    assert len(cases) == 150
    for i, (W, sf, thr, steps) in enumerate(cases):
        x, T, t, its, flags = tc.twin_allocate(W, sf, thr, steps)
        tc.check_rows(W, sf, thr, steps, x, T)
        t_ref = ref.level(W, sf, thr, steps)
        T_ref, near = ref.replay(t_ref)
        if near < NEAR:
            excluded += 1
            continue
        assert T == T_ref, (family, i, T, T_ref, t, t_ref)
        assert abs(t - t_ref) <= 1e-5 * t_ref, (family, i, t, t_ref)
    print(f"{family}: {excluded} of {len(cases)} excluded by the near-probe rule")
    assert excluded == 0  # the committed seeds: none (at most 2 % would be allowed)


def test_centre_fuzz_shares_within_1e_6_of_the_reference():
    cases = tc.centre_fuzz()
    assert len(cases) == 105
    worst = {f: 0.0 for f in tc.FAMILIES}
    thin = near_probe = 0
    for i, (fam, inst, (xr, T_ref, t_ref, margin, near)) in enumerate(cases):
        x, T, t, its, flags = tc.twin_allocate(*inst)
        tc.check_rows(*inst, x, T)
        if near < NEAR:
            near_probe += 1
            continue
        assert T == T_ref, (i, T, T_ref)
        if margin < 1e-3:
            thin += 1
            continue
        assert flags == 0 or not (inst[3] > 0.0).any()
        worst[fam] = max(worst[fam], float(np.abs(x - xr).max()))
    print(f"centre: worst max|x - x_ref| {worst}, margin below 1e-3: {thin}, near a probe: {near_probe}")
    assert near_probe == 0 and thin == 0  # the committed seeds: none (at most 10 % would be allowed)
    assert max(worst.values()) <= 1e-6


def _one_type_instances():
    rng = np.random.default_rng(612)
    out = []
    for _ in range(40):
        m = int(rng.integers(1, 40))
        G = int(rng.integers(1, 3 * m + 3))
        sf = rng.choice([1, 2, 4, 8], size=m).astype(np.int32)
        thr = rng.uniform(0.2, 4.0, size=m)
        steps = 10.0 ** rng.uniform(4.0, 6.0, size=m)
        steps[rng.random(size=m) < 0.1] = 0.0
        out.append((G, sf, thr, steps))
    return out


def test_one_type_agrees_with_the_one_type_call():
    compared = 0
    for G, sf, thr, steps in _one_type_instances():
        x1, T1, mu = mtd_ref.twin_allocate(sf, steps / thr, G)
        x, T, t, _, flags = tc.twin_allocate([G], sf, thr[:, None], steps)
        _, near = ref.replay(ref.level([G], sf, thr[:, None], steps))
        if near < NEAR:
            continue
        assert float(T).hex() == float(T1).hex()
        if mu == 0.0 or flags & tc.const("flag_thin"):  # a single point, or the thin rule
            continue
        compared += 1
        assert np.abs(x[:, 0] - x1).max() <= 1e-6
    assert compared >= 30


def test_thin_case():
    W, sf, thr, steps = tc.thin_case()
    x, T, t, its, flags = tc.twin_allocate(W, sf, thr, steps)
    assert flags & tc.const("flag_thin")
    assert T == tc.FIRST_PROBE
    tc.check_rows(W, sf, thr, steps, x, T)
    assert tc.const("thin") == 1e-7


def test_search_ranges():
    last_midpoint, _ = ref.search(lambda T: True)
    assert 100.0 < last_midpoint < 105.0
    W, sf, thr, steps = tc.short_case()
    x, T, t, _, flags = tc.twin_allocate(W, sf, thr, steps)
    assert 1.0 / t < 100.0 and T == last_midpoint and T * t - 1.0 > 1.0 and flags == 0
    tc.check_rows(W, sf, thr, steps, x, T)
    W, sf, thr, steps = tc.all_dead_case()
    x, T, t, _, flags = tc.twin_allocate(W, sf, thr, steps)
    assert T == last_midpoint and t == 0.0 and flags == tc.const("flag_idle")
    tc.check_rows(W, sf, thr, steps, x, T)
    W, sf, thr, steps = tc.long_case()
    x, T, t, _, flags = tc.twin_allocate(W, sf, thr, steps)
    assert 1.0 / t > 1e6 and T > 1e6 and flags == 0
    assert T == ref.replay(ref.level(W, sf, thr, steps))[0]
    tc.check_rows(W, sf, thr, steps, x, T)


def test_all_dead_is_the_centre_of_the_plain_polytope():
    W, sf, thr, steps = tc.all_dead_case()
    x, T, _, _, _ = tc.twin_allocate(W, sf, thr, steps)
    assert np.abs(x - ref.centre(W, sf, thr, steps, T)).max() <= 1e-6


def test_a_type_without_workers_gets_exact_zeros():
    W, sf, thr, steps = tc.zero_worker_case()
    x, T, t, _, _ = tc.twin_allocate(W, sf, thr, steps)
    assert (x[:, 1] == 0.0).all() and (x[:, [0, 2]] > 0.0).any()
    tc.check_rows(W, sf, thr, steps, x, T)


def test_throughputs_times_a_power_of_two():
    """The normalisation is by powers of two, so 2^k on all throughputs moves
    nothing but the level's exponent.  The allocation is unchanged wherever T
    is: with the steps multiplied along (the same coefficients), and without a
    live job (T is the last midpoint).  With the steps kept, T moves with the
    level and the polytope at T is another one; there the level must scale bit
    for bit."""
    W, sf, thr, steps = tc.dead_among_live_case()
    base = tc.twin_allocate(W, sf, thr, steps)
    for k in (-7, 3, 40):
        got = tc.twin_allocate(W, sf, thr * 2.0 ** k, steps * 2.0 ** k)
        assert np.array_equal(got[0], base[0]) and got[1:] == base[1:]
        got = tc.twin_allocate(W, sf, thr * 2.0 ** k, steps)
        assert got[2] == base[2] * 2.0 ** k
    W, sf, thr, steps = tc.all_dead_case()
    base = tc.twin_allocate(W, sf, thr, steps)
    for k in (-7, 3, 40):
        got = tc.twin_allocate(W, sf, thr * 2.0 ** k, steps)
        assert np.array_equal(got[0], base[0]) and got[1:] == base[1:]


def _policy_args(thr, sf, steps, W, types):
    m = len(sf)
    tp = {j: {t: float(thr[j, k]) for k, t in enumerate(types)} for j in range(m)}
    return tp, {j: int(sf[j]) for j in range(m)}, {j: float(steps[j]) for j in range(m)}, \
        {t: int(W[k]) for k, t in enumerate(types)}


def test_policy_default_still_raises_and_names_the_flag():
    W, sf, thr, steps = tc.shaped(5, 3)
    pol = mtd.MinTotalDurationPolicyWithPerf(native=tc.TwinEngine())
    with pytest.raises(NotImplementedError, match="worker_types=True"):
        pol.get_allocation(*_policy_args(thr, sf, steps, W, ["k80", "p100", "v100"]))


def test_policy_over_types_meets_every_row():
    W, sf, thr, steps = tc.dead_among_live_case()
    steps = steps.copy()
    steps[5] = -3.0  # a remainder below zero is taken as zero
    types = ["k80", "p100", "v100"]
    eng = tc.TwinEngine()
    pol = mtd.MinTotalDurationPolicyWithPerf(native=eng, worker_types=True)
    alloc = pol.get_allocation(*_policy_args(thr, sf, steps, W, types))
    assert eng.calls == ["mtd_allocate_types"]
    x = np.array([[alloc[j][t] for t in types] for j in range(len(sf))])
    assert ((x >= 0.0) & (x <= 1.0)).all()
    T, t, flags = pol.last_level
    tc.check_rows(W, sf, thr, np.maximum(steps, 0.0), x, T)
    xt, Tt, tt, _, ft = tc.twin_allocate(W, sf, thr, np.maximum(steps, 0.0))
    assert (T, t, flags) == (Tt, tt, ft) and np.array_equal(x, xt.clip(min=0.0).clip(max=1.0))


def test_policy_identical_throughputs_give_the_default_result():
    sf = np.array([1, 2, 4, 1, 2], dtype=np.int32)
    types = ["a", "b", "c"]
    thr = np.repeat(np.array([3.0, 4.0, 5.0, 6.0, 7.0])[:, None], 3, axis=1)
    args = _policy_args(thr, sf, np.full(5, 3e5), [2, 3, 5], types)
    e0, e1 = tc.TwinEngine(), tc.TwinEngine()
    a0 = mtd.MinTotalDurationPolicyWithPerf(native=e0).get_allocation(*args)
    p1 = mtd.MinTotalDurationPolicyWithPerf(native=e1, worker_types=True)
    a1 = p1.get_allocation(*args)
    assert a0 == a1 and e0.calls == e1.calls == ["mtd_allocate"] and len(p1.last_level) == 2


def test_policy_zero_throughput_live_job_raises():
    W, sf, thr, steps = tc.shaped(5, 3)
    thr = thr.copy()
    thr[3, :] = 0.0
    pol = mtd.MinTotalDurationPolicyWithPerf(native=tc.TwinEngine(), worker_types=True)
    with pytest.raises(ValueError, match="job 3"):
        pol.get_allocation(*_policy_args(thr, sf, steps, W, ["k80", "p100", "v100"]))
    # positive only on a type without workers: the same
    thr[3, 1] = 2.0
    W = np.array([W[0], 0, W[2]], dtype=np.int32)
    with pytest.raises(ValueError, match="job 3"):
        pol.get_allocation(*_policy_args(thr, sf, steps, W, ["k80", "p100", "v100"]))


def test_centred_mmf_twin_is_bit_for_bit_the_record():
    """tests/golden/mmfc_bits.json (tools/mmfc_bits_record.py) was written from
    the twin before csrc/sw_mmf_ipm.h learnt the per-row κ and residual scale."""
    with open(GOLDEN) as f:
        gold = json.load(f)
    shapes = [(1, 1), (1, 3), (2, 2), (5, 3), (33, 8), (40, 16), (513, 2), (1100, 3)]
    names = [f"{m}x{n}" for m, n in shapes] + ["zero_worker", "level_zero"]
    assert sorted(gold) == sorted(names)
    for name in names:
        inst = (mmfccases.zero_worker_case() if name == "zero_worker" else mmfccases.level_zero_case()
                if name == "level_zero" else mmfccases.shaped(*map(int, name.split("x"))))
        x, t, its = mmfccases.twin_allocate(*inst)
        bits = "".join(f"{int(b):016x}" for b in np.ascontiguousarray(x).view(np.uint64).ravel())
        assert its == gold[name]["steps"], name
        assert float(t).hex() == gold[name]["level"], name
        assert bits == gold[name]["x"], name
