"""Hierarchical (entity) water-filling allocation (sw_wfh_allocate): the CPU
twin of the HIP kernel against the reference's staged process in exact
rationals, its reductions to the flat water filling, and the stage loop
restated over HiGHS, with the two artefacts of the reference that DESIGN.md
§19 describes made executable."""
import numpy as np
import pytest

import wf_ref
import wfh_ref
import wfhcases as wc
from wfh_ref import FAIRNESS, FIFO


@pytest.mark.parametrize("name", sorted(wc.FIXED))
def test_fixed_list_against_the_exact_staged_process(name):
    inst = wc.FIXED[name]
    r = wfh_ref.twin_allocate(*inst)
    wc.check_properties(inst, *r)
    wc.check_against_fluid(inst, r[0])


def test_fixed_list_covers_what_it_names():
    F = wc.FIXED
    assert {len(v[0]) for v in F.values()} >= {1, 511, 512, 513, 2049}
    assert wc.total(F["sum_equals_G"]) == F["sum_equals_G"][5] == F["sum_is_G_plus_1"][5] + 1
    assert F["G1"][5] == 1 and F["sf255"][0].max() == 255
    assert not np.any(F["empty_entity"][2] == 1)
    sf, c, ent, W, _, _ = F["ties"]
    D = [int(sf[ent == e].sum()) for e in range(3)]
    assert c[0] == c[1] and ent[0] == ent[1] and D[0] / W[0] == D[1] / W[1]
    assert set(F["mixed"][4]) == {FAIRNESS, FIFO}


def test_random_instances_against_the_exact_staged_process():
    insts = wc.random_instances(200, seed=13)
    assert {len(set(i[4])) for i in insts} == {1, 2}
    for k, inst in enumerate(insts):
        r = wfh_ref.twin_allocate(*inst)
        wc.check_properties(inst, *r)
        wc.check_against_fluid(inst, r[0])


@pytest.mark.parametrize("lay", wc.LAYOUTS)
@pytest.mark.parametrize("kind", ["fairness", "fifo", "mixed"])
def test_large_instances_keep_the_properties(lay, kind):
    """Sizes at which the exact staged process would take minutes (up to one
    stage per job): the properties that need no reference."""
    rng = np.random.default_rng(wc.LAYOUTS.index(lay) * 7 + len(kind))
    for n in (511, 513, 2049):
        inst = wc.draw(rng, n, lay, kind, continuous=True)
        for G in (1, wc.total(inst) // 2, wc.total(inst) - 1, wc.total(inst), wc.total(inst) + 1):
            wc.check_properties(wc.with_G(inst, G), *wfh_ref.twin_allocate(*wc.with_G(inst, G)))


def test_empty_instance():
    x, g, level, used = wfh_ref.twin_allocate([], [], [], [1.0, 2.0], [0, 1], 4)
    assert len(x) == 0 and list(g) == [0.0, 0.0] and level == 0.0 and used == 0.0


# ---- reductions ----
def flat_instances():
    import wfcases

    return wfcases.random_instances(60, seed=19, max_n=700) + [wfcases.FIXED[k] for k in sorted(wfcases.FIXED)
                                                                if len(wfcases.FIXED[k][0]) <= 2049
                                                                and k != "spread"]


def close(a, b, rel=1e-12):
    return np.all(np.abs(a - b) <= rel * np.abs(b))


def test_one_fairness_entity_is_the_flat_water_filling():
    for sf, c, G in flat_instances():
        flat = wf_ref.twin_allocate(sf, c, G)[0]
        for W in (1.0, 0.3):
            x = wfh_ref.twin_allocate(sf, c, np.zeros(len(sf), dtype=np.int32), [W], [FAIRNESS], G)[0]
            assert close(x, flat), (len(sf), G)


def test_singleton_entities_with_the_jobs_weights_are_the_flat_water_filling():
    for sf, c, G in flat_instances():
        n = len(sf)
        flat = wf_ref.twin_allocate(sf, c, G)[0]
        for mode in (FAIRNESS, FIFO):
            x = wfh_ref.twin_allocate(sf, c, np.arange(n, dtype=np.int32), sf / c, np.full(n, mode, dtype=np.int32),
                                      G)[0]
            assert close(x, flat), (n, G, mode)


def test_a_common_power_of_two_on_the_entity_weights_changes_no_bit():
    for inst in wc.random_instances(60, seed=23) + [wc.FIXED["n513"], wc.FIXED["mixed"]]:
        sf, c, ent, W, modes, G = inst
        x, g, level, used = wfh_ref.twin_allocate(*inst)
        for k in (-20, -1, 3, 40):
            x2, g2, level2, used2 = wfh_ref.twin_allocate(sf, c, ent, W * 2.0 ** k, modes, G)
            assert x2.tobytes() == x.tobytes() and g2.tobytes() == g.tobytes() and used2 == used
            assert level2 == level * 2.0 ** -k


def test_relabelling_the_entities_moves_no_share_by_more_than_1e_12():
    rng = np.random.default_rng(3)
    for inst in wc.random_instances(60, seed=29) + [wc.FIXED["n512"]]:
        sf, c, ent, W, modes, G = inst
        x = wfh_ref.twin_allocate(*inst)[0]
        perm = rng.permutation(len(W))  # entity e becomes perm[e]
        W2, m2 = np.empty_like(W), np.empty_like(modes)
        W2[perm], m2[perm] = W, modes
        x2 = wfh_ref.twin_allocate(sf, c, perm[ent].astype(np.int32), W2, m2, G)[0]
        assert np.max(np.abs(x2 - x), initial=0.0) <= 1e-12


# ---- the reference's stage loop over HiGHS ----
def test_stage_loop_over_highs_agrees_on_fairness_entities():
    """60 all-fairness instances, the entity weights scaled by the power of two
    that makes every first-stage job weight ≥ 1 (see the artefact below).  No
    instance is left out; the worst difference from the twin here is 5.6e-16
    (2.2e-16 from the exact staged process), over up to 9 stages."""
    worst = 0.0
    for k, inst in enumerate(wc.stage_instances(60, seed=5)):
        x, stages, ok = wfh_ref.stage_loop(*inst, scale=wfh_ref.weight_scale(*inst[:5]))
        assert ok, k
        t = wfh_ref.twin_allocate(*inst)[0]
        worst = max(worst, float(np.max(np.abs(x - t))))
        assert np.max(np.abs(x - t)) <= 1e-6, (k, stages)
    print("worst |stage loop - twin|:", worst)


def test_artefact_the_big_M_of_the_stage_lp_is_not_big():
    """One fairness entity of weight 0.5 over ten jobs: the reweighted job
    weights are fractions of 0.5, sf_j/ω_j exceeds M = max sf = 8, the stage
    objective is capped by M once a job has frozen, and the loop stops far
    short of the staged process.  With the weights scaled by a power of two it
    reaches it."""
    sf = wc.i32(4, 1, 4, 4, 1, 1, 1, 8, 8, 4)
    w = wc.f64(3, 2, 2, 3, 1, 1, 2, 0.5, 1, 0.5)
    inst = (sf, (1.0 / w) * sf, np.zeros(10, dtype=np.int32), wc.f64(0.5), wc.i32(FAIRNESS), 18)
    ref = np.array([float(v) for v in wfh_ref.fluid(*inst)])
    raw, _, ok = wfh_ref.stage_loop(*inst, scale=1.0)
    assert ok and np.max(np.abs(raw - ref)) > 0.5
    scaled, _, ok = wfh_ref.stage_loop(*inst, scale=wfh_ref.weight_scale(*inst[:5]))
    assert ok and np.max(np.abs(scaled - ref)) <= 1e-6
    assert np.max(np.abs(wfh_ref.twin_allocate(*inst)[0] - ref)) <= 1e-12


def test_artefact_fifo_trips_the_bottleneck_milp():
    """A fifo entity's waiting jobs have so_far = 0 and z forced to 0, which
    makes the bottleneck MILP infeasible; the reference then freezes every
    weighted job after each stage.  Here that leaves job 0 (a fairness entity
    of its own) at 1/3 and hands the waiting job 4 a whole share, where the
    process that the reference's comments state gives job 0 a whole share and
    job 4, last in its fifo entity, none.  The kernel follows the comments."""
    sf = wc.i32(2, 1, 1, 1, 1)
    w = wc.f64(2, 2, 2, 2, 0.5)
    inst = (sf, (1.0 / w) * sf, wc.i32(0, 1, 1, 1, 1), wc.f64(2.0, 3.0), wc.i32(FAIRNESS, FIFO), 5)
    ref = [float(v) for v in wfh_ref.fluid(*inst)]
    assert ref == [1.0, 1.0, 1.0, 1.0, 0.0]
    x, _, ok = wfh_ref.stage_loop(*inst, scale=wfh_ref.weight_scale(*inst[:5]))
    assert ok and abs(x[0] - 1 / 3) <= 1e-6 and abs(x[4] - 1.0) <= 1e-6
    assert list(wfh_ref.twin_allocate(*inst)[0]) == ref
