"""Shared inputs and checks of the hierarchical water-filling tests
(test_wfh.py, test_wfh_policy.py, test_gpu_wfh.py).  An instance is
(sf, c, ent, W, modes, G) as in wfh_ref."""
import math
from fractions import Fraction

import numpy as np

import wfh_ref
from wfh_ref import FAIRNESS, FIFO

SF_VALUES, SF_WEIGHTS = [1, 2, 4, 8], [0.6, 0.3, 0.09, 0.01]  # the traces' scale-factor mix
PRIORITY_WEIGHTS = [0.5, 1.0, 2.0, 3.0]
DYADIC_WEIGHTS = [0.5, 1.0, 2.0, 4.0]

i32 = lambda *v: np.array(v, dtype=np.int32)
f64 = lambda *v: np.array(v, dtype=np.float64)


def total(inst):
    return int(np.sum(inst[0], dtype=np.int64))


def with_G(inst, G):
    return inst[:5] + (int(G),)


def modes_of(kind, E, rng):
    if kind == "fairness":
        return np.zeros(E, dtype=np.int32)
    if kind == "fifo":
        return np.ones(E, dtype=np.int32)
    m = rng.integers(0, 2, size=E).astype(np.int32)  # mixed: both modes present when E > 1
    if E > 1:
        m[0], m[1] = FAIRNESS, FIFO
    return m


def layout(name, n, rng):
    """The entity of every job and the number of entities."""
    if name == "one":
        return np.zeros(n, dtype=np.int32), 1
    if name == "singletons":
        return rng.permutation(n).astype(np.int32), n
    if name == "one_and_rest":  # {1 job, N − 1 jobs}
        ent = np.ones(n, dtype=np.int32)
        ent[int(rng.integers(0, n))] = 0
        return ent, 2
    if name == "thirds":  # ≈ N/3 entities, random membership
        E = max(1, n // 3)
        return rng.integers(0, E, size=n).astype(np.int32), E
    if name == "empty":  # entity 1 of 4 has no job
        return rng.choice([0, 2, 3], size=n).astype(np.int32), 4
    raise KeyError(name)


LAYOUTS = ("one", "singletons", "one_and_rest", "thirds", "empty")


def draw(rng, n, lay, kind, G=None, dyadic=False, continuous=False):
    sf = rng.choice(SF_VALUES, size=n, p=SF_WEIGHTS).astype(np.int32)
    if continuous:
        w = 2.0 ** rng.uniform(-2, 2, size=n)
    else:
        w = rng.choice(DYADIC_WEIGHTS if dyadic else PRIORITY_WEIGHTS, size=n)
    ent, E = layout(lay, n, rng)
    W = rng.choice([0.5, 1.0, 2.0, 4.0], size=E) if dyadic else rng.choice([0.5, 1.0, 1.5, 2.0, 3.0, 5.0], size=E)
    modes = modes_of(kind, E, rng)
    if G is None:
        G = int(rng.integers(1, int(sf.sum()) + 4))
    return sf, (1.0 / w) * sf, ent, W.astype(np.float64), modes, int(G)


def big(rng, n, G_frac):
    """A large instance whose staged process has few stages, so that the exact
    reference stays quick: six entities, dyadic weights (few distinct
    coefficients: jobs that tie saturate in one stage), the two fifo entities
    of at most 12 jobs."""
    sf = rng.choice(SF_VALUES, size=n, p=SF_WEIGHTS).astype(np.int32)
    w = rng.choice(DYADIC_WEIGHTS, size=n)
    ent = rng.integers(0, 4, size=n).astype(np.int32)
    small = rng.choice(n, size=min(n, 20), replace=False)
    ent[small[:12]] = 4
    ent[small[12:]] = 5
    W = f64(1.0, 2.0, 0.5, 4.0, 0.25, 1.0)
    modes = i32(FAIRNESS, FAIRNESS, FAIRNESS, FAIRNESS, FIFO, FIFO)
    return sf, (1.0 / w) * sf, ent, W, modes, max(1, int(G_frac * int(sf.sum())))


def fixed_instances():
    rng = np.random.default_rng(41)
    F, Q = FAIRNESS, FIFO
    base = (i32(1, 2, 4, 1, 2, 8), f64(1.0, 4.0, 2.0, 1 / 3, 2.0, 16.0), i32(0, 1, 0, 1, 2, 2), f64(1.0, 2.0, 0.5),
            i32(F, Q, F))
    out = {
        "n1": (i32(2), f64(2.0), i32(0), f64(1.0), i32(F), 4),
        "n1_binds": (i32(4), f64(4.0), i32(0), f64(3.0), i32(F), 2),
        "n1_fifo_binds": (i32(4), f64(4.0), i32(0), f64(3.0), i32(Q), 3),
        "one_entity": (i32(1, 2, 4, 8, 1), f64(2.0, 1.0, 4.0, 8 / 3, 0.5), np.zeros(5, dtype=np.int32), f64(2.0),
                       i32(F), 9),
        "one_entity_fifo": (i32(1, 2, 4, 8, 1), f64(2.0, 1.0, 4.0, 8 / 3, 0.5), np.zeros(5, dtype=np.int32),
                            f64(2.0), i32(Q), 9),
        "singletons": (i32(1, 2, 4, 8), f64(1.0, 2.0, 4.0, 8.0), i32(3, 0, 2, 1), f64(1.0, 3.0, 0.5, 2.0),
                       i32(F, Q, F, Q), 6),
        "empty_entity": (i32(1, 2, 4, 1), f64(1.0, 4.0, 2.0, 1 / 3), i32(0, 2, 2, 0), f64(1.0, 7.0, 2.0),
                         i32(F, Q, F), 5),
        "weights_1e-6_and_1e6": (i32(2, 2, 4, 1), f64(2.0, 1.0, 4.0, 1.0), i32(0, 0, 1, 1), f64(1e-6, 1e6),
                                 i32(F, F), 6),
        "sum_equals_G": base + (18,),
        "sum_is_G_plus_1": base + (17,),
        "G1": base + (1,),
        "sf255": (i32(255, 255, 1, 255), f64(255.0, 127.5, 1.0, 85.0), i32(0, 1, 1, 0), f64(1.0, 1.0), i32(F, Q),
                  300),
        # jobs 0, 1 tie in c within entity 0; D_e / W_e = 4 for entities 0 and 1
        "ties": (i32(2, 2, 4, 4, 4, 1), f64(2.0, 2.0, 8.0, 4.0, 4.0, 0.5), i32(0, 0, 0, 1, 1, 2),
                 f64(2.0, 2.0, 1.0), i32(F, F, Q), 11),
        "mixed": (i32(1, 2, 4, 8, 1, 2, 4, 1), f64(0.5, 2.0, 4.0, 8.0, 1.0, 1.0, 2.0, 3.0),
                  i32(0, 1, 0, 1, 2, 2, 1, 0), f64(1.0, 2.0, 3.0), i32(F, Q, F), 12),
    }
    for n, frac in [(511, 0.4), (512, 0.7), (513, 0.25), (2049, 0.5)]:
        out[f"n{n}"] = big(rng, n, frac)
    return out


FIXED = fixed_instances()


def random_instances(n_cases, seed, max_n=40):
    """N in 1..max_n, every layout and every kind of modes in turn, G uniform
    in 1..Σ sf + 3; a third of the instances with continuous priority weights."""
    rng = np.random.default_rng(seed)
    out = []
    for i in range(n_cases):
        n = int(rng.integers(1, max_n + 1))
        lay = LAYOUTS[i % len(LAYOUTS)]
        kind = ("fairness", "fifo", "mixed")[(i // len(LAYOUTS)) % 3]
        out.append(draw(rng, n, lay, kind, continuous=i % 3 == 0))
    return out


def stage_instances(n_cases=60, seed=5):
    """The stage-loop cross-check's instances: all-fairness, N in 1..12, at
    most 4 entities, priority weights in {0.5, 1, 2, 3}."""
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(n_cases):
        n = int(rng.integers(1, 13))
        E = int(rng.integers(1, 5))
        sf = rng.choice(SF_VALUES, size=n).astype(np.int32)
        w = rng.choice(PRIORITY_WEIGHTS, size=n)
        ent = rng.integers(0, E, size=n).astype(np.int32)
        W = rng.choice([0.5, 1.0, 1.5, 2.0, 3.0, 5.0], size=E).astype(np.float64)
        out.append((sf, (1.0 / w) * sf, ent, W, np.zeros(E, dtype=np.int32), int(rng.integers(1, int(sf.sum()) + 4))))
    return out


def same_bits(r1, r2):
    return (r1[0].tobytes() == r2[0].tobytes() and r1[1].tobytes() == r2[1].tobytes()
            and np.float64(r1[2]).tobytes() == np.float64(r2[2]).tobytes()
            and np.float64(r1[3]).tobytes() == np.float64(r2[3]).tobytes())


def check_properties(inst, x, g, level, used):
    """What holds of every result, whatever the size: the bounds, capacity,
    work conservation, saturated entities at exactly 1, the fifo shape."""
    sf, c, ent, W, modes, G = inst
    tot = total(inst)
    assert np.all(x >= 0.0) and np.all(x <= 1.0)
    fs = math.fsum(float(s) * float(v) for s, v in zip(sf, x))
    assert fs <= G * (1 + 1e-12), (fs, G)
    assert fs >= min(G, tot) * (1 - 1e-9), (fs, G, tot)
    assert abs(used - fs) <= 1e-12 * max(G, 1)
    assert math.fsum(g) <= G * (1 + 1e-12) or tot <= G
    for e in range(len(W)):
        jobs = np.flatnonzero(ent == e)
        D = int(sf[jobs].sum())
        if len(jobs) == 0:
            assert g[e] == 0.0
            continue
        assert g[e] <= D
        if g[e] >= D:
            assert np.all(x[jobs] == 1.0), e
        assert math.fsum(float(sf[j]) * float(x[j]) for j in jobs) <= g[e] * (1 + 1e-12)
        if modes[e] == FIFO:
            xe = x[jobs]
            part = np.flatnonzero((xe > 0.0) & (xe < 1.0))
            assert len(part) <= 1
            first_below = next((i for i, v in enumerate(xe) if v < 1.0), len(xe))
            assert np.all(xe[:first_below] == 1.0) and np.all(xe[first_below + 1:] == 0.0), (e, xe)
    if tot <= G:
        assert np.all(x == 1.0) and used == tot
        assert level == max(sf[ent == e].sum() / W[e] for e in range(len(W)) if np.any(ent == e))


def check_against_fluid(inst, x, rel=1e-12):
    """Every share within `rel` relative of the exact staged process.  The
    share of a job in a fairness entity is compared relative to itself.  The
    share of a job in a fifo entity is a difference, (g_e − Σ_{k<j} sf_k)/sf_j:
    g_e is known to a few ulps of g_e, not of the difference (a waiting job's
    exact share is 0, and no rounding of g_e is relative to that), so its
    capacity sf_j·x_j is compared relative to the entity's capacity g_e."""
    sf, ent, modes = inst[0], inst[2], inst[4]
    ref = wfh_ref.fluid(*inst)
    g = [Fraction(0)] * len(modes)
    for j, b in enumerate(ref):
        g[int(ent[j])] += int(sf[j]) * b
    for j, (a, b) in enumerate(zip(x, ref)):
        err = abs(Fraction(float(a)) - b)
        if modes[int(ent[j])] == FIFO:
            assert int(sf[j]) * err <= Fraction(rel) * g[int(ent[j])], (j, float(a), float(b))
        else:
            assert err <= Fraction(rel) * b, (j, float(a), float(b))
    return ref


# ---- the policy mirror's inputs (test_wfh_policy.py, test_gpu_wfh.py) ----
def policy_case(seed=7, n_jobs=300, n_entities=10):
    """The shape of the reference's tests/water_filling_tests_hierarchical.py:
    10 entities of weight 1..5 and a random mode each, 300 jobs of width 1, 2
    or 4 and priority 1..5 (1 in a fifo entity), three worker types of 64
    workers with sorted random throughputs."""
    rng = np.random.default_rng(seed)
    entities = [f"entity{e}" for e in range(n_entities)]
    policies = {e: ("fifo", "fairness")[int(rng.integers(0, 2))] for e in entities}
    policies[entities[0]], policies[entities[1]] = "fifo", "fairness"
    weights = {e: int(rng.integers(1, 6)) for e in entities}
    mapping = {e: [] for e in entities}
    worker_types = ["k80", "p100", "v100"]
    tp, sf, pw = {}, {}, {}
    for j in range(n_jobs):
        tp[j] = dict(zip(worker_types, sorted(float(v) for v in rng.random(3))))
        sf[j] = 2 ** int(rng.integers(0, 3))
        e = entities[int(rng.integers(0, n_entities))]
        pw[j] = 1.0 if policies[e] == "fifo" else int(rng.integers(1, 6))
        mapping[e].append(j)
    return dict(throughputs=tp, scale_factors=sf, priority_weights=pw, cluster_spec={wt: 64 for wt in worker_types},
                entity_weights=weights, entity_to_job_mapping=mapping, policies=policies)


def policy_run(engine, case=None, cls_name="MaxMinFairnessWaterFillingHierarchicalPolicy", **kw):
    import max_min_fairness_water_filling_hierarchical as wfh

    case = case or policy_case()
    pol = getattr(wfh, cls_name)(case["policies"], native=engine)
    out = pol.get_allocation(case["throughputs"], case["scale_factors"], case["priority_weights"],
                             case["cluster_spec"], entity_weights=case["entity_weights"],
                             entity_to_job_mapping=case["entity_to_job_mapping"], **kw)
    return out, pol
