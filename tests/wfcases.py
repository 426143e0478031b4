"""Shared inputs and checks of the water-filling MaxMinFairness tests
(test_wf.py, test_wf_policy.py, test_gpu_wf.py).  An instance is (sf, c, G):
scale factors, coefficients c_j = sf_j / priority weight, workers."""
import contextlib
import io
import math
import os

import numpy as np

import wf_ref

SF_VALUES, SF_WEIGHTS = [1, 2, 4, 8], [0.6, 0.3, 0.09, 0.01]  # the traces' scale-factor mix
PRIORITY_WEIGHTS = [0.5, 1.0, 2.0, 3.0]


def draw(rng, n, G, continuous=False, trace_mix=True):
    """Widths in {1, 2, 4, 8} (the traces' mix, or uniform), priority weights in
    {0.5, 1, 2, 3} or, continuous, log-uniform in 0.25..4; c = sf / w."""
    sf = rng.choice(SF_VALUES, size=n, p=SF_WEIGHTS if trace_mix else None).astype(np.int32)
    w = 2.0 ** rng.uniform(-2, 2, size=n) if continuous else rng.choice(PRIORITY_WEIGHTS, size=n)
    return sf, sf / w, int(G)


def fixed_instances():
    rng = np.random.default_rng(29)
    f = lambda *v: np.array(v, dtype=np.float64)
    i32 = lambda *v: np.array(v, dtype=np.int32)
    out = {
        "n1": (i32(2), f(2.0), 4),
        "n1_binds": (i32(4), f(4.0), 2),
        "sum_equals_G": (i32(1, 2, 4, 1), f(1.0, 4.0, 2.0, 1 / 3), 8),
        "sum_is_G_plus_1": (i32(1, 2, 4, 1), f(1.0, 4.0, 2.0, 1 / 3), 7),
        "all_saturate": (i32(1, 2, 4, 8, 1), f(2.0, 1.0, 4.0, 8 / 3, 0.5), 40),
        "none_saturates": (i32(1, 2, 4, 8), f(1.0, 2.0, 4.0, 8.0), 2),
        # the level reaches c = 1 exactly as capacity fills: 2 + 2·(1/2) = 3
        "tie_at_level": (i32(1, 1, 1, 1), f(1.0, 1.0, 2.0, 2.0), 3),
        # three jobs share the coefficient that is still rising at the level
        "tie_above_level": (i32(1, 2, 2, 2, 4), f(0.5, 2.0, 2.0, 2.0, 8.0), 5),
        "no_unit_width": (i32(2, 4, 8, 2), f(2.0, 2.0, 16.0, 2 / 3), 7),
        "sf255": (i32(255, 255, 1), f(255.0, 127.5, 1.0), 300),
        "G1": (i32(1, 2, 4), f(1.0, 1.0, 8.0), 1),
        # coefficients over 600 orders of magnitude; the jobs at 1e-300 and 1e-150
        # saturate (6 workers), the job at c = 1 takes the other 3 of its 8
        "spread": (i32(2, 4, 8, 4, 2), f(1e-300, 1e-150, 1.0, 1e150, 1e300), 9),
    }
    # the chunk-size steps (q = ⌈N/512⌉ changes at 513, 1025 and 2049) and the
    # step from the LDS path to the L2 path (2048 / 2049)
    for n, frac, cont in [(511, 0.0, True), (512, 0.6, False), (513, 0.3, True), (1025, 0.9, False),
                          (2048, 0.5, True), (2049, 0.5, True), (2500, 0.75, False), (2500, 1.5, True)]:
        sf, c, _ = draw(rng, n, 1, continuous=cont)
        G = 64 if frac == 0.0 else int(frac * sf.sum())
        out[f"n{n}_G{G}"] = (sf, c, G)
    return out


FIXED = fixed_instances()


def random_instances(n_cases, seed, max_n, max_g=2048):
    """N log-uniform in 1..max_n; G log-uniform in 1..max_g or uniform in
    1..Σ sf + 5 (so that some instances fit the cluster whole); half of the
    instances with continuous priority weights."""
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(n_cases):
        n = max(1, min(int(np.exp(rng.uniform(0.0, np.log(max_n + 1)))), max_n))
        sf, c, _ = draw(rng, n, 1, continuous=rng.random() < 0.5)
        if rng.random() < 0.5:
            G = max(1, min(int(np.exp(rng.uniform(0.0, np.log(max_g + 1)))), max_g))
        else:
            G = int(rng.integers(1, int(sf.sum()) + 6))
        out.append((sf, c, G))
    return out


def stage_instances(n_cases=60, seed=3):
    """The stage-loop cross-check's instances: N in 1..13, widths in
    {1, 2, 4, 8}, priority weights in {0.5, 1, 2, 3}, G in 1..Σ sf + 5.
    Returns (sf, w, G)."""
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(n_cases):
        n = int(rng.integers(1, 14))
        sf = rng.choice(SF_VALUES, size=n).astype(np.int32)
        w = rng.choice(PRIORITY_WEIGHTS, size=n)
        out.append((sf, w, int(rng.integers(1, int(sf.sum()) + 6))))
    return out


def check_allocation(inst, x, level, used):
    """The exact certificate and the sort-based closed form (both in
    Fractions, wf_ref) on one result."""
    sf, c, G = inst
    total = int(np.sum(sf, dtype=np.int64))
    assert np.all(x >= 0.0) and np.all(x <= 1.0)
    fs = math.fsum(float(s) * float(v) for s, v in zip(sf, x))
    assert fs <= G * (1 + 1e-12)
    assert abs(used - fs) <= 1e-12 * G
    with np.errstate(over="ignore"):
        assert np.all(np.abs(x - np.minimum(1.0, level / c)) <= 1e-15)
    assert np.all(x[c <= level] == 1.0)
    exact = wf_ref.closed_form_level(sf, c, G)
    if total <= G:
        assert np.all(x == 1.0) and level == c.max() == float(exact) and used == total
    else:
        assert wf_ref.certified(sf, c, G, level, 1e-9), level
        assert abs(exact - wf_ref.Fraction(level)) <= wf_ref.Fraction(1e-12) * exact, (level, float(exact))


def same_bits(r1, r2):
    return (r1[0].tobytes() == r2[0].tobytes()
            and np.float64(r1[1]).tobytes() == np.float64(r2[1]).tobytes()
            and np.float64(r1[2]).tobytes() == np.float64(r2[2]).tobytes())


# ---- the policy mirror's three-call sequence (test_wf_policy.py, test_gpu_wf.py) ----
def policy_sequence(engine):
    """Three successive calls on 6 workers: job 1 has left and job 3 has arrived
    at the second, job 0 has left at the third (which fits the cluster whole)."""
    import max_min_fairness_water_filling as wf

    pol = wf.MaxMinFairnessWaterFillingPolicyWithPerf(native=engine)
    calls = [
        dict(tp={0: 10.0, 1: 4.0, 2: 2.5}, sf={0: 1, 1: 2, 2: 4}, w={0: 1.0, 1: 2.0, 2: 1.0}),
        dict(tp={0: 10.0, 2: 2.5, 3: 7.0}, sf={0: 1, 2: 4, 3: 8}, w={0: 1.0, 2: 1.0, 3: 3.0}),
        dict(tp={2: 2.5, 3: 7.0}, sf={2: 4, 3: 2}, w={2: 1.0, 3: 0.5}),
    ]
    out = [pol.get_allocation({j: {"v100": v} for j, v in c["tp"].items()}, c["sf"], c["w"], {"v100": 6})
           for c in calls]
    return calls, out, pol


# ---- the 30-job simulation (test_wf_policy.py, test_gpu_wf.py) ----
def simulate_30(policy, record=None, **allocators):
    import sw_sim
    import sw_trace as st

    trace = os.path.join(st.DATA_DIR, "traces",
                         "120_0.2_5_100_40_25_0,0.5,0.5_0.6,0.3,0.09,0.01_multigpu_dynamic.trace")
    tp = st.load_throughputs()
    jobs, arr = st.parse_trace(trace)
    jobs, arr = jobs[:30], arr[:30]
    prof = st.synthesize_profiles(jobs, tp)
    for i, j in enumerate(jobs):
        j.duration = sum(prof[i]["duration_every_epoch"])
    sim = sw_sim.Simulator(policy, tp, prof, 120, **allocators)
    if record is not None:
        sched, alloc = sim._schedule_jobs_on_workers, sim._compute_allocation

        def checked_schedule():
            out = sched()
            record["workers"].append([w for ws in out.values() for w in ws])
            return out

        def checked_allocation():
            out = alloc()
            record["allocations"].append(dict(out))
            return out

        sim._schedule_jobs_on_workers = checked_schedule
        sim._compute_allocation = checked_allocation
    with contextlib.redirect_stdout(io.StringIO()):
        sim.simulate(8, arr, jobs)
    return sim.summary()
