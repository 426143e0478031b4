"""Shared inputs and checks of the MinTotalDuration tests (test_mtd.py,
test_mtd_policy.py, test_gpu_mtd.py).  An instance is (sf, p, G): scale
factors, full-allocation time still needed (steps left / throughput),
workers."""
import contextlib
import io
import math
import os
from fractions import Fraction

import numpy as np

import mtd_ref

SF_VALUES, SF_WEIGHTS = [1, 2, 4, 8], [0.6, 0.3, 0.09, 0.01]  # the traces' scale-factor mix
LDS_JOBS = 4096  # SW_MTD_LDS_JOBS (csrc/sw_mtd.hip): the largest instance staged in LDS


def draw_jobs(rng, n, zero_job=False):
    """sf with the trace's weights, whole steps log-uniform in 1e1..1e7,
    throughput uniform in 0.5..40; with zero_job one job has no steps left."""
    sf = rng.choice(SF_VALUES, size=n, p=SF_WEIGHTS).astype(np.int32)
    steps = np.floor(10.0 ** rng.uniform(1, 7, size=n))
    tp = rng.uniform(0.5, 40.0, size=n)
    if zero_job:
        steps[int(rng.integers(0, n))] = 0.0
    return sf, steps, tp


def draw(rng, n, G, zero_job=False):
    sf, steps, tp = draw_jobs(rng, n, zero_job)
    return sf, steps / tp, int(G)


def fixed_instances():
    rng = np.random.default_rng(31)
    f = lambda *v: np.array(v, dtype=np.float64)
    i32 = lambda *v: np.array(v, dtype=np.int32)
    out = {
        "n1": (i32(2), f(1000.0), 4),
        # one long job, ample G: max p sets T
        "box_sets_T": (i32(1, 1, 2, 1), f(8e4, 500.0, 900.0, 1.2e3), 16),
        # many jobs, small G: the capacity row sets T
        "cap_sets_T": (np.array([1, 2, 1, 4] * 10, dtype=np.int32),
                       np.linspace(1500.0, 2500.0, 40), 2),
        # every p far below 100: T ends at the search's floor
        "floor": (i32(1, 2, 1), f(3.0, 0.5, 7.25), 8),
        "all_zero": (i32(1, 2, 4, 1), f(0.0, 0.0, 0.0, 0.0), 2),
        "p0_mixed": (i32(1, 2, 1, 4, 1), f(0.0, 4e3, 0.0, 2e3, 6e3), 4),
        # climbs two decade rounds: T = 31093750.0 in 16 probes
        "decade": (i32(1), f(3e7), 1),
        # the first probe equals p: x = 1, cap = G, μ = 0, T = 500050.0 in 6 probes
        "exact_cap_pinned": (i32(1), f(500050.0), 1),
        # a job whose scale factor exceeds G
        "sf_above_G": (i32(8, 1, 1), f(3000.0, 1000.0, 500.0), 4),
    }
    # the chunk-size steps (q = ⌈N/512⌉ changes at 513 and 1025), the last
    # instance staged in LDS and the first that is not
    for n, G in [(511, 4), (512, 1024), (513, 96), (1025, 8), (LDS_JOBS, 16), (LDS_JOBS + 1, 8192)]:
        out[f"n{n}_G{G}"] = draw(rng, n, G, zero_job=(n % 2 == 1))
    return out


FIXED = fixed_instances()
# T and the number of probes of the cases whose search path is known by hand
KNOWN = {"floor": (103.81431579589844, 18), "all_zero": (103.81431579589844, 18),
         "decade": (31093750.0, 16), "exact_cap_pinned": (500050.0, 6)}


def random_instances(n_cases, seed, max_n, max_g=2048):
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(n_cases):
        n = max(1, min(int(np.exp(rng.uniform(0.0, np.log(max_n + 1)))), max_n))
        G = max(1, min(int(np.exp(rng.uniform(0.0, np.log(max_g + 1)))), max_g))
        out.append(draw(rng, n, G, zero_job=rng.random() < 0.15))
    return out


def above_staged(seed=5):
    """Three instances above the staged size (the L2 path)."""
    rng = np.random.default_rng(seed)
    return [draw(rng, n, G, zero_job=z) for n, G, z in
            [(LDS_JOBS + 1, 16, False), (LDS_JOBS + 700, 4096, True), (5 * 1024 + 3, 700, False)]]


LP_MARGIN = 1e-6


def lp_instances(n_cases=300, seed=7):
    """The HiGHS cross-check's instances: N ≤ 24, G ≤ 64, half on two identical
    worker types that split G.  Each is (tp[jobs][types], sf, steps, workers,
    p, admitted): an LP solver cannot decide a probe on the boundary, so an
    instance is admitted only when no probe of the exact search lies within
    LP_MARGIN (relative) of T* = max(max p, Σ sf·p / G) — a margin computed
    from the inputs alone."""
    rng = np.random.default_rng(seed)
    out = []
    for i in range(n_cases):
        n = int(rng.integers(1, 25))
        G = int(rng.integers(1, 65))
        sf, steps, tp = draw_jobs(rng, n, zero_job=rng.random() < 0.15)
        if i % 2 == 1 and G >= 2:
            g0 = int(rng.integers(1, G))
            workers = [g0, G - g0]
        else:
            workers = [G]
        tpm = np.repeat(tp[:, None], len(workers), axis=1)
        p = steps / tp
        _, probes, _ = mtd_ref.exact_search(sf, p, G)
        tstar = mtd_ref.least_feasible(sf, p, G)
        gap = min(abs(Fraction(T) - tstar) / tstar for T in probes) if tstar > 0 else Fraction(1)
        out.append((tpm, sf, steps, workers, p, gap > Fraction(LP_MARGIN), float(gap)))
    return out


def check_allocation(inst, x, T, mu):
    """The allocation against the reference's search and LP: T is the exact
    search's answer (feasible, and T/1.05 at or below the bound the search
    ended on, so not an answer it could have given), x a point of the feasible
    face at T, and the optimality conditions of the returned point (x = p/T
    where the face is a single point; otherwise the analytic centre's barrier
    stationarity, the bounds of ftfcases.check_allocation)."""
    sf, p, G = inst
    feasible = mtd_ref.exact_predicate(sf, p, G)
    assert feasible(T), T
    Tx, _, end_min = mtd_ref.exact_search(sf, p, G)
    assert T == Tx, (T, Tx)
    # end_min is an infeasible probe or the lower edge of the round's interval,
    # and the search answers only with probes above it
    assert not (1.05 * end_min < T), (end_min, T)
    low = p / T
    assert np.all(x >= low) and np.all(x <= 1.0)
    used = math.fsum(float(s) * float(v) for s, v in zip(sf, x))
    assert used <= G * (1 + 1e-12)
    if mu == 0.0:  # the face is the single point
        assert np.all(x == low)
        return
    slack = G - used
    assert abs(mu * slack - 1.0) < 1e-9
    free = low < 1.0  # p = T: lo = hi = 1
    assert np.all(x[~free] == 1.0)
    xf, sff, tf = x[free], sf[free], p[free]
    h = 1 / xf - 1 / (1 - xf) + T / (T * xf - tf) - sff * mu
    scale = 1 / xf + 1 / (1 - xf) + T / (T * xf - tf)
    assert np.all(np.abs(h) <= 1e-9 * scale)


def same_bits(r1, r2):
    return (r1[0].tobytes() == r2[0].tobytes()
            and np.float64(r1[1]).tobytes() == np.float64(r2[1]).tobytes()
            and np.float64(r1[2]).tobytes() == np.float64(r2[2]).tobytes())


# ---- the policy mirror's three-call sequence (test_mtd_policy.py, test_gpu_mtd.py) ----
def policy_sequence(engine):
    """Three successive calls: job 1 finishes after the second, job 3 arrives
    at the third.  Returns the calls, the allocations and the policy."""
    import min_total_duration as mtd

    pol = mtd.MinTotalDurationPolicyWithPerf(native=engine)
    calls = [
        dict(tp={0: 10.0, 1: 4.0, 2: 2.5}, sf={0: 1, 1: 2, 2: 4}, rem={0: 50000, 1: 9000, 2: 30000}),
        dict(tp={0: 10.0, 1: 4.0, 2: 2.5}, sf={0: 1, 1: 2, 2: 4}, rem={0: 42000, 1: 1500, 2: 27000}),
        dict(tp={0: 10.0, 2: 2.5, 3: 7.0}, sf={0: 1, 2: 4, 3: 1}, rem={0: 30000, 2: 26000, 3: 80000}),
    ]
    out = []
    for c in calls:
        out.append(pol.get_allocation({j: {"v100": v} for j, v in c["tp"].items()}, c["sf"], c["rem"],
                                      {"v100": 4}))
    return calls, out, pol


# ---- the 30-job simulation of ftfcases.simulate_30 (test_mtd_policy.py, test_gpu_mtd.py) ----
def simulate_30(engine, record=None):
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
    sim = sw_sim.Simulator("min_total_duration", tp, prof, 120, mtd_allocator=engine)
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
