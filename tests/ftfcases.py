"""Shared inputs and checks of the FinishTimeFairness tests (test_ftf.py,
test_ftf_policy.py, test_gpu_ftf.py).  An instance is (sf, p, a, E, G):
scale factors, full-allocation time still needed, elapsed time, expected
isolated time, workers."""
import contextlib
import io
import math
import os

import numpy as np

import ftf_ref

SF_VALUES, SF_WEIGHTS = [1, 2, 4, 8], [0.6, 0.3, 0.09, 0.01]  # the traces' scale-factor mix


def draw(rng, n, G, p_zero=0.0, a_hi=5.0):
    """sf with the trace's weights, p log-uniform in 1e2..1e5, a = 0 with
    probability 0.3 else log-uniform in 1e1..10^a_hi, E a random mix of a and
    the isolated remaining time p·max(1, n·sf/G).  A job that has run long on
    little isolated time (large a, small E) lifts ρ_box above what capacity
    asks for, so capacity binds mostly at small a_hi; a fraction p_zero of the
    jobs has no steps left."""
    sf = rng.choice(SF_VALUES, size=n, p=SF_WEIGHTS).astype(np.int32)
    p = 10.0 ** rng.uniform(2, 5, size=n)
    a = np.where(rng.random(n) < 0.3, 0.0, 10.0 ** rng.uniform(1, a_hi, size=n))
    if p_zero > 0.0:
        z = rng.random(n) < p_zero
        p = np.where(z, 0.0, p)
        a = np.where(z & (a == 0.0), 50.0, a)
    E = rng.uniform(0.0, 1.0, size=n) * a + p * np.maximum(1.0, n * sf / G)
    E = np.where(p > 0.0, E, a * rng.uniform(1.1, 4.0, size=n))  # a finished job: a/E in 0.25..0.9
    return sf, p, a, E, int(G)


def fixed_instances():
    rng = np.random.default_rng(23)
    f = lambda *v: np.array(v, dtype=np.float64)
    i32 = lambda *v: np.array(v, dtype=np.int32)
    out = {
        "n1": (i32(2), f(1000.0), f(50.0), f(1200.0), 4),
        "n1_binds": (i32(4), f(1000.0), f(50.0), f(1200.0), 2),
        "no_unit_width": (i32(2, 4, 8, 2), f(3e3, 5e3, 2e3, 7e3), f(0.0, 4e2, 1e3, 60.0),
                          f(4e3, 9e3, 5e3, 8e3), 12),
        # three identical jobs share the largest full-allocation ratio; capacity is ample
        "tie_at_box": (i32(1, 1, 1, 2, 1), f(900.0, 900.0, 900.0, 300.0, 100.0),
                       f(100.0, 100.0, 100.0, 0.0, 20.0), f(800.0, 800.0, 800.0, 1000.0, 400.0), 16),
        # identical jobs with m·sf = G: cap(ρ_box) = G exactly
        "cap_equals_G": (i32(2, 2, 2, 2), f(100.0, 100.0, 100.0, 100.0), f(0.0, 0.0, 0.0, 0.0),
                         f(100.0, 100.0, 100.0, 100.0), 8),
        "p0_binds": (i32(1, 2, 1, 4), f(0.0, 4e3, 6e3, 2e3), f(500.0, 100.0, 0.0, 300.0),
                     f(2e3, 5e3, 7e3, 3e3), 2),
        "p0_free": (i32(1, 2, 1, 4), f(0.0, 4e3, 6e3, 2e3), f(500.0, 100.0, 0.0, 300.0),
                    f(2e3, 5e3, 7e3, 3e3), 32),
        # a finished job holds the largest ratio (ρ_box = a/E of a p = 0 job)
        "p0_is_box": (i32(1, 1, 2), f(0.0, 1e3, 2e3), f(9e3, 10.0, 0.0), f(3e3, 2e3, 4e3), 8),
    }
    # the chunk-size steps (q = ⌈N/512⌉ changes at 513 and 1025) and one above the LDS path
    for n, G, a_hi in [(511, 64, 2.0), (512, 1024, 5.0), (513, 96, 5.0), (1025, 2048, 2.0), (2500, 256, 2.0),
                       (2500, 4096, 5.0)]:
        out[f"n{n}_G{G}"] = draw(rng, n, G, p_zero=0.01, a_hi=a_hi)
    return out


FIXED = fixed_instances()


def random_instances(n_cases, seed, max_n, max_g=2048):
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(n_cases):
        n = max(1, min(int(np.exp(rng.uniform(0.0, np.log(max_n + 1)))), max_n))
        G = max(1, min(int(np.exp(rng.uniform(0.0, np.log(max_g + 1)))), max_g))
        out.append(draw(rng, n, G, p_zero=0.05 if rng.random() < 0.3 else 0.0,
                        a_hi=2.0 if rng.random() < 0.4 else 5.0))
    return out


def slsqp_instances(n_cases=60, seed=2):
    """The cross-check's instances: N in 1..12, G in 1..16, every p > 0."""
    rng = np.random.default_rng(seed)
    return [draw(rng, int(rng.integers(1, 13)), int(rng.integers(1, 17))) for _ in range(n_cases)]


def check_allocation(inst, x, rho, mu):
    """The allocation against the program: feasible, every ratio ≤ ρ*, and
    the optimality conditions of the returned point (the unique optimum when
    capacity binds; otherwise the analytic centre's barrier stationarity, in
    the form of tests/test_mmf.py check_lp_optimal)."""
    sf, p, a, E, G = inst
    assert np.all(x >= 0.0) and np.all(x <= 1.0)
    used = math.fsum(float(s) * float(v) for s, v in zip(sf, x))
    assert used <= G * (1 + 1e-12)
    run = p > 0
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(run, (a + p / x) / E, a / E)
    assert np.all(ratio <= rho * (1 + 1e-12)), (ratio.max(), rho)
    d = rho * E - a
    pinned = run & ((d <= p) | ((a + p) / E >= rho))  # sw_ftf_pinned; ρ* > every (a+p)/E when ρ* > ρ_box
    with np.errstate(divide="ignore", invalid="ignore"):
        low = np.where(run, np.where(pinned, 1.0, p / d), 0.0)
    if mu == 0.0:  # capacity binds: the unique optimum
        assert np.all(np.abs(x - low) <= 1e-15)
        return
    free = ~pinned
    assert np.all(x[pinned] == 1.0)
    slack = G - used
    assert abs(mu * slack - 1.0) < 1e-9
    xf, sff = x[free], sf[free]
    cf = np.where(run[free], d[free], 1.0)  # a job with p = 0 has the barrier of c = 1, t = 0
    tf = p[free]
    h = 1 / xf - 1 / (1 - xf) + cf / (cf * xf - tf) - sff * mu
    scale = 1 / xf + 1 / (1 - xf) + cf / (cf * xf - tf)
    assert np.all(np.abs(h) <= 1e-9 * scale)


def same_bits(r1, r2):
    return (r1[0].tobytes() == r2[0].tobytes()
            and np.float64(r1[1]).tobytes() == np.float64(r2[1]).tobytes()
            and np.float64(r1[2]).tobytes() == np.float64(r2[2]).tobytes())


# ---- the policy mirror's three-call sequence (test_ftf_policy.py, test_gpu_ftf.py) ----
def policy_sequence(engine):
    """Three successive calls: job 1 finishes after the second, job 3 arrives
    at the third.  Returns the allocations and the policy."""
    import finish_time_fairness as ftf

    pol = ftf.FinishTimeFairnessPolicyWithPerf(native=engine)
    calls = [
        dict(tp={0: 10.0, 1: 4.0, 2: 2.5}, sf={0: 1, 1: 2, 2: 4}, t={0: 0.0, 1: 120.0, 2: 360.0},
             rem={0: 50000, 1: 9000, 2: 30000}),
        dict(tp={0: 10.0, 1: 4.0, 2: 2.5}, sf={0: 1, 1: 2, 2: 4}, t={0: 1920.0, 1: 2040.0, 2: 2280.0},
             rem={0: 42000, 1: 1500, 2: 27000}),
        dict(tp={0: 10.0, 2: 2.5, 3: 7.0}, sf={0: 1, 2: 4, 3: 1}, t={0: 3840.0, 2: 4200.0, 3: 30.0},
             rem={0: 30000, 2: 26000, 3: 80000}),
    ]
    out = []
    for c in calls:
        out.append(pol.get_allocation({j: {"v100": v} for j, v in c["tp"].items()}, c["sf"],
                                      {j: 1.0 for j in c["tp"]}, c["t"], c["rem"], {"v100": 4}))
    return calls, out, pol


# ---- the 30-job simulation (test_ftf_policy.py, test_gpu_ftf.py) ----
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
    sim = sw_sim.Simulator("finish_time_fairness", tp, prof, 120, ftf_allocator=engine)
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
