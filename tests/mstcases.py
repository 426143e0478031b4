"""Shared inputs and checks of the max-sum-throughput tests (test_mst.py,
test_mst_policy.py, test_gpu_mst.py).  An instance is (sf, w, l, G): scale
factors, weights (throughput / cost), floors (or None) and workers."""
import contextlib
import io
import os

import numpy as np

import mst_ref

SF_VALUES, SF_WEIGHTS = [1, 2, 4, 8], [0.6, 0.3, 0.09, 0.01]  # the traces' scale-factor mix
LDS_JOBS = 3072  # SW_MST_LDS_JOBS (csrc/sw_mst.hip): the largest instance staged in LDS
TYPE_TP = np.array([0.7, 1.9, 3.3, 5.0, 12.5, 33.0])  # steps/s of six job types on one worker
INF = float("inf")

# The bars of tests/test_mst.py, measured on the CPU twin over the fixed list and
# the 300 instances of random_instances(300, seed=3, max_n=60):
# the worst relative gap of the exact objective of the returned x to the exact
# optimum, and the worst exact capacity excess relative to G, each times 8.
# Their caps are 1e-9 and 1e-12, which the exact optimum meets with 0.
WORST_OBJ_GAP = 1.814170085120327e-16
WORST_CAP_EXCESS = 2.304503135871849e-16
OBJ_BAR = 8 * WORST_OBJ_GAP
CAP_BAR = 8 * WORST_CAP_EXCESS
assert OBJ_BAR <= 1e-9 and CAP_BAR <= 1e-12


def draw(rng, n, G=None, floors=None, zeros=0, jitter=0.5, fill=None):
    """Jobs of six types: a job's throughput is a function of its type and
    scale factor, so jobs of one type and scale factor tie exactly (the
    traces' case); a `jitter` share of the jobs gets a throughput of its own.
    `zeros` jobs have throughput 0.  G defaults to fill·Σ sf.  floors: None,
    "ok" (about a third of the jobs, Σ sf·l below G), "over" (one floor above
    1), "sum" (Σ sf·l above G) or "inf" (a floor of +inf)."""
    sf = rng.choice(SF_VALUES, size=n, p=SF_WEIGHTS).astype(np.int32)
    tp = TYPE_TP[rng.integers(0, len(TYPE_TP), size=n)] * sf.astype(np.float64) ** 0.75
    own = rng.random(n) < jitter
    tp = np.where(own, tp * rng.uniform(0.9, 1.1, size=n), tp)
    for j in rng.choice(n, size=min(zeros, n), replace=False):
        tp[j] = 0.0
    if G is None:
        G = max(1, int(fill * int(sf.sum())))
    l = None
    if floors is not None:
        has = rng.random(n) < 0.35
        l = np.where(has, rng.uniform(0.0, 1.0, size=n) * min(1.0, 0.8 * G / float(sf.sum())), 0.0)
        j = int(rng.integers(0, n))
        if floors == "over":
            l[j] = 1.25
        elif floors == "sum":
            l = np.minimum(1.0, l + 1.5 * G / float(sf.sum()))
        elif floors == "inf":
            l[j] = INF
    return sf, tp, l, int(G)


def fixed_instances():
    rng = np.random.default_rng(41)
    f = lambda *v: np.array(v, dtype=np.float64)
    i32 = lambda *v: np.array(v, dtype=np.int32)
    out = {
        "n1_slack": (i32(2), f(3.0), None, 4),
        "n1_short": (i32(4), f(3.0), None, 1),            # G = 1 below the only job's sf
        "n2_class_of_one": (i32(1, 1), f(5.0, 2.0), None, 1),
        # the densest job is wider than the cluster: it is the class, alone
        "sf_above_G": (i32(8, 1, 1), f(80.0, 3.0, 2.0), None, 4),
        "all_tied": (i32(1, 1, 1, 1, 1), f(2.5, 2.5, 2.5, 2.5, 2.5), None, 3),
        "tied_mixed_sf": (i32(1, 2, 4, 2), f(1.5, 3.0, 6.0, 3.0), None, 5),
        # f drops exactly to G at a class boundary: the class job keeps its floor 0
        "boundary": (i32(1, 1, 1, 1), f(4.0, 3.0, 2.0, 1.0), None, 2),
        # capacity holds exactly the class's floors: the face is that point
        "point_at_floors": (i32(1, 1, 2), f(1.0, 1.0, 0.5), f(0.5, 0.5, 0.0), 1),
        "slack_empty_class": (i32(1, 2, 1), f(1.0, 7.0, 3.0), None, 8),
        "slack_zero_tp": (i32(1, 2, 1, 1), f(1.0, 0.0, 3.0, 0.0), None, 8),
        # λ = 0 and the zero-throughput class has no room left
        "slack_point": (i32(1, 1), f(1.0, 0.0), None, 1),
        "floors_on_class": (i32(1, 1, 1, 2), f(2.0, 2.0, 2.0, 9.0), f(0.25, 0.0, 0.5, 0.0), 4),
        "floor_is_one": (i32(1, 1, 1), f(2.0, 2.0, 2.0), f(1.0, 0.0, 0.0), 2),
        "floor_above_one": (i32(1, 1, 1), f(2.0, 3.0, 2.0), f(1.5, 0.0, 0.25), 2),
        "floors_above_G": (i32(2, 2, 1), f(2.0, 3.0, 2.0), f(0.75, 0.5, 0.5), 2),
        "floor_inf": (i32(1, 1, 1), f(0.0, 3.0, 2.0), f(INF, 0.0, 0.25), 2),
        "floors_all_zero": (i32(1, 1, 1), f(2.0, 3.0, 2.0), f(0.0, 0.0, 0.0), 2),
        "zero_tp_floor_on_slack": (i32(1, 1, 2), f(0.0, 4.0, 0.0), f(0.0, 0.0, 0.25), 6),
    }
    # the chunk-size steps (q = ⌈N/512⌉ changes at 513 and 1025), the last
    # instance staged in LDS and the first that is not
    for n, fill, fl, z in [(511, 0.4, None, 0), (512, 0.7, "ok", 2), (513, 0.3, "ok", 0), (1025, 1.2, None, 3),
                           (LDS_JOBS, 0.5, "ok", 1), (LDS_JOBS + 1, 0.6, None, 0)]:
        out[f"n{n}"] = draw(rng, n, floors=fl, zeros=z, fill=fill)
    out["n513_all_tied"] = (np.full(513, 2, dtype=np.int32), np.full(513, 6.5), None, 400)
    return out


FIXED = fixed_instances()

ALL_PATHS = {"slack_empty", "slack_mu", "slack_point", "tight_nu_neg", "tight_nu_pos", "tight_point",
             "dropped", "null_floors", "floor_in_class", "floor_is_one", "class_of_one", "all_tied",
             "sf_above_G", "G1", "lds", "global", "q1", "q2", "q3", "q6", "q7", "n1", "n2"}


def paths(inst, result):
    """The names of the paths an instance takes, from its inputs and result."""
    sf, w, l, G = inst
    x, lam, m, _, dropped = result
    n = len(sf)
    d = np.where(w > 0, w / sf, 0.0)
    cls = d == lam
    lo = np.zeros(n) if (l is None or dropped) else l
    point = not np.any(cls & (x > lo))  # the class sits at its floors
    out = {f"q{(n + 511) // 512}", "lds" if n <= LDS_JOBS else "global"}
    if n <= 2:
        out.add(f"n{n}")
    if lam == 0.0:
        out.add("slack_empty" if not cls.any() else ("slack_point" if point else "slack_mu"))
    else:
        out.add("tight_point" if point else ("tight_nu_pos" if m > 0 else "tight_nu_neg"))
        if cls.sum() == 1:
            out.add("class_of_one")
        if cls.all() and n > 1:
            out.add("all_tied")
        if sf[np.argmax(d)] > G:
            out.add("sf_above_G")
    if dropped:
        out.add("dropped")
    if l is None:
        out.add("null_floors")
    elif not dropped and not point:
        if np.any(cls & (l > 0) & (l < 1)):
            out.add("floor_in_class")
        if np.any(cls & (l == 1)):
            out.add("floor_is_one")
    if G == 1:
        out.add("G1")
    return out


def random_instances(n_cases, seed, max_n):
    """Seeded instances with ties, floors (feasible and not), zero throughputs,
    tight and slack clusters."""
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(n_cases):
        n = max(1, min(int(np.exp(rng.uniform(0.0, np.log(max_n + 1)))), max_n))
        u = rng.random()
        floors = None if u < 0.5 else "ok" if u < 0.8 else ["over", "sum", "inf"][int(rng.integers(0, 3))]
        zeros = int(rng.integers(1, 4)) if rng.random() < 0.25 else 0
        out.append(draw(rng, n, floors=floors, zeros=zeros, jitter=float(rng.choice([0.0, 0.5, 1.0])),
                        fill=float(rng.uniform(0.03, 1.3))))
    return out


def above_staged(seed=5):
    """Three instances above the staged size (the global path)."""
    rng = np.random.default_rng(seed)
    return [draw(rng, n, floors=fl, zeros=z, fill=fill) for n, fl, z, fill in
            [(LDS_JOBS + 1, "ok", 0, 0.5), (LDS_JOBS + 700, None, 2, 0.9), (4 * 1024 + 3, "sum", 0, 0.2)]]


def same_bits(r1, r2):
    return (r1[0].tobytes() == r2[0].tobytes()
            and all(np.float64(a).tobytes() == np.float64(b).tobytes() for a, b in zip(r1[1:4], r2[1:4]))
            and bool(r1[4]) == bool(r2[4]))


# ---- the policy mirror's three-call sequence (test_mst_policy.py, test_gpu_mst.py) ----
def policy_sequence(engine):
    """Three successive calls: job 1 leaves after the second, job 3 arrives at
    the third, which also carries costs and an SLO.  Returns the calls, the
    allocations and the policy."""
    import max_sum_throughput as mst

    pol = mst.ThroughputNormalizedByCostSumWithPerfSLOs(native=engine)
    calls = [
        dict(tp={0: 10.0, 1: 4.0, 2: 10.0}, sf={0: 1, 1: 2, 2: 1}, kw={}),
        dict(tp={0: 10.0, 1: 4.0, 2: 10.0, 4: 10.0}, sf={0: 1, 1: 2, 2: 1, 4: 1}, kw={}),
        dict(tp={0: 10.0, 2: 10.0, 3: 7.0, 4: 10.0}, sf={0: 1, 2: 1, 3: 4, 4: 1},
             kw=dict(instance_costs={"v100": 2.5}, SLOs={3: 4000.0}, num_steps_remaining={3: 7000, 0: 10})),
    ]
    out = []
    for c in calls:
        out.append(pol.get_allocation({j: {"v100": v} for j, v in c["tp"].items()}, c["sf"], {"v100": 2},
                                      **c["kw"]))
    return calls, out, pol


# ---- the 30-job simulation of ftfcases.simulate_30 (test_mst_policy.py, test_gpu_mst.py) ----
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
    sim = sw_sim.Simulator("max_sum_throughput_perf", tp, prof, 120, mst_allocator=engine)
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
