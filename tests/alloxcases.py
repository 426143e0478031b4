"""tests/alloxcases.py — the AlloX instances shared by the CPU and the GPU
tests: fixed cases, seeded random sets, the boundary sizes, the three-call
policy sequence and the 30-job simulation.

An instance is (free_workers, p, d): free workers per type, processing times
[m][types], delays [m] (tests/allox_ref.py).
"""
import contextlib
import io
import os

import numpy as np

import allox_ref

# The worst relative gap |twin − scipy| / scipy of the total cost over the
# real-valued sets below (real_instances() and the real-valued half of
# boundary_instances()), as measured on this build; tests/test_allox.py
# asserts 8 × this and that the sets still give it.
WORST_REAL_GAP = 4.269434890057712e-16
GAP_FACTOR = 8
EPS = 2.0 ** -53

WAVE_SLOTS = 256  # csrc/sw_allox.hip SW_ALLOX_WAVE_SLOTS: one wave up to this many slots
LDS_BYTES = 65536 - 256  # csrc/sw_allox.hip SW_ALLOX_LDS_BYTES


def staged(inst):
    """Whether the kernel copies the instance's p and d into LDS: they fit
    behind the column state (25 B a slot, 8 B a row, rounded up to 8)."""
    m, n, t = len(inst[2]), int(inst[0].sum()), len(inst[0])
    return ((25 * (m + n) + 8 * m + 7) & ~7) + 8 * (m * t + m) <= LDS_BYTES


def _a(free, p, d):
    return allox_ref.arrays(free, p, d)


FIXED = {
    # one job, two workers of one type: position 1 on worker 0 (the lowest slot)
    "m1": _a([2], [[5.0]], [3.0]),
    # fewer jobs than workers: every job alone at position 1
    "m_lt_n": _a([5], [[4.0], [2.0], [9.0]], [1.0, 2.0, 3.0]),
    # m = n + 1, one type: the smallest p sits at position 2 and runs first
    "m_eq_n_plus_1": _a([3], [[7.0], [3.0], [9.0], [5.0]], [0.0, 0.0, 0.0, 0.0]),
    # the tie example: one type, two workers, p = 1, 2, 3 (cost 1·2 + 2 + 3 = 7)
    "tie_three": _a([2], [[1.0], [2.0], [3.0]], [0.0, 0.0, 0.0]),
    # two types: job 1 is slow everywhere but far less so on type 1, the slow type for job 0
    "two_types": _a([1, 1], [[10.0, 40.0], [500.0, 60.0]], [5.0, 7.0]),
    # a type without free workers between two that have some
    "empty_type": _a([1, 0, 2], [[3.0, 1.0, 6.0], [4.0, 1.0, 2.0], [8.0, 1.0, 8.0], [2.0, 1.0, 5.0]],
                     [0.0, 10.0, 20.0, 30.0]),
    "all_p_equal": _a([2, 1], np.full((7, 2), 6.0), np.arange(7.0)),
    "p_zero_rows": _a([2], [[0.0], [4.0], [0.0], [1.0], [0.0]], [1.0, 0.0, 2.0, 0.0, 3.0]),
    "all_zero": _a([1, 1], np.zeros((4, 2)), np.zeros(4)),
    "no_free_worker": _a([0, 0], [[1.0, 2.0], [3.0, 4.0]], [0.0, 1.0]),
    "no_jobs": _a([3], np.zeros((0, 1)), np.zeros(0)),
    # the validator's bounds themselves
    "bounds": _a([1], [[1e30], [0.0]], [1e15, 0.0]),
}


def split_workers(rng, n, types):
    """n workers over `types` types, any of which may be empty."""
    cuts = np.sort(rng.integers(0, n + 1, size=types - 1))
    return np.diff(np.concatenate([[0], cuts, [n]])).astype(np.int32)


def draw_integer(rng, m, n, types, hi=None):
    """Integer-valued p and d below 2^20 (every product k·p ≤ 1024·2^20 and
    every sum is exact in double); small ranges give heavy ties and p = 0."""
    hi = hi if hi is not None else int(rng.choice([3, 10, 1000, 1 << 20]))
    p = rng.integers(0, hi, size=(m, types)).astype(np.float64)
    d = rng.integers(0, hi, size=m).astype(np.float64)
    return _a(split_workers(rng, n, types), p, d)


def draw_real(rng, m, n, types):
    """Processing times like the trace's (steps / throughput), delays up to 4e4."""
    steps = rng.uniform(1e3, 1e6, size=(m, 1))
    tput = rng.uniform(0.5, 50.0, size=(m, types))
    return _a(split_workers(rng, n, types), steps / tput, rng.uniform(0.0, 4e4, size=m))


def _sizes(rng, count, max_m, max_n):
    for _ in range(count):
        yield int(rng.integers(1, max_m + 1)), int(rng.integers(1, max_n + 1)), int(rng.integers(1, 4))


def integer_instances(count=200, seed=3, max_m=25, max_n=8):
    rng = np.random.default_rng(seed)
    return [draw_integer(rng, m, n, t) for m, n, t in _sizes(rng, count, max_m, max_n)]


def real_instances(count=120, seed=5, max_m=40, max_n=12):
    rng = np.random.default_rng(seed)
    return [draw_real(rng, m, n, t) for m, n, t in _sizes(rng, count, max_m, max_n)]


def gpu_instances(count=200, seed=7, max_m=60, max_n=16):
    """The GPU fuzz set: m ≤ 60, alternately integer- and real-valued."""
    rng = np.random.default_rng(seed)
    return [(draw_integer if k % 2 else draw_real)(rng, m, n, t)
            for k, (m, n, t) in enumerate(_sizes(rng, count, max_m, max_n))]


# (m, n) with m + n at the sizes where a wave, the one-wave path and the
# 512-thread workgroup fill up; n is large where m·m·n has to stay below
# allox_ref.DENSE_CAP for scipy.
BOUNDARY_SIZES = [(40, 23), (41, 23), (41, 24), (12, 51), (13, 51), (13, 52),
                  (60, 195), (60, 196), (60, 197), (91, 420), (92, 420), (90, 423)]


def boundary_instances(seed=9):
    """Two instances per boundary size, one integer- and one real-valued, with
    1, 2 and 3 types in turn."""
    rng = np.random.default_rng(seed)
    out = []
    for k, (m, n) in enumerate(BOUNDARY_SIZES):
        out.append(draw_integer(rng, m, n, 1 + k % 3))
        out.append(draw_real(rng, m, n, 1 + (k + 1) % 3))
    return out


def tall_instances(seed=13):
    """Sizes scipy's dense matrix cannot hold within the cap (twin and GPU
    only): long chains at the 512-slot boundary, and the caps themselves."""
    rng = np.random.default_rng(seed)
    return [draw_real(rng, 447, 64, 3), draw_integer(rng, 448, 64, 2, hi=1000), draw_real(rng, 449, 64, 1),
            draw_real(rng, 250, 7, 2), draw_real(rng, 1024, 1024, 3)]


def real_gap_instances():
    return real_instances() + boundary_instances()[1::2]


def same_bits(a, b):
    """(job_worker, job_position, worker_first, cost) equal, the cost bit for bit."""
    return (np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2])
            and np.float64(a[3]).tobytes() == np.float64(b[3]).tobytes())


# ---- the policy mirror over three calls -------------------------------------------------------
TYPES = ["k80", "v100"]  # sorted, as policy.flatten orders them
SPEC = {"v100": 2, "k80": 1}


def policy_sequence(engine, alpha=1.0):
    """Three consecutive get_allocation calls on a two-type cluster: after
    each, the lowest-id job that holds a worker finishes and a new job
    arrives; the clock moves 120 s.  Returns (the calls' arguments, the
    allocations, the policy)."""
    import allox

    tput = {0: (2.0, 8.0), 1: (1.0, 9.0), 2: (3.0, 3.5), 3: (0.5, 6.0), 4: (4.0, 5.0), 5: (1.5, 7.0),
            6: (2.5, 2.5)}
    steps = {0: 4000, 1: 9000, 2: 1500, 3: 7000, 4: 2500, 5: 6000, 6: 800}
    arrival = {0: 0.0, 1: 60.0, 2: 60.0, 3: 100.0, 4: 130.0, 5: 250.0, 6: 250.0}
    pol = allox.AlloXPolicy(alpha=alpha, native=engine)
    active, waiting_room = [3, 0, 2, 1], [4, 5, 6]  # insertion order is not id order
    calls, out = [], []
    for k in range(3):
        now = 120.0 * (k + 1)
        args = dict(tp={j: dict(zip(TYPES, tput[j])) for j in active}, sf={j: 1 for j in active},
                    tss={j: now - arrival[j] for j in active},
                    steps={j: steps[j] - 300 * k for j in active}, spec=dict(SPEC))
        a = pol.get_allocation(args["tp"], args["sf"], args["tss"], args["steps"], args["spec"])
        calls.append(args)
        out.append({j: dict(r) for j, r in a.items()})
        holders = sorted(j for j in active if sum(a[j].values()) == 1.0)
        active = [j for j in active if j != holders[0]] + [waiting_room[k]]
    return calls, out, pol


# ---- the 30-job simulation ------------------------------------------------------------------------
def simulate_30(engine, record=None, policy="allox"):
    """The first 30 scale-factor-1 jobs of the 120-job trace on 8 GPUs."""
    import sw_sim
    import sw_trace as st

    trace = os.path.join(st.DATA_DIR, "traces",
                         "120_0.2_5_100_40_25_0,0.5,0.5_0.6,0.3,0.09,0.01_multigpu_dynamic.trace")
    tp = st.load_throughputs()
    jobs, arr = st.parse_trace(trace)
    keep = [i for i, j in enumerate(jobs) if j.scale_factor == 1][:30]
    jobs, arr = [jobs[i] for i in keep], [arr[i] for i in keep]
    prof = st.synthesize_profiles(jobs, tp)
    for i, j in enumerate(jobs):
        j.duration = sum(prof[i]["duration_every_epoch"])
    sim = sw_sim.Simulator(policy, tp, prof, 120, allox_allocator=engine)
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
