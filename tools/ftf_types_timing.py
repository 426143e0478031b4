"""Wall time per sw_ftf_allocate_types call (FinishTimeFairness over worker
types that differ: the start's bisection and every level solve in one launch)
with the level solves and Newton steps taken, next to
sw_mmf_allocate_types_centred on the rows c(ρ*) of the same inputs in the same
process — the cost of one level solve, so that "time ≈ solves × one centred
call" can be read off — sw_ftf_allocate at one type, and the batched rate at
30 jobs × 3 types.

Each call ends in a stream synchronise, so a host clock around it is the call's
time.  Every shape is warmed up; each figure is the median of WINDOWS windows
of at least MIN_WINDOW_S seconds, with the windows' spread beside it.
    python tools/ftf_types_timing.py [out.json]"""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "shockwave-replication_amd"))
import numpy as np  # noqa: E402

import sw_native as sn  # noqa: E402

SHAPES = [(30, 3), (120, 3), (400, 3), (400, 8), (2048, 3)]
BATCH = 256
WINDOWS = 5
MIN_WINDOW_S = 0.25


def instance(rng, m, n):
    """A schedule under way on a cluster a quarter the size of the demand:
    a fifth of the jobs fresh, the others 0–90 % done after 0.3–0.8 times the
    time of the isolated split of the four times larger cluster."""
    W = rng.integers(m // 16 + 1, m // 8 + 2, size=n).astype(np.int32)
    sf = rng.choice([1, 2, 4, 8], size=m, p=[0.6, 0.3, 0.09, 0.01]).astype(np.int32)
    thr = rng.uniform(0.2, 3.0, size=(m, n)) * sf[:, None]
    total = 10.0 ** rng.uniform(4.0, 6.0, size=m)
    x = 4.0 * W[None, :] / m / sf[:, None]
    iso = (thr * x / np.maximum(x.sum(axis=1), 1.0)[:, None]).sum(axis=1)
    done = np.where(rng.random(size=m) < 0.2, 0.0, rng.uniform(0.0, 0.9, size=m))
    return W, sf, thr, total * (1.0 - done), total * done / iso * rng.uniform(0.3, 0.8, size=m), total / iso


def timed(fn, args):
    """(median ms per call, (min, max) over the windows, the last result)."""
    r = fn(*args)
    t0 = time.perf_counter()
    fn(*args)
    one = max(time.perf_counter() - t0, 1e-5)
    reps = max(3, int(MIN_WINDOW_S / one) + 1)
    ms = []
    for _ in range(WINDOWS):
        t0 = time.perf_counter()
        for _ in range(reps):
            r = fn(*args)
        ms.append((time.perf_counter() - t0) / reps * 1e3)
    return float(np.median(ms)), (min(ms), max(ms)), r


def main():
    s = sn.Solver(device=0)
    rng = np.random.default_rng(0)
    rows = []
    for m, n in SHAPES:
        W, sf, thr, steps, a, E = instance(rng, m, n)
        ms, spread, (x, rho, t, its, solves, flags) = timed(s.ftf_allocate_types, (W, sf, thr, steps, a, E))
        c = thr * ((rho * E - a) / steps)[:, None]
        ms_c, spread_c, (xc, tc, its_c) = timed(s.mmf_allocate_types_centred, (W, sf, c))
        rows.append({"jobs": m, "types": n, "ms_per_call": ms, "ms_min_max": spread, "level_solves": solves,
                     "newton_steps": its, "rho": rho, "level": t, "flags": flags,
                     "one_level_solve_ms_per_call": ms_c, "one_level_solve_ms_min_max": spread_c,
                     "one_level_solve_newton_steps": its_c, "one_level_solve_level": tc,
                     "ms_over_solves_times_one": ms / (solves * ms_c)})
    one_type = []
    for m in (30, 400, 2048):
        W, sf, thr, steps, a, E = instance(rng, m, 1)
        ms, spread, (x, rho, mu) = timed(s.ftf_allocate, (sf, steps / thr[:, 0], a, E, int(W[0])))
        ms_t, spread_t, r = timed(s.ftf_allocate_types, (W, sf, thr, steps, a, E))
        one_type.append({"jobs": m, "ftf_allocate_ms_per_call": ms, "ftf_allocate_ms_min_max": spread, "rho": rho,
                         "ftf_allocate_types_ms_per_call": ms_t, "ftf_allocate_types_ms_min_max": spread_t,
                         "ftf_allocate_types_rho": r[1], "level_solves": r[4]})
    insts = [instance(rng, 30, 3) for _ in range(BATCH)]
    ms_b, spread_b, out = timed(s.ftf_allocate_types_batch, (insts,))
    res = {"per_call": rows, "one_type": one_type,
           "batch": {"jobs": 30, "types": 3, "instances": BATCH, "ms_per_batch": ms_b, "ms_min_max": spread_b,
                     "allocations_per_s": BATCH / (ms_b * 1e-3),
                     "level_solves_mean": float(np.mean([o[4] for o in out]))}}
    s.close()
    text = json.dumps(res)
    print(text)
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
