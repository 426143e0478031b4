"""Wall time per sw_wf_allocate_types call (water-filling MaxMinFairness over
worker types that differ: every stage's level solve and the repeat of the last
in one launch) with the stages and Newton steps taken, next to
sw_mmf_allocate_types_centred on the first stage's rows of the same inputs in
the same process — the cost of one level solve, so that "time ≈ level solves ×
one centred call" can be read off (level solves = stages, plus the repeat when
there is more than one stage) — and the batched rate at 30 jobs × 3 types.

Each call ends in a stream synchronise, so a host clock around it is the call's
time.  Every shape is warmed up; each figure is the median of WINDOWS windows
of at least MIN_WINDOW_S seconds, with the windows' spread beside it.  A shape
the call refuses (SW_ERR_CAPACITY) is recorded with its error text.
    python tools/wf_types_timing.py [out.json]"""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "shockwave-replication_amd"))
import numpy as np  # noqa: E402

import sw_native as sn  # noqa: E402

SHAPES = [(30, 3), (120, 3), (400, 3), (400, 8)]
BATCH = 256
WINDOWS = 5
MIN_WINDOW_S = 0.25


def instance(rng, m, n):
    """A cluster an eighth to a quarter the size of the demand; scale factors
    and weights as in the tests' family, c_jk = thr_jk / prop_j · (1/w_j)·sf_j."""
    W = rng.integers(m // 16 + 1, m // 8 + 2, size=n).astype(np.int32)
    sf = rng.choice([1, 2, 4, 8], size=m, p=[0.6, 0.3, 0.09, 0.01]).astype(np.int32)
    w = rng.choice([0.5, 1.0, 2.0, 4.0], size=m)
    thr = rng.uniform(0.2, 5.0, size=(m, n)) * rng.uniform(0.5, 2.0, size=n)[None, :]
    x = np.tile(W / m, (m, 1))
    prop = (thr * (x / x.sum(axis=1).max())).sum(axis=1)
    return W, sf, thr / prop[:, None] * ((1.0 / w) * sf)[:, None]


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
        W, sf, c = instance(rng, m, n)
        ms_c, spread_c, (xc, tc, its_c) = timed(s.mmf_allocate_types_centred, (W, sf, c))
        row = {"jobs": m, "types": n, "one_level_solve_ms_per_call": ms_c, "one_level_solve_ms_min_max": spread_c,
               "one_level_solve_newton_steps": its_c, "one_level_solve_level": tc}
        try:
            ms, spread, (x, F, level, its, stages, flags) = timed(s.wf_allocate_types, (W, sf, c))
            solves = stages + (stages > 1)
            row.update({"ms_per_call": ms, "ms_min_max": spread, "stages": stages, "level_solves": solves,
                        "newton_steps": its, "last_level": level, "first_level": float(F.min()), "flags": flags,
                        "ms_over_solves_times_one": ms / (solves * ms_c)})
        except sn.NativeError as e:
            row["error"] = str(e)
        rows.append(row)
    insts = [instance(rng, 30, 3) for _ in range(BATCH)]
    try:
        ms_b, spread_b, out = timed(s.wf_allocate_types_batch, (insts,))
        batch = {"jobs": 30, "types": 3, "instances": BATCH, "ms_per_batch": ms_b, "ms_min_max": spread_b,
                 "allocations_per_s": BATCH / (ms_b * 1e-3), "stages_mean": float(np.mean([o[4] for o in out]))}
    except sn.NativeError as e:
        batch = {"jobs": 30, "types": 3, "instances": BATCH, "error": str(e)}
    res = {"per_call": rows, "batch": batch}
    s.close()
    text = json.dumps(res)
    print(text)
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
