"""Wall time per sw_mtd_allocate_types call (MinTotalDuration over worker types
that differ: the level, the search and the centre in one launch) next to
sw_mmf_allocate_types_centred on the level program's coefficients
(throughput / steps) of the same inputs in the same process, so that the cost
of the search and the centring phase can be read off, with the Newton steps
taken, and the batched rate at 30 jobs × 3 types.
    python tools/mtd_types_timing.py [out.json]"""
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


def instance(rng, m, n):
    W = rng.integers(m // 4 + 1, m // 2 + 2, size=n).astype(np.int32)
    sf = rng.choice([1, 2, 4, 8], size=m, p=[0.6, 0.3, 0.09, 0.01]).astype(np.int32)
    thr = rng.uniform(0.2, 3.0, size=(m, n)) * sf[:, None]
    steps = 10.0 ** rng.uniform(4.0, 6.0, size=m)
    return W, sf, thr, steps


def per_call(fn, args, reps):
    fn(*args)
    t0 = time.perf_counter()
    for _ in range(reps):
        r = fn(*args)
    return (time.perf_counter() - t0) / reps * 1e3, r


def main():
    s = sn.Solver(device=0)
    rng = np.random.default_rng(0)
    rows = []
    for m, n in SHAPES:
        W, sf, thr, steps = instance(rng, m, n)
        reps = 10 if m <= 400 else 3
        ms, (x, T, t, its, flags) = per_call(s.mtd_allocate_types, (W, sf, thr, steps), reps)
        ms_c, (xc, tc, its_c) = per_call(s.mmf_allocate_types_centred, (W, sf, thr / steps[:, None]), reps)
        rows.append({"jobs": m, "types": n, "ms_per_call": ms, "newton_steps": its, "T": T, "level": t,
                     "margin": T * t - 1.0, "flags": flags, "level_only_ms_per_call": ms_c,
                     "level_only_newton_steps": its_c, "level_only_level": tc})
    insts = [instance(rng, 30, 3) for _ in range(BATCH)]
    s.mtd_allocate_types_batch(insts)
    reps = 5
    t0 = time.perf_counter()
    for _ in range(reps):
        s.mtd_allocate_types_batch(insts)
    dt = (time.perf_counter() - t0) / reps
    out = {"per_call": rows,
           "batch": {"jobs": 30, "types": 3, "instances": BATCH, "ms_per_batch": dt * 1e3,
                     "allocations_per_s": BATCH / dt}}
    s.close()
    text = json.dumps(out)
    print(text)
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
