"""Wall time per sw_mmf_allocate_types_centred call (the worker-type
MaxMinFairness LP by the interior-point kernel, the analytic centre of the
optimal face) next to sw_mmf_allocate_types (the simplex, an optimal vertex) on
the same inputs in the same process, with the Newton steps and the pivots
taken, and the batched rate at 30 jobs × 3 types.
    python tools/mmf_centred_timing.py [out.json]"""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "shockwave-replication_amd"))
import numpy as np  # noqa: E402

import sw_native as sn  # noqa: E402

SHAPES = [(30, 3), (120, 3), (400, 3), (400, 8), (2048, 3)]
CENTRED_ONLY = [(8192, 3)]  # the simplex call stops at 2048 jobs
BATCH = 256


def instance(rng, m, n):
    W = rng.integers(m // 4 + 1, m // 2 + 2, size=n).astype(np.int32)
    sf = rng.choice([1, 2, 4, 8], size=m, p=[0.6, 0.3, 0.09, 0.01]).astype(np.int32)
    return W, sf, rng.uniform(0.2, 3.0, size=(m, n)) * sf[:, None]


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
    for m, n in SHAPES + CENTRED_ONLY:
        inst = instance(rng, m, n)
        reps = 10 if m <= 400 else 3
        ms_c, (xc, tc, steps) = per_call(s.mmf_allocate_types_centred, inst, reps)
        row = {"jobs": m, "types": n, "centred_ms_per_call": ms_c, "newton_steps": steps, "centred_level": tc}
        if (m, n) in SHAPES:
            try:
                ms_v, (xv, tv, piv) = per_call(s.mmf_allocate_types, inst, reps if m <= 400 else 1)
                row.update({"simplex_ms_per_call": ms_v, "pivots": piv, "simplex_level": tv,
                            "level_rel_diff": abs(tc - tv) / max(1.0, tv)})
            except sn.NativeError as e:  # the tableau's 256 MB cap
                row["simplex_error"] = str(e)
        rows.append(row)
    insts = [instance(rng, 30, 3) for _ in range(BATCH)]
    s.mmf_allocate_types_centred_batch(insts)
    reps = 5
    t0 = time.perf_counter()
    for _ in range(reps):
        s.mmf_allocate_types_centred_batch(insts)
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
