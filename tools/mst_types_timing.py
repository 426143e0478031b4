"""Wall time per sw_mst_allocate_types call (max sum throughput over worker
types that differ: the transportation problem by successive best paths in one
launch; host checks and copies included, every call ends in a stream
synchronise) with its augmentations and row recomputations, next to HiGHS
(scipy.optimize.linprog, one core) on the same LP and to sw_mst_allocate (one
worker type) at the same job counts in the same process, and the batched rate
at 30 jobs × 3 types.  Every shape is warmed up; a figure is the median of
WINDOWS windows of at least MIN_WINDOW seconds each, with the windows' spread.
    python tools/mst_types_timing.py [out.json]    (default profiles/mst_types_timing.json)"""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "shockwave-replication_amd"))
import numpy as np  # noqa: E402
from scipy.optimize import linprog  # noqa: E402
from scipy.sparse import identity, kron, vstack  # noqa: E402

import sw_native as sn  # noqa: E402

SHAPES = [(30, 3), (120, 3), (400, 3), (400, 8), (2048, 3)]
BATCH = 256
WINDOWS = 5
MIN_WINDOW = 0.2


def instance(rng, m, n):
    sf = rng.choice([1, 2, 4, 8], size=m, p=[0.6, 0.3, 0.09, 0.01]).astype(np.int32)
    W = np.maximum(rng.multinomial(int(sf.sum() / 1.6), np.ones(n) / n), 1).astype(np.int32)  # capacity binds
    w = rng.uniform(0.2, 3.0, size=(m, n)) * sf[:, None] * np.linspace(0.6, 1.8, n)[None, :]
    return W, sf, w


def timed(fn):
    """(median ms per call, (min, max) ms over the windows, last result)"""
    r = fn()
    t0 = time.perf_counter()
    r = fn()
    reps = max(1, int(MIN_WINDOW / max(time.perf_counter() - t0, 1e-6)))
    ms = []
    for _ in range(WINDOWS):
        t0 = time.perf_counter()
        for _ in range(reps):
            r = fn()
        ms.append((time.perf_counter() - t0) / reps * 1e3)
    return float(np.median(ms)), (min(ms), max(ms)), r


def highs(W, sf, w):
    m, n = w.shape
    A = vstack([kron(identity(m), np.ones((1, n))), kron(sf.astype(np.float64).reshape(1, m), identity(n))],
               format="csr")
    b = np.concatenate([np.ones(m), W.astype(np.float64)])
    r = linprog(-w.ravel(), A_ub=A, b_ub=b, bounds=(0, None), method="highs")
    assert r.status == 0, r.message
    return -float(r.fun)


def main():
    s = sn.Solver(device=0)
    rng = np.random.default_rng(0)
    rows = []
    for m, n in SHAPES:
        W, sf, w = instance(rng, m, n)
        ms, spread, (x, prices, obj, augs, nrows, flags) = timed(lambda: s.mst_allocate_types(W, sf, w))
        ms_h, spread_h, obj_h = timed(lambda: highs(W, sf, w))
        ms_1, spread_1, _ = timed(lambda: s.mst_allocate(sf, w[:, 0], None, int(W.sum())))
        rows.append({"jobs": m, "types": n, "ms_per_call": ms, "ms_min_max": spread, "augmentations": augs,
                     "row_recomputations": nrows, "flags": flags, "objective": obj,
                     "highs_ms_per_call": ms_h, "highs_ms_min_max": spread_h,
                     "objective_rel_diff_to_highs": abs(obj - obj_h) / obj_h,
                     "one_type_ms_per_call": ms_1, "one_type_ms_min_max": spread_1})
    insts = [instance(rng, 30, 3) for _ in range(BATCH)]
    ms_b, spread_b, _ = timed(lambda: s.mst_allocate_types_batch(insts))
    out = {"per_call": rows,
           "batch": {"jobs": 30, "types": 3, "instances": BATCH, "ms_per_batch": ms_b, "ms_min_max": spread_b,
                     "allocations_per_s": BATCH / (ms_b * 1e-3)}}
    s.close()
    text = json.dumps(out)
    print(text)
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "mst_types_timing.json")
    with open(path, "w") as f:
        f.write(text + "\n")


if __name__ == "__main__":
    main()
