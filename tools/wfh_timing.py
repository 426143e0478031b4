"""Wall time per sw_wfh_allocate call (hierarchical water filling on the GPU)
at (jobs, entities) = (30, 3), (300, 10), (900, 30), (900, 900 singletons),
(900, 1) and (3,072, 64), all-fairness, all-fifo and mixed modes, with
sw_wf_allocate at the same jobs in the same process as the yardstick, and the
throughput of sw_wfh_allocate_batch at 4,096 instances of (30, 3).  Every call
is synchronous (it ends in a stream synchronise), so the host clock around it
is the call's time.  Per shape: warm-up, then the variants interleaved call by
call, the median per variant and its quartiles (the spread the medians are
read against).  The cluster holds 60 % of the demand, so that the outer and
the inner searches both run.

    python tools/wfh_timing.py [--calls 300] [--out profiles/wfh_timing.json]
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "shockwave-replication_amd"))
import numpy as np  # noqa: E402

import sw_native as sn  # noqa: E402

SF_VALUES, SF_WEIGHTS = [1, 2, 4, 8], [0.6, 0.3, 0.09, 0.01]
SHAPES = ((30, 3), (300, 10), (900, 30), (900, 900), (900, 1), (3072, 64))


def draw(rng, n, E):
    """Widths with the traces' mix, priority weights log-uniform in 0.25..4,
    entity weights in 1..5; E = n: singletons, else random membership with
    every entity present."""
    sf = rng.choice(SF_VALUES, size=n, p=SF_WEIGHTS).astype(np.int32)
    c = sf / 2.0 ** rng.uniform(-2, 2, size=n)
    ent = rng.permutation(n) if E == n else np.concatenate([np.arange(E), rng.integers(0, E, size=n - E)])
    W = rng.integers(1, 6, size=E).astype(np.float64)
    return sf, c, ent.astype(np.int32), W


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=300)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    s = sn.Solver(device=0)
    rng = np.random.default_rng(0)
    out = {"calls_per_variant": a.calls, "single": [], "batch": None}
    for n, E in SHAPES:
        sf, c, ent, W = draw(rng, n, E)
        G = int(0.6 * sf.sum())
        modes = {"fairness": np.zeros(E, dtype=np.int32), "fifo": np.ones(E, dtype=np.int32),
                 "mixed": (np.arange(E) % 2).astype(np.int32)}
        variants = {"wfh_" + k: (lambda m=m: s.wfh_allocate(sf, c, ent, W, m, G)) for k, m in modes.items()}
        variants["wfh_whole"] = lambda: s.wfh_allocate(sf, c, ent, W, modes["fairness"], 16 * n)  # Σ sf ≤ G: no probe
        variants["wf_flat"] = lambda: s.wf_allocate(sf, c, G)
        res = {}
        for name, fn in variants.items():  # warm-up of every shape
            for _ in range(20):
                res[name] = fn()
        t = {name: [] for name in variants}
        for _ in range(a.calls):
            for name, fn in variants.items():
                t0 = time.perf_counter()
                fn()
                t[name].append(time.perf_counter() - t0)
        assert np.all(res["wfh_whole"][0] == 1.0)
        rec = {"jobs": n, "entities": E, "workers": G,
               "saturated_entities": int((res["wfh_fairness"][1] >= np.bincount(ent, weights=sf, minlength=E)).sum()),
               "saturated_jobs_fairness": int((res["wfh_fairness"][0] == 1.0).sum()),
               "saturated_jobs_flat": int((res["wf_flat"][0] == 1.0).sum())}
        for k, v in t.items():
            q1, med, q3 = (float(z) * 1e6 for z in np.percentile(v, [25, 50, 75]))
            rec[k + "_us"] = round(med, 2)
            rec[k + "_iqr_us"] = [round(q1, 2), round(q3, 2)]
        out["single"].append(rec)
        print(json.dumps(rec), flush=True)
    # the batch: 4,096 instances of (30, 3), mixed modes, packed once, timed at the C-ABI
    count, n, E = 4096, 30, 3
    insts = [draw(rng, n, E) for _ in range(count)]
    off = np.arange(count + 1, dtype=np.int64) * n
    eoff = np.arange(count + 1, dtype=np.int64) * E
    sf, c, ent, W = (np.ascontiguousarray(np.concatenate([q[k] for q in insts])) for k in range(4))
    modes = np.ascontiguousarray(np.tile(np.array([0, 1, 0], dtype=np.int32), count))
    g = np.array([max(1, int(0.6 * q[0].sum())) for q in insts], dtype=np.int32)
    x, cap, lv = np.zeros(count * n), np.zeros(count * E), np.zeros((count, 2))
    dp, ip, lp = C.POINTER(C.c_double), C.POINTER(C.c_int32), C.POINTER(C.c_int64)

    def run_wfh():
        rc = s.lib.sw_wfh_allocate_batch(s.h, count, off.ctypes.data_as(lp), eoff.ctypes.data_as(lp),
                                         g.ctypes.data_as(ip), sf.ctypes.data_as(ip), c.ctypes.data_as(dp),
                                         ent.ctypes.data_as(ip), W.ctypes.data_as(dp), modes.ctypes.data_as(ip),
                                         x.ctypes.data_as(dp), cap.ctypes.data_as(dp), lv.ctypes.data_as(dp))
        assert rc == 0, s.error()

    def run_wf():
        rc = s.lib.sw_wf_allocate_batch(s.h, count, off.ctypes.data_as(lp), g.ctypes.data_as(ip),
                                        sf.ctypes.data_as(ip), c.ctypes.data_as(dp), x.ctypes.data_as(dp),
                                        lv.ctypes.data_as(dp))
        assert rc == 0, s.error()

    rec = {"instances": count, "jobs": n, "entities": E}
    for name, run in (("wfh", run_wfh), ("wf_flat", run_wf)):
        for _ in range(3):
            run()
        ts = []
        for _ in range(30):
            t0 = time.perf_counter()
            run()
            ts.append(time.perf_counter() - t0)
        rec[name + "_ms"] = round(float(np.median(ts)) * 1e3, 3)
        rec[name + "_allocations_per_s"] = round(count / float(np.median(ts)))
    out["batch"] = rec
    print(json.dumps(rec), flush=True)
    s.close()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        json.dump(out, open(a.out, "w"), indent=1)


if __name__ == "__main__":
    main()
