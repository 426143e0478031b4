"""Wall time per sw_wf_allocate call (water-filling MaxMinFairness allocation
on the GPU) at N = 120, 900 and 5,000 jobs on 64 workers, with sw_mmf_allocate
and sw_ftf_allocate (both of their cases) at the same sizes in the same
process, the LDS path against the L2 path (SW_WF_LDS=0), and the throughput of
sw_wf_allocate_batch at 4,096 instances of 220 jobs.  Every call is synchronous
(it ends in a stream synchronise), so the host clock around it is the call's
time.  Per size: warm-up, then the variants interleaved call by call, the
median per variant and its quartiles (the spread the medians are read against).

    python tools/wf_timing.py [--calls 300] [--out profiles/wf_timing.json]
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


def draw_wf(rng, n):
    """Widths with the traces' mix, priority weights log-uniform in 0.25..4."""
    sf = rng.choice(SF_VALUES, size=n, p=SF_WEIGHTS).astype(np.int32)
    return sf, sf / 2.0 ** rng.uniform(-2, 2, size=n)


def draw_ftf(rng, n, G, a_hi):
    """tools/ftf_timing.py draw: a simulator-like FinishTimeFairness state."""
    sf = rng.choice(SF_VALUES, size=n, p=SF_WEIGHTS).astype(np.int32)
    p = 10.0 ** rng.uniform(2, 5, size=n)
    a = np.where(rng.random(n) < 0.3, 0.0, 10.0 ** rng.uniform(1, a_hi, size=n))
    E = rng.uniform(0.0, 1.0, size=n) * a + p * np.maximum(1.0, n * sf / G)
    return sf, p, a, E, G


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=300)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    s = sn.Solver(device=0)
    rng = np.random.default_rng(0)
    out = {"calls_per_variant": a.calls, "single": [], "batch": None}
    for n in (120, 900, 5000):
        sf, c = draw_wf(rng, n)
        part = int(0.6 * sf.sum())  # a cluster on which a part of the jobs saturates
        ftf_binds = draw_ftf(rng, n, 64, 2.0)
        ftf_free = draw_ftf(rng, n, 64, 5.0)
        variants = {
            "wf_64": lambda: s.wf_allocate(sf, c, 64),         # a loaded cluster: few jobs or none saturate
            "wf_part": lambda: s.wf_allocate(sf, c, part),     # the bisection past saturated jobs
            "wf_whole": lambda: s.wf_allocate(sf, c, 16 * n),  # Σ sf ≤ G: one pass, no probe
            "ftf_binds": lambda: s.ftf_allocate(*ftf_binds),
            "ftf_free": lambda: s.ftf_allocate(*ftf_free),
            "mmf_binds": lambda: s.mmf_allocate(sf, c, 64),
            "mmf_free": lambda: s.mmf_allocate(sf, c, part),
        }
        order = [("wf_64", "1"), ("wf_part", "1"), ("wf_whole", "1"), ("wf_64_l2", "0"), ("wf_part_l2", "0"),
                 ("ftf_binds", "1"), ("ftf_free", "1"), ("mmf_binds", "1"), ("mmf_free", "1")]
        res = {}
        for name, lds in order:  # warm-up of every shape and path
            os.environ["SW_WF_LDS"] = lds
            for _ in range(20):
                res[name] = variants[name.replace("_l2", "")]()
        t = {name: [] for name, _ in order}
        for _ in range(a.calls):
            for name, lds in order:
                os.environ["SW_WF_LDS"] = lds
                fn = variants[name.replace("_l2", "")]
                t0 = time.perf_counter()
                fn()
                t[name].append(time.perf_counter() - t0)
        os.environ["SW_WF_LDS"] = "1"
        assert np.all(res["wf_whole"][0] == 1.0) and 0 < (res["wf_part"][0] == 1.0).sum() < n
        assert res["wf_64"][0].tobytes() == res["wf_64_l2"][0].tobytes()
        assert res["wf_part"][0].tobytes() == res["wf_part_l2"][0].tobytes()
        rec = {"jobs": n, "workers": 64, "workers_part": part, "lds_path": n <= 2048,
               "saturated_64": int((res["wf_64"][0] == 1.0).sum()),
               "saturated_part": int((res["wf_part"][0] == 1.0).sum()),
               # which case of the other two kernels ran (μ = 0: capacity binds)
               "ftf_binds_mu": res["ftf_binds"][2], "ftf_free_mu": res["ftf_free"][2],
               "mmf_binds_mu": res["mmf_binds"][2], "mmf_free_mu": res["mmf_free"][2]}
        for k, v in t.items():
            q1, med, q3 = (float(z) * 1e6 for z in np.percentile(v, [25, 50, 75]))
            rec[k + "_us"] = round(med, 2)
            rec[k + "_iqr_us"] = [round(q1, 2), round(q3, 2)]
        out["single"].append(rec)
        print(json.dumps(rec), flush=True)
    # the batch: 4,096 instances of 220 jobs, packed once, timed at the C-ABI
    count, n = 4096, 220
    insts = [draw_wf(rng, n) for _ in range(count)]
    off = (np.arange(count + 1, dtype=np.int64) * n)
    sf, c = (np.ascontiguousarray(np.concatenate([q[k] for q in insts])) for k in range(2))
    g = rng.integers(8, 513, size=count).astype(np.int32)
    x = np.zeros(count * n)
    lv = np.zeros((count, 2))
    dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int32)

    def run():
        rc = s.lib.sw_wf_allocate_batch(s.h, count, off.ctypes.data_as(C.POINTER(C.c_int64)), g.ctypes.data_as(ip),
                                        sf.ctypes.data_as(ip), c.ctypes.data_as(dp), x.ctypes.data_as(dp),
                                        lv.ctypes.data_as(dp))
        assert rc == 0, s.error()

    rec = {"instances": count, "jobs": n, "whole_instances": None}
    for name, lds in (("lds", "1"), ("l2", "0")):
        os.environ["SW_WF_LDS"] = lds
        for _ in range(3):
            run()
        ts = []
        for _ in range(30):
            t0 = time.perf_counter()
            run()
            ts.append(time.perf_counter() - t0)
        rec[name + "_ms"] = round(float(np.median(ts)) * 1e3, 3)
        rec[name + "_allocations_per_s"] = round(count / float(np.median(ts)))
    os.environ["SW_WF_LDS"] = "1"
    rec["whole_instances"] = int((x.reshape(count, n) == 1.0).all(axis=1).sum())
    out["batch"] = rec
    print(json.dumps(rec), flush=True)
    s.close()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        json.dump(out, open(a.out, "w"), indent=1)


if __name__ == "__main__":
    main()
