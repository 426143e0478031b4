"""Wall time per sw_mtd_allocate call (MinTotalDuration allocation on the GPU)
at N = 120, 900, 4,000 and 5,000 jobs on 64 workers, the LDS path against the
L2 path (SW_MTD_LDS=0), and the throughput of sw_mtd_allocate_batch at 4,096
instances of 220 jobs, with the CPU restatement of the reference beside each:
the reference's search with one HiGHS LP per probe (tests/mtd_ref.py
lp_search — the reference ran ECOS, absent here), and the kernel's CPU twin.
Every GPU call is synchronous (it ends in a stream synchronise), so the host
clock around it is the call's time.  Per size: warm-up, then the variants
interleaved call by call, the median per variant.

    python tools/mtd_timing.py [--calls 200] [--out profiles/mtd_timing.json]
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "shockwave-replication_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402

import mtd_ref  # noqa: E402
import sw_native as sn  # noqa: E402

SF_VALUES, SF_WEIGHTS = [1, 2, 4, 8], [0.6, 0.3, 0.09, 0.01]
LDS_JOBS = 4096  # SW_MTD_LDS_JOBS


def draw(rng, n, G):
    """A simulator-like state: steps left log-uniform in 1e1..1e7, throughput
    in 0.5..40."""
    sf = rng.choice(SF_VALUES, size=n, p=SF_WEIGHTS).astype(np.int32)
    steps = np.floor(10.0 ** rng.uniform(1, 7, size=n))
    tp = rng.uniform(0.5, 40.0, size=n)
    return sf, steps, tp, G


def median_us(samples):
    return float(np.median(samples)) * 1e6


def cpu_times(sf, steps, tp, G, reps):
    """(HiGHS-LP search seconds, probes, twin seconds) for one state, medians."""
    p = steps / tp
    lp, tw, probes = [], [], 0
    for _ in range(reps):
        t0 = time.perf_counter()
        T, pr, _ = mtd_ref.lp_search(tp[:, None], sf, steps, [G])
        lp.append(time.perf_counter() - t0)
        probes = len(pr)
        t0 = time.perf_counter()
        r = mtd_ref.twin_allocate(sf, p, G)
        tw.append(time.perf_counter() - t0)
        assert r[1] == T, (r[1], T)
    return float(np.median(lp)), probes, float(np.median(tw))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    s = sn.Solver(device=0)
    rng = np.random.default_rng(0)
    out = {"calls_per_variant": a.calls, "lds_jobs": LDS_JOBS, "single": [], "batch": None}
    for n in (120, 900, 4000, 5000):
        sf, steps, tp, G = draw(rng, n, 64)
        p = steps / tp
        order = [("mtd", "1"), ("mtd_l2", "0")]
        for name, lds in order:  # warm-up of both paths
            os.environ["SW_MTD_LDS"] = lds
            for _ in range(10):
                r = s.mtd_allocate(sf, p, G)
        t = {name: [] for name, _ in order}
        for _ in range(a.calls):
            for name, lds in order:
                os.environ["SW_MTD_LDS"] = lds
                t0 = time.perf_counter()
                s.mtd_allocate(sf, p, G)
                t[name].append(time.perf_counter() - t0)
        os.environ["SW_MTD_LDS"] = "1"
        lp_s, probes, twin_s = cpu_times(sf, steps, tp, G, 3)
        rec = {"jobs": n, "workers": G, "lds_path": n <= LDS_JOBS, "T": r[1], "mu": r[2], "probes": probes}
        rec.update({k + "_us": round(median_us(v), 2) for k, v in t.items()})
        rec["cpu_highs_search_us"] = round(lp_s * 1e6, 1)
        rec["cpu_twin_us"] = round(twin_s * 1e6, 1)
        out["single"].append(rec)
        print(json.dumps(rec), flush=True)
    # the batch: 4,096 instances of 220 jobs, packed once, timed at the C-ABI
    count, n = 4096, 220
    insts = [draw(rng, n, int(rng.integers(8, 129))) for _ in range(count)]
    off = (np.arange(count + 1, dtype=np.int64) * n)
    sf = np.ascontiguousarray(np.concatenate([q[0] for q in insts]))
    p = np.ascontiguousarray(np.concatenate([q[1] / q[2] for q in insts]))
    g = np.array([q[3] for q in insts], dtype=np.int32)
    x = np.zeros(count * n)
    lv = np.zeros((count, 2))
    dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int32)

    def run():
        rc = s.lib.sw_mtd_allocate_batch(s.h, count, off.ctypes.data_as(C.POINTER(C.c_int64)), g.ctypes.data_as(ip),
                                         sf.ctypes.data_as(ip), p.ctypes.data_as(dp), x.ctypes.data_as(dp),
                                         lv.ctypes.data_as(dp))
        assert rc == 0, s.error()

    rec = {"instances": count, "jobs": n}
    for name, lds in (("lds", "1"), ("l2", "0")):
        os.environ["SW_MTD_LDS"] = lds
        for _ in range(2):
            run()
        ts = []
        for _ in range(10):
            t0 = time.perf_counter()
            run()
            ts.append(time.perf_counter() - t0)
        rec[name + "_ms"] = round(float(np.median(ts)) * 1e3, 3)
        rec[name + "_allocations_per_s"] = round(count / float(np.median(ts)))
    os.environ["SW_MTD_LDS"] = "1"
    # the CPU restatement on the first 32 instances of the batch, scaled to the batch
    lp_s = tw_s = 0.0
    sample = 32
    for q in insts[:sample]:
        l, _, w = cpu_times(*q, 1)
        lp_s += l
        tw_s += w
    rec["cpu_sample_instances"] = sample
    rec["cpu_highs_search_ms_per_instance"] = round(lp_s / sample * 1e3, 3)
    rec["cpu_twin_ms_per_instance"] = round(tw_s / sample * 1e3, 3)
    rec["cpu_highs_allocations_per_s"] = round(sample / lp_s, 1)
    out["batch"] = rec
    print(json.dumps(rec), flush=True)
    s.close()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        json.dump(out, open(a.out, "w"), indent=1)


if __name__ == "__main__":
    main()
