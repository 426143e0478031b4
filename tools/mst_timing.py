"""Wall time per sw_mst_allocate call (max-sum-throughput allocation on the GPU)
at N = 30, 900, 3,072 and 10,000 jobs on a cluster half the jobs' demand, the
LDS path against the global path (SW_MST_LDS=0), and the throughput of
sw_mst_allocate_batch at the same sizes, with the CPU beside each: the
reference's LP through scipy.optimize.linprog (HiGHS; tests/mst_ref.py
lp_optimum — the reference ran ECOS, absent here) on one host core, and the
kernel's CPU twin.  A third of the jobs carry a feasible floor; half of them tie
with jobs of their type and scale factor (tests/mstcases.py draw).
Every GPU call is synchronous (it ends in a stream synchronise), so the host
clock around it is the call's time.  Per size: warm-up, then the variants
interleaved call by call, the median per variant.

    python tools/mst_timing.py [--calls 200] [--out profiles/mst_timing.json]
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

import mst_ref  # noqa: E402
import mstcases as mc  # noqa: E402
import sw_native as sn  # noqa: E402

SIZES = (30, 900, 3072, 10000)
BATCH = {30: 4096, 900: 1024, 3072: 256, 10000: 64}  # instances per batch


def median_us(samples):
    return float(np.median(samples)) * 1e6


def cpu_times(inst, reps):
    """(HiGHS seconds, twin seconds, (θ-probes, multiplier probes)), medians."""
    lp, tw, probes = [], [], []
    for _ in range(reps):
        t0 = time.perf_counter()
        obj, _ = mst_ref.lp_optimum(*inst)
        lp.append(time.perf_counter() - t0)
        t0 = time.perf_counter()
        r = mst_ref.twin_allocate(*inst, probes)
        tw.append(time.perf_counter() - t0)
        assert abs(obj - r[3]) <= 1e-7 * max(1.0, obj), (obj, r[3])
    return float(np.median(lp)), float(np.median(tw)), probes[-1]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    s = sn.Solver(device=0)
    rng = np.random.default_rng(0)
    out = {"calls_per_variant": a.calls, "lds_jobs": mc.LDS_JOBS, "single": [], "batch": []}
    order = [("mst", "1"), ("mst_global", "0")]
    for n in SIZES:
        inst = mc.draw(rng, n, floors="ok", fill=0.5)
        for name, lds in order:  # warm-up of both paths
            os.environ["SW_MST_LDS"] = lds
            for _ in range(10):
                r = s.mst_allocate(*inst)
        t = {name: [] for name, _ in order}
        for _ in range(a.calls):
            for name, lds in order:
                os.environ["SW_MST_LDS"] = lds
                t0 = time.perf_counter()
                s.mst_allocate(*inst)
                t[name].append(time.perf_counter() - t0)
        os.environ["SW_MST_LDS"] = "1"
        lp_s, twin_s, probes = cpu_times(inst, 3)
        assert mc.same_bits(r, mst_ref.twin_allocate(*inst))
        rec = {"jobs": n, "workers": inst[3], "lds_path": n <= mc.LDS_JOBS, "lambda": r[1], "multiplier": r[2],
               "objective": r[3], "theta_probes": probes[0], "multiplier_probes": probes[1]}
        rec.update({k + "_us": round(median_us(v), 2) for k, v in t.items()})
        rec["cpu_highs_us"] = round(lp_s * 1e6, 1)
        rec["cpu_twin_us"] = round(twin_s * 1e6, 1)
        out["single"].append(rec)
        print(json.dumps(rec), flush=True)
    # the batches: packed once, timed at the C-ABI
    dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int32)
    for n in SIZES:
        count = BATCH[n]
        insts = [mc.draw(rng, n, floors="ok", fill=float(rng.uniform(0.2, 0.8))) for _ in range(count)]
        off = (np.arange(count + 1, dtype=np.int64) * n)
        sf = np.ascontiguousarray(np.concatenate([q[0] for q in insts]))
        w = np.ascontiguousarray(np.concatenate([q[1] for q in insts]))
        l = np.ascontiguousarray(np.concatenate([q[2] for q in insts]))
        g = np.array([q[3] for q in insts], dtype=np.int32)
        x = np.zeros(count * n)
        lv = np.zeros((count, 4))

        def run():
            rc = s.lib.sw_mst_allocate_batch(s.h, count, off.ctypes.data_as(C.POINTER(C.c_int64)),
                                             g.ctypes.data_as(ip), sf.ctypes.data_as(ip), w.ctypes.data_as(dp),
                                             l.ctypes.data_as(dp), x.ctypes.data_as(dp), lv.ctypes.data_as(dp))
            assert rc == 0, s.error()

        rec = {"instances": count, "jobs": n}
        ts = {"lds": [], "global": []}
        for lds in ("1", "0"):
            os.environ["SW_MST_LDS"] = lds
            for _ in range(2):
                run()
        for _ in range(10):
            for name, lds in (("lds", "1"), ("global", "0")):
                os.environ["SW_MST_LDS"] = lds
                t0 = time.perf_counter()
                run()
                ts[name].append(time.perf_counter() - t0)
        os.environ["SW_MST_LDS"] = "1"
        for name, v in ts.items():
            rec[name + "_ms"] = round(float(np.median(v)) * 1e3, 3)
            rec[name + "_allocations_per_s"] = round(count / float(np.median(v)))
        # the CPU on the first instances of the batch
        sample = min(count, 8)
        lp_s = tw_s = 0.0
        for q in insts[:sample]:
            a_lp, a_tw, _ = cpu_times(q, 1)
            lp_s += a_lp
            tw_s += a_tw
        rec["cpu_sample_instances"] = sample
        rec["cpu_highs_ms_per_instance"] = round(lp_s / sample * 1e3, 3)
        rec["cpu_twin_ms_per_instance"] = round(tw_s / sample * 1e3, 3)
        rec["cpu_highs_allocations_per_s"] = round(sample / lp_s, 1)
        out["batch"].append(rec)
        print(json.dumps(rec), flush=True)
    s.close()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        json.dump(out, open(a.out, "w"), indent=1)


if __name__ == "__main__":
    main()
