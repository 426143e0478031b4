"""Wall time per sw_ftf_allocate call (FinishTimeFairness allocation on the
GPU) at N = 120, 900 and 5,000 jobs on 64 workers, with sw_mmf_allocate at the
same sizes in the same process for scale, the LDS path against the L2 path
(SW_FTF_LDS=0), and the throughput of sw_ftf_allocate_batch at 4,096 instances
of 220 jobs.  Every call is synchronous (it ends in a stream synchronise), so
the host clock around it is the call's time.  Per size: warm-up, then the
variants interleaved call by call, the median per variant.

    python tools/ftf_timing.py [--calls 400] [--out profiles/ftf_timing.json]
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


def draw(rng, n, G, a_hi):
    """A simulator-like state: remaining time p, elapsed a (up to 10^a_hi s),
    isolated time E a mix of a and p·max(1, n·sf/G)."""
    sf = rng.choice(SF_VALUES, size=n, p=SF_WEIGHTS).astype(np.int32)
    p = 10.0 ** rng.uniform(2, 5, size=n)
    a = np.where(rng.random(n) < 0.3, 0.0, 10.0 ** rng.uniform(1, a_hi, size=n))
    E = rng.uniform(0.0, 1.0, size=n) * a + p * np.maximum(1.0, n * sf / G)
    return sf, p, a, E, G


def median_us(samples):
    return float(np.median(samples)) * 1e6


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=400)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    s = sn.Solver(device=0)
    rng = np.random.default_rng(0)
    out = {"calls_per_variant": a.calls, "single": [], "batch": None}
    for n in (120, 900, 5000):
        binds = draw(rng, n, 64, 2.0)   # short histories: capacity binds (ρ-bisection)
        free = draw(rng, n, 64, 5.0)    # a long-running job sets ρ_box: the free face (μ-bisection)
        sf = binds[0]
        variants = {
            "ftf_binds": lambda: s.ftf_allocate(*binds),
            "ftf_free": lambda: s.ftf_allocate(*free),
            "mmf_binds": lambda: s.mmf_allocate(sf, sf.astype(np.float64), 64),
            "mmf_free": lambda: s.mmf_allocate(sf, sf.astype(np.float64) * (1.0 + np.arange(n) % 3), 16 * n),
        }
        order = [("ftf_binds", "1"), ("ftf_free", "1"), ("ftf_binds_l2", "0"), ("ftf_free_l2", "0"),
                 ("mmf_binds", "1"), ("mmf_free", "1")]
        mus = {}
        for name, lds in order:  # warm-up of every shape and path
            os.environ["SW_FTF_LDS"] = lds
            for _ in range(20):
                r = variants[name.replace("_l2", "")]()
            mus[name] = r[2]
        t = {name: [] for name, _ in order}
        for _ in range(a.calls):
            for name, lds in order:
                os.environ["SW_FTF_LDS"] = lds
                fn = variants[name.replace("_l2", "")]
                t0 = time.perf_counter()
                fn()
                t[name].append(time.perf_counter() - t0)
        os.environ["SW_FTF_LDS"] = "1"
        assert mus["ftf_binds"] == 0.0 and mus["ftf_free"] > 0.0, mus
        assert mus["mmf_binds"] == 0.0 and mus["mmf_free"] > 0.0, mus
        rec = {"jobs": n, "workers": 64, "lds_path": n <= 2048}
        rec.update({k + "_us": round(median_us(v), 2) for k, v in t.items()})
        out["single"].append(rec)
        print(json.dumps(rec), flush=True)
    # the batch: 4,096 instances of 220 jobs, packed once, timed at the C-ABI
    count, n = 4096, 220
    insts = [draw(rng, n, int(rng.integers(8, 129)), 2.0 if i % 2 else 5.0) for i in range(count)]
    off = (np.arange(count + 1, dtype=np.int64) * n)
    sf, p, el, E = (np.ascontiguousarray(np.concatenate([q[k] for q in insts])) for k in range(4))
    g = np.array([q[4] for q in insts], dtype=np.int32)
    x = np.zeros(count * n)
    lv = np.zeros((count, 2))
    dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int32)

    def run():
        rc = s.lib.sw_ftf_allocate_batch(s.h, count, off.ctypes.data_as(C.POINTER(C.c_int64)), g.ctypes.data_as(ip),
                                         sf.ctypes.data_as(ip), p.ctypes.data_as(dp), el.ctypes.data_as(dp),
                                         E.ctypes.data_as(dp), x.ctypes.data_as(dp), lv.ctypes.data_as(dp))
        assert rc == 0, s.error()

    rec = {"instances": count, "jobs": n, "binding_instances": None}
    for name, lds in (("lds", "1"), ("l2", "0")):
        os.environ["SW_FTF_LDS"] = lds
        for _ in range(3):
            run()
        ts = []
        for _ in range(30):
            t0 = time.perf_counter()
            run()
            ts.append(time.perf_counter() - t0)
        rec[name + "_ms"] = round(float(np.median(ts)) * 1e3, 3)
        rec[name + "_allocations_per_s"] = round(count / float(np.median(ts)))
    os.environ["SW_FTF_LDS"] = "1"
    rec["binding_instances"] = int((lv[:, 1] == 0.0).sum())
    out["batch"] = rec
    print(json.dumps(rec), flush=True)
    s.close()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        json.dump(out, open(a.out, "w"), indent=1)


if __name__ == "__main__":
    main()
