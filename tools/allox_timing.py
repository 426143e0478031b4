"""Wall time per sw_allox_assign call (the AlloX assignment on the GPU) at
(jobs, free workers, types) = (30, 8, 1), (300, 64, 3), (900, 256, 1) and
(900, 256, 3), with p and d staged in LDS (the default) against read from
global memory (SW_ALLOX_STAGE=0), the one-wave path against the 512-thread
path (SW_ALLOX_WAVE_SLOTS=0) where both can run, and the throughput of
sw_allox_assign_batch at (30, 8, 1), with the host beside each: the kernel's
CPU twin, and scipy.optimize.linear_sum_assignment on the reference's dense
m × (m·n) matrix, its construction included (tests/allox_ref.py
dense_optimum), where that matrix fits — (30, 8, 1) and (300, 64, 3).  At
(900, 256, ·) the matrix has 900 · 900 · 256 = 207 M doubles, 1.66 GB: no scipy
figure is taken there.

Costs are real-valued, like the trace's (tests/alloxcases.py draw_real), the
workers split evenly over the types.  Every GPU call is synchronous (it ends
in a stream synchronise), so the host clock around it is the call's time.  Per
point: warm-up, then the variants interleaved call by call, the median per
variant.  Every point runs in a child process of its own under a time limit;
the first point that fails or times out ends the run.

    python tools/allox_timing.py [--out profiles/allox_timing.json]
"""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "shockwave-replication_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402

SINGLE = ((30, 8, 1), (300, 64, 3), (900, 256, 1), (900, 256, 3))
AB = ((30, 8, 1), (192, 64, 3))  # ≤ 256 slots: one wave (default) against 512 threads
BATCH = (30, 8, 1, 4096)
DENSE_FITS = 8_000_000  # entries (64 MB) up to which the dense matrix is built for scipy
POINT_TIMEOUT_S = 300
NO_SCIPY = ("not taken: the reference's dense matrix is m x (m*n) = {} doubles ({:.2f} GB); "
            "scipy needs it in memory, so the reference cannot run this size")


def instance(m, n, types, seed=0):
    import alloxcases as ac
    import allox_ref

    rng = np.random.default_rng(seed)
    steps = rng.uniform(1e3, 1e6, size=(m, 1))
    tput = rng.uniform(0.5, 50.0, size=(m, types))
    free = [n // types + (1 if t < n % types else 0) for t in range(types)]
    assert ac.WAVE_SLOTS == 256
    return allox_ref.arrays(free, steps / tput, rng.uniform(0.0, 4e4, size=m))


def median_us(v):
    return round(float(np.median(v)) * 1e6, 2)


def timed(fn, calls):
    out = []
    for _ in range(calls):
        t0 = time.perf_counter()
        fn()
        out.append(time.perf_counter() - t0)
    return out


def interleaved(s, inst_call, variants, calls, warm):
    """variants: [(name, {environment switch: value})]; returns {name: [seconds]}."""
    def setenv(v):
        for k in ("SW_ALLOX_WAVE_SLOTS", "SW_ALLOX_STAGE"):
            os.environ.pop(k, None)
        os.environ.update(v)
    for _, v in variants:
        setenv(v)
        for _ in range(warm):
            inst_call()
    t = {name: [] for name, _ in variants}
    for _ in range(calls):
        for name, v in variants:
            setenv(v)
            t0 = time.perf_counter()
            inst_call()
            t[name].append(time.perf_counter() - t0)
    setenv({})
    return t


def point_single(m, n, types, ab):
    import alloxcases as ac
    import allox_ref
    import sw_native as sn

    inst = instance(m, n, types)
    s = sn.Solver(device=0)
    steps = []
    t0 = time.perf_counter()
    want = allox_ref.twin_assign(*inst, steps=steps)
    twin_s = time.perf_counter() - t0
    calls, warm = (200, 10) if m <= 300 else (7, 2)
    one_wave = m + n <= ac.WAVE_SLOTS
    variants = [("gpu", {}), ("gpu_p_d_in_global", {"SW_ALLOX_STAGE": "0"})]
    if ab and one_wave:
        variants.append(("gpu_512_threads", {"SW_ALLOX_WAVE_SLOTS": "0"}))
    got = {}

    def call():
        got["r"] = s.allox_assign(*inst)

    t = interleaved(s, call, variants, calls, warm)
    assert ac.same_bits(got["r"], want), "GPU result differs from the twin"
    allox_ref.check_structure(*inst, *got["r"])
    rec = {"jobs": m, "free_workers": n, "types": types, "slots": m + n, "calls": calls,
           "path": "one wave" if one_wave else "512 threads", "search_steps": steps[0], "cost": want[3]}
    for name, v in t.items():
        rec[name + "_us"] = median_us(v)
        rec[name + "_min_us"] = round(min(v) * 1e6, 2)
        rec[name + "_max_us"] = round(max(v) * 1e6, 2)
    rec["gpu_ns_per_search_step"] = round(rec["gpu_us"] * 1e3 / steps[0], 1)
    rec["cpu_twin_us"] = round(twin_s * 1e6, 1)
    if m * m * n <= DENSE_FITS:
        reps = 5 if m <= 30 else 1
        sc = timed(lambda: got.__setitem__("opt", allox_ref.dense_optimum(*inst)), reps)
        rec["cpu_scipy_dense_us"] = median_us(sc)
        rec["scipy_relative_cost_gap"] = abs(want[3] - got["opt"]) / got["opt"]
    else:
        rec["cpu_scipy_dense_us"] = None
        rec["cpu_scipy_dense_note"] = NO_SCIPY.format(m * m * n, m * m * n * 8 / 1e9)
    s.close()
    return rec


def point_batch(m, n, types, count):
    import alloxcases as ac
    import allox_ref
    import sw_native as sn

    insts = [instance(m, n, types, seed=1 + k) for k in range(count)]
    s = sn.Solver(device=0)
    joff = np.arange(count + 1, dtype=np.int64) * m
    woff = np.arange(count + 1, dtype=np.int64) * n
    free = np.zeros((count, 8), dtype=np.int32)
    for k, q in enumerate(insts):
        free[k, :types] = q[0]
    nt = np.full(count, types, dtype=np.int32)
    p = np.ascontiguousarray(np.concatenate([q[1].reshape(-1) for q in insts]))
    d = np.ascontiguousarray(np.concatenate([q[2] for q in insts]))
    jw, jp = np.zeros(count * m, dtype=np.int32), np.zeros(count * m, dtype=np.int32)
    wf = np.zeros(count * n, dtype=np.int32)
    costs = np.zeros(count)
    dp, ip, lp = C.POINTER(C.c_double), C.POINTER(C.c_int32), C.POINTER(C.c_int64)

    def run():  # packed once, timed at the C-ABI
        rc = s.lib.sw_allox_assign_batch(s.h, count, joff.ctypes.data_as(lp), nt.ctypes.data_as(ip),
                                         free.ctypes.data_as(ip), p.ctypes.data_as(dp), d.ctypes.data_as(dp),
                                         jw.ctypes.data_as(ip), jp.ctypes.data_as(ip), wf.ctypes.data_as(ip),
                                         woff.ctypes.data_as(lp), costs.ctypes.data_as(dp))
        assert rc == 0, s.error()

    t = interleaved(s, run, [("one_wave", {}), ("512_threads", {"SW_ALLOX_WAVE_SLOTS": "0"}),
                           ("one_wave_p_d_in_global", {"SW_ALLOX_STAGE": "0"})], 20, 3)
    sample = 16
    tw = []
    for k in range(sample):
        t0 = time.perf_counter()
        w = allox_ref.twin_assign(*insts[k])
        tw.append(time.perf_counter() - t0)
        assert ac.same_bits((jw[k * m:(k + 1) * m], jp[k * m:(k + 1) * m], wf[k * n:(k + 1) * n], costs[k]), w)
    sc = timed(lambda: allox_ref.dense_optimum(*insts[0]), 5)
    rec = {"instances": count, "jobs": m, "free_workers": n, "types": types}
    for name, v in t.items():
        rec[name + "_ms"] = round(float(np.median(v)) * 1e3, 3)
        rec[name + "_assignments_per_s"] = round(count / float(np.median(v)))
    rec["cpu_twin_us_per_instance"] = median_us(tw)
    rec["cpu_scipy_dense_us_per_instance"] = median_us(sc)
    s.close()
    return rec


def child(spec):
    kind, *nums = spec.split(":")
    nums = [int(v) for v in nums]
    rec = point_batch(*nums) if kind == "batch" else point_single(*nums[:3], ab=kind == "ab")
    print("RESULT " + json.dumps(rec), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        return child(a.child)
    out = {"wave_slots": 256, "single": [], "one_wave_vs_512_threads": [], "batch": [], "failed": None}
    points = ([("single", "single:%d:%d:%d" % s) for s in SINGLE]
              + [("one_wave_vs_512_threads", "ab:%d:%d:%d" % s) for s in AB]
              + [("batch", "batch:%d:%d:%d:%d" % BATCH)])
    for key, spec in points:
        try:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", spec], capture_output=True,
                               text=True, timeout=POINT_TIMEOUT_S)
        except subprocess.TimeoutExpired:
            out["failed"] = {"point": spec, "reason": "time limit of %d s" % POINT_TIMEOUT_S}
            break
        lines = [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")]
        if r.returncode != 0 or not lines:
            out["failed"] = {"point": spec, "returncode": r.returncode, "stderr": r.stderr[-2000:]}
            break  # nothing more is started on the GPU after a failure
        rec = json.loads(lines[-1][len("RESULT "):])
        out[key].append(rec)
        print(spec, json.dumps(rec), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        json.dump(out, open(a.out, "w"), indent=1)
    if out["failed"]:
        print("FAILED", json.dumps(out["failed"]), flush=True)
        sys.exit(1)


if __name__ == "__main__":
    main()
