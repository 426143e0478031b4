"""The GPU side of tests/test_gpu_loop_split.py: a separate process, because the
library reads its path thresholds once per process.  The parent starts it with
SW_LOOP_MIN=1 and SW_SPLIT_MIN=1, so that even these small batches run the pack
stage as the sort, round-loop and place kernels (csrc/sw_api.hip
loop_min_count).  Solves the batches below through sw_native.Solver and writes
every result field of every instance to <outdir>/<case>.npz.

    python tests/loop_split_worker.py <outdir>

The batches are built here so that the parent (which imports this module)
compares the same instances with the CPU twin.
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (os.path.join(ROOT, "shockwave-replication_amd"), os.path.join(ROOT, "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

SCALARS = ("objective", "utility", "makespan", "p2_objective", "bound")
# the sizes of test_gpu_split_pack_loop_widths_match_twin (tests/test_gpu_fuzz.py)
SYNTH_SIZES = [(60, 32), (150, 64), (300, 96), (420, 128), (600, 160), (900, 256), (1024, 384),
               (1024, 512)]
FUZZ_SEEDS = range(110)  # those with T ≤ 32: 68 instances


def main_batch():
    """Mixed N, T, G and widths (unaligned job offsets), the eight C3-shaped
    sizes, and one-job and 1,024-job corner instances."""
    import sw_synth as ss
    from fuzzcases import fuzz_problem

    probs = [a for a in (fuzz_problem(s) for s in FUZZ_SEEDS) if a.T <= 32]
    probs += [ss.synth_problem(7000 + i, *sz) for i, sz in enumerate(SYNTH_SIZES)]
    for s in range(400, 500):  # the first one-job and 1,024-job fuzz instances with T ≤ 32
        a = fuzz_problem(s, max_n=1, min_n=1)
        if a.T <= 32 and a.G >= a.w[0]:
            probs.append(a)
            break
    for s in range(500, 600):
        a = fuzz_problem(s, max_n=1024, min_n=1024)
        if a.T <= 32:
            probs.append(a)
            break
    return probs


def stale_batches():
    """Two batches for one handle: many positions per instance, then few."""
    import sw_synth as ss
    from fuzzcases import fuzz_problem

    large = [ss.synth_problem(7100 + i, *SYNTH_SIZES[5 + i % 2]) for i in range(4)]
    small = [ss.synth_problem(7200 + i, *SYNTH_SIZES[i % 2]) for i in range(4)]
    small += [a for a in (fuzz_problem(s) for s in range(20)) if a.T <= 32 and a.N <= 128]
    return large, small


def save(path, batch, results, masks):
    out = {}
    for i, (a, r) in enumerate(zip(batch, results)):
        out[f"plan{i}"] = r["plan"]
        out[f"cnt{i}"] = r["planned_rounds"]
        out[f"scal{i}"] = np.array([r[x] for x in SCALARS], dtype=np.float64)
        out[f"meta{i}"] = np.array([r["rc"], r["status"], r["iters"]], dtype=np.int64)
        if masks:
            out[f"masks{i}"] = r["plan_masks"]
    np.savez(path, **out)


def load(path, i, masks):
    """Instance i of a saved case as a result dict (helpers.assert_same_result)."""
    z = np.load(path)
    r = {"plan": z[f"plan{i}"], "planned_rounds": z[f"cnt{i}"]}
    r.update({x: float(v) for x, v in zip(SCALARS, z[f"scal{i}"])})
    r["rc"], r["status"], r["iters"] = (int(v) for v in z[f"meta{i}"])
    if masks:
        r["plan_masks"] = z[f"masks{i}"]
    return r


def main():
    outdir = sys.argv[1]
    assert os.environ.get("SW_LOOP_MIN") == "1" and os.environ.get("SW_SPLIT_MIN") == "1"
    import sw_native as sn

    batch = main_batch()
    s = sn.Solver(device=0)
    s.upload(batch)
    for keep in (False, True):
        s.keep_masks(keep)
        s.run()
        save(os.path.join(outdir, f"keep{int(keep)}.npz"), batch, s.download(masks=keep), keep)
    s.close()
    large, small = stale_batches()
    s = sn.Solver(device=0)
    s.upload(large)
    s.run()
    save(os.path.join(outdir, "stale_large.npz"), large, s.download(), False)
    s.upload(small)
    s.run()
    save(os.path.join(outdir, "stale_small.npz"), small, s.download(), False)
    s.close()


if __name__ == "__main__":
    main()
