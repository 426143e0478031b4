"""The GPU side of tests/test_gpu_place_rank.py: a separate process, because the
library reads its path thresholds once per process.  The parent starts it with
SW_SPLIT_MIN=1 and SW_LOOP_MIN=1 (the pack stage as sort, round-loop and place
kernels) or a large SW_LOOP_MIN (the fused pack kernel).  Solves the batch
below through sw_native.Solver and writes every result field of every instance
to <outdir>/<name>.npz (tests/loop_split_worker.py save / load).

    python tests/place_rank_worker.py <outdir> <name>

The batch is built here so that the parent (which imports this module)
compares the same instances with the CPU twin.
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (os.path.join(ROOT, "shockwave-replication_amd"), os.path.join(ROOT, "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

N, G, T = 120, 32, 30
SEEDS = list(range(9000, 9010)) + [9024]  # plain, repaired, exchanged and one the pack stage leaves to the full kernel
NEAR_TIE_SEED = 9100


def near_tie_problem(seed=NEAR_TIE_SEED):
    """Jobs in pairs (2i, 2i + 1) with the same inputs but the priority: p of
    2i has its 11 lowest mantissa bits clear, p of 2i + 1 one of bits 4 … 9 set.
    With equal counts their p/n differ by tens of ulps: the density key (the
    ratio without its 11 lowest bits) mostly ties and puts 2i first, the
    exchange key (without the 3 lowest) puts 2i + 1 first."""
    import sw_synth as ss
    from sw_native import ProblemArrays

    w, d, F, E, R, p = ss.synth_arrays(seed, N, G, T)
    rng = np.random.default_rng(seed)
    pb = p.view(np.uint64).copy()
    for i in range(0, N, 2):
        for x in (w, d, F, E, R):
            x[i + 1] = x[i]
        pb[i] &= ~np.uint64(0x7FF)
        pb[i + 1] = pb[i] | np.uint64(1 << int(rng.integers(4, 10)))
    return ProblemArrays(w, d, F, E, R, pb.view(np.float64), T, G, 120.0, 1e5, ss.BASES)


def batch():
    import sw_synth as ss

    return [ss.synth_problem(s, N, G, T) for s in SEEDS] + [near_tie_problem()]


def main():
    outdir, name = sys.argv[1], sys.argv[2]
    assert os.environ.get("SW_SPLIT_MIN") == "1" and os.environ.get("SW_LOOP_MIN")
    import loop_split_worker as lw
    import sw_native as sn

    probs = batch()
    s = sn.Solver(device=0)
    s.upload(probs)
    s.keep_masks(True)
    s.run()
    lw.save(os.path.join(outdir, name + ".npz"), probs, s.download(masks=True), True)
    s.close()


if __name__ == "__main__":
    main()
