#!/usr/bin/env python3
"""Records the CPU twin's output of sw_mmf_allocate_types_centred at the eight
shapes of tests/test_gpu_mmf_centre.py and its two degenerate cases into
tests/golden/mmfc_bits.json: the allocation as hex, the level, the Newton
steps.  tests/test_mtd_types.py holds the twin to the record, so that a change
to csrc/sw_mmf_ipm.h that moves a bit of the centred MaxMinFairness call is seen.

Run it only on a commit whose sw_mmf_ipm.h is the one to be pinned:
    python tools/mmfc_bits_record.py
"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "oracle"))

SHAPES = [(1, 1), (1, 3), (2, 2), (5, 3), (33, 8), (40, 16), (513, 2), (1100, 3)]
NAMES = [f"{m}x{n}" for m, n in SHAPES] + ["zero_worker", "level_zero"]


def inputs(name):
    import mmfccases as mc

    if name == "zero_worker":
        return mc.zero_worker_case()
    if name == "level_zero":
        return mc.level_zero_case()
    m, n = name.split("x")
    return mc.shaped(int(m), int(n))


def record(name):
    import mmfccases as mc

    x, t, its = mc.twin_allocate(*inputs(name))
    bits = np.ascontiguousarray(x).view(np.uint64).ravel()
    return {"x": "".join(f"{int(b):016x}" for b in bits), "level": float(t).hex(), "steps": int(its)}


def main():
    out = {name: record(name) for name in NAMES}
    path = os.path.join(ROOT, "tests", "golden", "mmfc_bits.json")
    with open(path, "w") as f:
        json.dump(out, f, indent=0, sort_keys=True)
        f.write("\n")
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
