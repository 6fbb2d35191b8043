#!/usr/bin/env python3
"""Regenerates tests/golden/proj_it1.npz (run from the repo root: python tests/golden/make_golden_proj.py).

What is pinned: the outputs of the CPU checker tools/proj_ref.c (five-argument Projection_GPU::PlaneProjection, reference
constants) on LabelEquivalenceSeg's outputs stored in les_it1.npz, cropped to 160 x 120, plus the synthetic points of
tests/proj_cases.golden_inputs().  Floats are stored as their bit patterns, as the other goldens.  This pins the
restatement, not the CUDA binary.
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

HERE = os.path.dirname(os.path.abspath(__file__))


def main():
    import proj_cases as PC
    from tools import proj_ref
    f32 = lambda a: np.ascontiguousarray(a, np.float32).view(np.uint32)
    case = PC.golden_inputs(generate=True)
    o = proj_ref.plane_projection(*case)
    b = PC.branch_counts(o, case[3], case[1], case[2], case[4], PC.MIN_SIZE)
    path = os.path.join(HERE, "proj_it1.npz")
    np.savez_compressed(path, points=f32(case[3]), plane_fitted=f32(o["plane_fitted"]), prefilter_z=f32(o["prefilter"][..., 2]),
                        optimized_z=f32(o["optimized"][..., 2]),
                        branches=np.array([b[k] for k in ("projected", "kept", "replaced", "blended", "small_region")]))
    print(path, os.path.getsize(path), "bytes; branches:", b)


if __name__ == "__main__":
    main()
