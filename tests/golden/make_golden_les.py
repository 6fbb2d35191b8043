#!/usr/bin/env python3
"""Regenerates tests/golden/les_it1.npz and les_it3.npz (run from the repo root: python tests/golden/make_golden_les.py).

What is pinned: the outputs of the CPU checker tools/les_ref.c (LabelEquivalenceSeg::labelImage, 10 rounds, pi/8, 150 mm)
on the labels, centres and normals stored in nasp_it1.npz / nasp_it3.npz (320 x 240, 10 x 10 superpixels).  Labels are
stored as int16, float outputs as their bit patterns, as the NASP goldens.  These pin the restatement, not the CUDA binary.
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

HERE = os.path.dirname(os.path.abspath(__file__))


def main():
    from tools import les_ref
    f32 = lambda a: np.ascontiguousarray(a, np.float32).view(np.uint32)
    for it in (1, 3):
        g = np.load(os.path.join(HERE, f"nasp_it{it}.npz"))
        normals, centers = g["normals"].view(np.float32).reshape(-1, 3), g["centers"].view(np.float32).reshape(-1, 3)
        o = les_ref.label_image(normals, g["labels"].astype(np.int32), centers)
        path = os.path.join(HERE, f"les_it{it}.npz")
        np.savez_compressed(path, merged_label=o["merged_label"].astype(np.int16), merged_nd=f32(o["merged_nd"]),
                            input_nd=f32(o["input_nd"]), size=o["size"], variance=f32(o["variance"]), changed=o["changed"])
        print(path, os.path.getsize(path), "bytes; regions:", len(set(np.unique(o["merged_label"]).tolist()) - {-1}),
              "changed per round:", o["changed"].tolist())


if __name__ == "__main__":
    main()
