"""Throughput of NormalAdaptiveSuperpixel (nasp_kernels.hip) on the MI355X, with DepthAdaptiveSuperpixel at the same geometry
as the yardstick and the CPU checker as the baseline.

    python tools/bench_nasp.py [--steps K] [--out profiles/nasp_bench.json] [--quick]

Reports, for Segmentation(10, 50, 50, 150, it) with it = 1 and 5 at 64 x 640x480 and 8 x 1920x1080 (rows 15, cols 20): ms per
batch call, ms per frame and Gpixel/s (median of K timed calls after a wake-up load and warm-up, HIP events on the current
stream); kde_dasp_segmentation(10, 50, 50, it) on one frame of the same size (it has no batched form: ms per frame of a
single-frame call, launch overhead included); and the single-thread time of tools/nasp_ref.c on one frame.  --quick runs one
timed call per case, for a profiler run of its own (rocprofv3 --kernel-trace --stats -- python tools/bench_nasp.py --quick).
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CASES = [(64, 640, 480), (8, 1920, 1080)]
ROWS, COLS = 15, 20
SIGMAS = (10.0, 50.0, 50.0, 150.0)       # KinectDepthEnhancement.cpp:67


def frame(seed, W, H):
    from kinectdepthmapenhancement_amd import synth
    from oracle import oracle as O
    from tools import normals_ref
    bgr, depth = synth.make_frame(seed, W, H)
    pts = O.p2r_depth(depth, synth.intrinsics(W, H)).view(np.float32).reshape(H, W, 3).copy()
    nrm, _, _ = normals_ref.normals(pts, normals_ref.CM, want_band=False)
    return np.ascontiguousarray(bgr), pts, np.ascontiguousarray(nrm)


def timed(torch, fn, steps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(steps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ts.append(e0.elapsed_time(e1))
    return float(np.median(ts)), float(min(ts))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--quick", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.quick:
        a.steps, a.warmup = 1, 1
    import torch
    from kinectdepthmapenhancement_amd import filters, synth
    from tools import nasp_ref as R
    from tools.wake import wake
    torch.cuda.set_device(0)
    res = {"device": torch.cuda.get_device_name(0), "steps": a.steps, "rows": ROWS, "cols": COLS, "sigmas": SIGMAS, "nasp": [],
           "dasp_single_frame": [], "cpu_checker": []}
    for n, W, H in CASES:
        frames = [frame(s, W, H) for s in (1, 2)]
        dev = [torch.from_numpy(np.stack([frames[k % 2][j] for k in range(n)])).cuda() for j in range(3)]
        K = synth.intrinsics(W, H)
        sp = filters.NormalAdaptiveSuperpixel(W, H, max_batch=n)
        sp.SetParametor(ROWS, COLS, K)
        dasp = filters.DepthAdaptiveSuperpixel(W, H)
        dasp.SetParametor(ROWS, COLS, K)
        wake(torch)
        for it in (1, 5):
            ms, ms_min = timed(torch, lambda: sp.segmentation_batch(*dev, *SIGMAS, it), a.steps, a.warmup)
            px = n * W * H
            res["nasp"].append({"frames": n, "width": W, "height": H, "iteration": it, "ms_per_call": round(ms, 4),
                                "ms_per_frame": round(ms / n, 5), "gpixel_per_s": round(px / (ms * 1e-3) / 1e9, 3),
                                "ms_min": round(ms_min, 4)})
            print(json.dumps(res["nasp"][-1]), flush=True)
            ms, ms_min = timed(torch, lambda: dasp.Segmentation(dev[0][0], dev[1][0], SIGMAS[0], SIGMAS[1], SIGMAS[2], it),
                               a.steps, a.warmup)
            res["dasp_single_frame"].append({"width": W, "height": H, "iteration": it, "ms_per_frame": round(ms, 5),
                                             "gpixel_per_s": round(W * H / (ms * 1e-3) / 1e9, 3), "ms_min": round(ms_min, 5)})
            print(json.dumps(res["dasp_single_frame"][-1]), flush=True)
        sp.close()
        dasp.close()
        if not a.quick:
            for it in (1, 5):
                t0 = time.perf_counter()
                R.segmentation(*frames[0], ROWS, COLS, K, *SIGMAS, it)
                dt = time.perf_counter() - t0
                res["cpu_checker"].append({"width": W, "height": H, "iteration": it, "ms_per_frame": round(dt * 1e3, 1),
                                           "mpixel_per_s": round(W * H / dt / 1e6, 3)})
                print(json.dumps(res["cpu_checker"][-1]), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
