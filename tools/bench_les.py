"""Throughput of LabelEquivalenceSeg::labelImage (les_kernels.hip) on the MI355X, next to the NormalAdaptiveSuperpixel call
that feeds it and with the CPU checker as the baseline.

    python tools/bench_les.py [--steps K] [--out profiles/les_bench.json] [--quick]

Cases: 64 x 640x480 and 8 x 1920x1080 at 15 x 20 superpixels, 8 x 1920x1080 at 40 x 40; the inputs are the outputs of
NormalAdaptiveSuperpixel::Segmentation(10, 50, 50, 150, 1) on synthetic frames (normals by NormalMapGenerator, CM), all on the
device.  Reports ms per batch call, ms per frame and Gpixel/s (median of K timed calls after a wake-up load and warm-up, HIP
events on the current stream), the same for the NASP call on the same batch, the float4 streaming copy of
tools/hooks/libkde_hooks.so over 24 B per pixel of the batch (the paint pass reads 4 B and writes 20 B per pixel: its
ceiling), and the single-thread time of tools/les_ref.c on one frame.  --quick runs one timed call per case, for a profiler
run of its own (rocprofv3 --kernel-trace --stats -- python tools/bench_les.py --quick).
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

CASES = [(64, 640, 480, 15, 20), (8, 1920, 1080, 15, 20), (8, 1920, 1080, 40, 40)]
SIGMAS = (10.0, 50.0, 50.0, 150.0)       # KinectDepthEnhancement.cpp:67


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
    from tools import les_ref as R
    from tools.hooks import hooks
    from tools.wake import wake
    torch.cuda.set_device(0)
    res = {"device": torch.cuda.get_device_name(0), "steps": a.steps, "nasp_sigmas": SIGMAS, "les": [], "cpu_checker": []}
    for n, W, H, rows, cols in CASES:
        K = synth.intrinsics(W, H)
        k = rows * cols
        frames = [synth.make_frame(s, W, H) for s in (1, 2)]
        bgr = torch.from_numpy(np.stack([frames[i % 2][0] for i in range(n)])).cuda()
        depth = torch.from_numpy(np.stack([frames[i % 2][1] for i in range(n)])).cuda()
        conv = filters.DimensionConvertor()
        conv.setCameraParameters(K, W, H)
        pts = torch.empty((n, H, W, 3), dtype=torch.float32, device="cuda")
        conv.projectiveToReal(depth, pts)
        gen = filters.NormalMapGenerator(W, H, max_batch=n)
        gen.setNormalEstimationMethods(gen.CM)
        nrm = torch.empty((n, H, W, 3), dtype=torch.float32, device="cuda")
        gen.generateNormalMapBatch(n, pts, nrm)
        sp = filters.NormalAdaptiveSuperpixel(W, H, max_batch=n)
        sp.SetParametor(rows, cols, K)
        sp.segmentation_batch(bgr, pts, nrm, *SIGMAS, 1)
        normals, labels, centers = (sp.getNormalsDevice().reshape(n, k, 3), sp.getLabelDevice().reshape(n, H, W),
                                    sp.getCentersDevice().reshape(n, k, 3))
        seg = filters.LabelEquivalenceSeg(W, H, max_batch=n)
        src = torch.empty(n * W * H * 12, dtype=torch.uint8, device="cuda")     # 12 B read + 12 B written per pixel
        dst = torch.empty_like(src)
        wake(torch)
        ms, ms_min = timed(torch, lambda: seg.label_image_batch(normals, labels, centers), a.steps, a.warmup)
        nasp_ms, _ = timed(torch, lambda: sp.segmentation_batch(bgr, pts, nrm, *SIGMAS, 1), a.steps, a.warmup)
        copy_ms, _ = timed(torch, lambda: hooks.hbm_copy(src, dst, torch.cuda.current_stream().cuda_stream), a.steps, a.warmup)
        torch.cuda.synchronize()
        m = seg.getMergedClusterLabel_Host().reshape(n, H, W)
        px = n * W * H
        res["les"].append({"frames": n, "width": W, "height": H, "rows": rows, "cols": cols, "ms_per_call": round(ms, 4),
                           "ms_per_frame": round(ms / n, 5), "gpixel_per_s": round(px / (ms * 1e-3) / 1e9, 3), "ms_min": round(ms_min, 4),
                           "nasp_it1_ms_per_call": round(nasp_ms, 4), "fraction_of_nasp": round(ms / nasp_ms, 4),
                           "copy_24B_per_px_ms": round(copy_ms, 4), "copy_gbyte_per_s": round(px * 24 / (copy_ms * 1e-3) / 1e9, 1),
                           "regions_frame0": len(set(np.unique(m[0]).tolist()) - {-1})})
        print(json.dumps(res["les"][-1]), flush=True)
        if not a.quick:
            hn, hl, hc = normals[0].cpu().numpy(), labels[0].cpu().numpy(), centers[0].cpu().numpy()
            t0 = time.perf_counter()
            R.label_image(hn, hl, hc)
            dt = time.perf_counter() - t0
            res["cpu_checker"].append({"width": W, "height": H, "rows": rows, "cols": cols, "ms_per_frame": round(dt * 1e3, 1),
                                       "mpixel_per_s": round(W * H / dt / 1e6, 3)})
            print(json.dumps(res["cpu_checker"][-1]), flush=True)
        seg.close(); sp.close(); gen.close(); conv.close()
        del src, dst, bgr, depth, pts, nrm
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
