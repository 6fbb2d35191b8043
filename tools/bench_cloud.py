"""Throughput of PointCloudXYZRGB (cloud_kernels.hip), the output step of the reference (main.cpp:211-300), on the MI355X.

    python tools/bench_cloud.py [--steps K] [--out profiles/cloud_bench.json] [--quick]

Cases: 64 x 640x480 and 8 x 1920x1080, about 70 % of the pixels valid, a colour image per frame.  Reports per case, mode
(dense, organised) and source format (float3 cloud, float depth map, uint16 depth map) the median of K timed calls after a
wake-up load and warm-up (HIP events on the current stream), next to
  (a) the float4 streaming copy of tools/hooks/libkde_hooks.so over as many bytes as the mode MUST move: the source once, the
      colour image once and the records written (16 B per valid pixel in dense mode, 16 B per pixel in organised mode): its
      fraction of that copy ceiling.  The dense path reads the source twice (count, then scatter); the second reading is not
      in the ceiling, so it counts against the fraction;
  (b) today's road, once per case: the organised float3 cloud and the colour image copied to the host and the rule applied
      there with numpy (mask, divide, negate, pack).
The tool checks that the three source formats give the same bytes.  --quick runs one timed call per measurement and skips (b).
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
SOURCE_BYTES = {"points": 12, "depth_f32": 4, "depth_u16": 2}


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


def host_road(cloud, bgr):
    """the organised cloud and the image copied out and the rule applied on the host: seconds for the copies, seconds for numpy"""
    t0 = time.perf_counter()
    p, c = cloud.cpu().numpy(), bgr.cpu().numpy()
    t1 = time.perf_counter()
    dt = np.dtype([("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("rgb", "<u4")])
    frames = []
    for f in range(p.shape[0]):
        q, col = p[f].reshape(-1, 3), c[f].reshape(-1, 3)
        v = (q[:, 2] > 50.0) & (q[:, 2] < 15000.0)
        q, col = q[v], col[v].astype(np.uint32)
        rec = np.empty(q.shape[0], dt)
        rec["x"], rec["y"], rec["z"] = q[:, 0] / np.float32(1000.0), q[:, 1] / np.float32(1000.0), -(q[:, 2] / np.float32(1000.0))
        rec["rgb"] = (col[:, 2] << 16) | (col[:, 1] << 8) | col[:, 0]
        frames.append(rec)
    t2 = time.perf_counter()
    return t1 - t0, t2 - t1, frames


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
    from tools.hooks import hooks
    from tools.wake import wake
    torch.cuda.set_device(0)
    stream = lambda: torch.cuda.current_stream().cuda_stream
    res = {"device": torch.cuda.get_device_name(0), "steps": a.steps, "cases": []}
    for n, W, H in CASES:
        px = n * W * H
        K = synth.intrinsics(W, H)
        gen = torch.Generator(device="cuda").manual_seed(n + W)
        depth = torch.round(torch.rand((n, H, W), device="cuda", generator=gen) * 7600.0 + 400.0)
        depth = torch.where(torch.rand((n, H, W), device="cuda", generator=gen) < 0.3, torch.zeros_like(depth), depth)
        bgr = torch.randint(0, 256, (n, H, W, 3), device="cuda", generator=gen, dtype=torch.uint8)
        conv = filters.DimensionConvertor()
        conv.setCameraParameters(K, W, H)
        cloud = conv.projectiveToReal(depth, torch.empty((n, H, W, 3), dtype=torch.float32, device="cuda"))
        sources = {"points": cloud, "depth_f32": depth, "depth_u16": depth.to(torch.int32).to(torch.int16)}   # 0..8000: int16 bits = uint16 bits
        out = torch.empty((n, H * W, 16), dtype=torch.uint8, device="cuda")
        valid = int(((depth > 50.0) & (depth < 15000.0)).sum().item())

        def copy_ms(nbytes):
            src = torch.empty(nbytes // 2, dtype=torch.uint8, device="cuda")
            dst = torch.empty_like(src)
            ms, _ = timed(torch, lambda: hooks.hbm_copy(src, dst, stream()), a.steps, a.warmup)
            return ms

        wake(torch)
        case = {"frames": n, "width": W, "height": H, "valid_fraction": round(valid / px, 4)}
        for organized in (False, True):
            mode = "organized" if organized else "dense"
            C = filters.PointCloudXYZRGB(W, H, max_batch=n, organized=organized)
            C.set_camera(K)
            want = None
            for name, src in sources.items():
                ms, ms_min = timed(torch, lambda: C.build(src, bgr, out), a.steps, a.warmup)
                counts = C.counts()
                assert int(counts.sum()) == valid, (mode, name, int(counts.sum()), valid)
                got = [r.tobytes() for r in C.points_host()]
                if want is None:
                    want = got
                must = px * (SOURCE_BYTES[name] + 3) + 16 * (px if organized else valid)
                cms = copy_ms(must)
                case[f"{mode}_{name}"] = {"bytes_must_move": must, "ms_per_call": round(ms, 4), "ms_min": round(ms_min, 4),
                                          "ms_per_frame": round(ms / n, 5), "gpixel_per_s": round(px / (ms * 1e-3) / 1e9, 3),
                                          "gbyte_per_s": round(must / (ms * 1e-3) / 1e9, 1), "copy_same_bytes_ms": round(cms, 4),
                                          "copy_gbyte_per_s": round(must / (cms * 1e-3) / 1e9, 1),
                                          "fraction_of_copy_ceiling": round(cms / ms, 4), "equals_points": got == want}
            if not organized and not a.quick:
                torch.cuda.synchronize()
                copy_s, numpy_s, frames = host_road(cloud, bgr)
                C.build(cloud, bgr, out)
                same = [r.tobytes() for r in C.points_host()] == [r.tobytes() for r in frames]
                t0 = time.perf_counter()
                C.build(cloud, bgr, out)
                C.points_host()
                t1 = time.perf_counter()
                case["host_road"] = {"d2h_bytes": px * 15, "copy_s": round(copy_s, 3), "numpy_s": round(numpy_s, 3),
                                     "device_call_and_d2h_of_the_records_s": round(t1 - t0, 3), "same_bytes": same,
                                     "total_over_device_call": round((copy_s + numpy_s) * 1e3 / case["dense_points"]["ms_per_call"], 1),
                                     "total_over_device_call_and_d2h": round((copy_s + numpy_s) / (t1 - t0), 1)}
            C.close()
        res["cases"].append(case)
        print(json.dumps(case), flush=True)
        conv.close()
        del cloud, depth, bgr, out, sources
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
