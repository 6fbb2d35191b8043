"""Throughput of MeanError3D (error3d_kernels.hip), the reference's quality figure (main.cpp:220-308), on the MI355X.

    python tools/bench_error3d.py [--steps K] [--out profiles/error3d_bench.json] [--quick]

Cases: five candidates against one truth (a frame of its own per frame of the batch) at 64 x 640x480 and 8 x 1920x1080.
Reports per case (median of K timed calls after a wake-up load and warm-up, HIP events on the current stream):
  points      the call with float3 sources (12 B per pixel and source, 72 B per pixel of the batch), next to
              (a) the float4 streaming copy of tools/hooks/libkde_hooks.so over half those bytes, i.e. as many bytes moved as
                  the call must read: its fraction of that copy ceiling;
              (b) the road without the stage: the six clouds copied to the host and reduced there with numpy (one run);
  one_truth   the same call with truth_frames = 1 (60 B per pixel and a resident truth frame);
  depth_f32 / depth_u16   the same call with depth-map sources (4 or 2 B per pixel and source), against the copy of as many
              bytes: what the projection and the narrower loads cost;
  split       five calls of one candidate each: the truth read once per candidate instead of once per pixel (the records are
              the same bytes, which the tool checks).
--quick runs one timed call per measurement and skips the host road.
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
M = 5


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


def host_road(clouds, truth):
    """the clouds copied out and the rule evaluated on the host: seconds for the copies, seconds for the loop, the means"""
    t0 = time.perf_counter()
    hc, ht = [c.cpu().numpy() for c in clouds], truth.cpu().numpy()
    t1 = time.perf_counter()
    means = []
    tz = ht[..., 2]
    tv = (tz > 50.0) & (tz < 15000.0)
    for p in hc:
        v = tv & (p[..., 2] > 50.0) & (p[..., 2] < 15000.0)
        d = p - ht
        e = np.sqrt((d[..., 2] * d[..., 2] + d[..., 1] * d[..., 1]) + d[..., 0] * d[..., 0])
        e = np.where(v, e, np.float32(0)).astype(np.float64)
        means.append((e.sum(axis=(1, 2)) / v.sum(axis=(1, 2))).astype(np.float32))
    t2 = time.perf_counter()
    return t1 - t0, t2 - t1, np.stack(means, axis=1)


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
    res = {"device": torch.cuda.get_device_name(0), "steps": a.steps, "candidates": M, "cases": []}
    for n, W, H in CASES:
        px = n * W * H
        K = synth.intrinsics(W, H)
        gen = torch.Generator(device="cuda").manual_seed(n + W)
        tdepth = torch.round(torch.rand((n, H, W), device="cuda", generator=gen) * 7600.0 + 400.0)
        tdepth = torch.where(torch.rand((n, H, W), device="cuda", generator=gen) < 0.05, torch.zeros_like(tdepth), tdepth)
        cdepth = [torch.where(tdepth > 0, tdepth + float(c + 1), tdepth) for c in range(M)]
        conv = filters.DimensionConvertor()
        conv.setCameraParameters(K, W, H)
        cloud = lambda d: conv.projectiveToReal(d, torch.empty((n, H, W, 3), dtype=torch.float32, device="cuda"))
        tcloud, cclouds = cloud(tdepth), [cloud(d) for d in cdepth]
        u16 = lambda d: d.to(torch.int32).to(torch.int16)          # 400..8005: the uint16 bits are the int16 bits
        tdepth16, cdepth16 = u16(tdepth), [u16(d) for d in cdepth]
        E = filters.MeanError3D(W, H, max_batch=n, max_candidates=M)
        E.set_camera(K)

        def copy_ms(bytes_read):
            src = torch.empty(bytes_read // 2, dtype=torch.uint8, device="cuda")
            dst = torch.empty_like(src)
            ms, _ = timed(torch, lambda: hooks.hbm_copy(src, dst, stream()), a.steps, a.warmup)
            return ms

        wake(torch)
        case = {"frames": n, "width": W, "height": H}
        for name, cands, truth, bpp in (("points", cclouds, tcloud, 12 * (M + 1)), ("one_truth", cclouds, tcloud[:1], 12 * M),
                                        ("depth_f32", cdepth, tdepth, 4 * (M + 1)), ("depth_u16", cdepth16, tdepth16, 2 * (M + 1))):
            ms, ms_min = timed(torch, lambda: E.compare(cands, truth), a.steps, a.warmup)
            table = E.results_host()
            if name == "points":
                want = table.copy()
                case["mean_frame0"] = [float(v) for v in table["mean"][0]]
            elif name != "one_truth":
                case[f"{name}_equals_points"] = bool(np.array_equal(table.view(np.uint8), want.view(np.uint8)))
            cms = copy_ms(px * bpp)
            case[name] = {"bytes_read_per_pixel": bpp, "ms_per_call": round(ms, 4), "ms_min": round(ms_min, 4),
                          "ms_per_frame": round(ms / n, 5), "gpixel_per_s": round(px / (ms * 1e-3) / 1e9, 3),
                          "read_gbyte_per_s": round(px * bpp / (ms * 1e-3) / 1e9, 1),
                          "copy_same_bytes_ms": round(cms, 4), "copy_gbyte_per_s": round(px * bpp / (cms * 1e-3) / 1e9, 1),
                          "fraction_of_copy_ceiling": round(cms / ms, 4)}
        # the truth once per candidate: five calls of one candidate
        rows = []

        def split():
            for c in range(M):
                E.compare([cclouds[c]], tcloud)

        sms, _ = timed(torch, split, a.steps, a.warmup)
        for c in range(M):
            E.compare([cclouds[c]], tcloud)
            rows.append(E.results_host()[:, 0])
        case["split"] = {"bytes_read_per_pixel": 24 * M, "ms_per_5_calls": round(sms, 4),
                         "one_call_over_split": round(case["points"]["ms_per_call"] / sms, 4),
                         "equals_one_call": bool(np.array_equal(np.stack(rows, axis=1).view(np.uint8), want.view(np.uint8)))}
        if not a.quick:
            torch.cuda.synchronize()
            copy_s, loop_s, means = host_road(cclouds, tcloud)
            case["host_road"] = {"d2h_bytes": px * 12 * (M + 1), "copy_s": round(copy_s, 3), "numpy_loop_s": round(loop_s, 3),
                                 "total_over_device_call": round((copy_s + loop_s) * 1e3 / case["points"]["ms_per_call"], 1),
                                 "max_rel_diff_of_means": float(np.max(np.abs(means - want["mean"]) / want["mean"]))}
        res["cases"].append(case)
        print(json.dumps(case), flush=True)
        E.close()
        conv.close()
        del tcloud, cclouds, tdepth, cdepth, tdepth16, cdepth16
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
