"""Throughput of LensUndistortion (undist_kernels.hip) on the MI355X.

    python tools/bench_undist.py [--steps K] [--out profiles/undist_bench.json] [--quick]

Cases: 64 x (640x480 -> 640x480) and 8 x (1920x1080 -> 1920x1080), a moderate barrel distortion (k1 -0.25, k2 0.07, small
tangential terms, the pinhole view keeps K), about a tenth of the depth invalid.  Reports per case the median of K timed calls
after a wake-up load and warm-up (HIP events on the current stream) for the colour remap, the depth remap with the nearest
rule and the depth remap with the guarded bilinear rule (max_gap 50 mm), the depth ones with float and with uint16 on both
sides, next to
  (a) the float4 streaming copy of tools/hooks/libkde_hooks.so over the bytes that MUST move -- the source read once, the
      output written once: the call's fraction of that copy ceiling;
  (b) the road through the host, on the first frames of the case: the frames copied out, the numpy statement of the rule
      (tests/undist_cases.py) run there, the result copied back.
kde_reg_color_to_depth_batch, the other gather that stores through LDS, is timed on the same frames beside the colour remap.
The tool checks the device's bytes against the statement on those frames.  --quick runs one timed call per measurement and
skips (b).
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
sys.path.insert(0, os.path.join(ROOT, "tests"))

#        frames  size          focal length
CASES = [(64, (640, 480), 575.8), (8, (1920, 1080), 1060.0)]
DIST = (-0.25, 0.07, 0.0008, -0.0005, 0.0, 0.0, 0.0, 0.0)
MAX_GAP = 50.0
HOST_FRAMES = 2


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
    import reg_cases as RC
    import undist_cases as UC
    from kinectdepthmapenhancement_amd import _native, filters
    from tools.hooks import hooks
    from tools.wake import wake
    torch.cuda.set_device(0)
    stream = lambda: torch.cuda.current_stream().cuda_stream
    res = {"device": torch.cuda.get_device_name(0), "steps": a.steps, "dist": list(DIST), "max_gap": MAX_GAP, "cases": []}
    for n, (w, h), f in CASES:
        px = n * w * h
        K = RC.camera(w, h, f)
        c = UC.calib(K, DIST)
        few = min(n, HOST_FRAMES)
        head = RC.depth_maps(n + w, few, h, w, integer=True)             # whole millimetres: the same scene in both formats
        depth = torch.from_numpy(np.concatenate([head] * (n // few))).cuda()
        sources = {"f32": depth, "u16": depth.to(torch.int32).to(torch.int16)}   # 0..65535: int16 bits = uint16 bits
        outs = {"f32": torch.empty((n, h, w), dtype=torch.float32, device="cuda"),
                "u16": torch.empty((n, h, w), dtype=torch.int16, device="cuda")}
        bgr_head = RC.bgr_images(n, few, h, w)
        bgr = torch.from_numpy(np.concatenate([bgr_head] * (n // few))).cuda()
        bgr_out = torch.empty_like(bgr)

        def copy_ms(nbytes):
            src = torch.empty(nbytes // 2, dtype=torch.uint8, device="cuda")
            dst = torch.empty_like(src)
            ms, _ = timed(torch, lambda: hooks.hbm_copy(src, dst, stream()), a.steps, a.warmup)
            return ms

        def entry(ms, ms_min, must):
            cms = copy_ms(must)
            return {"bytes_must_move": must, "ms_per_call": round(ms, 4), "ms_min": round(ms_min, 4), "ms_per_frame": round(ms / n, 5),
                    "gpixel_per_s": round(px / (ms * 1e-3) / 1e9, 3), "copy_same_bytes_ms": round(cms, 4),
                    "copy_gbyte_per_s": round(must / (cms * 1e-3) / 1e9, 1), "fraction_of_copy_ceiling": round(cms / ms, 4)}

        wake(torch)
        case = {"frames": n, "size": [w, h]}
        U = filters.LensUndistortion((w, h), (w, h), n)
        U.set_calibration(K, DIST)
        ms, ms_min = timed(torch, lambda: U.color(bgr, out=bgr_out), a.steps, a.warmup)
        r = entry(ms, ms_min, 6 * px)
        if not a.quick:
            want = np.stack([UC.color(b, c, (w, h)) for b in bgr_head])
            r["equals_statement"] = bool(bgr_out[:few].cpu().numpy().tobytes() == want.tobytes())
            r["black_fraction"] = round(float((want.reshape(-1, 3).max(1) == 0).mean()), 4)
        case["color"] = r
        U.close()
        # the same gather-and-LDS-store shape, for comparison: kde_reg_color_to_depth_batch (R3 of reg_kernels.hip) on these
        # frames, two equal pinhole cameras 25 mm apart; it reads the depth (4 B), gathers one colour and writes one
        G = filters.DepthRegistration((w, h), (w, h), n)
        G.set_calibration(K, K, np.eye(3), (25.0, 0.0, 0.0))
        ms, ms_min = timed(torch, lambda: G.color_to_depth(sources["f32"], bgr, bgr_out), a.steps, a.warmup)
        case["reg_color_to_depth_f32"] = entry(ms, ms_min, 10 * px)
        G.close()
        for interp in (0, 1):
            mode = "nearest" if interp == 0 else "bilinear"
            U = filters.LensUndistortion((w, h), (w, h), n, _native.UndistParams(0.0, float(UC.FLT_MAX), interp, MAX_GAP if interp else 0.0))
            U.set_calibration(K, DIST)
            for fmt in ("f32", "u16"):
                src, out = sources[fmt], outs[fmt]
                ms, ms_min = timed(torch, lambda: U.depth(src, out), a.steps, a.warmup)
                filled = U.filled()
                esz = {"f32": 4, "u16": 2}[fmt]
                r = entry(ms, ms_min, 2 * px * esz)
                r["filled_fraction"] = round(float(filled.sum()) / px, 4)
                if not a.quick:
                    dt = np.float32 if fmt == "f32" else np.uint16
                    st = [UC.depth(head[k].astype(dt), c, (w, h), interp=interp, max_gap=MAX_GAP, out_dtype=dt) for k in range(few)]
                    got = out[:few].cpu().numpy()
                    r["equals_statement"] = bool(got.tobytes() == np.stack([v for v, _ in st]).tobytes() and
                                                 filled[:few].tolist() == [k for _, k in st])
                    if interp:
                        parts = UC.depth_parts(head[0].astype(dt), c, (w, h), interp=1, max_gap=MAX_GAP)
                        r["blended_fraction"] = round(float(parts["blended"].mean()), 4)
                case[f"depth_{mode}_{fmt}"] = r
            U.close()
        if not a.quick:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            hd, hb = sources["f32"][:few].cpu().numpy(), bgr[:few].cpu().numpy()
            t1 = time.perf_counter()
            und = np.stack([UC.depth(hd[k], c, (w, h))[0] for k in range(few)])
            t2 = time.perf_counter()
            col = np.stack([UC.color(hb[k], c, (w, h)) for k in range(few)])
            t3 = time.perf_counter()
            torch.from_numpy(und).cuda()
            torch.from_numpy(col).cuda()
            torch.cuda.synchronize()
            t4 = time.perf_counter()
            dev_ms = case["depth_nearest_f32"]["ms_per_frame"] + case["color"]["ms_per_frame"]
            case["host_road"] = {"frames": few, "copies_s_per_frame": round((t1 - t0 + t4 - t3) / few, 5),
                                 "numpy_depth_s_per_frame": round((t2 - t1) / few, 4), "numpy_color_s_per_frame": round((t3 - t2) / few, 4),
                                 "total_over_device_calls": round((t4 - t0) / few * 1e3 / dev_ms, 1)}
        res["cases"].append(case)
        print(json.dumps(case), flush=True)
        del depth, sources, outs, bgr, bgr_out
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
