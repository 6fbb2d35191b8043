"""Throughput of DepthRegistration (reg_kernels.hip), the registration of Kinect.cpp:71-75, on the MI355X.

    python tools/bench_reg.py [--steps K] [--out profiles/reg_bench.json] [--quick]

Cases: 64 x (640x480 -> 640x480), Kinect-like (baseline 25 mm, 1 degree, focal lengths 2 % apart), and 8 x (512x424 -> 1920x1080),
Kinect-v2-like.  Reports per case, mode (point, max_splat 4) and format (float or uint16, in and out) the median of K timed calls
after a wake-up load and warm-up (HIP events on the current stream), next to
  (a) the float4 streaming copy of tools/hooks/libkde_hooks.so over the bytes that MUST move -- the source read once, the
      output written once: its fraction of that copy ceiling.  The z-buffer's own traffic is reported beside it: 4 B per target
      pixel set by the memset, 4 B read by the finalise, plus one 4-byte atomic per (source pixel, covered target pixel);
  (b) the road through the host, on the first frames of the case: the depth copied out, the numpy statement of the rule
      (tests/reg_cases.py) run there, the result copied back.
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

#        frames  depth        colour        fd     fc      baseline
CASES = [(64, (640, 480), (640, 480), 575.8, 587.3, 25.0), (8, (512, 424), (1920, 1080), 365.0, 1060.0, 52.0)]
HOST_FRAMES = 4


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
    from kinectdepthmapenhancement_amd import _native, filters
    from tools.hooks import hooks
    from tools.wake import wake
    torch.cuda.set_device(0)
    stream = lambda: torch.cuda.current_stream().cuda_stream
    res = {"device": torch.cuda.get_device_name(0), "steps": a.steps, "cases": []}
    for n, (wd, hd), (wc, hc), fd, fc, base in CASES:
        pxd, pxc = n * wd * hd, n * wc * hc
        c = RC.calib(RC.camera(wd, hd, fd), RC.camera(wc, hc, fc, 0.4, -0.3), RC.rotation(1.0), (base, 0.0, 0.0))
        few = min(n, HOST_FRAMES)
        head = RC.depth_maps(n + wd, few, hd, wd, integer=True)          # whole millimetres: the same scene in both formats
        depth = torch.from_numpy(np.concatenate([head] * (n // few))).cuda()
        sources = {"f32": depth, "u16": depth.to(torch.int32).to(torch.int16)}   # 0..65535: int16 bits = uint16 bits
        outs = {"f32": torch.empty((n, hc, wc), dtype=torch.float32, device="cuda"),
                "u16": torch.empty((n, hc, wc), dtype=torch.int16, device="cuda")}

        def copy_ms(nbytes):
            src = torch.empty(nbytes // 2, dtype=torch.uint8, device="cuda")
            dst = torch.empty_like(src)
            ms, _ = timed(torch, lambda: hooks.hbm_copy(src, dst, stream()), a.steps, a.warmup)
            return ms

        wake(torch)
        case = {"frames": n, "depth": [wd, hd], "color": [wc, hc]}
        for splat in (0, 4):
            mode = "point" if splat == 0 else f"splat{splat}"
            R = filters.DepthRegistration((wd, hd), (wc, hc), n, _native.RegParams(0.0, float(RC.FLT_MAX), splat))
            R.set_calibration(c.Kd, c.Kc, c.R, c.T)
            zb = [RC.keys(head[f], c, (wc, hc), max_splat=splat) for f in range(few)] if not a.quick else None
            for fin, fout in (("f32", "f32"), ("u16", "u16"), ("u16", "f32"), ("f32", "u16")):
                src, out = sources[fin], outs[fout]
                ms, ms_min = timed(torch, lambda: R.register(src, out), a.steps, a.warmup)
                filled = R.filled()
                esz = {"f32": 4, "u16": 2}
                must = pxd * esz[fin] + pxc * esz[fout]
                cms = copy_ms(must)
                r = {"bytes_must_move": must, "zbuffer_bytes_set_and_read": 8 * pxc, "ms_per_call": round(ms, 4), "ms_min": round(ms_min, 4),
                     "ms_per_frame": round(ms / n, 5), "source_gpixel_per_s": round(pxd / (ms * 1e-3) / 1e9, 3),
                     "target_gpixel_per_s": round(pxc / (ms * 1e-3) / 1e9, 3), "copy_same_bytes_ms": round(cms, 4),
                     "copy_gbyte_per_s": round(must / (cms * 1e-3) / 1e9, 1), "fraction_of_copy_ceiling": round(cms / ms, 4),
                     "filled_fraction": round(float(filled.sum()) / pxc, 4)}
                if zb is not None:
                    want = np.stack([RC.finalise(z, np.float32 if fout == "f32" else np.uint16)[0] for z in zb])
                    r["equals_statement"] = bool(out[:few].cpu().numpy().tobytes() == want.tobytes() and
                                                 filled[:few].tolist() == [RC.finalise(z)[1] for z in zb])
                case[f"{mode}_{fin}_to_{fout}"] = r
            if not a.quick:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                h = sources["f32"][:few].cpu().numpy()
                t1 = time.perf_counter()
                reg = np.stack([RC.statement(h[f], c, (wc, hc), max_splat=splat)[0] for f in range(few)])
                t2 = time.perf_counter()
                torch.from_numpy(reg).cuda()
                torch.cuda.synchronize()
                t3 = time.perf_counter()
                dev_ms = case[f"{mode}_f32_to_f32"]["ms_per_frame"]
                case[f"{mode}_host_road"] = {"frames": few, "copies_s_per_frame": round((t1 - t0 + t3 - t2) / few, 5),
                                             "numpy_s_per_frame": round((t2 - t1) / few, 4),
                                             "total_over_device_call": round((t3 - t0) / few * 1e3 / dev_ms, 1)}
            R.close()
        res["cases"].append(case)
        print(json.dumps(case), flush=True)
        del depth, sources, outs
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
