"""Throughput and quality of DepthDecimation (decimate_kernels.hip) on the MI355X.

    python tools/bench_decimate.py [--steps K] [--out profiles/decimate_bench.json] [--quick] [--only vga|1080p] [--no-quality]

Throughput.  64 x VGA and 8 x 1080p of synth frames, k = 2, 3, 4 and 8, both modes, the guard off and on (max_gap 50), float and
uint16 on either side, and the colour call.  Reports per setting the median of K timed calls after a wake-up load and warm-up
(HIP events on the current stream), next to
  (a) the float4 streaming copy of tools/hooks/libkde_hooks.so over the bytes that MUST move -- the source read once, the output
      written once: the call's fraction of that copy ceiling;
  (b) what a user writes today on the same device tensors: torch's avg_pool2d (which mixes the sensor's 0 into valid depths and
      invents depths between surfaces) and a strided slice made contiguous (which drops k^2 - 1 of k^2 samples);
  (c) the numpy statement of the rule (tests/decimate_cases.py) on the host, on the first frame.
The tool checks the device's frames and counts against the statement on the first frame of every k, mode and guard.

Every factor: k = 2 .. 8, float, median and guarded mean, ms per call.

Multi-resolution (4 x 1080p synth frames, MeanError3D against the generator's noise-free depth, time of the whole chain):
  (a) the window-19 JBF at full 1080p;
  (b) decimate k = 2 (depth and guide) -> JBF window 9 -> GuidedDepthUpsampling to 1080p;
  (c) the same with k = 4 and window 5: the window that covers the same field of view, the spatial sigma divided by k.
--quick runs one timed call per measurement and skips (c) of the throughput part."""
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

CASES = [("vga", 64, (640, 480)), ("1080p", 8, (1920, 1080))]
FACTORS = (2, 3, 4, 8)
MAX_GAP = 50.0
FORMATS = (("f32", "f32"), ("u16", "u16"), ("f32", "u16"), ("u16", "f32"))


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
    ap.add_argument("--only", default=None)
    ap.add_argument("--no-quality", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.quick:
        a.steps, a.warmup = 1, 1
    import torch
    import decimate_cases as DC
    from kinectdepthmapenhancement_amd import _native, filters, synth
    from tools.hooks import hooks
    from tools.wake import wake
    torch.cuda.set_device(0)
    stream = lambda: torch.cuda.current_stream().cuda_stream
    esz = {"f32": 4, "u16": 2}
    tdt = {"f32": torch.float32, "u16": torch.int16}
    copies = {}

    def copy_ms(nbytes):
        nbytes = max(32, nbytes // 32 * 32)
        if nbytes not in copies:
            s = torch.empty(nbytes // 2, dtype=torch.uint8, device="cuda")
            t = torch.empty_like(s)
            copies[nbytes] = timed(torch, lambda: hooks.hbm_copy(s, t, stream()), a.steps, a.warmup)[0]
        return copies[nbytes]

    def params(k, mode, gap):
        return _native.DecimateParams(k, mode, 1, gap, 0.0, float(np.finfo(np.float32).max))

    res = {"device": torch.cuda.get_device_name(0), "steps": a.steps, "max_gap": MAX_GAP, "cases": [], "multi_resolution": []}
    for name, n, size in CASES:
        if a.only and a.only != name:
            continue
        w, h = size
        px = w * h
        distinct = min(n, 4)
        bgr4, depth4 = synth.make_batch(21, distinct, w, h)
        depth_np = np.rint(np.concatenate([depth4] * (n // distinct))).astype(np.float32)      # whole millimetres: one scene in both formats
        bgr_np = np.concatenate([bgr4] * (n // distinct))
        bgr = torch.from_numpy(bgr_np).cuda()
        sources = {"f32": torch.from_numpy(depth_np).cuda(), "u16": torch.from_numpy(depth_np.astype(np.uint16).view(np.int16)).cuda()}
        wake(torch)
        case = {"case": name, "frames": n, "size": [w, h], "factors": {}}
        for k in FACTORS:
            ow, oh = DC.out_size(size, k)
            opx = ow * oh
            outs = {f: torch.empty((n, oh, ow), dtype=tdt[f], device="cuda") for f in esz}
            fk = {"out_size": [ow, oh]}
            for mode, mname in ((0, "median"), (1, "mean")):
                for gap in (0.0, MAX_GAP):
                    D = filters.DepthDecimation(size, n, params(k, mode, gap))
                    for fi, fo in FORMATS:
                        s, o = sources[fi], outs[fo]
                        ms, ms_min = timed(torch, lambda: D.decimate(s, o), a.steps, a.warmup)
                        must = n * (px * esz[fi] + opx * esz[fo])
                        cp = copy_ms(must)
                        fk[f"{mname}{'_guard' if gap else ''}_{fi}_{fo}"] = {
                            "bytes_must_move": must, "ms_per_call": round(ms, 4), "ms_min": round(ms_min, 4),
                            "source_gpixel_per_s": round(n * px / (ms * 1e-3) / 1e9, 3), "copy_same_bytes_ms": round(cp, 4),
                            "fraction_of_copy_ceiling": round(cp / ms, 4)}
                    # the device against the statement on the first frame: float, and uint16 where the median is exact
                    for fi in (("f32", "u16") if mode == 0 and not gap else ("f32",)):
                        got = D.decimate(sources[fi][:1], out_format=torch.float32).cpu().numpy()
                        src_np = depth_np[:1] if fi == "f32" else depth_np[:1].astype(np.uint16)
                        t0 = time.perf_counter()
                        want, filled, mixed = DC.decimate_batch(src_np, k, mode=mode, min_valid=1, max_gap=np.float32(gap))
                        host_s = time.perf_counter() - t0
                        ok = bool(got.tobytes() == want.tobytes() and D.filled().tolist() == filled.tolist() and D.mixed().tolist() == mixed.tolist())
                        assert ok, (name, k, mname, gap, fi)
                    fk[f"{mname}{'_guard' if gap else ''}_equals_statement"] = True
                    if not a.quick:
                        fk[f"{mname}{'_guard' if gap else ''}_numpy_statement_s_per_frame"] = round(host_s, 4)
                    D.close()
            # the colour call
            D = filters.DepthDecimation(size, n, params(k, 0, 0.0))
            small = torch.empty((n, oh, ow, 3), dtype=torch.uint8, device="cuda")
            ms, ms_min = timed(torch, lambda: D.decimate_color(bgr, small), a.steps, a.warmup)
            must = n * 3 * (px + opx)
            cp = copy_ms(must)
            assert small[:1].cpu().numpy().tobytes() == DC.decimate_color(bgr_np[0], k)[None].tobytes(), (name, k, "colour")
            fk["color"] = {"bytes_must_move": must, "ms_per_call": round(ms, 4), "ms_min": round(ms_min, 4), "copy_same_bytes_ms": round(cp, 4),
                           "fraction_of_copy_ceiling": round(cp / ms, 4), "equals_statement": True}
            D.close()
            # what a user writes today, on the same device tensors
            f4 = sources["f32"][:, None]
            ms, _ = timed(torch, lambda: torch.nn.functional.avg_pool2d(f4, k, ceil_mode=True), a.steps, a.warmup)
            fk["torch_avg_pool2d_f32_ms"] = round(ms, 4)
            ms, _ = timed(torch, lambda: sources["f32"][:, ::k, ::k].contiguous(), a.steps, a.warmup)
            fk["torch_strided_slice_f32_ms"] = round(ms, 4)
            ms, _ = timed(torch, lambda: sources["u16"][:, ::k, ::k].contiguous(), a.steps, a.warmup)
            fk["torch_strided_slice_u16_ms"] = round(ms, 4)
            case["factors"][str(k)] = fk
            del outs
        # every factor, float in and out
        table = {}
        for k in range(2, 9):
            ow, oh = DC.out_size(size, k)
            o = torch.empty((n, oh, ow), dtype=torch.float32, device="cuda")
            row = {}
            for mode, gap, label in ((0, 0.0, "median"), (1, MAX_GAP, "mean_guard")):
                D = filters.DepthDecimation(size, n, params(k, mode, gap))
                row[f"{label}_ms"] = round(timed(torch, lambda: D.decimate(sources["f32"], o), a.steps, a.warmup)[0], 4)
                D.close()
            table[str(k)] = row
        case["every_factor_f32"] = table
        res["cases"].append(case)
        print(json.dumps(case), flush=True)
        del sources, bgr

    if not a.no_quality and (not a.only or a.only == "1080p"):
        w, h, n = 1920, 1080, 4
        frames = [synth.make_frame(31 + i, w, h, clean=True) for i in range(n)]
        bgr = torch.from_numpy(np.stack([f[0] for f in frames])).cuda()
        depth = torch.from_numpy(np.stack([f[1] for f in frames])).cuda()
        truth = torch.from_numpy(np.stack([f[2] for f in frames])).cuda()
        base = filters.JointBilateralFilter.default_params()

        def jbf_of(size, window, k):
            p = filters.JointBilateralFilter.default_params()
            p.window_size, p.spatial_sigma = window, base.spatial_sigma / k
            return filters.JointBilateralFilter(size[0], size[1], p, max_batch=n)

        wake(torch)
        results, times = {"raw": depth}, {}
        J = jbf_of((w, h), 19, 1)
        full_out = torch.empty_like(depth)
        times["a_jbf19_full"] = {"ms": round(timed(torch, lambda: J.process_batch(depth, bgr, full_out), a.steps, a.warmup)[0], 4)}
        results["a_jbf19_full"] = full_out
        J.close()
        for label, k, window in (("b_k2_jbf9_upsample", 2, 9), ("c_k4_jbf5_upsample", 4, 5)):
            D = filters.DepthDecimation((w, h), n, params(k, 0, 0.0))
            ow, oh = D.out_size
            J = jbf_of((ow, oh), window, k)
            U = filters.GuidedDepthUpsampling((ow, oh), (w, h), n, _native.UpsampleParams(2, 30.0, MAX_GAP, 0.0, float(np.finfo(np.float32).max)))
            low = torch.empty((n, oh, ow), dtype=torch.float32, device="cuda")
            guide = torch.empty((n, oh, ow, 3), dtype=torch.uint8, device="cuda")
            filt = torch.empty_like(low)
            up = torch.empty_like(depth)
            steps = {"decimate_depth": lambda: D.decimate(depth, low), "decimate_color": lambda: D.decimate_color(bgr, guide),
                     "jbf": lambda: J.process_batch(low, guide, filt), "upsample": lambda: U.upsample(filt, bgr, up)}

            def chain():
                for fn in steps.values():
                    fn()

            t = {"window": window, "small_size": [ow, oh], "ms": round(timed(torch, chain, a.steps, a.warmup)[0], 4)}
            for sname, fn in steps.items():
                t[sname + "_ms"] = round(timed(torch, fn, a.steps, a.warmup)[0], 4)
            times[label] = t
            results[label] = up
            results[label.split("_")[0] + f"_k{k}_decimate_upsample_no_jbf"] = U.upsample(low, bgr, torch.empty_like(depth))
            for obj in (D, J, U):
                obj.close()
        E = filters.MeanError3D(w, h, n, 8)
        E.set_camera(synth.intrinsics(w, h))
        labels = list(results)
        E.compare([results[label] for label in labels], truth)
        table = E.results_host()
        q = {"size": [w, h], "frames": n, "times": times, "mean_error_3d_mm": {}, "valid_pixels": {}}
        for c, label in enumerate(labels):
            count = int(table["count"][:, c].sum())
            q["mean_error_3d_mm"][label] = round(float(np.sum(table["sum"][:, c]) / max(1, count)), 4)
            q["valid_pixels"][label] = count
        E.close()
        res["multi_resolution"].append(q)
        print(json.dumps(q), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
