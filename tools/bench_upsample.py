"""Throughput and quality of GuidedDepthUpsampling (upsample_kernels.hip) on the MI355X.

    python tools/bench_upsample.py [--steps K] [--out profiles/upsample_bench.json] [--quick]

Throughput.  Cases: 64 x (320x240 -> 640x480), 8 x (960x540 -> 1920x1080) and 8 x (512x424 -> 1920x1080); radius 2, sigma_color
30; the guard off and on (max_gap 100 mm); float and uint16 on both sides; the synthetic RGB-D generator's frames (a few,
repeated), their depth decimated at gx_of / gy_of.  Reports per setting the median of K timed calls after a wake-up load and
warm-up (HIP events on the current stream), next to
  (a) the float4 streaming copy of tools/hooks/libkde_hooks.so over the bytes that MUST move -- the source depth once, the
      guide once, the output once: the call's fraction of that copy ceiling;
  (b) kde_reg_register_batch with max_splat = the ratio rounded up on the same frames, two pinhole cameras that show the same
      view at the two sizes: the road to a full-size depth map that existed before;
  (c) the road through the host, on the first frame of the case: the frames copied out, the numpy statement of the rule
      (tests/upsample_cases.py) run there, the result copied back.
The tool checks the device's bytes against the statement on that frame.

Quality.  The generator's frames at full size with their noise-free depth; the noisy depth decimated at gx_of / gy_of and
brought back by: guided r = 2 without and with the guard, sigma_color 1e6 (the plain tent, no guidance), and the splat of
(b).  MeanError3D (the reference's figure, main.cpp:220-308) of each against the noise-free full-size depth, and the fraction
of the truth's valid pixels each fills.  --quick runs one timed call per measurement and skips (c) and the quality part.
"""
from __future__ import annotations

import argparse
import json
import math
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

#        frames  source      output
CASES = [(64, (320, 240), (640, 480)), (8, (960, 540), (1920, 1080)), (8, (512, 424), (1920, 1080))]
QUALITY = [((320, 240), (640, 480)), ((512, 424), (1920, 1080))]
RADIUS, SIGMA, MAX_GAP = 2, 30.0, 100.0
DISTINCT = 2                                              # generator frames per case (repeated to fill the batch)


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


def same_view(K, src, out):
    """the camera of the same view at the low resolution: pixel centres at (q + 0.5) / src_w of the width"""
    ax, ay = src[0] / out[0], src[1] / out[1]
    return np.array([[K[0, 0] * ax, 0.0, (K[0, 2] + 0.5) * ax - 0.5], [0.0, K[1, 1] * ay, (K[1, 2] + 0.5) * ay - 0.5], [0.0, 0.0, 1.0]])


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
    import upsample_cases as UC
    from kinectdepthmapenhancement_amd import _native, filters, synth
    from tools.hooks import hooks
    from tools.wake import wake
    torch.cuda.set_device(0)
    stream = lambda: torch.cuda.current_stream().cuda_stream
    Params = _native.UpsampleParams
    FLT_MAX = float(UC.FLT_MAX)
    res = {"device": torch.cuda.get_device_name(0), "steps": a.steps, "radius": RADIUS, "sigma_color": SIGMA, "max_gap": MAX_GAP, "cases": [],
           "quality": []}

    def frames(src, out, count):
        """count generator frames at the output size: (bgr, noisy depth decimated to src, noise-free depth)"""
        t = UC.tables(src, out, SIGMA)
        made = [synth.make_frame(31 + k, out[0], out[1], clean=True) for k in range(count)]
        low = np.stack([m[1][t.gy_of][:, t.gx_of] for m in made])
        return np.stack([m[0] for m in made]), np.ascontiguousarray(low), np.stack([m[2] for m in made])

    for n, src, out in CASES:
        (sw, sh), (ow, oh) = src, out
        opx, spx = n * ow * oh, n * sw * sh
        bgr_head, low_head, _ = frames(src, out, DISTINCT)
        low_head = np.rint(low_head)                                   # whole millimetres: the same scene in both formats
        bgr = torch.from_numpy(np.concatenate([bgr_head] * (n // DISTINCT))).cuda()
        depth = torch.from_numpy(np.concatenate([low_head] * (n // DISTINCT))).cuda()
        sources = {"f32": depth, "u16": depth.to(torch.int32).to(torch.int16)}
        outs = {"f32": torch.empty((n, oh, ow), dtype=torch.float32, device="cuda"),
                "u16": torch.empty((n, oh, ow), dtype=torch.int16, device="cuda")}

        def copy_ms(nbytes):
            s = torch.empty(nbytes // 2, dtype=torch.uint8, device="cuda")
            d = torch.empty_like(s)
            ms, _ = timed(torch, lambda: hooks.hbm_copy(s, d, stream()), a.steps, a.warmup)
            return ms

        def entry(ms, ms_min, must):
            cms = copy_ms(must)
            return {"bytes_must_move": must, "ms_per_call": round(ms, 4), "ms_min": round(ms_min, 4), "ms_per_frame": round(ms / n, 5),
                    "gpixel_out_per_s": round(opx / (ms * 1e-3) / 1e9, 3), "copy_same_bytes_ms": round(cms, 4),
                    "copy_gbyte_per_s": round(must / (cms * 1e-3) / 1e9, 1), "fraction_of_copy_ceiling": round(cms / ms, 4)}

        wake(torch)
        case = {"frames": n, "source": [sw, sh], "output": [ow, oh]}
        for gap in (0.0, MAX_GAP):
            U = filters.GuidedDepthUpsampling(src, out, n, Params(RADIUS, SIGMA, gap, 0.0, FLT_MAX))
            for fmt in ("f32", "u16"):
                s, o = sources[fmt], outs[fmt]
                ms, ms_min = timed(torch, lambda: U.upsample(s, bgr, o), a.steps, a.warmup)
                filled = U.filled()
                esz = {"f32": 4, "u16": 2}[fmt]
                r = entry(ms, ms_min, spx * esz + opx * 3 + opx * esz)
                r["filled_fraction"] = round(float(filled.sum()) / opx, 4)
                if not a.quick:
                    dt = np.float32 if fmt == "f32" else np.uint16
                    t = UC.tables(src, out, SIGMA, U.range_table())
                    want, kept = UC.upsample(low_head[0].astype(dt), bgr_head[0], t, out, RADIUS, gap, out_dtype=dt)
                    got = o[:1].cpu().numpy()
                    got = got.view(np.uint16) if fmt == "u16" else got
                    r["equals_statement"] = bool(got[0].tobytes() == want.tobytes() and int(filled[0]) == kept)
                case[f"guided_{'guard' if gap else 'plain'}_{fmt}"] = r
            U.close()
        # (b) the square splat of the registration on the same frames
        splat = min(16, max(math.ceil(ow / sw), math.ceil(oh / sh)))
        K = synth.intrinsics(ow, oh)
        G = filters.DepthRegistration(src, out, n, _native.RegParams(0.0, FLT_MAX, splat))
        G.set_calibration(same_view(K, src, out), K, np.eye(3), (0.0, 0.0, 0.0))
        for fmt in ("f32", "u16"):
            s, o = sources[fmt], outs[fmt]
            ms, ms_min = timed(torch, lambda: G.register(s, o), a.steps, a.warmup)
            esz = {"f32": 4, "u16": 2}[fmt]
            r = entry(ms, ms_min, spx * esz + opx * esz)
            r["max_splat"] = splat
            r["filled_fraction"] = round(float(G.filled().sum()) / opx, 4)
            case[f"reg_splat_{fmt}"] = r
        G.close()
        if not a.quick:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            hd, hb = sources["f32"][:1].cpu().numpy(), bgr[:1].cpu().numpy()
            t1 = time.perf_counter()
            up, _ = UC.upsample(hd[0], hb[0], UC.tables(src, out, SIGMA), out, RADIUS, 0.0)
            t2 = time.perf_counter()
            torch.from_numpy(up).cuda()
            torch.cuda.synchronize()
            t3 = time.perf_counter()
            case["host_road"] = {"frames": 1, "copies_s_per_frame": round(t1 - t0 + t3 - t2, 5), "numpy_s_per_frame": round(t2 - t1, 4),
                                 "total_over_device_call": round((t3 - t0) * 1e3 / case["guided_plain_f32"]["ms_per_frame"], 1)}
        res["cases"].append(case)
        print(json.dumps(case), flush=True)
        del depth, sources, outs, bgr

    for src, out in ([] if a.quick else QUALITY):
        (sw, sh), (ow, oh) = src, out
        n = DISTINCT
        bgr_np, low_np, truth_np = frames(src, out, n)
        bgr, low, truth = (torch.from_numpy(x).cuda() for x in (bgr_np, low_np, truth_np))
        K = synth.intrinsics(ow, oh)
        cands = {}
        for label, sigma, gap in (("guided_r2", SIGMA, 0.0), ("guided_r2_guard", SIGMA, MAX_GAP), ("tent_r2", 1e6, 0.0), ("tent_r2_guard", 1e6, MAX_GAP)):
            U = filters.GuidedDepthUpsampling(src, out, n, Params(RADIUS, sigma, gap, 0.0, FLT_MAX))
            cands[label] = U.upsample(low, bgr, torch.empty((n, oh, ow), dtype=torch.float32, device="cuda"))
            U.close()
        splat = min(16, max(math.ceil(ow / sw), math.ceil(oh / sh)))
        G = filters.DepthRegistration(src, out, n, _native.RegParams(0.0, FLT_MAX, splat))
        G.set_calibration(same_view(K, src, out), K, np.eye(3), (0.0, 0.0, 0.0))
        cands["reg_splat"] = G.register(low, torch.empty((n, oh, ow), dtype=torch.float32, device="cuda"))
        E = filters.MeanError3D(ow, oh, n, len(cands))
        E.set_camera(K)
        E.compare(list(cands.values()), truth)
        table = E.results_host()
        valid = int((truth_np > 0).sum())
        q = {"source": [sw, sh], "output": [ow, oh], "frames": n, "truth_valid_pixels": valid, "max_splat": splat, "methods": {}}
        for c, label in enumerate(cands):
            q["methods"][label] = {"mean_error_3d_mm": round(float(np.sum(table["sum"][:, c]) / max(1, int(table["count"][:, c].sum()))), 4),
                                   "compared_fraction_of_truth": round(int(table["count"][:, c].sum()) / valid, 4)}
        E.close()
        G.close()
        res["quality"].append(q)
        print(json.dumps(q), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
