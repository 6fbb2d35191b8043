"""Throughput and quality of DepthHoleFilling (holefill_kernels.hip) on the MI355X.

    python tools/bench_holefill.py [--steps K] [--out profiles/holefill_bench.json] [--quick]

Throughput.  Cases: the synthetic RGB-D generator's frames (a few, repeated) at 64 x VGA and 8 x 1080p -- they carry the shadow
band left of every object (8 pixels at VGA, 24 at 1080p) and 1 % salt -- and the output of kde_reg_register_batch in point mode
on 8 x (512x424 -> 1920x1080), which has cracks.  The defaults (8 passes, 3 taps, sigma_space 2, sigma_color 30) with r = 1, 2,
3, float and uint16 on both sides, the guard off and on (max_gap 100 mm, gap_rule 1).  Reports per setting the median of K
timed calls after a wake-up load and warm-up (HIP events on the current stream), next to
  (a) the float4 streaming copy of tools/hooks/libkde_hooks.so over the bytes that MUST move -- the depth once, the guide once,
      the output once: the call's fraction of that copy ceiling;
  (b) the same call at passes_per_launch 1: what fusing buys; and, for float frames without and with the guard, every k = 1 .. 4;
  (c) a call on the same frames with every hole closed beforehand: the floor, every tile on the copy path, at the library's
      k and at every k = 1 .. 4;
  (d) kde_jbf_process_batch (no pre-smoothing) at window 19, the smallest that reaches across the generator's VGA band: the
      only way to close such a band before;
  (e) the road through the host, on the first frame of the case (not the registration case): the frames copied out, the numpy
      statement of the rule (tests/holefill_cases.py) run there, the result copied back.
The tool checks the device's bytes against the statement on that frame.

Quality, at VGA.  The generator gives no truth under its shadow bands (its noise-free depth is 0 there), so the holes that are
scored are punched by this tool: the hole mask of a generator frame of another seed -- bands of the same width and 1 % salt,
at places unrelated to this frame's edges -- is cut out of the noisy depth in addition to the frame's own holes.  MeanError3D
(the reference's figure, main.cpp:220-308) against the noise-free depth over the punched pixels that have a truth, and the
share of them and of all holes of the input each method closes: the fill (guard off, on with gap_rule 1 and with gap_rule 0), the fill followed by the window-5
JBF, and the window-19 JBF alone.  --quick runs one timed call per measurement and skips (e) and the quality part.
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

#        name     frames  size
CASES = [("vga", 64, (640, 480)), ("1080p", 8, (1920, 1080)), ("registered", 8, (1920, 1080))]
REG_SOURCE = (512, 424)
MAX_GAP, GAP_RULE = 100.0, 1
JBF_WIDE = 19
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
    import holefill_cases as HC
    from kinectdepthmapenhancement_amd import _native, filters, synth
    from tools.hooks import hooks
    from tools.wake import wake
    torch.cuda.set_device(0)
    stream = lambda: torch.cuda.current_stream().cuda_stream
    FLT_MAX = float(HC.FLT_MAX)
    defaults = filters.DepthHoleFilling.default_params()

    def params(radius, gap=0.0, fuse=0):
        return _native.HolefillParams(radius, defaults.iterations, defaults.min_taps, defaults.sigma_space, defaults.sigma_color, gap,
                                      GAP_RULE if gap else 0, 0.0, FLT_MAX, fuse)

    res = {"device": torch.cuda.get_device_name(0), "steps": a.steps, "iterations": defaults.iterations, "min_taps": defaults.min_taps,
           "sigma_space": defaults.sigma_space, "sigma_color": defaults.sigma_color, "max_gap": MAX_GAP, "gap_rule": GAP_RULE,
           "jbf_wide_window": JBF_WIDE, "cases": [], "quality": []}

    def jbf(size, n, window):
        p = filters.JointBilateralFilter.default_params()
        p.window_size, p.presmooth = window, 0
        return filters.JointBilateralFilter(size[0], size[1], p, max_batch=n)

    for name, n, size in CASES:
        w, h = size
        px = n * w * h
        if name == "registered":                                       # the generator's depth at 512 x 424, warped to 1080p in point mode
            made = [synth.make_frame(31 + k, *REG_SOURCE) for k in range(DISTINCT)]
            K = synth.intrinsics(w, h)
            G = filters.DepthRegistration(REG_SOURCE, size, DISTINCT, _native.RegParams(0.0, FLT_MAX, 0))
            G.set_calibration(same_view(K, REG_SOURCE, size), K, np.eye(3), (12.0, 0.0, 0.0))
            depth_head = np.rint(G.register(torch.from_numpy(np.stack([m[1] for m in made])).cuda()).cpu().numpy())
            G.close()
            bgr_head = np.stack([synth.make_frame(31 + k, w, h)[0] for k in range(DISTINCT)])
        else:
            made = [synth.make_frame(31 + k, w, h) for k in range(DISTINCT)]
            bgr_head = np.stack([m[0] for m in made])
            depth_head = np.rint(np.stack([m[1] for m in made]))       # whole millimetres: the same scene in both formats
        bgr = torch.from_numpy(np.concatenate([bgr_head] * (n // DISTINCT))).cuda()
        depth = torch.from_numpy(np.concatenate([depth_head] * (n // DISTINCT))).cuda()
        sources = {"f32": depth, "u16": depth.to(torch.int32).to(torch.int16)}
        outs = {"f32": torch.empty((n, h, w), dtype=torch.float32, device="cuda"),
                "u16": torch.empty((n, h, w), dtype=torch.int16, device="cuda")}
        esz = {"f32": 4, "u16": 2}

        def copy_ms(nbytes):
            s = torch.empty(nbytes // 2, dtype=torch.uint8, device="cuda")
            d = torch.empty_like(s)
            ms, _ = timed(torch, lambda: hooks.hbm_copy(s, d, stream()), a.steps, a.warmup)
            return ms

        copies = {fmt: copy_ms(px * (2 * esz[fmt] + 3)) for fmt in esz}

        def entry(ms, ms_min, fmt):
            must = px * (2 * esz[fmt] + 3)
            return {"bytes_must_move": must, "ms_per_call": round(ms, 4), "ms_min": round(ms_min, 4), "ms_per_frame": round(ms / n, 5),
                    "gpixel_per_s": round(px / (ms * 1e-3) / 1e9, 3), "copy_same_bytes_ms": round(copies[fmt], 4),
                    "fraction_of_copy_ceiling": round(copies[fmt] / ms, 4)}

        def run(radius, gap, fuse, fmt, src=None):
            H = filters.DepthHoleFilling(size, n, params(radius, gap, fuse))
            s, o = (sources[fmt] if src is None else src), outs[fmt]
            ms, ms_min = timed(torch, lambda: H.fill(s, bgr, o), a.steps, a.warmup)
            r = entry(ms, ms_min, fmt)
            r["passes_per_launch"] = H.passes_per_launch()
            r["filled"], r["remaining"] = int(H.filled().sum()), int(H.remaining().sum())
            return H, r

        wake(torch)
        holes = int((depth_head == 0).sum()) * (n // DISTINCT)
        case = {"case": name, "frames": n, "size": [w, h], "hole_fraction_in": round(holes / px, 4), "copy_ms": {k: round(v, 4) for k, v in copies.items()}}
        for radius in (1, 2, 3):
            for gap in (0.0, MAX_GAP):
                for fmt in ("f32", "u16"):
                    H, r = run(radius, gap, 0, fmt)
                    r["closed_fraction"] = round(r["filled"] / max(holes, 1), 4)
                    if not a.quick and name != "registered" and radius == 2 and (name == "vga" or (fmt == "f32" and not gap)):
                        dt = np.float32 if fmt == "f32" else np.uint16
                        want, _, filled, remaining = HC.fill(depth_head[0].astype(dt), bgr_head[0], H.space_table(), H.range_table(), dt, radius=radius,
                                                              iterations=defaults.iterations, min_taps=defaults.min_taps, max_gap=gap,
                                                              gap_rule=GAP_RULE if gap else 0)
                        got = outs[fmt][:1].cpu().numpy()
                        got = got.view(np.uint16) if fmt == "u16" else got
                        r["equals_statement"] = bool(got[0].tobytes() == want.tobytes() and int(H.filled()[0]) == filled and int(H.remaining()[0]) == remaining)
                    H.close()
                    H1, r1 = run(radius, gap, 1, fmt)                  # (b)
                    H1.close()
                    r["ms_at_one_pass_per_launch"] = r1["ms_per_call"]
                    r["fusing_buys"] = round(r1["ms_per_call"] / r["ms_per_call"], 3)
                    case[f"r{radius}_{'guard' if gap else 'plain'}_{fmt}"] = r
            for gap, key in ((0.0, f"r{radius}_ms_by_passes_per_launch"), (MAX_GAP, f"r{radius}_guard_ms_by_passes_per_launch")):
                sweep = {}
                for fuse in (1, 2, 3, 4):
                    Hk, rk = run(radius, gap, fuse, "f32")
                    Hk.close()
                    sweep[str(fuse)] = rk["ms_per_call"]
                case[key] = sweep
        # (c) the floor: the same frames with every hole closed by a first call
        H, _ = run(2, 0.0, 0, "f32")
        closed = outs["f32"].clone()
        for _ in range(4):
            closed = H.fill(closed, bgr, torch.empty_like(closed))
        H.close()
        closed = torch.where(closed > 0, closed, torch.full_like(closed, 3000.0))
        H, r = run(2, 0.0, 0, "f32", closed)
        H.close()
        assert r["filled"] == 0 and r["remaining"] == 0
        case["hole_free_floor_r2_f32"] = r
        case["hole_free_floor_r2_f32_ms_by_passes_per_launch"] = {}
        for fuse in (1, 2, 3, 4):                                      # the floor is a copy per launch: 8, 4, 3 and 2 of them
            Hk, rk = run(2, 0.0, fuse, "f32", closed)
            Hk.close()
            case["hole_free_floor_r2_f32_ms_by_passes_per_launch"][str(fuse)] = rk["ms_per_call"]
        # (d) the wide-window JBF on the same frames
        J = jbf(size, n, JBF_WIDE)
        ms, ms_min = timed(torch, lambda: J.process_batch(sources["f32"], bgr, outs["f32"]), a.steps, a.warmup)
        J.close()
        case[f"jbf_window_{JBF_WIDE}_f32"] = {"ms_per_call": round(ms, 4), "ms_min": round(ms_min, 4),
                                             "over_fill_r2_plain_f32": round(ms / case["r2_plain_f32"]["ms_per_call"], 2)}
        if not a.quick and name != "registered":
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            hd, hb = sources["f32"][:1].cpu().numpy(), bgr[:1].cpu().numpy()
            t1 = time.perf_counter()
            up = HC.fill(hd[0], hb[0], HC.space_table(2, defaults.sigma_space), HC.range_table(defaults.sigma_color), radius=2,
                         iterations=defaults.iterations, min_taps=defaults.min_taps)[0]
            t2 = time.perf_counter()
            torch.from_numpy(up).cuda()
            torch.cuda.synchronize()
            t3 = time.perf_counter()
            case["host_road"] = {"frames": 1, "copies_s_per_frame": round(t1 - t0 + t3 - t2, 5), "numpy_s_per_frame": round(t2 - t1, 4),
                                 "total_over_device_call": round((t3 - t0) * 1e3 / case["r2_plain_f32"]["ms_per_frame"], 1)}
        res["cases"].append(case)
        print(json.dumps(case), flush=True)
        del depth, sources, outs, bgr, closed

    if not a.quick:
        w, h = size = (640, 480)
        n = DISTINCT
        made = [synth.make_frame(31 + k, w, h, clean=True) for k in range(n)]
        other = [synth.make_frame(131 + k, w, h)[1] == 0 for k in range(n)]
        bgr_np, noisy, truth = (np.stack([m[i] for m in made]) for i in range(3))
        punched = np.stack(other)
        own = noisy == 0
        given = np.where(punched, np.float32(0), noisy)
        scored = punched & ~own & (truth > 0)                           # made holes by this tool, with a truth under them
        holes = given == 0
        bgr, depth = torch.from_numpy(bgr_np).cuda(), torch.from_numpy(given).cuda()
        results = {}
        for label, gap, rule in (("fill_r2", 0.0, 0), ("fill_r2_guard", MAX_GAP, GAP_RULE), ("fill_r2_guard_heaviest", MAX_GAP, 0)):
            q = params(2, gap)
            q.gap_rule = rule
            H = filters.DepthHoleFilling(size, n, q)
            results[label] = H.fill(depth, bgr, torch.empty_like(depth))
            H.close()
        J5, JW = jbf(size, n, 5), jbf(size, n, JBF_WIDE)
        results["fill_r2_then_jbf5"] = J5.process_batch(results["fill_r2"], bgr, torch.empty_like(depth))
        results["fill_r2_guard_then_jbf5"] = J5.process_batch(results["fill_r2_guard"], bgr, torch.empty_like(depth))
        results[f"jbf{JBF_WIDE}_alone"] = JW.process_batch(depth, bgr, torch.empty_like(depth))
        results["jbf5_alone"] = J5.process_batch(depth, bgr, torch.empty_like(depth))
        mask = torch.from_numpy(scored).cuda()
        cands = {k: torch.where(mask, v, torch.zeros_like(v)) for k, v in results.items()}
        K = synth.intrinsics(w, h)
        E = filters.MeanError3D(w, h, n, len(cands))
        E.set_camera(K)
        E.compare(list(cands.values()), torch.from_numpy(truth).cuda())
        table = E.results_host()
        q = {"size": [w, h], "frames": n, "holes_in": int(holes.sum()), "own_holes": int(own.sum()), "punched_and_scored": int(scored.sum()), "methods": {}}
        for c, label in enumerate(cands):
            z = results[label].cpu().numpy()
            count = int(table["count"][:, c].sum())
            q["methods"][label] = {"mean_error_3d_mm_over_scored_holes": round(float(np.sum(table["sum"][:, c]) / max(1, count)), 4),
                                   "scored_holes_closed": round(count / int(scored.sum()), 4),
                                   "all_holes_closed": round(int(((z > 0) & holes).sum()) / int(holes.sum()), 4)}
        E.close()
        J5.close()
        JW.close()
        res["quality"].append(q)
        print(json.dumps(q), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
