"""Throughput and quality of DepthTemporalFilter (temporal_kernels.hip) on the MI355X.

    python tools/bench_temporal.py [--steps K] [--out profiles/temporal_bench.json] [--quick] [--only vga|1080p]

Throughput.  64 x VGA and 8 x 1080p as ONE sequence each (synth.make_sequence: a static scene, one moving rectangle, depth
noise and dropouts drawn per frame), float and uint16 (the same format on both sides), with and without guide.  Reports per
setting the median of K timed calls after a wake-up load and warm-up (HIP events on the current stream), next to
  (a) the float4 streaming copy of tools/hooks/libkde_hooks.so over the bytes that MUST move -- depth in, depth out and the guide
      per frame, plus 16 B per pixel of state per call (8 B read, 8 B written): the call's fraction of that copy ceiling;
  (b) the same frames as n calls of one frame, the live case, which pays for the state n times;
  (c) kde_buffer2d_update_sequence on the same float frames: the one other code that looks along time, a plain average with one
      output for the whole sequence;
  (d) the numpy statement of the rule (tests/temporal_cases.py) on the host, on the first frames.
The tool checks the device's depth, state and counts against the statement on the first frames of every case.

The P x U table: every pixels-per-thread (1, 2, 4, 8) and load-ahead (1, 2, 4) at both shapes, float with the guide and uint16
without, through kde_temporal_set_shape; the library's own choice is named beside it.

Quality (MeanError3D against the generator's noise-free truth, 32 x VGA, frames 4 .. 31): the raw sequence, the temporal filter at
every color_thresh candidate (24, 48, 96, 765) and without a guide, DepthHoleFilling alone and the temporal filter followed by it;
over the whole frame, over the static region (never covered by the rectangle) and over the rectangle's trail (covered within the
last eight frames, not now), so that ghosting shows as a number.  --quick runs one timed call per measurement and skips (d)."""
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
SHAPES = [(p, u) for p in (1, 2, 4, 8) for u in (1, 2, 4)]
CANDIDATES = (24, 48, 96, 765)


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
    import temporal_cases as TC
    from kinectdepthmapenhancement_amd import _native, filters, synth
    from tools.hooks import hooks
    from tools.wake import wake
    torch.cuda.set_device(0)
    stream = lambda: torch.cuda.current_stream().cuda_stream
    d = filters.DepthTemporalFilter.default_params()

    def params(color_thresh=None):
        return _native.TemporalParams(d.alpha, d.max_diff, d.rel_diff, d.persist_min, d.color_thresh if color_thresh is None else color_thresh,
                                      d.z_min, d.z_max)

    def statement_params(color_thresh=None):
        return dict(alpha=d.alpha, max_diff=d.max_diff, rel_diff=d.rel_diff, persist_min=d.persist_min,
                    color_thresh=d.color_thresh if color_thresh is None else color_thresh, z_min=d.z_min, z_max=d.z_max)

    res = {"device": torch.cuda.get_device_name(0), "steps": a.steps,
           "defaults": {k: getattr(d, k) for k, _ in d._fields_}, "cases": [], "quality": []}
    esz = {"f32": 4, "u16": 2}
    for name, n, size in CASES:
        if a.only and a.only != name:
            continue
        w, h = size
        px = w * h
        bgr_np, depth_np, _, _ = synth.make_sequence(7, n, w, h)
        depth_np = np.rint(depth_np).astype(np.float32)             # whole millimetres: the same scene in both formats
        bgr = torch.from_numpy(bgr_np).cuda()
        sources = {"f32": torch.from_numpy(depth_np).cuda(), "u16": torch.from_numpy(depth_np.astype(np.uint16).view(np.int16)).cuda()}
        outs = {"f32": torch.empty((n, h, w), dtype=torch.float32, device="cuda"), "u16": torch.empty((n, h, w), dtype=torch.int16, device="cuda")}

        def copy_ms(nbytes):
            s = torch.empty(nbytes // 2, dtype=torch.uint8, device="cuda")
            t = torch.empty_like(s)
            return timed(torch, lambda: hooks.hbm_copy(s, t, stream()), a.steps, a.warmup)[0]

        def must_move(frames, fmt, guide):
            return frames * px * (2 * esz[fmt] + (3 if guide else 0)) + 16 * px

        wake(torch)
        case = {"case": name, "frames": n, "size": [w, h]}
        T = filters.DepthTemporalFilter(size, n, params())
        case["library_shape"] = {"batch": list(T.shape(n)), "live": list(T.shape(1))}
        for fmt in ("f32", "u16"):
            for guide in (False, True):
                key = f"{fmt}{'_guide' if guide else ''}"
                s, o, g = sources[fmt], outs[fmt], (bgr if guide else None)
                T.reset()
                ms, ms_min = timed(torch, lambda: T.filter(s, g, o), a.steps, a.warmup)
                must = must_move(n, fmt, guide)
                cp = copy_ms(must)
                r = {"bytes_must_move": must, "ms_per_call": round(ms, 4), "ms_min": round(ms_min, 4), "ms_per_frame": round(ms / n, 5),
                     "gpixel_per_s": round(n * px / (ms * 1e-3) / 1e9, 3), "copy_same_bytes_ms": round(cp, 4),
                     "fraction_of_copy_ceiling": round(cp / ms, 4)}
                # (b) the live case: n calls of one frame
                T.reset()

                def live():
                    for f in range(n):
                        T.filter(s[f:f + 1], None if g is None else g[f:f + 1], o[f:f + 1])

                lms, lmin = timed(torch, live, max(1, a.steps // 4), 1)
                lmust = n * must_move(1, fmt, guide)
                lcp = copy_ms(must_move(1, fmt, guide))
                r["live"] = {"ms_for_n_calls": round(lms, 4), "ms_per_frame": round(lms / n, 5), "bytes_must_move": lmust,
                             "copy_one_frame_ms": round(lcp, 5), "fraction_of_copy_ceiling": round(n * lcp / lms, 4),
                             "live_over_batch": round(lms / ms, 3)}
                # the device against the statement on the first frames
                k = min(n, 4)
                T.reset()
                got = T.filter(s[:k], None if g is None else g[:k], o[:k])
                src_np = depth_np[:k] if fmt == "f32" else depth_np[:k].astype(np.uint16)
                t0 = time.perf_counter()
                want = TC.filter_sequence(src_np, bgr_np[:k] if guide else None, np.float32 if fmt == "f32" else np.uint16, **statement_params())
                r["numpy_statement_s_per_frame"] = round((time.perf_counter() - t0) / k, 4)
                value, hist = T.state()
                gnp = got.cpu().numpy()
                r["equals_statement"] = bool((gnp.view(np.uint16) if fmt == "u16" else gnp).tobytes() == want.out.tobytes() and
                                             value.cpu().numpy().tobytes() == want.value.tobytes() and
                                             hist.cpu().numpy().view(np.uint32).tobytes() == want.hist.tobytes() and
                                             all(getattr(T, c)().tolist() == getattr(want, c).tolist() for c in TC.COUNTS))
                assert r["equals_statement"], (name, key)
                case[key] = r
        # (c) the plain running average over the same float frames
        B = filters.Buffer2D(w, h)
        bms, bmin = timed(torch, lambda: B.updateData(sources["f32"]), a.steps, a.warmup)
        case["buffer2d_update_sequence_f32"] = {"ms_per_call": round(bms, 4), "ms_min": round(bmin, 4), "outputs": 1}
        B.close()
        # the P x U table
        table = {}
        for fmt, guide in (("f32", True), ("u16", False), ("f32", False)):
            key = f"{fmt}{'_guide' if guide else ''}"
            table[key] = {}
            live_table = {}
            for shape in SHAPES:
                T.set_shape(*shape)
                T.reset()
                s, o, g = sources[fmt], outs[fmt], (bgr if guide else None)
                ms, _ = timed(torch, lambda: T.filter(s, g, o), a.steps, a.warmup)
                table[key][f"P{shape[0]}_U{shape[1]}"] = round(ms, 4)
                if shape[1] == 1:
                    lms, _ = timed(torch, lambda: T.filter(s[:1], None if g is None else g[:1], o[:1]), a.steps, a.warmup)
                    live_table[f"P{shape[0]}"] = round(lms, 5)
            table[key + "_one_frame"] = live_table
            T.set_shape(0, 0)
        case["shape_table_ms"] = table
        T.close()
        res["cases"].append(case)
        print(json.dumps(case), flush=True)
        del sources, outs, bgr

    if not a.no_quality and (not a.only or a.only == "vga"):
        w, h, n, first = 640, 480, 32, 4
        bgr_np, depth_np, truth_np, rect = synth.make_sequence(11, n, w, h)
        covered = np.zeros((n, h, w), bool)
        for t, (x0, y0, x1, y1) in enumerate(rect):
            covered[t, y0:y1, x0:x1] = True
        static = ~covered.any(0)
        trail = np.zeros_like(covered)
        for t in range(n):
            trail[t] = covered[max(0, t - 8):t].any(0) & ~covered[t]
        bgr, dg = torch.from_numpy(bgr_np).cuda(), torch.from_numpy(depth_np).cuda()
        results = {"raw": dg}
        H = filters.DepthHoleFilling((w, h), n)
        results["holefill_alone"] = H.fill(dg, bgr, torch.empty_like(dg))
        counts = {}
        for label, thresh, guide in [(f"temporal_t{c}", c, True) for c in CANDIDATES] + [("temporal_no_guide", None, False)]:
            T = filters.DepthTemporalFilter((w, h), n, params(thresh))
            results[label] = T.filter(dg, bgr if guide else None, torch.empty_like(dg))
            counts[label] = {c: int(getattr(T, c)().sum()) for c in TC.COUNTS}
            results[label + "_then_holefill"] = H.fill(results[label], bgr, torch.empty_like(dg))
            T.close()
        H.close()
        labels = list(results)
        E = filters.MeanError3D(w, h, n, 8)
        E.set_camera(synth.intrinsics(w, h))
        q = {"size": [w, h], "frames": n, "judged_frames": [first, n - 1], "step_px_per_frame": [3, 1], "counts": counts, "mean_error_3d_mm": {},
             "valid_pixels": {}}
        regions = {"all": np.ones((n, h, w), bool), "static": np.broadcast_to(static, (n, h, w)), "trail": trail}
        for region, mask in regions.items():
            truth = torch.from_numpy(np.where(mask, truth_np, 0.0).astype(np.float32)).cuda()
            q["mean_error_3d_mm"][region], q["valid_pixels"][region] = {}, {}
            for at in range(0, len(labels), 8):                         # MeanError3D takes eight candidates per call
                some = labels[at:at + 8]
                E.compare([results[label] for label in some], truth)
                table = E.results_host()
                for c, label in enumerate(some):
                    count = int(table["count"][first:, c].sum())
                    q["mean_error_3d_mm"][region][label] = round(float(np.sum(table["sum"][first:, c]) / max(1, count)), 4)
                    q["valid_pixels"][region][label] = count
        E.close()
        err = q["mean_error_3d_mm"]
        best = min(CANDIDATES, key=lambda c: (err["all"][f"temporal_t{c}_then_holefill"], err["trail"][f"temporal_t{c}_then_holefill"]))
        q["color_thresh_winner"] = {"rule": "the lowest whole-frame MeanError3D (to 0.0001 mm) of the temporal filter followed by DepthHoleFilling; "
                                            "on a tie the lowest over the trail, the region the threshold is there for",
                                    "winner": best, "library_default": int(d.color_thresh)}
        res["quality"].append(q)
        print(json.dumps(q), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
