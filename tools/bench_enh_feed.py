"""Host-fed KinectDepthEnhancement::Process (kde_enh_feed_process) against the resident batch and a serial host round trip.

For 64 x 640x480 and 8 x 1920x1080 with 15 x 20 superpixels, on the synthetic frames of synth.py (8 distinct frames tiled to
the batch, as bench.py does), one JSON line with, all measured in this one process:
  * resident: kde_enh_process_batch on frames already in HBM, HIP events around each call;
  * serial: what a caller without the feed writes -- on ONE stream, from and to pinned memory: copy-in of the depth (uint16 or
    float) and the colour, the widening of uint16 depth, kde_enh_process_batch on the whole batch, kde_points_to_depth for the
    two depth formats, copy-out of the same bytes the feed returns (12, 4 or 2 B/px) -- host clock, start to synchronised end;
  * host_fed: the feed's wall time per call for pinned and pageable buffers, uint16 and float depth, the three output
    formats and chunk in {1, 2, 4, ..., max_batch}, with the per-stream event spans;
  * headline: for pinned uint16 input and each output format, feed wall time at its best chunk over the serial wall time,
    with the spread (min and max of the repetitions) of both, and whether the feed's gain exceeds the serial baseline's own
    run-to-run spread.
Every figure is the median of --steps timed repetitions after --warmup untimed ones (and a wake-up load first).

usage: python tools/bench_enh_feed.py [--steps 5] [--warmup 2] [--out FILE] [--configs vga,fhd]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

CONFIGS = {"vga": (64, 640, 480), "fhd": (8, 1920, 1080)}
ROWS, COLS = 15, 20
OUTPUTS = {"points": (12, np.float32, (3,)), "depth": (4, np.float32, ()), "depth_u16": (2, np.uint16, ())}


def frames(synth, n, w, h, distinct=8):
    bgr, depth = synth.make_batch(1000, min(distinct, n), w, h)
    reps = -(-n // bgr.shape[0])
    return np.ascontiguousarray(np.tile(bgr, (reps, 1, 1, 1))[:n]), np.ascontiguousarray(np.tile(depth, (reps, 1, 1))[:n])


def pinned(torch, a):
    """a pinned copy of `a` as a numpy array (uint16 through an int16 tensor) and the tensor that owns the memory"""
    t = torch.from_numpy(a.view(np.int16) if a.dtype == np.uint16 else a).pin_memory()
    return t.numpy().view(a.dtype), t


def summary(ms):
    return {"ms": float(np.median(ms)), "ms_min": float(min(ms)), "ms_max": float(max(ms)), "ms_all": [round(float(v), 4) for v in ms]}


def resident(torch, enh, bgr, depth, steps, warmup):
    d, c = torch.from_numpy(depth).cuda(), torch.from_numpy(bgr).cuda()
    fn = lambda: enh.process_batch(d, c)
    t0 = time.perf_counter()
    while time.perf_counter() - t0 < 0.15:          # wake-up: an idle MI355X needs ~100 ms of load to reach its clock
        fn()
        torch.cuda.synchronize()
    for _ in range(warmup):
        fn()
    ms = []
    for _ in range(steps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    r = summary(ms)
    r["mpix_s"] = depth.size / (r["ms"] * 1e-3) / 1e6
    return r


def serial(torch, F, enh, depth_t, bgr_t, out_t, output, steps, warmup):
    """pinned tensors in and out, everything on torch's current stream, one batch"""
    n, h, w = depth_t.shape
    d_in = torch.empty_like(depth_t, device="cuda")
    d_f32 = d_in if depth_t.dtype == torch.float32 else torch.empty((n, h, w), dtype=torch.float32, device="cuda")
    c_in = torch.empty_like(bgr_t, device="cuda")
    o_dev = None if output == "points" else torch.empty((n, h, w), dtype=out_t.dtype, device="cuda")

    def fn():
        d_in.copy_(depth_t, non_blocking=True)
        c_in.copy_(bgr_t, non_blocking=True)
        if d_f32 is not d_in:
            d_f32.copy_(d_in)                       # int16 view of uint16 millimetres below 32768: the same values
        enh.process_batch(d_f32, c_in)
        pts = enh.getOptimizedPoints_Device().reshape(n, h, w, 3)
        if output == "points":
            out_t.copy_(pts, non_blocking=True)
        else:
            F.points_to_depth(pts, o_dev, dtype=out_t.dtype)
            out_t.copy_(o_dev, non_blocking=True)
        torch.cuda.current_stream().synchronize()

    for _ in range(warmup):
        fn()
    ms = []
    for _ in range(steps):
        t0 = time.perf_counter()
        fn()
        ms.append((time.perf_counter() - t0) * 1e3)
    return summary(ms)


def host_fed(F, enh, depth_in, bgr_in, out, output, chunk, steps, warmup):
    feed = F.KinectDepthEnhancementFeed(enh, chunk)
    for _ in range(warmup):
        feed.process(depth_in, bgr_in, out, output=output)
    runs = []
    for _ in range(steps):
        feed.process(depth_in, bgr_in, out, output=output)
        runs.append(feed.last_stats())
    feed.close()
    med = lambda k: float(np.median([r[k] for r in runs]))
    r = summary([r["wall_ms"] for r in runs])
    r.update({"chunk": chunk, "h2d_ms": med("h2d_ms"), "compute_ms": med("compute_ms"), "d2h_ms": med("d2h_ms"),
              "inputs_staged": runs[-1]["inputs_staged"], "outputs_staged": runs[-1]["outputs_staged"],
              "h2d_bytes": runs[-1]["h2d_bytes"], "d2h_bytes": runs[-1]["d2h_bytes"]})
    return r


def run_config(torch, F, synth, name, steps, warmup):
    n, w, h = CONFIGS[name]
    bgr, depth = frames(synth, n, w, h)
    d16 = np.where(depth > 0, np.rint(depth), 0).astype(np.uint16)
    assert d16.max() < 32768                        # the serial baseline widens through torch's int16
    enh = F.KinectDepthEnhancement(w, h, max_batch=n)
    enh.SetParametor(ROWS, COLS, synth.intrinsics(w, h))
    chunks = [c for c in (1, 2, 4, 8, 16, 32, 64) if c <= n]
    res = {"frames": n, "width": w, "height": h, "superpixels": [ROWS, COLS], "chunks": chunks}
    res["resident"] = resident(torch, enh, bgr, depth, steps, warmup)
    pin = {"f32": pinned(torch, depth), "u16": pinned(torch, d16), "bgr": pinned(torch, bgr)}
    page = {"f32": depth, "u16": d16, "bgr": bgr}
    res["serial"], res["host_fed"], res["headline"] = {}, {}, {}
    for output, (_, odt, trailing) in OUTPUTS.items():
        shape = (n, h, w) + trailing
        out_pin, out_t = pinned(torch, np.zeros(shape, odt))
        out_page = np.zeros(shape, odt)
        for fmt in ("u16", "f32"):
            res["serial"][f"{fmt}_{output}"] = serial(torch, F, enh, pin[fmt][1], pin["bgr"][1], out_t, output, steps, warmup)
            for mem, bufs, out in (("pinned", {k: v[0] for k, v in pin.items()}, out_pin), ("pageable", page, out_page)):
                res["host_fed"][f"{mem}_{fmt}_{output}"] = [host_fed(F, enh, bufs[fmt], bufs["bgr"], out, output, c, steps, warmup)
                                                            for c in chunks]
        base = res["serial"][f"u16_{output}"]
        best = min(res["host_fed"][f"pinned_u16_{output}"], key=lambda r: r["ms"])
        res["headline"][output] = {
            "input": "pinned u16", "best_chunk": best["chunk"], "feed_ms": best["ms"], "feed_ms_min": best["ms_min"],
            "feed_ms_max": best["ms_max"], "serial_ms": base["ms"], "serial_ms_min": base["ms_min"], "serial_ms_max": base["ms_max"],
            "feed_over_serial": best["ms"] / base["ms"], "feed_over_resident": best["ms"] / res["resident"]["ms"],
            "mpix_s": n * w * h / (best["ms"] * 1e-3) / 1e6,
            # the gain counts only when it is larger than what the baseline varies by from run to run
            "beats_serial_beyond_its_spread": bool(base["ms"] - best["ms"] > base["ms_max"] - base["ms_min"])}
        del out_t
    enh.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--configs", default="vga,fhd")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    if args.steps < 5:
        raise SystemExit("--steps must be >= 5 (median of at least five)")
    import torch
    from kinectdepthmapenhancement_amd import filters as F, synth
    if not torch.cuda.is_available():
        raise SystemExit("bench_enh_feed needs a GPU (the feed has no CPU path)")
    torch.cuda.set_device(0)
    line = {"tool": "bench_enh_feed", "device": torch.cuda.get_device_name(0), "steps": args.steps, "warmup": args.warmup,
            "statistic": "median", "configs": {}}
    for name in args.configs.split(","):
        line["configs"][name] = run_config(torch, F, synth, name, args.steps, args.warmup)
    text = json.dumps(line)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
