"""Host-fed JointBilateralFilter::Process (kde_jbf_feed_process) against the resident batch and the host link.

For 64 x 640x480 at window 11 (bench.py's headline) and 32 x 1920x1080 at window 19 (its 1080p leg), on the synthetic
frames of synth.py (8 distinct frames tiled to the batch, as bench.py does), one JSON line with:
  * resident: kde_jbf_process_batch on frames already in HBM, HIP events around each call (bench.py's figure);
  * link: pinned hipMemcpyAsync of the same byte counts -- copy-in (f32: 7 B/px, u16: 5 B/px) and copy-out (4 B/px)
    alone, and both at once on two streams -- and the rate the concurrent copy bounds (`link_bound_mpix_s`);
  * host_fed: the feed's wall time per call for pinned and pageable buffers, float and uint16 depth, chunk in
    {1, 2, 4, 8, 16, 32}, with the per-stream event spans, and `frac` = host-fed rate / min(resident, link bound).
Every figure is the median of --steps timed repetitions after --warmup untimed ones (and a wake-up load first).

usage: python tools/bench_host_feed.py [--steps 5] [--warmup 2] [--out FILE] [--configs vga_w11,fhd_w19]
       python tools/bench_host_feed.py --trace-one      # one warm-up + ONE host-fed call (pinned, f32, chunk 8, VGA):
                                                         # the command to run under rocprofv3 --kernel-trace --memory-copy-trace
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

CONFIGS = {"vga_w11": (64, 640, 480, 11), "fhd_w19": (32, 1920, 1080, 19)}
SIGMAS = (3.0, 7.65, 20.0)           # bench.py: spatial, colour, depth
CHUNKS = (1, 2, 4, 8, 16, 32)


def frames(synth, n, w, h, distinct=8):
    bgr, depth = synth.make_batch(1000, min(distinct, n), w, h)
    reps = -(-n // bgr.shape[0])
    return np.ascontiguousarray(np.tile(bgr, (reps, 1, 1, 1))[:n]), np.ascontiguousarray(np.tile(depth, (reps, 1, 1))[:n])


def make_jbf(F, w, h, window, n):
    p = F.JointBilateralFilter.default_params()
    p.window_size, (p.spatial_sigma, p.color_sigma, p.depth_sigma) = window, SIGMAS
    return F.JointBilateralFilter(w, h, p, max_batch=n)


def event_median(torch, fn, steps, warmup):
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
    return float(np.median(ms)), ms


def resident(torch, jbf, bgr, depth, steps, warmup):
    d, c = torch.from_numpy(depth).cuda(), torch.from_numpy(bgr).cuda()
    out = torch.empty_like(d)
    fn = lambda: jbf.process_batch(d, c, out)
    t0 = time.perf_counter()
    while time.perf_counter() - t0 < 0.15:          # wake-up: an idle MI355X needs ~100 ms of load to reach its clock
        fn()
        torch.cuda.synchronize()
    med, ms = event_median(torch, fn, steps, warmup)
    return {"ms": med, "ms_all": ms, "mpix_s": depth.size / (med * 1e-3) / 1e6}


def link(torch, px, in_bpp, steps, warmup):
    """pinned copies of px * in_bpp bytes in and px * 4 out: each alone, then both at once on two streams"""
    h_in = torch.empty(px * in_bpp, dtype=torch.uint8, pin_memory=True)
    h_out = torch.empty(px * 4, dtype=torch.uint8, pin_memory=True)
    d_in = torch.empty(px * in_bpp, dtype=torch.uint8, device="cuda")
    d_out = torch.empty(px * 4, dtype=torch.uint8, device="cuda")
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    cur = torch.cuda.current_stream()

    def both(h2d=True, d2h=True):
        s1.wait_stream(cur)
        s2.wait_stream(cur)
        if h2d:
            with torch.cuda.stream(s1):
                d_in.copy_(h_in, non_blocking=True)
        if d2h:
            with torch.cuda.stream(s2):
                h_out.copy_(d_out, non_blocking=True)
        cur.wait_stream(s1)
        cur.wait_stream(s2)

    h2d_ms, _ = event_median(torch, lambda: both(d2h=False), steps, warmup)
    d2h_ms, _ = event_median(torch, lambda: both(h2d=False), steps, warmup)
    both_ms, _ = event_median(torch, both, steps, warmup)
    del h_in, h_out, d_in, d_out
    return {"in_bytes_per_px": in_bpp, "h2d_GBs": px * in_bpp / (h2d_ms * 1e-3) / 1e9, "d2h_GBs": px * 4 / (d2h_ms * 1e-3) / 1e9,
            "concurrent_ms": both_ms, "concurrent_h2d_GBs": px * in_bpp / (both_ms * 1e-3) / 1e9,
            "concurrent_d2h_GBs": px * 4 / (both_ms * 1e-3) / 1e9, "link_bound_mpix_s": px / (both_ms * 1e-3) / 1e6}


def host_fed(torch, F, jbf, depth_in, bgr_in, out, chunk, steps, warmup):
    feed = F.JointBilateralFilterFeed(jbf, chunk)
    for _ in range(warmup):
        feed.process(depth_in, bgr_in, out)
    runs = []
    for _ in range(steps):
        feed.process(depth_in, bgr_in, out)
        runs.append(feed.last_stats())
    feed.close()
    med = lambda k: float(np.median([r[k] for r in runs]))
    px = int(np.prod(out.shape))
    return {"chunk": chunk, "wall_ms": med("wall_ms"), "wall_ms_all": [round(r["wall_ms"], 4) for r in runs],
            "h2d_ms": med("h2d_ms"), "compute_ms": med("compute_ms"), "d2h_ms": med("d2h_ms"),
            "inputs_staged": runs[-1]["inputs_staged"], "outputs_staged": runs[-1]["outputs_staged"],
            "h2d_bytes": runs[-1]["h2d_bytes"], "d2h_bytes": runs[-1]["d2h_bytes"], "mpix_s": px / (med("wall_ms") * 1e-3) / 1e6}


def run_config(torch, F, synth, name, steps, warmup, chunks):
    n, w, h, window = CONFIGS[name]
    bgr, depth = frames(synth, n, w, h)
    d16 = np.where(depth > 0, np.rint(depth), 0).astype(np.uint16)
    jbf = make_jbf(F, w, h, window, n)
    px = n * w * h
    res = {"frames": n, "width": w, "height": h, "window": window, "sigmas": list(SIGMAS)}
    res["resident"] = resident(torch, jbf, bgr, depth, steps, warmup)
    res["link"] = {"f32": link(torch, px, 7, steps, warmup), "u16": link(torch, px, 5, steps, warmup)}
    pinned = {"f32": torch.from_numpy(depth).pin_memory(), "u16": torch.from_numpy(d16.view(np.int16)).pin_memory(),
              "bgr": torch.from_numpy(bgr).pin_memory(), "out": torch.empty(depth.shape, dtype=torch.float32, pin_memory=True)}
    pageable = {"f32": depth, "u16": d16, "bgr": bgr, "out": np.empty(depth.shape, np.float32)}
    res["host_fed"] = {}
    for mem, bufs in (("pinned", pinned), ("pageable", pageable)):
        for fmt in ("f32", "u16"):
            din = bufs[fmt]
            if mem == "pinned" and fmt == "u16":            # the same pinned bytes seen as uint16 (numpy view, no copy)
                din = bufs[fmt].numpy().view(np.uint16)
            bound = min(res["resident"]["mpix_s"], res["link"][fmt]["link_bound_mpix_s"])
            rows = []
            for chunk in chunks:
                r = host_fed(torch, F, jbf, din, bufs["bgr"], bufs["out"], chunk, steps, warmup)
                r["frac"] = r["mpix_s"] / bound
                rows.append(r)
            res["host_fed"][f"{mem}_{fmt}"] = rows
    # the figures the PR / DESIGN quote: pinned rate at the best chunk >= 8 over min(resident, link bound)
    best = {}
    for key, rows in res["host_fed"].items():
        cand = [r for r in rows if r["chunk"] >= 8] or rows
        b = max(cand, key=lambda r: r["mpix_s"])
        best[key] = {"chunk": b["chunk"], "mpix_s": b["mpix_s"], "frac": b["frac"]}
    res["best_chunk_ge8"] = best
    del pinned
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--configs", default="vga_w11,fhd_w19")
    ap.add_argument("--chunks", default=",".join(map(str, CHUNKS)))
    ap.add_argument("--out", default="")
    ap.add_argument("--trace-one", action="store_true")
    args = ap.parse_args()
    if args.steps < 5:
        raise SystemExit("--steps must be >= 5 (median of at least five)")
    import torch
    from kinectdepthmapenhancement_amd import filters as F, synth
    if not torch.cuda.is_available():
        raise SystemExit("bench_host_feed needs a GPU (the feed has no CPU path)")
    torch.cuda.set_device(0)
    if args.trace_one:
        n, w, h, window = CONFIGS["vga_w11"]
        bgr, depth = frames(synth, n, w, h)
        pd, pc = torch.from_numpy(depth).pin_memory(), torch.from_numpy(bgr).pin_memory()
        out = torch.empty(depth.shape, dtype=torch.float32, pin_memory=True)
        feed = F.JointBilateralFilterFeed(make_jbf(F, w, h, window, 1), 8)
        feed.process(pd, pc, out)        # warm-up: sizes the slots, loads the kernels
        torch.cuda.synchronize()
        feed.process(pd, pc, out)
        print(json.dumps({"trace_one": feed.last_stats(), "frames": n, "width": w, "height": h, "window": window, "chunk": 8,
                          "buffers": "pinned", "depth": "f32"}))
        return
    chunks = [int(c) for c in args.chunks.split(",")]
    line = {"tool": "bench_host_feed", "device": torch.cuda.get_device_name(0), "steps": args.steps, "warmup": args.warmup,
            "statistic": "median", "configs": {}}
    for name in args.configs.split(","):
        line["configs"][name] = run_config(torch, F, synth, name, args.steps, args.warmup, chunks)
    text = json.dumps(line)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
