"""Throughput of NormalMapGenerator (normal_kernels.hip) on the MI355X, and the CPU checker as the baseline.

    python tools/bench_normals.py [--steps K] [--out profiles/normals_bench.json] [--quick]

Reports, for BILATERAL and CM at 64 x 640x480 and 32 x 1920x1080: ms per batch call and Mpixel/s (median of K timed calls
after warm-up, HIP events on the current stream), the HBM fraction of the 24 B/px compulsory traffic (12 B of points in,
12 B of normals out) against the 6.2 TB/s streaming-copy ceiling of this chip, the single-thread time of the
CPU checker (tools/normals_ref.c) on one frame of each size, and the checker's band census.  --quick runs one timed call
per case, for a profiler run (rocprofv3 --kernel-trace --stats -- python tools/bench_normals.py --quick).
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

COPY_CEILING_TBS = 6.2
CASES = [(64, 640, 480), (32, 1920, 1080)]


def points(seed, W, H):
    from kinectdepthmapenhancement_amd import synth
    from oracle import oracle as O
    _, depth = synth.make_frame(seed, W, H)
    return O.p2r_depth(depth, synth.intrinsics(W, H)).view(np.float32).reshape(H, W, 3).copy()


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
    from kinectdepthmapenhancement_amd import filters
    from tools import normals_ref as R
    torch.cuda.set_device(0)
    res = {"device": torch.cuda.get_device_name(0), "steps": a.steps, "cases": [], "cpu_checker": [], "band_census": {}}
    for n, W, H in CASES:
        frames = [points(s, W, H) for s in (1, 2, 3, 4)]
        batch = torch.from_numpy(np.stack([frames[k % 4] for k in range(n)])).cuda()
        out = torch.empty_like(batch)
        g = filters.NormalMapGenerator(W, H, max_batch=n)
        for name, method in (("BILATERAL", g.BILATERAL), ("CM", g.CM)):
            g.setNormalEstimationMethods(method)
            for _ in range(a.warmup):
                g.generateNormalMapBatch(n, batch, out)
            torch.cuda.synchronize()
            ts = []
            for _ in range(a.steps):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                g.generateNormalMapBatch(n, batch, out)
                e1.record()
                e1.synchronize()
                ts.append(e0.elapsed_time(e1))
            ms = float(np.median(ts))
            px = n * W * H
            hbm = 24.0 * px / (ms * 1e-3) / 1e12
            res["cases"].append({"method": name, "frames": n, "width": W, "height": H, "ms_per_call": round(ms, 4),
                                 "mpixel_per_s": round(px / (ms * 1e-3) / 1e6, 1), "compulsory_tb_per_s": round(hbm, 4),
                                 "hbm_fraction": round(hbm / COPY_CEILING_TBS, 4), "ms_min": round(min(ts), 4)})
            print(json.dumps(res["cases"][-1]), flush=True)
        g.close()
        if not a.quick:
            for name, method in (("BILATERAL", R.BILATERAL), ("CM", R.CM)):
                t0 = time.perf_counter()
                R.normals(frames[0], method, want_band=False)
                dt = time.perf_counter() - t0
                res["cpu_checker"].append({"method": name, "width": W, "height": H, "ms_per_frame": round(dt * 1e3, 2),
                                           "mpixel_per_s": round(W * H / dt / 1e6, 2)})
                print(json.dumps(res["cpu_checker"][-1]), flush=True)
            for s in (1, 2, 3):
                _, _, band = R.normals(frames[s - 1], R.CM)
                res["band_census"][f"{W}x{H}_seed{s}"] = int(band.sum())
            print(json.dumps(res["band_census"]), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
