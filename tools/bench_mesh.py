"""Throughput of OrganizedMesh (mesh_kernels.hip over cloud_kernels.hip) on the MI355X.

    python tools/bench_mesh.py [--steps K] [--out profiles/mesh_bench.json] [--quick]
    python tools/bench_mesh.py --trace-one vga|fhd             # three calls of one case and nothing else, for a kernel trace
    python tools/bench_mesh.py --merge-stats STATS.csv --out profiles/mesh_bench.json      # no GPU: fold the trace's stats in

Cases: 64 x 640x480 and 8 x 1920x1080 on the generator's frames (synth.make_batch: walls, rectangles, sensor noise, holes), a
colour image per frame.  Reports per case the valid fraction and the triangles per pixel, and per source format (float3 cloud,
float depth map, uint16 depth map) the median of K timed calls after a wake-up load and warm-up (HIP events on the current
stream), next to
  (a) the float4 streaming copy of tools/hooks/libkde_hooks.so over as many bytes as the call MUST move: the source once, the
      colour image once, 16 B per vertex and 12 B per triangle written: its fraction of that copy ceiling.  The call reads the
      source three times (count, scatter, classify) and part of it a fourth time (the row below); only the first reading is
      in the ceiling;
  (b) kde_cloud_build_batch alone on the same frames: the multiple of the cloud call, and the call's time beyond the cloud
      call next to the copy of its own extra bytes (12 B per triangle);
  (c) the host road, once per case: the organised grid (depth and colour) copied out and the vectorised numpy statement of
      the rule (tests/mesh_cases.py) applied per frame.
--trace-one runs the wake-up load and three calls of one case with the float3 source, for
`rocprofv3 --kernel-trace --stats -- python tools/bench_mesh.py --trace-one fhd`; --merge-stats reads that run's
kernel_stats.csv and records the average time per launch of M1 (mesh_classify_kernel), M2 (cloud_scan_kernel: the same kernel
scans the vertex and the triangle table, two launches per call), M3 (mesh_emit_kernel) and the vertex part (cloud_count_kernel,
cloud_write_kernel).  The tool checks that the three source formats give the same bytes.  --quick runs one timed call per
measurement and skips (c).
"""
from __future__ import annotations

import argparse
import csv
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CASES = {"vga": (64, 640, 480), "fhd": (8, 1920, 1080)}
SOURCE_BYTES = {"points": 12, "depth_f32": 4, "depth_u16": 2}
KERNELS = {"M1_classify": "mesh_classify_kernel", "M2_scan": "cloud_scan_kernel", "M3_emit": "mesh_emit_kernel",
           "vertices_count": "cloud_count_kernel", "vertices_write": "cloud_write_kernel"}


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


def frames_of(torch, synth, filters, n, W, H):
    """the generator's frames on the device: (depth float32 whole millimetres, bgr, float3 cloud, K)"""
    bgr, depth = synth.make_batch(1000 + W, n, W, H)
    depth = np.rint(depth)                                           # whole millimetres: the uint16 map holds the same z
    K = synth.intrinsics(W, H)
    d, c = torch.from_numpy(depth).cuda(), torch.from_numpy(bgr).cuda()
    conv = filters.DimensionConvertor()
    conv.setCameraParameters(K, W, H)
    cloud = conv.projectiveToReal(d, torch.empty((n, H, W, 3), dtype=torch.float32, device="cuda"))
    conv.close()
    return d, c, cloud, K


def host_road(depth, bgr):
    """the organised grid copied out and the numpy statement applied per frame: seconds for the copies, seconds for numpy"""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import mesh_cases as MC
    t0 = time.perf_counter()
    z, c = depth.cpu().numpy(), bgr.cpu().numpy()
    t1 = time.perf_counter()
    tris = [MC.records(MC.triangles(z[f])) for f in range(z.shape[0])]
    t2 = time.perf_counter()
    return t1 - t0, t2 - t1, tris, c


def merge_stats(path, out):
    rows = list(csv.DictReader(open(path)))
    got = {}
    for key, needle in KERNELS.items():
        hit = [r for r in rows if needle in r["Name"]]
        got[key] = {"launches": sum(int(r["Calls"]) for r in hit),
                    "average_us": round(sum(float(r["TotalDurationNs"]) for r in hit) / max(1, sum(int(r["Calls"]) for r in hit)) / 1e3, 2),
                    "total_us": round(sum(float(r["TotalDurationNs"]) for r in hit) / 1e3, 1)}
    total = sum(v["total_us"] for v in got.values())
    for v in got.values():
        v["share_of_the_call"] = round(v["total_us"] / total, 4) if total else None
    res = json.load(open(out)) if os.path.exists(out) else {}
    res["kernels_of_trace_one"] = {"source": "rocprofv3 --kernel-trace --stats -- python tools/bench_mesh.py --trace-one (float3 source, "
                                             "three calls; cloud_scan_kernel runs twice per call)", "stats_file": os.path.basename(path), **got}
    with open(out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res["kernels_of_trace_one"]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--quick", action="store_true")
    ap.add_argument("--trace-one", choices=sorted(CASES), default=None)
    ap.add_argument("--merge-stats", default=None)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.merge_stats:
        if not a.out:
            ap.error("--merge-stats needs --out")
        merge_stats(a.merge_stats, a.out)
        return
    if a.quick:
        a.steps, a.warmup = 1, 1
    import torch
    from kinectdepthmapenhancement_amd import filters, synth
    from tools.hooks import hooks
    from tools.wake import wake
    torch.cuda.set_device(0)
    stream = lambda: torch.cuda.current_stream().cuda_stream
    if a.trace_one:
        n, W, H = CASES[a.trace_one]
        depth, bgr, cloud, K = frames_of(torch, synth, filters, n, W, H)
        M = filters.OrganizedMesh(W, H, max_batch=n)
        wake(torch)
        for _ in range(3):
            M.build(cloud, bgr)
        torch.cuda.synchronize()
        print(json.dumps({"case": a.trace_one, "vertices": int(M.counts().sum()), "triangles": int(M.tri_counts().sum())}))
        M.close()
        return
    res = {"device": torch.cuda.get_device_name(0), "steps": a.steps, "cases": []}
    for tag, (n, W, H) in CASES.items():
        px = n * W * H
        depth, bgr, cloud, K = frames_of(torch, synth, filters, n, W, H)
        sources = {"points": cloud, "depth_f32": depth, "depth_u16": depth.to(torch.int32).to(torch.int16)}   # < 32768: int16 bits = uint16 bits
        assert float(depth.max()) < 32768.0
        vout = torch.empty((n, H * W, 16), dtype=torch.uint8, device="cuda")
        tout = torch.empty((n, 2 * (W - 1) * (H - 1), 12), dtype=torch.uint8, device="cuda")

        def copy_ms(nbytes):
            src = torch.empty(nbytes // 32 * 16, dtype=torch.uint8, device="cuda")        # read + write = nbytes, whole float4
            dst = torch.empty_like(src)
            ms, _ = timed(torch, lambda: hooks.hbm_copy(src, dst, stream()), a.steps, a.warmup)
            return ms

        wake(torch)
        M = filters.OrganizedMesh(W, H, max_batch=n)
        M.set_camera(K)
        C = filters.PointCloudXYZRGB(W, H, max_batch=n)
        C.set_camera(K)
        case = {"case": tag, "frames": n, "width": W, "height": H}
        want = None
        for name, src in sources.items():
            ms, ms_min = timed(torch, lambda: M.build(src, bgr, vout, tout), a.steps, a.warmup)
            vertices, triangles = int(M.counts().sum()), int(M.tri_counts().sum())
            got = ([r.tobytes() for r in M.vertices_host()], [r.tobytes() for r in M.triangles_host()])
            if want is None:
                want = got
                case["valid_fraction"] = round(vertices / px, 4)
                case["triangles_per_pixel"] = round(triangles / px, 4)
            cloud_ms, _ = timed(torch, lambda: C.build(src, bgr, vout), a.steps, a.warmup)
            assert int(C.counts().sum()) == vertices
            must = px * (SOURCE_BYTES[name] + 3) + 16 * vertices + 12 * triangles
            cms, extra_ms = copy_ms(must), copy_ms(12 * triangles)
            case[name] = {"bytes_must_move": must, "ms_per_call": round(ms, 4), "ms_min": round(ms_min, 4),
                          "ms_per_frame": round(ms / n, 5), "gpixel_per_s": round(px / (ms * 1e-3) / 1e9, 3),
                          "gbyte_per_s": round(must / (ms * 1e-3) / 1e9, 1), "copy_same_bytes_ms": round(cms, 4),
                          "copy_gbyte_per_s": round(must / (cms * 1e-3) / 1e9, 1), "fraction_of_copy_ceiling": round(cms / ms, 4),
                          "cloud_call_ms": round(cloud_ms, 4), "multiple_of_cloud_call": round(ms / cloud_ms, 3),
                          "beyond_cloud_call_ms": round(ms - cloud_ms, 4), "copy_of_triangle_bytes_ms": round(extra_ms, 4),
                          "equals_points": got == want}
        if not a.quick:
            torch.cuda.synchronize()
            copy_s, numpy_s, tris, _ = host_road(depth, bgr)
            M.build(depth, bgr, vout, tout)
            same = [r.tobytes() for r in M.triangles_host()] == [r.tobytes() for r in tris]
            t0 = time.perf_counter()
            M.build(depth, bgr, vout, tout)
            M.vertices_host()
            M.triangles_host()
            t1 = time.perf_counter()
            case["host_road"] = {"d2h_bytes": px * 7, "copy_s": round(copy_s, 3), "numpy_triangles_s": round(numpy_s, 3),
                                 "device_call_and_d2h_of_the_records_s": round(t1 - t0, 3), "same_triangles": same,
                                 "total_over_device_call": round((copy_s + numpy_s) * 1e3 / case["depth_f32"]["ms_per_call"], 1),
                                 "total_over_device_call_and_d2h": round((copy_s + numpy_s) / (t1 - t0), 1)}
        M.close()
        C.close()
        res["cases"].append(case)
        print(json.dumps(case), flush=True)
        del cloud, depth, bgr, vout, tout, sources
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
