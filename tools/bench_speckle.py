"""Throughput and quality of DepthSpeckleFilter (speckle_kernels.hip) on the MI355X.

    python tools/bench_speckle.py [--steps K] [--out profiles/speckle_bench.json] [--quick] [--only vga|1080p]

Throughput.  The call at 64 x VGA and 8 x 1080p, float and uint16, connectivity 4 and 8, with and without labels, on
  generator   the synthetic RGB-D generator's frames (a few, repeated)
  injected    those frames with half of the pixels beside a depth edge set between the two surfaces and 5 % of the hole pixels
              given a random depth (tests/speckle_cases.injected_frame)
  checker     alternating 1000 / 2000 mm: no link at all with 4, two components held by diagonals only with 8
  noise       white noise: nearly every pixel its own component
  snake       a one-pixel-wide serpentine over the whole frame: one component, the longest chains across tiles
since labelling time depends on content.  Reports per setting the median of K timed calls after a wake-up load and warm-up (HIP
events on the current stream), next to
  (a) the float4 streaming copy of tools/hooks/libkde_hooks.so over the bytes that MUST move -- depth in, depth out, labels when
      asked; the union-find scratch is not in it: the call's fraction of that copy ceiling;
  (b) DepthHoleFilling on hole-free frames, which moves the same depth bytes (profiles/holefill_bench.json has 0.201 / 0.172 ms
      per frame); measured again here on the generator's frames with every hole set to 3000 mm;
  (c) the numpy statement of the rule (tests/speckle_cases.py) on the host, on the first frame.
The tool checks the device's bytes, labels and counts against the statement on the first frame of every content, and that
capped is 0 everywhere.

Quality, at VGA and 1080p, seeds 0 .. 2: the fraction of a clean frame's valid pixels the defaults remove, the fraction of the
injected outliers they remove (4 and 8), and MeanError3D against the generator's noise-free depth of the injected frames through
DepthHoleFilling alone and through DepthSpeckleFilter then DepthHoleFilling.  --quick runs one timed call per measurement and
skips (c) and the quality part."""
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
DISTINCT = 2
CONTENTS = ("generator", "injected", "checker", "noise", "snake")


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


def content(SC, synth, name, k, w, h):
    """frame k of a content, whole millimetres (the same scene in both formats)"""
    y, x = np.mgrid[0:h, 0:w]
    if name == "generator":
        z = synth.make_frame(31 + k, w, h)[1]
    elif name == "injected":
        z = SC.injected_frame(31 + k, w, h, salt=False)[0]
    elif name == "checker":
        z = np.where((x + y + k) % 2 == 1, 2000.0, 1000.0)
    elif name == "noise":
        z = np.random.default_rng(k).uniform(500.0, 5000.0, (h, w))
    else:
        z = np.where(SC._serpentine(w, h, offset=k % 2), 1500.0, 0.0)
    return np.rint(z).astype(np.float32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--quick", action="store_true")
    ap.add_argument("--only", default=None)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.quick:
        a.steps, a.warmup = 1, 1
    import torch
    import speckle_cases as SC
    from kinectdepthmapenhancement_amd import _native, filters, synth
    from tools.hooks import hooks
    from tools.wake import wake
    torch.cuda.set_device(0)
    stream = lambda: torch.cuda.current_stream().cuda_stream
    d = filters.DepthSpeckleFilter.default_params()

    def params(conn, min_size=None):
        return _native.SpeckleParams(d.min_size if min_size is None else min_size, d.max_diff, d.rel_diff, conn, d.z_min, d.z_max)

    res = {"device": torch.cuda.get_device_name(0), "steps": a.steps, "min_size": d.min_size, "max_diff": d.max_diff, "rel_diff": d.rel_diff,
           "tile": [32, 16], "cases": [], "quality": []}
    esz = {"f32": 4, "u16": 2}
    for name, n, size in CASES:
        if a.only and a.only != name:
            continue
        w, h = size
        px = n * w * h
        outs = {"f32": torch.empty((n, h, w), dtype=torch.float32, device="cuda"), "u16": torch.empty((n, h, w), dtype=torch.int16, device="cuda")}
        labels = torch.empty((n, h, w), dtype=torch.int32, device="cuda")

        def copy_ms(nbytes):
            s = torch.empty(nbytes // 2, dtype=torch.uint8, device="cuda")
            t = torch.empty_like(s)
            return timed(torch, lambda: hooks.hbm_copy(s, t, stream()), a.steps, a.warmup)[0]

        copies = {(fmt, lab): copy_ms(px * (2 * esz[fmt] + (4 if lab else 0))) for fmt in esz for lab in (False, True)}
        wake(torch)
        case = {"case": name, "frames": n, "size": [w, h], "copy_ms": {f"{f}{'_labels' if l else ''}": round(v, 4) for (f, l), v in copies.items()}}
        for what in CONTENTS:
            head = np.stack([content(SC, synth, what, k, w, h) for k in range(DISTINCT)])
            depth = torch.from_numpy(np.concatenate([head] * (n // DISTINCT))).cuda()
            sources = {"f32": depth, "u16": depth.to(torch.int32).to(torch.int16)}
            for conn in (4, 8):
                for fmt in ("f32", "u16"):
                    for lab in (False, True):
                        if what != "generator" and (fmt == "u16" or not lab) and not (what == "injected" and fmt == "f32"):
                            continue                                    # the adversarial contents: float with labels only
                        S = filters.DepthSpeckleFilter(size, n, params(conn))
                        s, o, l = sources[fmt], outs[fmt], (labels if lab else None)
                        ms, ms_min = timed(torch, lambda: S.filter(s, o, labels=l), a.steps, a.warmup)
                        must = px * (2 * esz[fmt] + (4 if lab else 0))
                        r = {"bytes_must_move": must, "ms_per_call": round(ms, 4), "ms_min": round(ms_min, 4), "ms_per_frame": round(ms / n, 5),
                             "gpixel_per_s": round(px / (ms * 1e-3) / 1e9, 3), "copy_same_bytes_ms": round(copies[(fmt, lab)], 4),
                             "fraction_of_copy_ceiling": round(copies[(fmt, lab)] / ms, 4), "removed": int(S.removed().sum()),
                             "components": int(S.components().sum()), "capped": int(S.capped().sum())}
                        assert r["capped"] == 0, r
                        if lab and fmt == "f32":
                            t0 = time.perf_counter()
                            want, wl, wr, wc = SC.filter(head[0], np.float32, min_size=d.min_size, max_diff=d.max_diff, rel_diff=d.rel_diff,
                                                         connectivity=conn)
                            r["numpy_statement_s_per_frame"] = round(time.perf_counter() - t0, 4)
                            r["equals_statement"] = bool(o[0].cpu().numpy().tobytes() == want.tobytes() and l[0].cpu().numpy().tobytes() == wl.tobytes() and
                                                         int(S.removed()[0]) == wr and int(S.components()[0]) == wc)
                            assert r["equals_statement"], (name, what, conn)
                        S.close()
                        case[f"{what}_c{conn}_{fmt}{'_labels' if lab else ''}"] = r
            if what == "generator":                                      # (b) the hole filler on the same frames without a hole
                bgr = torch.from_numpy(np.concatenate([np.stack([synth.make_frame(31 + k, w, h)[0] for k in range(DISTINCT)])] * (n // DISTINCT))).cuda()
                full = torch.where(depth > 0, depth, torch.full_like(depth, 3000.0))
                H = filters.DepthHoleFilling(size, n)
                ms, ms_min = timed(torch, lambda: H.fill(full, bgr, outs["f32"]), a.steps, a.warmup)
                H.close()
                case["holefill_hole_free_f32"] = {"ms_per_call": round(ms, 4), "ms_min": round(ms_min, 4), "ms_per_frame": round(ms / n, 5)}
                del bgr, full
            del depth, sources
        res["cases"].append(case)
        print(json.dumps(case), flush=True)
        del outs, labels

    if not a.quick:
        for w, h in ((640, 480), (1920, 1080)):
            if a.only and a.only != {640: "vga", 1920: "1080p"}[w]:
                continue
            seeds = (0, 1, 2)
            made = [synth.make_frame(s, w, h, clean=True) for s in seeds]
            bgr_np, noisy, truth = (np.stack([m[i] for m in made]) for i in range(3))
            inj = [SC.injected_frame(s, w, h, salt=False) for s in seeds]
            given, mask = np.stack([i[0] for i in inj]), np.stack([i[2] for i in inj])
            bgr, dg, dn = torch.from_numpy(bgr_np).cuda(), torch.from_numpy(given).cuda(), torch.from_numpy(noisy).cuda()
            q = {"size": [w, h], "frames": len(seeds), "injected_outliers": int(mask.sum())}
            results = {}
            H = filters.DepthHoleFilling((w, h), len(seeds))
            results["holefill_alone"] = H.fill(dg, bgr, torch.empty_like(dg))
            for conn in (4, 8):
                S = filters.DepthSpeckleFilter((w, h), len(seeds), params(conn))
                clean = S.filter(dn, torch.empty_like(dn))
                q[f"clean_removed_fraction_c{conn}"] = [round(float(r) / int((f > 0).sum()), 7) for r, f in zip(S.removed(), noisy)]
                out = S.filter(dg, torch.empty_like(dg)).cpu().numpy()
                q[f"injected_removed_fraction_c{conn}"] = [round(float(((o == 0) & m).sum()) / int(m.sum()), 4) for o, m in zip(out, mask)]
                assert int(S.capped().sum()) == 0
                results[f"speckle_c{conn}_then_holefill"] = H.fill(torch.from_numpy(out).cuda(), bgr, torch.empty_like(dg))
                S.close()
                del clean
            H.close()
            results["input"] = dg
            E = filters.MeanError3D(w, h, len(seeds), len(results))
            E.set_camera(synth.intrinsics(w, h))
            E.compare(list(results.values()), torch.from_numpy(truth).cuda())
            table = E.results_host()
            q["mean_error_3d_mm"] = {label: round(float(np.sum(table["sum"][:, c]) / max(1, int(table["count"][:, c].sum()))), 4)
                                     for c, label in enumerate(results)}
            E.close()
            res["quality"].append(q)
            print(json.dumps(q), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
