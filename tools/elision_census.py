#!/usr/bin/env python3
"""Census of K1's rule elision (csrc/jbf_fast.hip, jbf_pk_kernel) on the CPU, numpy only.

The tuned K1 kernels pick, per wavefront, a body without the colour and / or the depth Q1 rule when the value ranges of the
wavefront's REGION -- its footprint of pixels plus the window radius on every side -- prove that the rule cannot trip.  This
tool evaluates the kernel's own predicates for every region of a given footprint on synthetic frames (synth.make_frame) and
prints
  * the fraction of regions that need each rule, for a list of footprints (the smaller the fraction, the fewer rule
    instructions the kernel issues), and
  * the per-wavefront body mix to expect from a footprint (body = colour rule + 2 * depth rule; windows >= 15 only know the
    bodies 0 and 3), for comparison with the counters of the stage build (tools/hooks/stage.py, jbf_stage_run).

    python tools/elision_census.py                        # the table of EXPERIMENTS.md Part I item 13
    python tools/elision_census.py --footprint 32x8 --window 11 --mix

`region_needs_rules` is the predicate on one region; tests/test_k1_wave_elision.py holds it against a brute-force search
over every (centre, tap) pair of the region.
"""
from __future__ import annotations

import argparse
import json
import math
import os
import sys

import numpy as np
from numpy.lib.stride_tricks import sliding_window_view

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

F32 = np.float32
LOG2E = 1.4426950408889634
MIN_VALID_MM = 50.0              # a depth is valid when it is > 50 mm; the kernel stages every other one as 0


def exp_zero_threshold() -> np.float32:
    """smallest float32 x with exp(-x) rounding to 0 in binary32 (csrc/kde_host_math.h)"""
    t = 150.0 * 0.693147180559945309417232121458
    f = F32(t)
    while float(f) <= t:
        f = np.nextafter(f, F32(np.inf))
    while float(np.nextafter(f, F32(0))) > t:
        f = np.nextafter(f, F32(0))
    return f


def thresholds(sigma_c: float, sigma_d: float) -> dict:
    """the launch constants of K1's rules, as kde_api.cpp / launch_jbf_fast form them: cd_skip (int), d2_skip, sd and t_skip (float32)"""
    xz = exp_zero_threshold()
    cden = F32(2) * (F32(sigma_c) * F32(sigma_c))
    dden = F32(2) * (F32(sigma_d) * F32(sigma_d))
    lo, hi = 0, 195076
    while lo < hi:                                   # smallest integer cd with (float)cd / den >= xz
        mid = (lo + hi) // 2
        if F32(mid) / cden >= xz:
            hi = mid
        else:
            lo = mid + 1
    cd_skip = lo
    lo, hi = 0, 0x7f800000                           # smallest float q with q / den >= xz
    val = lambda b: np.array([b], np.uint32).view(F32)[0]
    while lo < hi:
        mid = lo + (hi - lo) // 2
        if val(mid) / dden >= xz:
            hi = mid
        else:
            lo = mid + 1
    d2_skip = val(lo)
    sd = F32(math.sqrt(LOG2E / float(dden)))
    t_skip = F32(math.sqrt(float(d2_skip)) * math.sqrt(LOG2E / float(dden)))
    return {"cd_skip": cd_skip, "d2_skip": d2_skip, "sd": sd, "t_skip": t_skip}


def colour_needed(cmin, cmax, cd_skip):
    """kernel predicate: sum over channels of (max - min)^2 >= cd_skip.  cmin / cmax: [..., 3] integers; a region without any
    in-image pixel (max < min) keeps the rule"""
    r = cmax.astype(np.int64) - cmin.astype(np.int64)
    return (cmax[..., 0] < cmin[..., 0]) | ((r * r).sum(axis=-1) >= cd_skip)


def depth_needed(dmin, dmax, window, sd, t_skip):
    """kernel predicate in float32: no valid depth (dmax == 0) -> no rule; else not ((range * 1.0001 + slack) * sd < t_skip) with
    slack = dmax * (window^2 + 8) * 2^-24"""
    dmin, dmax = np.asarray(dmin, F32), np.asarray(dmax, F32)
    with np.errstate(invalid="ignore", over="ignore"):
        rng = dmax - dmin
        slack = dmax * F32(window * window + 8) * F32(2.0 ** -24)
        calm = (rng * F32(1.0001) + slack) * F32(sd) < F32(t_skip)
    return np.where(dmax == 0, False, ~calm)


def region_needs_rules(bgr, depth, x0, y0, fw, fh, window, thr):
    """(colour rule needed, depth rule needed) for the wavefront whose pixels are columns x0 .. x0+fw-1, rows y0 .. y0+fh-1:
    the statistics run over the in-image pixels of the footprint grown by the window radius"""
    h, w = depth.shape
    r = window // 2
    ya, yb, xa, xb = max(y0 - r, 0), min(y0 + fh + r, h), max(x0 - r, 0), min(x0 + fw + r, w)
    c = bgr[ya:yb, xa:xb].reshape(-1, 3).astype(np.int64)
    d = depth[ya:yb, xa:xb].astype(F32).ravel()
    d = d[d > MIN_VALID_MM]
    if c.shape[0] == 0:
        need_c = True
    else:
        need_c = bool(colour_needed(c.min(axis=0), c.max(axis=0), thr["cd_skip"]))
    if d.size == 0:
        need_d = False
    else:
        need_d = bool(depth_needed(d.min(), d.max(), window, thr["sd"], thr["t_skip"]))
    return need_c, need_d


def census(bgr, depth, fw, fh, window, thr):
    """region_needs_rules for every footprint of the grid that starts at (0, 0): two bool arrays [ceil(H / fh), ceil(W / fw)]"""
    h, w = depth.shape
    r = window // 2
    ny, nx = -(-h // fh), -(-w // fw)
    ph, pw = ny * fh + 2 * r, nx * fw + 2 * r            # padded so that every region is a full (fh + 2r) x (fw + 2r) window

    def windows(a, fill):
        p = np.full((ph, pw), fill, a.dtype)
        p[r:r + h, r:r + w] = a
        return sliding_window_view(p, (fh + 2 * r, fw + 2 * r))[::fh, ::fw]

    d = depth.astype(F32)
    valid = d > MIN_VALID_MM
    dmin = windows(np.where(valid, d, F32(np.inf)), F32(np.inf)).min(axis=(2, 3))
    dmax = windows(np.where(valid, d, F32(0)), F32(0)).max(axis=(2, 3))
    dmin = np.where(dmax == 0, F32(0), dmin)
    cmin = np.stack([windows(bgr[..., c].astype(np.int16), np.int16(256)).min(axis=(2, 3)) for c in range(3)], -1)
    cmax = np.stack([windows(bgr[..., c].astype(np.int16), np.int16(-1)).max(axis=(2, 3)) for c in range(3)], -1)
    return colour_needed(cmin, cmax, thr["cd_skip"]), depth_needed(dmin, dmax, window, thr["sd"], thr["t_skip"])


def body_mix(need_c, need_d, window):
    """counts of the bodies 0..3 the wavefronts run (windows >= 15: both rules or none)"""
    if window >= 15:
        both = need_c | need_d
        return [int((~both).sum()), 0, 0, int(both.sum())]
    body = need_c.astype(int) + 2 * need_d.astype(int)
    return [int((body == b).sum()) for b in range(4)]


def parse_footprint(s):
    a, b = s.lower().split("x")
    return int(a), int(b)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--width", type=int, default=640)
    ap.add_argument("--height", type=int, default=480)
    ap.add_argument("--seeds", type=int, nargs="+", default=[0, 1, 2])
    ap.add_argument("--window", type=int, default=11)
    ap.add_argument("--color-sigma", type=float, default=7.65)
    ap.add_argument("--depth-sigma", type=float, default=20.0)
    ap.add_argument("--footprint", type=parse_footprint, nargs="+",
                    default=[(64, 16), (64, 4), (32, 8), (16, 16), (4, 1)], metavar="WxH", help="pixels of one region, without the halo")
    ap.add_argument("--mix", action="store_true", help="also print the body mix of every footprint")
    a = ap.parse_args()
    from kinectdepthmapenhancement_amd import synth
    thr = thresholds(a.color_sigma, a.depth_sigma)
    frames = [synth.make_frame(s, a.width, a.height) for s in a.seeds]
    print(f"# {len(frames)} frames {a.width}x{a.height} (seeds {a.seeds}), window {a.window}: cd_skip {thr['cd_skip']}, "
          f"depth range limit {float(thr['t_skip']) / float(thr['sd']):.1f} mm")
    print("| region (pixels + halo %d) | colour | depth |" % (a.window // 2))
    print("|---|---|---|")
    for fw, fh in a.footprint:
        nc = nd = n = 0
        mix = np.zeros(4, np.int64)
        for bgr, depth in frames:
            c, d = census(bgr, depth, fw, fh, a.window, thr)
            nc, nd, n = nc + int(c.sum()), nd + int(d.sum()), n + c.size
            mix += body_mix(c, d, a.window)
        print(f"| {fw}x{fh} | {nc / n:.2f} | {nd / n:.2f} |")
        if a.mix:
            print(json.dumps({"footprint": f"{fw}x{fh}", "regions": n, "body_counts": mix.tolist(),
                              "body_fractions": [round(float(v) / n, 4) for v in mix]}))


if __name__ == "__main__":
    main()
