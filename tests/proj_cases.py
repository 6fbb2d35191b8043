"""Shared by tests/test_proj_ref.py and tests/test_gpu_proj.py (not a test module): an independent numpy transcription of the
five-argument Projection_GPU::PlaneProjection under P1-P5 ("Plane projection (five-argument)"), vectorised over
the frame, and the inputs of the parity cases."""
import os

import numpy as np

from les_cases import acos_threshold

F = np.float32
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
WINDOW, SPATIAL_SIGMA, DEPTH_SIGMA, MIN_SIZE = 7, F(20.0), F(100.0), 1300
MAX_ANGLE = F(3.141592653) / F(8.0)


def intrinsics(W, H):
    """a Kinect-like camera scaled to the frame, with fractional principal point (P5 truncates it)"""
    return np.array([[525.0 * W / 640.0, 0.0, W / 2.0 - 0.5], [0.0, 525.0 * W / 640.0, H / 2.0 - 0.5], [0.0, 0.0, 1.0]])


def np_rays(W, H, K):
    K = np.asarray(K, np.float64).reshape(3, 3)
    fx, fy, cx, cy = F(K[0, 0]), F(K[1, 1]), int(K[0, 2]), int(K[1, 2])
    x, y = np.meshgrid(np.arange(W, dtype=F), np.arange(H, dtype=F))
    return ((x - F(cx)) / fx).astype(F), ((F(cy) - y) / fy).astype(F)


def np_plane_projection(nd, labels, variance, points, size, K, window_size=WINDOW, spatial_sigma=SPATIAL_SIGMA,
                        depth_sigma=DEPTH_SIGMA, max_angle=MAX_ANGLE, min_size=MIN_SIZE):
    """dict like tools/proj_ref.plane_projection (exp is numpy's float32 exp, not libm's expf: `optimized` agrees with the C
    checker to a few ulp, everything before the filter to the bit)"""
    nd, points = np.asarray(nd, F), np.asarray(points, F)
    variance, size = np.asarray(variance, F), np.asarray(size, np.int32)
    H, W = labels.shape
    nc = len(variance)
    rx, ry = np_rays(W, H, K)
    thr = acos_threshold(max_angle)
    lab = labels.astype(np.int64)
    inr = (lab >= 0) & (lab < nc)                                                   # P1
    ls = np.where(inr, lab, 0)
    with np.errstate(all="ignore"):
        v = variance[ls]
        small = inr & (v <= F(1)) & (v > thr)                                       # P3
        pz = np.abs(nd[..., 3] / ((nd[..., 0] * rx + nd[..., 1] * ry) + nd[..., 2])).astype(F)
        fitted = np.where(small[..., None], np.stack([pz * rx, pz * ry, pz], -1), points).astype(F)
        z = points[..., 2]
        diff = np.abs(z - fitted[..., 2])
        gate = (fitted[..., 2] > F(50)) & (diff < z * F(0.03)) & small & (size[ls] > min_size)
        blend = (fitted[..., 2] * v + z * (F(1) - v)).astype(F)
        z1 = np.where(gate, np.where(diff < z * F(0.01), fitted[..., 2], blend), z).astype(F)
        r = window_size // 2
        pad = np.zeros((H + 2 * r, W + 2 * r), F)                                   # 0 is an absent tap like any z <= 50
        pad[r:r + H, r:r + W] = z1
        num, den, den64 = np.zeros((H, W), F), np.zeros((H, W), F), np.zeros((H, W), np.float64)
        two_s2, two_d2 = F(2) * (F(spatial_sigma) * F(spatial_sigma)), F(2) * (F(depth_sigma) * F(depth_sigma))
        for i in range(window_size):
            for j in range(window_size):
                zt = pad[i:i + H, j:j + W]
                ok = zt > F(50)
                dz = (zt - z1).astype(F)
                arg = (-(dz * dz) / two_d2).astype(F)
                sp = np.exp(-(F((j - r) * (j - r)) + F((i - r) * (i - r))) / two_s2, dtype=F)
                wgt = (np.exp(arg, dtype=F) * sp).astype(F)
                num = np.where(ok, num + zt * wgt, num).astype(F)
                den = np.where(ok, den + wgt, den).astype(F)
                den64 = np.where(ok, den64 + np.exp(arg.astype(np.float64)) * np.float64(sp), den64)
        zo = np.where(den == 0, F(0), num / den).astype(F)
    prefilter = points.copy()
    prefilter[..., 2] = z1
    return {"plane_fitted": fitted, "prefilter": prefilter, "optimized": np.stack([rx * zo, ry * zo, zo], -1).astype(F),
            "den64": den64}


# ---- inputs ------------------------------------------------------------------------------------------------------------
def micro_frame():
    """13 x 1, camera fx = fy = 1, cx = cy = 0: ray (x, 0); planes n = (0, 0, 1), so the projected depth is d itself"""
    #            label  d      z
    px = [(0, 1005.0, 1000.0),     # :204 inside 1 %: replaced by 1005
          (0, 1020.0, 1000.0),     # :206 inside 3 %: blended by 0.95
          (0, 1060.0, 1000.0),     # :203 outside 3 %: kept, plane-fitted 1060
          (1, 1005.0, 1000.0),     # :38 variance 0.5, acos above pi/8: plane-fitted = point
          (-1, 1005.0, 1000.0),    # :38 no label
          (7, 1005.0, 1000.0),     # P1 label >= n_clusters
          (2, 1005.0, 1000.0),     # :203 size 100 <= 1300: projected but kept
          (3, 1000.0, 1000.0),     # plane denominator 0 (n = 0): inf
          (0, 40.0, 40.2),         # :201 plane-fitted z <= 50: kept although inside 1 %
          (0, 1000.0, 0.0),        # a hole: diff < 0 never holds; the filter gives 0 (:239)
          (4, 1020.0, 1000.0),     # variance 1: acos 0 passes, blend by 1 is the plane's depth
          (5, 1005.0, 1000.0),     # variance > 1: acos NaN fails
          (6, 1005.0, 1000.0)]     # variance NaN fails
    W = len(px)
    labels = np.array([[p[0] for p in px]], np.int32)
    nd = np.zeros((1, W, 4), F)
    nd[0, :, 2] = 1
    nd[0, :, 3] = [p[1] for p in px]
    nd[0, 7, :3] = 0
    z = np.array([p[2] for p in px], F)
    points = np.stack([np.arange(W, dtype=F) * z, np.zeros(W, F), z], -1)[None]
    variance = np.array([0.95, 0.5, 0.95, 0.95, 1.0, np.nextafter(F(1), F(2)), np.nan], F)
    size = np.array([2000, 2000, 100, 2000, 2000, 2000, 2000], np.int32)
    return nd, labels, variance, points, size, np.eye(3)


def synthetic_case(seed, W, H, nc, zmax=1200.0, hole_frac=0.08):
    """Blocks of equal labels (with -1, negative and out-of-range labels), one near-frontal plane per label 700-1100 mm
    away, (n, d) painted per pixel as LabelEquivalenceSeg does (0 where the label is no label).  Points lie on their ray at
    the plane's depth times 1, 1.005, 1.02 or 1.06 (inside 1 %, inside 3 %, outside), clipped to [600, zmax]; holes are 0.
    The variance table mixes agreeing regions (above the pi/8 threshold), 1, disagreeing ones, > 1 and NaN; the size table
    straddles `min_size_for(W, H)`.  Returns (nd, labels, variance, points, size, K)."""
    rng = np.random.default_rng(seed)
    K = intrinsics(W, H)
    rx, ry = np_rays(W, H, K)
    bw, bh = max(1, W // 7), max(1, H // 5)
    coarse = rng.integers(0, nc, ((H + bh - 1) // bh, (W + bw - 1) // bw))
    labels = np.kron(coarse, np.ones((bh, bw), np.int64))[:H, :W].astype(np.int32)
    r = rng.random((H, W))
    labels[r < 0.03] = -1
    labels[(r >= 0.03) & (r < 0.05)] = nc + rng.integers(0, 3)
    labels[(r >= 0.05) & (r < 0.06)] = -7
    n = np.array([0.0, 0.0, 1.0]) + 0.15 * rng.normal(size=(nc, 3))
    n = (n / np.linalg.norm(n, axis=1, keepdims=True)).astype(F)
    d = rng.uniform(700, 1100, nc).astype(F)
    variance = rng.uniform(0.93, 0.999, nc).astype(F)
    kind = rng.random(nc)
    variance[kind < 0.15] = rng.uniform(0.2, 0.9, int((kind < 0.15).sum()))
    variance[(kind >= 0.15) & (kind < 0.22)] = 1.0
    variance[(kind >= 0.22) & (kind < 0.27)] = 1.0 + 2.0 ** -20
    variance[(kind >= 0.27) & (kind < 0.32)] = np.nan
    size = np.where(rng.random(nc) < 0.6, min_size_for(W, H) + 1 + rng.integers(0, 50, nc), rng.integers(0, min_size_for(W, H) + 1, nc)).astype(np.int32)
    if nc == 1:
        variance[0], size[0] = F(0.97), min_size_for(W, H) + 1
    inr = (labels >= 0) & (labels < nc)
    ls = np.where(inr, labels, 0)
    nd = np.where(inr[..., None], np.concatenate([n, d[:, None]], 1)[ls], F(0)).astype(F)
    with np.errstate(all="ignore"):
        zp = np.abs(nd[..., 3] / ((nd[..., 0] * rx + nd[..., 1] * ry) + nd[..., 2]))
    zp = np.where(inr & np.isfinite(zp), zp, 900.0)
    factor = rng.choice(np.array([1.0, 1.005, 0.995, 1.02, 0.98, 1.06]), size=(H, W))
    z = np.clip(zp * factor, 600.0, zmax).astype(F)
    z[rng.random((H, W)) < hole_frac] = 0
    points = np.stack([rx * z, ry * z, z], -1).astype(F)
    return nd, labels, variance, points, size, K


def min_size_for(W, H):
    """the lowered `size` gate of the small frames: a fiftieth of the frame"""
    return max(1, W * H // 50)


def deep_case(seed, W, H, nc):
    """as synthetic_case with 4 % holes and a third of the frame, in blocks of 10 x 10, 3.3 times as far (up to 3960 mm): a
    hole whose window holds only surfaces beyond about 1290 mm sums weights below 2^-120 (BAND)"""
    nd, labels, variance, points, size, K = synthetic_case(seed, W, H, nc, zmax=1200.0, hole_frac=0.04)
    rng = np.random.default_rng(seed + 1000)
    far = np.kron(rng.random(((H + 9) // 10, (W + 9) // 10)) < 0.35, np.ones((10, 10), bool))[:H, :W]
    scale = np.where(far, F(3.3), F(1)).astype(F)
    points = (points * scale[..., None]).astype(F)
    nd = nd.copy()
    nd[..., 3] = nd[..., 3] * scale
    return nd, labels, variance, points, size, K


DENORMAL_TAP = F(2155.418)


def denormal_weight_case():
    """Found by the seeded sweep (plane_sweep `proj`, seed 3, index 0, pixel (126, 47)), here at its smallest: 3 x 1, no labels,
    a hole on either side of one surface pixel of 2155.418 mm, window 3, depth_sigma 150.  The holes' only tap has the weight
    exp(-2155.418^2 / 45000) * exp(-1 / 800) = 1.04 units of 2^-149: z * w rounds to 2155 units and the quotient is 2155, below
    the only valid z of the window.  Returns (nd, labels, variance, points, size, K) and the parameters."""
    z = np.array([0, DENORMAL_TAP, 0], F)
    points = np.stack([np.zeros(3, F), np.zeros(3, F), z], -1)[None]
    case = (np.zeros((1, 3, 4), F), np.full((1, 3), -1, np.int32), np.zeros(1, F), points, np.zeros(1, np.int32), np.eye(3))
    return case, dict(window_size=3, depth_sigma=150.0)


def golden_inputs(generate=False):
    """LabelEquivalenceSeg's four outputs from tests/golden/les_it1.npz (320 x 240, 100 superpixels), rows 60-179 and
    columns 80-239, plus the synthetic points stored in tests/golden/proj_it1.npz: on each region's plane times 1 / 1.005 /
    1.02 / 1.06 by 8 x 8 blocks, 4 % holes (generate=True draws them anew: tests/golden/make_golden_proj.py)"""
    g = np.load(os.path.join(GOLDEN, "les_it1.npz"))
    sl = (slice(60, 180), slice(80, 240))
    labels = g["merged_label"].astype(np.int32)[sl]
    nd = np.ascontiguousarray(g["merged_nd"].view(F)[sl])
    variance, size = g["variance"].view(F), g["size"].astype(np.int32)
    H, W = labels.shape
    K = intrinsics(W, H)
    if not generate:
        return nd, labels, variance, np.load(os.path.join(GOLDEN, "proj_it1.npz"))["points"].view(F), size, K
    rx, ry = np_rays(W, H, K)
    rng = np.random.default_rng(77)
    with np.errstate(all="ignore"):
        zp = np.abs(nd[..., 3] / ((nd[..., 0] * rx + nd[..., 1] * ry) + nd[..., 2]))
    zp = np.where((labels > -1) & np.isfinite(zp), zp, 900.0)
    factor = np.kron(rng.choice(np.array([1.0, 1.005, 1.02, 1.06]), size=(H // 8, W // 8)), np.ones((8, 8)))
    z = np.clip(zp * factor, 600.0, 1200.0).astype(F)
    z[rng.random((H, W)) < 0.04] = 0
    return nd, labels, variance, np.stack([rx * z, ry * z, z], -1).astype(F), size, K


def branch_counts(exp, points, labels, variance, size, min_size, max_angle=MAX_ANGLE):
    """how many pixels took each branch of .cu:38 and :201-208, from the checker's outputs"""
    nc = len(variance)
    thr = acos_threshold(max_angle)
    inr = (labels >= 0) & (labels < nc)
    with np.errstate(all="ignore"):
        v = np.asarray(variance, F)[np.where(inr, labels, 0)]
        small = inr & (v <= 1) & (v > thr)
    z0, z1, pz = points[..., 2], exp["prefilter"][..., 2], exp["plane_fitted"][..., 2]
    changed = z0.view(np.uint32) != z1.view(np.uint32)
    return {"projected": int(small.sum()), "kept": int((~small).sum()), "replaced": int((changed & (z1 == pz)).sum()),
            "blended": int((changed & (z1 != pz)).sum()),
            "small_region": int((small & (np.asarray(size)[np.where(inr, labels, 0)] <= min_size)).sum())}
