"""The rule of MeanError3D (main.cpp:220-308) stated in numpy, and the inputs its tests share.

For a candidate point p and the truth point t of the same pixel:
    valid  iff p.z > z_min and p.z < z_max and t.z > z_min and t.z < z_max    (defaults 50 and 15000; NaN, +-inf invalid)
    term   dz = p.z - t.z; dy = p.y - t.y; dx = p.x - t.x; e = sqrt((dz*dz + dy*dy) + dx*dx)   in float32, no fused multiply-add
    count  the number of valid pixels; sum = the EXACT sum of the terms (math.fsum); mean = float32(sum / count), NaN at 0
Every operation below is a float32 elementwise numpy operation in that association; np.sqrt on float32 is correctly rounded.
"""
import math

import numpy as np

F32 = np.float32
Z_MIN, Z_MAX = F32(50.0), F32(15000.0)
RESULT = np.dtype([("sum", "<f8"), ("count", "<u4"), ("mean", "<f4")])


def valid_mask(points, truth, z_min=Z_MIN, z_max=Z_MAX):
    pz, tz = np.asarray(points, F32)[..., 2], np.asarray(truth, F32)[..., 2]
    with np.errstate(invalid="ignore"):
        return (pz > F32(z_min)) & (pz < F32(z_max)) & (tz > F32(z_min)) & (tz < F32(z_max))


def terms_of(p, t):
    """float32 terms of points p, t [..., 3] (every pixel, valid or not)"""
    p, t = np.asarray(p, F32), np.asarray(t, F32)
    with np.errstate(invalid="ignore", over="ignore"):
        dz, dy, dx = p[..., 2] - t[..., 2], p[..., 1] - t[..., 1], p[..., 0] - t[..., 0]
        e = np.sqrt((dz * dz + dy * dy) + dx * dx)
    assert e.dtype == F32
    return e


def terms_contracted(p, t):
    """the same expression as a compiler contracts it, fma(dx, dx, fma(dz, dz, dy*dy)): the products of float32 are exact in
    binary64, so each fma is one binary64 addition rounded to float32 (the double rounding is far rarer than the effect)"""
    p, t = np.asarray(p, F32), np.asarray(t, F32)
    dz, dy, dx = p[..., 2] - t[..., 2], p[..., 1] - t[..., 1], p[..., 0] - t[..., 0]
    inner = (dz.astype(np.float64) * dz.astype(np.float64) + (dy * dy).astype(np.float64)).astype(F32)
    return np.sqrt((dx.astype(np.float64) * dx.astype(np.float64) + inner.astype(np.float64)).astype(F32))


def statement(points, truth, z_min=Z_MIN, z_max=Z_MAX):
    """one frame, points and truth [H, W, 3] (or [k, 3]): dict(count, terms, sum, mean) with the exact sum of the float32 terms"""
    p, t = np.asarray(points, F32).reshape(-1, 3), np.asarray(truth, F32).reshape(-1, 3)
    v = valid_mask(p, t, z_min, z_max)
    e = terms_of(p[v], t[v])
    count = int(v.sum())
    if np.all(np.isfinite(e)):
        total = math.fsum(float(x) for x in e)
    else:
        total = float(np.sum(e.astype(np.float64)))      # a NaN or inf term: the sum is that, in any order
    mean = F32(np.float64(total) / np.float64(count)) if count else F32(np.nan)
    return {"count": count, "terms": e, "sum": total, "mean": mean}


def mean_bound(count):
    """relative bound on |mean - reference's float32 raster-order mean|: count * 2^-24 for the float32 accumulation of `count`
    non-negative terms (first order), 2^-23 for the reference's float division and our float conversion of the mean"""
    return count * 2.0 ** -24 + 2.0 ** -23


def camera(w, h):
    """a Kinect-like intrinsic matrix with non-integer principal point (the library truncates cx, cy)"""
    f = 575.8 * w / 640.0
    return np.array([[f, 0.0, w / 2.0 + 0.37], [0.0, f, h / 2.0 + 0.61], [0.0, 0.0, 1.0]], np.float64)


def depth_maps(seed, n, h, w, invalid=0.08, integer=False):
    """n depth maps [n, h, w] float32 in millimetres at Kinect ranges (400..8000), a fraction `invalid` of the pixels 0"""
    rng = np.random.default_rng(seed)
    z = rng.uniform(400.0, 8000.0, (n, h, w))
    z = np.rint(z) if integer else z
    z = np.where(rng.random((n, h, w)) < invalid, 0.0, z)
    return z.astype(F32)


def project(depth, K):
    """DimensionConvertor::projectiveToReal(float*) in numpy float32 (DimensionConvertor.h:34-62): subtract, divide, multiply,
    with cx, cy truncated to int"""
    depth = np.asarray(depth, F32)
    h, w = depth.shape[-2:]
    fx, fy, cx, cy = F32(K[0][0]), F32(K[1][1]), F32(int(K[0][2])), F32(int(K[1][2]))
    y, x = np.meshgrid(np.arange(h, dtype=F32), np.arange(w, dtype=F32), indexing="ij")
    px = ((x - cx) / fx) * depth
    py = ((cy - y) / fy) * depth
    return np.stack([px, py, depth], axis=-1).astype(F32)


def clouds(seed, n, h, w, m=1):
    """(candidates [m, n, h, w, 3], truth [n, h, w, 3]): the truth is the cloud of a random depth map, a candidate the same
    surface disturbed by a few millimetres in all three coordinates, each with its own invalid pixels"""
    K = camera(w, h)
    truth = project(depth_maps(seed, n, h, w), K)
    rng = np.random.default_rng(seed + 7919)
    cands = []
    for c in range(m):
        p = truth + rng.normal(0.0, 3.0 + c, truth.shape).astype(F32)
        p[..., 2] = np.where(rng.random((n, h, w)) < 0.05, 0.0, p[..., 2])
        cands.append(p.astype(F32))
    return np.stack(cands), truth
