"""The rule of PointCloudXYZRGB (main.cpp:211-300) stated in numpy, and the inputs its tests share.

For pixel i in raster order, with point p in millimetres and colour bytes (b, g, r):
    valid   iff p.z > z_min and p.z < z_max                     (defaults 50 and 15000; NaN and +-inf are invalid)
    record  x = p.x / divisor, y = p.y / divisor, z = -(p.z / divisor) (or p.z / divisor), rgb = (r << 16) | (g << 8) | b
    dense   the records of the valid pixels, in raster order; organised: every pixel, an invalid one as three quiet NaNs
            (0x7fc00000) and its colour
The statement is: mask, float32 `/`, negate, pack.  numpy's float32 division is correctly rounded.
"""
import numpy as np

import error3d_cases as EC

F32 = np.float32
Z_MIN, Z_MAX, DIVISOR = F32(50.0), F32(15000.0), F32(1000.0)
POINT = np.dtype([("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("rgb", "<u4")])
QNAN = np.uint32(0x7FC00000)


def valid_mask(points, z_min=Z_MIN, z_max=Z_MAX):
    z = np.asarray(points, F32)[..., 2]
    with np.errstate(invalid="ignore"):
        return (z > F32(z_min)) & (z < F32(z_max))


def statement(points, bgr, z_min=Z_MIN, z_max=Z_MAX, divisor=DIVISOR, negate_z=True, organized=False):
    """one frame, points [H, W, 3] (or [k, 3]) float32 and bgr of the same pixels uint8: the records (POINT) the frame gives,
    count of them valid"""
    p = np.asarray(points, F32).reshape(-1, 3)
    c = np.asarray(bgr, np.uint8).reshape(-1, 3).astype(np.uint32)
    v = valid_mask(p, z_min, z_max)
    rec = np.empty(p.shape[0], POINT)
    with np.errstate(invalid="ignore", over="ignore", under="ignore"):
        d = F32(divisor)
        x, y, z = p[:, 0] / d, p[:, 1] / d, p[:, 2] / d
        z = -z if negate_z else z
    assert x.dtype == F32 and z.dtype == F32
    rec["x"], rec["y"], rec["z"] = x, y, z
    rec["rgb"] = (c[:, 2] << 16) | (c[:, 1] << 8) | c[:, 0]
    if not organized:
        return rec[v]
    for name in ("x", "y", "z"):
        rec[name].view(np.uint32)[~v] = QNAN
    return rec


def count(points, z_min=Z_MIN, z_max=Z_MAX):
    return int(valid_mask(np.asarray(points, F32).reshape(-1, 3), z_min, z_max).sum())


def special_z(z_min=Z_MIN, z_max=Z_MAX):
    """the z values every case holds: NaN, +-inf, -0, and z_min, z_max with their neighbours on both sides"""
    lo, hi, inf = F32(z_min), F32(z_max), F32(np.inf)
    return np.array([np.nan, np.inf, -np.inf, -0.0, lo, hi, np.nextafter(lo, inf), np.nextafter(lo, -inf), np.nextafter(hi, inf),
                     np.nextafter(hi, -inf)], F32)


SPECIAL_VALID = np.array([0, 0, 0, 0, 0, 0, 1, 0, 0, 1], bool)      # which of special_z() the rule admits


def _special_at(px):
    """ten distinct pixel indices of a frame of px pixels (px >= 10), the first and the last pixel among them"""
    at = (np.arange(10) * (px - 1)) // 9
    assert len(set(at.tolist())) == 10
    return at


def bgr_images(seed, n, h, w):
    return np.random.default_rng(seed + 31).integers(0, 256, (n, h, w, 3), dtype=np.uint8)


def clouds(seed, n, h, w, valid=0.7, z_min=Z_MIN, z_max=Z_MAX):
    """n organised clouds [n, h, w, 3] float32: about `valid` of the pixels inside (z_min, z_max), the others 0, below, above,
    negative or NaN; every frame holds special_z() at ten pixels (the first and the last of the frame among them), and a NaN,
    an inf and a -0 in the x or y of pixels that are valid"""
    rng = np.random.default_rng(seed)
    lo, hi = float(z_min), float(z_max)
    p = np.empty((n, h * w, 3), F32)
    p[..., 0] = rng.uniform(-4000.0, 4000.0, (n, h * w))
    p[..., 1] = rng.uniform(-3000.0, 3000.0, (n, h * w))
    z = (lo + min(hi - lo, 8000.0) * rng.uniform(0.01, 0.99, (n, h * w))).astype(F32)
    bad = np.array([0.0, lo - 1.0, hi + 1.0, -1000.0, np.nan, lo * 0.5, hi * 2.0], F32)
    pick = bad[rng.integers(0, bad.size, (n, h * w))]
    p[..., 2] = np.where(rng.random((n, h * w)) < valid, z, pick)
    at = _special_at(h * w)
    for f in range(n):
        p[f, at, 2] = np.roll(special_z(z_min, z_max), f)           # another special value first in every frame
        ok = np.flatnonzero(valid_mask(p[f], z_min, z_max))
        if ok.size >= 3:
            p[f, ok[0], 0] = np.nan
            p[f, ok[ok.size // 2], 1] = np.inf
            p[f, ok[-1], 0] = -0.0
    return p.reshape(n, h, w, 3)


def depth_maps(seed, n, h, w, valid=0.7, integer=False):
    """n depth maps [n, h, w] float32 with about `valid` of the pixels inside (50, 15000); the special values of special_z() at
    ten pixels of every frame (integer=True: maps a uint16 holds, with 0, 49, 50, 51, 14999, 15000, 15001, 65535 instead)"""
    rng = np.random.default_rng(seed)
    z = rng.uniform(400.0, 8000.0, (n, h * w))
    z = np.rint(z) if integer else z
    bad = np.array([0.0, 20.0, 16000.0, 49.0, 15001.0], np.float64)
    z = np.where(rng.random((n, h * w)) < valid, z, bad[rng.integers(0, bad.size, (n, h * w))]).astype(F32)
    at = _special_at(h * w)
    special = np.array([0, 49, 50, 51, 14999, 15000, 15001, 65535, 0, 51], F32) if integer else special_z()
    for f in range(n):
        z[f, at] = np.roll(special, f)
    return z.reshape(n, h, w)


def hand_case():
    """four pixels worked out by hand from main.cpp:222-236: (points, bgr, dense records, organised records)"""
    pts = np.array([[1000.0, -2000.0, 3000.0],      # valid: (1, -2, -3)
                    [5.0, 5.0, 50.0],               # z == 50 is not > 50
                    [123.456, 0.0, 15000.0],        # z == 15000 is not < 15000
                    [-250.0, 125.0, 50.5]], F32)    # valid: (-0.25, 0.125, -0.0505)
    bgr = np.array([[10, 20, 30], [1, 2, 3], [4, 5, 6], [255, 0, 128]], np.uint8)
    dense = np.array([(1.0, -2.0, -3.0, 0x1E140A), (-0.25, 0.125, -0.0505, 0x8000FF)], POINT)
    nan = F32(np.nan)
    org = np.array([(1.0, -2.0, -3.0, 0x1E140A), (nan, nan, nan, 0x030201), (nan, nan, nan, 0x060504),
                    (-0.25, 0.125, -0.0505, 0x8000FF)], POINT)
    for name in ("x", "y", "z"):
        org[name].view(np.uint32)[1:3] = QNAN
    return pts, bgr, dense, org


camera = EC.camera


def project(depth, K):
    """error3d_cases.project (projectiveToReal in numpy) for maps that hold NaN and +-inf as well"""
    with np.errstate(invalid="ignore"):
        return EC.project(depth, K)
