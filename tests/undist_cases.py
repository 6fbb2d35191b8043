"""LensUndistortion (kde_undist_*): the rule in numpy, and the named cases of the tests.

Every operation below is one IEEE binary32 operation in the order written (numpy float32 arithmetic rounds each result to
binary32 and never fuses a multiply with an add); divisions are the correctly rounded `/`.

  calibration  the source (distorted) camera (fx, fy, cx, cy) and the target (pinhole) camera (fxn, fyn, cxn, cyn), each from a
               row-major 3 x 3 double matrix converted to float (K_new None: K); cx and cy stay floats; the coefficients
               k1, k2, p1, p2, k3, k4, k5, k6 (OpenCV's order, the rational model) doubles converted to float
  map          for output pixel (i, j):
               x  = ((float)i - cxn) / fxn;  y = ((float)j - cyn) / fyn
               xx = x * x;  yy = y * y;  xy = x * y;  r2 = xx + yy
               num = ((k3 * r2 + k2) * r2 + k1) * r2 + 1;  den = ((k6 * r2 + k5) * r2 + k4) * r2 + 1;  rad = num / den
               xd = (x * rad + p1 * (xy + xy)) + p2 * (r2 + (xx + xx));  yd = (y * rad + p1 * (r2 + (yy + yy))) + p2 * (xy + xy)
               us = fx * xd + cx;  vs = fy * yd + cy
  bilinear     x0 = floor(us), ax = us - x0, y0, ay likewise; taps p00 = p(x0, y0), p01 = p(x0 + 1, y0), p10 = p(x0, y0 + 1),
               p11 = p(x0 + 1, y0 + 1); top = p00 + ax * (p01 - p00); bot = p10 + ax * (p11 - p10); top + ay * (bot - top)
  colour       (0, 0, 0) unless us > -1 and us < sw and vs > -1 and vs < sh (on the floats; a NaN fails); a tap outside the
               source is (0, 0, 0); per channel rint(bilinear) clamped to 0 .. 255
  depth        valid iff z > z_min and z < z_max.  nearest: fu = rint(us), fv = rint(vs) (ties to even); kept iff 0 <= fu <=
               sw - 1 and 0 <= fv <= sh - 1 on the floats and the sample is valid, else 0.  depth_interp 1: bilinear iff
               x0 >= 0 and x0 + 1 <= sw - 1 and y0 >= 0 and y0 + 1 <= sh - 1, the four taps are valid and max - min <= max_gap;
               the nearest rule in every other case.  Output: the float, or depth_to_u16 of it; filled = the pixels kept.
"""
from collections import namedtuple

import numpy as np

F = np.float32
FLT_MAX = np.finfo(np.float32).max

Calib = namedtuple("Calib", "fx fy cx cy fxn fyn cxn cyn k K dist Knew")


def calib(K, dist, K_new=None):
    """the floats the library keeps (k = k1, k2, p1, p2, k3, k4, k5, k6), and the double arrays it is given"""
    K = np.asarray(K, np.float64).reshape(3, 3)
    Kn = K if K_new is None else np.asarray(K_new, np.float64).reshape(3, 3)
    d = np.zeros(8, np.float64)
    dist = np.asarray(dist, np.float64).reshape(-1)
    d[:dist.size] = dist
    return Calib(F(K[0, 0]), F(K[1, 1]), F(K[0, 2]), F(K[1, 2]), F(Kn[0, 0]), F(Kn[1, 1]), F(Kn[0, 2]), F(Kn[1, 2]),
                 d.astype(np.float32), K, d, None if K_new is None else Kn)


def source_points(c, out_size, pixels=None):
    """(us, vs) as float32 arrays: for all output pixels in raster order, or for the raster indices `pixels` in that order"""
    ow, oh = out_size
    p = np.arange(ow * oh) if pixels is None else np.asarray(pixels)
    i, j = (p % ow).astype(np.float32), (p // ow).astype(np.float32)
    k1, k2, p1, p2, k3, k4, k5, k6 = c.k
    with np.errstate(all="ignore"):
        x = (i - c.cxn) / c.fxn
        y = (j - c.cyn) / c.fyn
        xx, yy, xy = x * x, y * y, x * y
        r2 = xx + yy
        num = ((k3 * r2 + k2) * r2 + k1) * r2 + F(1)
        den = ((k6 * r2 + k5) * r2 + k4) * r2 + F(1)
        rad = num / den
        xd = (x * rad + p1 * (xy + xy)) + p2 * (r2 + (xx + xx))
        yd = (y * rad + p1 * (r2 + (yy + yy))) + p2 * (xy + xy)
        us = c.fx * xd + c.cx
        vs = c.fy * yd + c.cy
    assert us.dtype == np.float32 and vs.dtype == np.float32
    return us, vs


def undist_map(c, out_size):
    """what kde_undist_map_device holds: float32 [oh, ow, 2]"""
    ow, oh = out_size
    us, vs = source_points(c, out_size)
    return np.stack([us, vs], -1).reshape(oh, ow, 2)


def _bilinear(p00, p01, p10, p11, ax, ay):
    with np.errstate(all="ignore"):
        top = p00 + ax * (p01 - p00)
        bot = p10 + ax * (p11 - p10)
        return top + ay * (bot - top)


def color_parts(bgr, c, out_size, pixels=None):
    """one frame bgr [sh, sw, 3] uint8: (values [m, 3] uint8, taps inside the source per pixel 0..4 -- 0 where the range test fails)"""
    sh, sw = bgr.shape[:2]
    us, vs = source_points(c, out_size, pixels)
    with np.errstate(all="ignore"):
        inside = (us > F(-1)) & (us < F(sw)) & (vs > F(-1)) & (vs < F(sh))
        x0, y0 = np.floor(us), np.floor(vs)
        ax, ay = us - x0, vs - y0
    ix, iy = np.where(inside, x0, 0).astype(np.int64), np.where(inside, y0, 0).astype(np.int64)
    count = np.zeros(us.shape, np.int64)

    def tap(x, y):
        ok = inside & (x >= 0) & (x < sw) & (y >= 0) & (y < sh)
        v = bgr[np.clip(y, 0, sh - 1), np.clip(x, 0, sw - 1)].astype(np.float32)
        v[~ok] = 0
        count[...] += ok
        return v

    p00, p01, p10, p11 = tap(ix, iy), tap(ix + 1, iy), tap(ix, iy + 1), tap(ix + 1, iy + 1)
    v = _bilinear(p00, p01, p10, p11, ax[:, None], ay[:, None])
    v = np.where(inside[:, None], np.clip(np.rint(v), 0, 255), 0)
    return v.astype(np.uint8), count


def color(bgr, c, out_size, pixels=None):
    """one frame: uint8 [oh, ow, 3], or [m, 3] for the raster indices `pixels`"""
    ow, oh = out_size
    v, _ = color_parts(bgr, c, out_size, pixels)
    return v.reshape(oh, ow, 3) if pixels is None else v


def widen(depth):
    """(float)u16 for uint16 input, the floats themselves otherwise"""
    depth = np.asarray(depth)
    assert depth.dtype in (np.float32, np.uint16)
    return depth.astype(np.float32)


def depth_to_u16(z):
    """kde::depth_to_u16: rounded half to even; 0 for what the format does not hold"""
    with np.errstate(all="ignore"):
        r = np.rint(np.asarray(z, np.float32))
        ok = (r >= 1) & (r <= 65535)
    return np.where(ok, r, 0).astype(np.uint16)


def depth_parts(depth, c, out_size, z_min=F(0), z_max=FLT_MAX, interp=0, max_gap=F(0), pixels=None):
    """one frame [sh, sw]: a dict of flat arrays over the pixels -- z (float32, 0 where no depth), kept, and the branches of
    the guard: blended, hole (four taps inside, one invalid), gap (four valid taps further apart than max_gap), border (a tap
    outside)"""
    z = widen(depth)
    sh, sw = z.shape
    z_min, z_max, max_gap = F(z_min), F(z_max), F(max_gap)
    lastx, lasty = F(sw - 1), F(sh - 1)
    us, vs = source_points(c, out_size, pixels)
    with np.errstate(all="ignore"):
        fu, fv = np.rint(us), np.rint(vs)
        near_in = (fu >= 0) & (fu <= lastx) & (fv >= 0) & (fv <= lasty)
        zn = z[np.where(near_in, fv, 0).astype(np.int64), np.where(near_in, fu, 0).astype(np.int64)]
        kept = near_in & (zn > z_min) & (zn < z_max)
        out = np.where(kept, zn, F(0)).astype(np.float32)
        x0, y0 = np.floor(us), np.floor(vs)
        taps_in = (x0 >= 0) & (x0 + F(1) <= lastx) & (y0 >= 0) & (y0 + F(1) <= lasty)
        ix, iy = np.where(taps_in, x0, 0).astype(np.int64), np.where(taps_in, y0, 0).astype(np.int64)
        ix1, iy1 = np.minimum(ix + 1, sw - 1), np.minimum(iy + 1, sh - 1)
        z00, z01, z10, z11 = z[iy, ix], z[iy, ix1], z[iy1, ix], z[iy1, ix1]
        valid = np.ones(us.shape, bool)
        for t in (z00, z01, z10, z11):
            valid &= (t > z_min) & (t < z_max)
        hi = np.maximum(np.maximum(z00, z01), np.maximum(z10, z11))
        lo = np.minimum(np.minimum(z00, z01), np.minimum(z10, z11))
        near = (hi - lo) <= max_gap
        blended = taps_in & valid & near
        b = _bilinear(z00, z01, z10, z11, us - x0, vs - y0)
    parts = dict(blended=blended, hole=taps_in & ~valid, gap=taps_in & valid & ~near, border=~taps_in)
    if interp:
        out = np.where(blended, b, out).astype(np.float32)
        kept = blended | kept
    return dict(parts, z=out, kept=kept)


def depth(depth_map, c, out_size, z_min=F(0), z_max=FLT_MAX, interp=0, max_gap=F(0), out_dtype=np.float32, pixels=None):
    """one frame: (undistorted depth [oh, ow] of out_dtype -- flat for `pixels` --, filled)"""
    ow, oh = out_size
    p = depth_parts(depth_map, c, out_size, z_min, z_max, interp, max_gap, pixels)
    v = p["z"] if out_dtype == np.float32 else depth_to_u16(p["z"])
    return (v.reshape(oh, ow) if pixels is None else v), int(p["kept"].sum())


# ---- the cases -------------------------------------------------------------------------------------------------------
def K3(fx, fy, cx, cy):
    return np.array([[fx, 0.0, cx], [0.0, fy, cy], [0.0, 0.0, 1.0]], np.float64)


Case = namedtuple("Case", "name src out K dist Knew z_range max_gap why")
MAX_GAP = 50.0

CASES = {c.name: c for c in (
    Case("barrel", (37, 23), (41, 19), K3(30.0, 30.4, 18.3, 10.8), (-0.2, 0.0, 0.0, 0.0, 0.0), K3(20.0, 20.2, 19.7, 9.2), None, MAX_GAP,
         "widths no multiple of 4 and sizes that differ; k1 < 0 and a target camera wide enough that the target's corners and the "
         "ends of its rows show points outside the source: the colour paths with no tap, some taps and all taps inside"),
    Case("rational_tangential", (37, 23), (37, 23), K3(31.0, 30.0, 17.6, 11.3), (-0.28, 0.09, 0.004, -0.003, -0.02, 0.05, 0.02, 0.004),
         K3(29.0, 28.5, 18.2, 10.9), (400.0, 3000.0), MAX_GAP,
         "all eight coefficients non-zero and principal points that are no integers: every term of the model, a swapped p1 / p2 "
         "or a wrong power of r shows"),
    Case("identity", (13, 9), (13, 9), K3(16.0, 8.0, 6.5, 4.25), (0.0,) * 8, None, (400.0, 3000.0), MAX_GAP,
         "all coefficients zero and K_new NULL: dyadic focal lengths and principal points make the map exact (us == i), so the "
         "statement returns the source, in the bilinear mode as well"),
    Case("half_ties", (12, 10), (20, 16), K3(8.0, 4.0, 0.5, 0.5), (0.0,) * 8, K3(16.0, 8.0, 0.0, 0.0), None, MAX_GAP,
         "no distortion, fxn = 2 fx: us = i / 2 + 0.5 exactly, so every even i is a tie -- ties to an even and to an odd integer "
         "in the nearest rule, ax = 0.5 in the bilinear one"),
    Case("one_pixel", (1, 1), (1, 1), K3(5.0, 5.0, 0.0, 0.0), (-0.1, 0.01, 0.001, 0.001, 0.0), None, None, MAX_GAP,
         "1 x 1 -> 1 x 1: the smallest frame, one lane of one wave"),
    Case("sliver", (5, 3), (3, 5), K3(4.0, 4.0, 2.2, 1.1), (-0.15, 0.02, 0.002, -0.001, 0.0), K3(3.0, 3.0, 1.1, 2.2), None, MAX_GAP,
         "5 x 3 -> 3 x 5: less than one wave, a partial quad at the frame's end"),
    Case("tail", (64, 4), (257, 1), K3(40.0, 40.0, 31.5, 1.4), (-0.05, 0.0, 0.0, 0.0, 0.0), K3(160.0, 160.0, 128.0, 0.0), None, MAX_GAP,
         "64 x 4 -> 257 x 1: a full wave of quads plus one pixel, the wave that holds the frame's end beside a whole one"),
    Case("blocks", (96, 64), (131, 67), K3(80.0, 81.0, 47.3, 31.6), (-0.22, 0.06, 0.001, -0.0008, -0.01), K3(84.0, 84.5, 65.2, 33.4),
         (400.0, 3000.0), MAX_GAP,
         "96 x 64 -> 131 x 67 = 8777 pixels: more than the 8192 one workgroup of the depth kernel takes and nine workgroups of the "
         "colour kernel, so the workgroup index enters the pixel index; rows that are no multiple of the quad"),
)}
IDS = list(CASES)


def case_calib(name):
    c = CASES[name]
    return calib(c.K, c.dist, c.Knew)


def case_range(name):
    zr = CASES[name].z_range
    return (F(0), FLT_MAX) if zr is None else (F(zr[0]), F(zr[1]))


def depth_frames(name, n=1, integer=False, specials=True):
    """n source frames [n, sh, sw] float32 of a case: a ramp of 2 mm per column and 1.5 mm per row (far smaller than max_gap)
    with a block 400 mm nearer on its right (a step far larger than max_gap); with `specials`, single pixels of 0, NaN, +-inf
    and negatives (float) or 0 and 65535 (integer: whole millimetres, a uint16 map as well) where the frame has room for them"""
    sw, sh = CASES[name].src
    rng = np.random.default_rng(sum(map(ord, name)) + (1 if integer else 0))
    y, x = np.mgrid[0:sh, 0:sw].astype(np.float32)
    out = np.empty((n, sh, sw), np.float32)
    for f in range(n):
        z = F(1000.0 + 30.0 * f) + F(2.0) * x + F(1.5) * y + (F(0) if integer else rng.uniform(0, 0.5, (sh, sw)).astype(np.float32))
        if sw >= 5:
            z[sh // 4:, (3 * sw) // 5:] -= F(400.0)
        if integer:
            z = np.rint(z)
        sp = np.array([0.0, 65535.0, 0.0, 1.0] if integer else [0.0, np.nan, np.inf, -np.inf, -5.0, -0.0, 0.0, 0.0], np.float32)
        if specials:
            sp = sp[:max(0, min(sp.size, (sw * sh) // 6))]
            at = rng.choice(sw * sh, sp.size, replace=False)
            z.reshape(-1)[at] = sp
        out[f] = z
    return out


def bgr_frames(name, n=1):
    sw, sh = CASES[name].src
    return np.random.default_rng(1000 + sum(map(ord, name))).integers(0, 256, (n, sh, sw, 3), dtype=np.uint8)
