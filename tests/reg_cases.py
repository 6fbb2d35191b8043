"""DepthRegistration (kde_reg_*, Kinect.cpp:71-75): the rule in numpy, and the inputs of the tests.

Every operation below is one IEEE binary32 operation in the order written (numpy float32 arithmetic rounds each result to
binary32 and never fuses a multiply with an add); divisions are the correctly rounded `/`.

  calibration  depth camera (fxd, fyd, cxd, cyd), colour camera (fxc, fyc, cxc, cyc), each from a row-major 3 x 3 double matrix
               converted to float -- cx and cy stay floats, they are NOT truncated as DimensionConvertor does; R (row-major)
               and t (millimetres) converted to float, P_colour = R * P_depth + t; x right, y down, z forward, pixel centres
               at integer coordinates
  valid        z > z_min && z < z_max
  project(a, b)  xn = (a - cxd) / fxd; yn = (b - cyd) / fyd; X = xn * z; Y = yn * z
               Xc = ((r00 * X + r01 * Y) + r02 * z) + tx, Yc, Zc likewise; fails unless Zc > z_min && Zc < z_max
               uc = fxc * (Xc / Zc) + cxc; vc = fyc * (Yc / Zc) + cyc
  key          the bits of the centre's Zc as uint32
  point mode   iu = rint(uc), iv = rint(vc) (ties to even); kept iff 0 <= iu <= Wc - 1 and 0 <= iv <= Hc - 1 on the floats
  splat mode   corners project(u - 0.5, v - 0.5) and project(u + 0.5, v + 0.5); columns max(ceil(min(ua, ub)), 0) ..
               min(ceil(max(ua, ub)) - 1, Wc - 1), cut to max_splat from the first; rows likewise
  zbuf         np.minimum.at on the uint32 keys, 0xFFFFFFFF where nothing came
  finalise     0 where nothing came, else Zc (float) or depth_to_u16(Zc); filled = the number of keys reached
"""
from collections import namedtuple

import numpy as np

F = np.float32
EMPTY = np.uint32(0xFFFFFFFF)
FLT_MAX = np.finfo(np.float32).max

Calib = namedtuple("Calib", "fxd fyd cxd cyd fxc fyc cxc cyc r t Kd Kc R T")


def calib(Kd, Kc, R, t):
    """the floats the library keeps, and the double arrays it was given"""
    Kd, Kc, R = (np.asarray(m, np.float64).reshape(3, 3) for m in (Kd, Kc, R))
    t = np.asarray(t, np.float64).reshape(3)
    return Calib(F(Kd[0, 0]), F(Kd[1, 1]), F(Kd[0, 2]), F(Kd[1, 2]), F(Kc[0, 0]), F(Kc[1, 1]), F(Kc[0, 2]), F(Kc[1, 2]),
                 R.astype(np.float32).reshape(9), t.astype(np.float32), Kd, Kc, R, t)


def project(a, b, z, c, z_min, z_max):
    """(uc, vc, Zc, ok) of float32 arrays a, b, z"""
    with np.errstate(all="ignore"):
        xn = (a - c.cxd) / c.fxd
        yn = (b - c.cyd) / c.fyd
        X = xn * z
        Y = yn * z
        r, t = c.r, c.t
        Xc = ((r[0] * X + r[1] * Y) + r[2] * z) + t[0]
        Yc = ((r[3] * X + r[4] * Y) + r[5] * z) + t[1]
        Zc = ((r[6] * X + r[7] * Y) + r[8] * z) + t[2]
        ok = (Zc > z_min) & (Zc < z_max)
        uc = c.fxc * (Xc / Zc) + c.cxc
        vc = c.fyc * (Yc / Zc) + c.cyc
    assert all(v.dtype == np.float32 for v in (uc, vc, Zc))
    return uc, vc, Zc, ok


def widen(depth):
    """(float)u16 for uint16 input, the floats themselves otherwise"""
    depth = np.asarray(depth)
    assert depth.dtype in (np.float32, np.uint16)
    return depth.astype(np.float32)


def _span(a, b, last, max_splat):
    """first and last integer of [min(a, b), max(a, b)) inside 0 .. last, cut to max_splat; (i0, i1, nonempty)"""
    with np.errstate(all="ignore"):
        lo, hi = np.minimum(a, b), np.maximum(a, b)
        f0 = np.maximum(np.ceil(lo), F(0))
        f1 = np.minimum(np.ceil(hi) - F(1), F(last))
        some = f0 <= f1
    i0 = np.where(some, f0, 0).astype(np.int64)
    i1 = np.where(some, f1, -1).astype(np.int64)
    i1 = np.minimum(i1, i0 + max_splat - 1)
    return i0, i1, some


def centre_targets(depth, c, color_size, z_min=F(0), z_max=FLT_MAX):
    """per source pixel of one frame [Hd, Wd]: (kept, iu, iv, Zc) of point mode"""
    z = widen(depth)
    hd, wd = z.shape
    wc, hc = color_size
    z_min, z_max = F(z_min), F(z_max)
    v, u = np.meshgrid(np.arange(hd, dtype=np.float32), np.arange(wd, dtype=np.float32), indexing="ij")
    with np.errstate(all="ignore"):
        valid = (z > z_min) & (z < z_max)
        uc, vc, Zc, ok = project(u, v, z, c, z_min, z_max)
        iu, iv = np.rint(uc), np.rint(vc)
        kept = valid & ok & (iu >= 0) & (iu <= F(wc - 1)) & (iv >= 0) & (iv <= F(hc - 1))
    return kept, np.where(kept, iu, 0).astype(np.int64), np.where(kept, iv, 0).astype(np.int64), Zc


def keys(depth, c, color_size, z_min=F(0), z_max=FLT_MAX, max_splat=0, order=None):
    """the z-buffer of one frame [Hd, Wd] (float32 or uint16): uint32 [Hc, Wc].  order: a permutation of the source pixels
    (raster indices), the order in which they are offered to the z-buffer"""
    z = widen(depth)
    hd, wd = z.shape
    wc, hc = color_size
    z_min, z_max = F(z_min), F(z_max)
    zbuf = np.full(wc * hc, EMPTY, np.uint32)
    kept, iu, iv, Zc = centre_targets(depth, c, color_size, z_min, z_max)
    key = Zc.view(np.uint32)
    if order is None:
        order = np.arange(hd * wd)
    flat = lambda a: a.reshape(-1)[order]
    if max_splat == 0:
        m = flat(kept)
        np.minimum.at(zbuf, (flat(iv) * wc + flat(iu))[m], flat(key)[m])
        return zbuf.reshape(hc, wc)
    v, u = np.meshgrid(np.arange(hd, dtype=np.float32), np.arange(wd, dtype=np.float32), indexing="ij")
    with np.errstate(all="ignore"):
        valid = (z > z_min) & (z < z_max)
        _, _, _, ok = project(u, v, z, c, z_min, z_max)
        ua, va, _, oka = project(u - F(0.5), v - F(0.5), z, c, z_min, z_max)
        ub, vb, _, okb = project(u + F(0.5), v + F(0.5), z, c, z_min, z_max)
        alive = valid & ok & oka & okb & ~(np.isnan(ua) | np.isnan(va) | np.isnan(ub) | np.isnan(vb))
    i0, i1, si = _span(ua, ub, wc - 1, max_splat)
    j0, j1, sj = _span(va, vb, hc - 1, max_splat)
    alive = alive & si & sj
    alive, i0, i1, j0, j1, key = (flat(a) for a in (alive, i0, i1, j0, j1, key))
    for dj in range(max_splat):
        for di in range(max_splat):
            m = alive & (i0 + di <= i1) & (j0 + dj <= j1)
            if m.any():
                np.minimum.at(zbuf, ((j0 + dj) * wc + (i0 + di))[m], key[m])
    return zbuf.reshape(hc, wc)


def depth_to_u16(z):
    """kde::depth_to_u16: rounded half to even; 0 for what the format does not hold"""
    with np.errstate(all="ignore"):
        r = np.rint(np.asarray(z, np.float32))
        ok = (r >= 1) & (r <= 65535)
    return np.where(ok, r, 0).astype(np.uint16)


def finalise(zbuf, out_dtype=np.float32):
    """(registered depth, filled) of a z-buffer"""
    reached = zbuf != EMPTY
    zc = np.where(reached, zbuf, np.uint32(0)).astype(np.uint32).view(np.float32)
    return (zc if out_dtype == np.float32 else depth_to_u16(zc)), int(reached.sum())


def statement(depth, c, color_size, z_min=F(0), z_max=FLT_MAX, max_splat=0, out_dtype=np.float32, order=None):
    """one frame: (registered depth [Hc, Wc] of out_dtype, filled)"""
    return finalise(keys(depth, c, color_size, z_min, z_max, max_splat, order), out_dtype)


def color_to_depth(depth, bgr, c, z_min=F(0), z_max=FLT_MAX):
    """the companion gather of one frame: bgr [Hc, Wc, 3] as the depth camera sees it, [Hd, Wd, 3]; no occlusion test"""
    hc, wc = bgr.shape[:2]
    kept, iu, iv, _ = centre_targets(depth, c, (wc, hc), z_min, z_max)
    return np.where(kept[..., None], bgr[iv, iu], np.uint8(0)).astype(np.uint8)


# ---- inputs ----------------------------------------------------------------------------------------------------------
def camera(w, h, f, dx=0.0, dy=0.0):
    """a 3 x 3 intrinsic matrix with a principal point that is no integer"""
    return np.array([[f, 0.0, (w - 1) / 2.0 + 0.3 + dx], [0.0, f * 1.01, (h - 1) / 2.0 - 0.2 + dy], [0.0, 0.0, 1.0]], np.float64)


def rotation(deg_y, deg_x=0.0):
    a, b = np.deg2rad(deg_y), np.deg2rad(deg_x)
    ry = np.array([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]])
    rx = np.array([[1, 0, 0], [0, np.cos(b), -np.sin(b)], [0, np.sin(b), np.cos(b)]])
    return ry @ rx


def special_z(z_min, z_max):
    """what no rule may mishandle: NaN, +-inf, 0, -0, negatives, and both ends of the range with their neighbours"""
    z_min, z_max = F(z_min), F(z_max)
    with np.errstate(over="ignore"):
            return np.array([np.nan, np.inf, -np.inf, 0.0, -0.0, -5.0, -1e30, z_min, np.nextafter(z_min, F(np.inf)),
                         np.nextafter(z_min, F(-np.inf)), z_max, np.nextafter(z_max, F(-np.inf)), np.nextafter(z_max, F(np.inf))],
                        np.float32)


def depth_maps(seed, n, h, w, z_min=F(0), z_max=FLT_MAX, integer=False):
    """n frames [h, w] float32: a tilted plane, boxes at several depths in front of it, about a tenth of the pixels invalid
    (0), and the special values.  integer: whole millimetres in 0..65535 (a uint16 map as well), with 0 and 65535 among them"""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w].astype(np.float32)
    out = np.empty((n, h, w), np.float32)
    for f in range(n):
        z = F(1800.0 + 40.0 * f) + F(900.0 / w) * x + F(500.0 / h) * y + rng.uniform(0, 3, (h, w)).astype(np.float32)
        for near in (1300.0, 900.0, 650.0):
            bw, bh = max(1, w // 4), max(1, h // 3)
            x0, y0 = rng.integers(0, w - bw + 1), rng.integers(0, h - bh + 1)
            z[y0:y0 + bh, x0:x0 + bw] = F(near) + rng.uniform(0, 2, (bh, bw)).astype(np.float32)
        z[rng.random((h, w)) < 0.1] = 0.0
        if integer:
            z = np.rint(z)
            sp = np.array([0.0, 65535.0, 1.0, 65534.0] + [float(v) for v in (z_min, z_max) if 0 <= v <= 65535 and v == np.rint(v)], np.float32)
            sp = np.concatenate([sp, np.clip(sp[4:] + 1, 0, 65535), np.clip(sp[4:] - 1, 0, 65535)])
        else:
            sp = special_z(z_min, z_max)
        at = rng.choice(h * w, sp.size, replace=False)
        z.reshape(-1)[at] = sp
        out[f] = z
    return out


def bgr_images(seed, n, h, w):
    return np.random.default_rng(1000 + seed).integers(0, 256, (n, h, w, 3), dtype=np.uint8)
