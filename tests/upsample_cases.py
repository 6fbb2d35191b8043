"""GuidedDepthUpsampling (kde_upsample_*): the rule in numpy, the tables, and the named cases of the tests.

Every operation below is one IEEE binary32 operation in the order written (numpy float32 arithmetic rounds each result to
binary32 and never fuses a multiply with an add); divisions are the correctly rounded `/`.

  tables   sx = (float)src_w / (float)out_w, sy = (float)src_h / (float)out_h
           gx_of[qx] = clamp((int)rint(((float)qx + 0.5) / sx - 0.5), 0, out_w - 1), gy_of[qy] likewise: the output pixel that
           "is" low-resolution sample q
           range[k] = (float)exp(-(double)(k * k) / (2 sigma_color^2)) for k = 0 .. 765 (sigma_color widened to double)
  pixel    for output pixel (i, j) with guide colour c = bgr(i, j):
           u = ((float)i + 0.5) * sx - 0.5, v = ((float)j + 0.5) * sy - 0.5, x0 = floor(u), y0 = floor(v)
           taps qy = y0 - r + 1 .. y0 + r (outer), qx = x0 - r + 1 .. x0 + r (inner); absent outside the source frame and where
           the depth is not z > z_min and z < z_max
           wx = max(1 - |(float)qx - u| / (float)r, 0), wy likewise; k = |db| + |dg| + |dr| between c and
           bgr(gx_of[qx], gy_of[qy]); w = (wx * wy) * range[k]; a tap with w == 0 is absent
           max_gap > 0: zref = the depth of the tap with the largest w (the first in tap order wins a tie); taps with
           |z - zref| > max_gap are absent
           num = den = 0; per remaining tap in tap order num = num + w * z, den = den + w; the pixel is num / den, or 0 when no
           tap remains; filled = the pixels with a remaining tap (before any rounding to uint16)
"""
from collections import namedtuple

import numpy as np

F = np.float32
FLT_MAX = np.finfo(np.float32).max
RANGE_SIZE = 766

Tables = namedtuple("Tables", "sx sy gx_of gy_of range")


def range_table(sigma_color):
    """range[k] for k = 0 .. 765 as the library makes it: binary64 exp of a binary64 argument, rounded once to binary32"""
    k = np.arange(RANGE_SIZE, dtype=np.float64)
    s = np.float64(np.float32(sigma_color))
    with np.errstate(under="ignore"):
        return np.exp(-(k * k) / (2.0 * s * s)).astype(np.float32)


def _nearest_of(count, scale, out_count):
    q = np.arange(count, dtype=np.float32)
    g = np.rint((q + F(0.5)) / scale - F(0.5))
    assert g.dtype == np.float32
    return np.clip(g.astype(np.int64), 0, out_count - 1)


def tables(src_size, out_size, sigma_color, range_=None):
    """the tables of an object; range_ replaces the numpy range table (the tests pass the library's own)"""
    (sw, sh), (ow, oh) = src_size, out_size
    sx, sy = F(sw) / F(ow), F(sh) / F(oh)
    r = range_table(sigma_color) if range_ is None else np.asarray(range_, np.float32)
    assert r.shape == (RANGE_SIZE,)
    return Tables(sx, sy, _nearest_of(sw, sx, ow), _nearest_of(sh, sy, oh), r)


def widen(depth):
    depth = np.asarray(depth)
    assert depth.dtype in (np.float32, np.uint16)
    return depth.astype(np.float32)


def depth_to_u16(z):
    """kde::depth_to_u16: rounded half to even; 0 for what the format does not hold"""
    with np.errstate(all="ignore"):
        r = np.rint(np.asarray(z, np.float32))
        ok = (r >= 1) & (r <= 65535)
    return np.where(ok, r, 0).astype(np.uint16)


def upsample_parts(depth, bgr, t, out_size, radius=2, max_gap=F(0), z_min=F(0), z_max=FLT_MAX):
    """one frame: depth [sh, sw] float32 / uint16, bgr [oh, ow, 3] uint8 -> dict(z float32 [oh, ow], kept bool [oh, ow])"""
    z = widen(depth)
    sh, sw = z.shape
    ow, oh = out_size
    assert bgr.shape == (oh, ow, 3) and bgr.dtype == np.uint8
    r = int(radius)
    z_min, z_max, max_gap, fr = F(z_min), F(z_max), F(max_gap), F(r)
    i = np.arange(ow, dtype=np.float32)[None, :].repeat(oh, 0)
    j = np.arange(oh, dtype=np.float32)[:, None].repeat(ow, 1)
    u = (i + F(0.5)) * t.sx - F(0.5)
    v = (j + F(0.5)) * t.sy - F(0.5)
    assert u.dtype == np.float32 and v.dtype == np.float32
    x0, y0 = np.floor(u).astype(np.int64), np.floor(v).astype(np.int64)
    own = bgr.astype(np.int64)
    offs = [(ty, tx) for ty in range(2 * r) for tx in range(2 * r)]
    ws, zs, present = [], [], []
    with np.errstate(all="ignore"):
        for ty, tx in offs:
            qx, qy = x0 - r + 1 + tx, y0 - r + 1 + ty
            inside = (qx >= 0) & (qx < sw) & (qy >= 0) & (qy < sh)
            cx, cy = np.clip(qx, 0, sw - 1), np.clip(qy, 0, sh - 1)
            zt = z[cy, cx]
            ok = inside & (zt > z_min) & (zt < z_max)
            wx = np.maximum(F(1) - np.abs(qx.astype(np.float32) - u) / fr, F(0))
            wy = np.maximum(F(1) - np.abs(qy.astype(np.float32) - v) / fr, F(0))
            k = np.abs(own - bgr[t.gy_of[cy], t.gx_of[cx]].astype(np.int64)).sum(-1)
            w = (wx * wy) * t.range[k]
            assert w.dtype == np.float32
            ok &= w > F(0)
            ws.append(np.where(ok, w, F(0)).astype(np.float32))
            zs.append(np.where(ok, zt, F(0)).astype(np.float32))
            present.append(ok)
        if max_gap > 0:
            best = np.zeros((oh, ow), np.float32)
            zref = np.zeros((oh, ow), np.float32)
            for w, zt, p in zip(ws, zs, present):
                better = p & (w > best)
                best = np.where(better, w, best)
                zref = np.where(better, zt, zref)
            present = [p & ~(np.abs(zt - zref) > max_gap) for zt, p in zip(zs, present)]
        num = np.zeros((oh, ow), np.float32)
        den = np.zeros((oh, ow), np.float32)
        kept = np.zeros((oh, ow), bool)
        for w, zt, p in zip(ws, zs, present):
            num = np.where(p, num + w * zt, num)
            den = np.where(p, den + w, den)
            kept |= p
        assert num.dtype == np.float32 and den.dtype == np.float32
        out = np.where(kept, num / den, F(0)).astype(np.float32)
    return dict(z=out, kept=kept)


def upsample(depth, bgr, t, out_size, radius=2, max_gap=F(0), z_min=F(0), z_max=FLT_MAX, out_dtype=np.float32):
    """one frame: (upsampled depth [oh, ow] of out_dtype, filled)"""
    p = upsample_parts(depth, bgr, t, out_size, radius, max_gap, z_min, z_max)
    return (p["z"] if out_dtype == np.float32 else depth_to_u16(p["z"])), int(p["kept"].sum())


# ---- the cases -------------------------------------------------------------------------------------------------------
# The kernel (upsample_kernels.hip) gives a workgroup of 256 threads four consecutive tiles of 32 x 8 output pixels, stages
# each tile's taps in LDS, and stores a tile's rows as 16-byte (float) or 8-byte (uint16) vectors where the output frame
# starts on such a boundary and its width is a multiple of four, elements elsewhere.
Case = namedtuple("Case", "name src out why")
CASES = {c.name: c for c in (
    Case("fraction", (16, 12), (41, 29), "non-integer ratios, partial tiles in both directions; an odd width: element stores in every frame"),
    Case("double", (20, 15), (40, 30), "ratio 2: every gx_of is a tie of rint; width a multiple of 4: vector stores where the frame is aligned"),
    Case("quad", (10, 8), (40, 32), "ratio 4: ties of rint in gx_of and gy_of; four full tile rows; vector stores"),
    Case("identity", (13, 9), (13, 9), "equal sizes: with r = 1 the output is the input"),
    Case("one_pixel", (1, 1), (5, 3), "a one-pixel source: every tap but one is outside"),
    Case("cell", (3, 2), (67, 45), "ratio > 16: whole tiles inside one source cell, a tap window of 2r x 2r"),
    Case("row", (257, 1), (600, 1), "a single row: 19 tiles in five workgroups, the last with three tiles; taps above and below the frame"),
    Case("blocks", (70, 40), (131, 67), "5 x 9 = 45 tiles: twelve workgroups per frame, workgroups that span two tile rows"),
    Case("strip", (36, 5), (36, 11), "equal widths: a tile's tap window of 31 + 2r columns; with r = 4 more taps (39 x 11) than the workgroup has threads"),
)}
IDS = list(CASES)
RADII = {"fraction": (1, 2, 3, 4), "identity": (1, 2), "strip": (2, 4)}      # every other case: r = 2
Z_RANGE = (F(400.0), F(6000.0))
MAX_GAP = 100.0


def depth_frames(name, n=1, integer=False, invalid=0.1):
    """n source frames [n, sh, sw] float32: a ramp with a block 1500 mm further on the right; a tenth of the samples invalid
    (0, NaN, +-inf, negatives, values outside Z_RANGE; for `integer` whole millimetres and 0, 65535, 100, 7000)"""
    sw, sh = CASES[name].src
    rng = np.random.default_rng(sum(map(ord, name)) + (7 if integer else 0))
    y, x = np.mgrid[0:sh, 0:sw].astype(np.float32)
    out = np.empty((n, sh, sw), np.float32)
    bad = np.array([0.0, 65535.0, 100.0, 7000.0] if integer else [0.0, np.nan, np.inf, -np.inf, -5.0, 100.0, 7000.0, 399.99], np.float32)
    for f in range(n):
        z = F(1000.0 + 30.0 * f) + F(7.0) * x + F(3.5) * y + (F(0) if integer else rng.uniform(0, 0.5, (sh, sw)).astype(np.float32))
        z[:, (sw + 1) // 2:] += F(1500.0)
        if integer:
            z = np.rint(z)
        if sw * sh > 1:
            hit = rng.random((sh, sw)) < invalid
            z[hit] = bad[rng.integers(0, bad.size, int(hit.sum()))]
        out[f] = z
    return out


def bgr_frames(name, n=1):
    """n guides [n, oh, ow, 3] uint8: two flat regions that meet a little right of the depth step, +-6 of noise per channel,
    so that k spreads over 0 .. 36 within a region and sits near 300 across"""
    ow, oh = CASES[name].out
    rng = np.random.default_rng(2000 + sum(map(ord, name)))
    img = np.empty((n, oh, ow, 3), np.int64)
    edge = (ow + 1) // 2 + 1
    img[:, :, :edge] = (60, 90, 120)
    img[:, :, edge:] = (180, 170, 200)
    img += rng.integers(-6, 7, img.shape)
    return np.clip(img, 0, 255).astype(np.uint8)


# ---- the step-edge scene of the issue ----------------------------------------------------------------------------------
def step_scene(flat_colour=False):
    """16 x 12 -> 41 x 29; depth 1000 | 3000 with the step at low-resolution column 8; the colour edge at output column 20
    with +-4 of noise (or one flat colour); sigma_color 10"""
    src, out = (16, 12), (41, 29)
    depth = np.full((12, 16), 1000.0, np.float32)
    depth[:, 8:] = 3000.0
    rng = np.random.default_rng(11)
    img = np.empty((29, 41, 3), np.int64)
    if flat_colour:
        img[...] = 128
    else:
        img[:, :20] = (40, 60, 80)
        img[:, 20:] = (200, 180, 160)
        img += rng.integers(-4, 5, img.shape)
    return src, out, depth, np.clip(img, 0, 255).astype(np.uint8)
