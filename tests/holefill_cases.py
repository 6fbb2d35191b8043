"""DepthHoleFilling (kde_holefill_*): the rule in numpy, the tables, and the named cases of the tests.

Every operation below is one IEEE binary32 operation in the order written (numpy float32 arithmetic rounds each result to
binary32 and never fuses a multiply with an add); divisions are the correctly rounded `/`.  With r = radius, N = iterations:

  tables   space[dy + r][dx + r] = (float)exp(-(double)(dx * dx + dy * dy) / (2 sigma_space^2))
           range[k] = (float)exp(-(double)(k * k) / (2 sigma_color^2)) for k = 0 .. 765 (each sigma widened to double)
  state    a float image z in which 0 means "hole"
  pass 0   z = (d > z_min && d < z_max) ? (float)d : 0 (NaN and +-inf become holes, uint16 is widened);
           pass_of = 0 where z > 0 and 255 elsewhere
  pass p   = 1 .. N reads the state of pass p - 1 as a snapshot and writes a new state.  For each pixel with z == 0:
           1. its taps are dy = -r .. r (outer), dx = -r .. r (inner), without the centre
           2. a tap is absent if it lies outside the frame or has z == 0
           3. k = |db| + |dg| + |dr| between the guide at the pixel and the guide at the tap
           4. w = space[dy + r][dx + r] * range[k]; a tap with w == 0 is absent: w > 0 is the test
           5. support = the number of taps that remain
           6. max_gap > 0: zref = the depth of the heaviest remaining tap, the first in tap order winning a tie (gap_rule 0),
              or the largest depth among the remaining taps (gap_rule 1); taps with |z - zref| > max_gap become absent;
              support is not recounted
           7. num = num + w * z, den = den + w over the remaining taps in tap order; v = num / den
           8. the pixel becomes v with pass_of = p iff support >= min_taps and v > 0; otherwise it stays 0
           pixels with z > 0 never change
  result   out = the state, as float or depth_to_u16 of it; filled = the pixels with 1 <= pass_of <= N, remaining = the pixels
           still 0, both before any uint16 rounding; pass_of: 0 original, p filled in pass p, 255 still a hole
"""
from collections import namedtuple

import numpy as np

F = np.float32
FLT_MAX = np.finfo(np.float32).max
RANGE_SIZE = 766


def space_table(radius, sigma_space):
    """space[dy + r][dx + r] as the library makes it: binary64 exp of a binary64 argument, rounded once to binary32"""
    r = int(radius)
    d = np.arange(-r, r + 1, dtype=np.float64)
    s = np.float64(np.float32(sigma_space))
    with np.errstate(under="ignore"):
        return np.exp(-(d[None, :] * d[None, :] + d[:, None] * d[:, None]) / (2.0 * s * s)).astype(np.float32)


def range_table(sigma_color):
    """range[k] for k = 0 .. 765, made the same way"""
    k = np.arange(RANGE_SIZE, dtype=np.float64)
    s = np.float64(np.float32(sigma_color))
    with np.errstate(under="ignore"):
        return np.exp(-(k * k) / (2.0 * s * s)).astype(np.float32)


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


def sanitise(depth, z_min=F(0), z_max=FLT_MAX):
    """pass 0: the state of a frame"""
    d = widen(depth)
    with np.errstate(invalid="ignore"):
        return np.where((d > F(z_min)) & (d < F(z_max)), d, F(0)).astype(np.float32)


def one_pass(z, bgr, space, range_, radius, min_taps, max_gap=F(0), gap_rule=0):
    """one pass on the state z [h, w] float32 under the guide bgr [h, w, 3] uint8: (the new state, the pixels it filled)"""
    r = int(radius)
    h, w = z.shape
    assert z.dtype == np.float32 and bgr.shape == (h, w, 3) and bgr.dtype == np.uint8
    assert space.shape == (2 * r + 1, 2 * r + 1) and space.dtype == np.float32 and range_.shape == (RANGE_SIZE,) and range_.dtype == np.float32
    max_gap = F(max_gap)
    zp = np.zeros((h + 2 * r, w + 2 * r), np.float32)          # a tap outside the frame is absent, like a hole
    zp[r:r + h, r:r + w] = z
    gp = np.zeros((h + 2 * r, w + 2 * r, 3), np.int64)
    gp[r:r + h, r:r + w] = bgr
    own = bgr.astype(np.int64)
    ws, zs, present = [], [], []
    with np.errstate(all="ignore"):
        for dy in range(-r, r + 1):
            for dx in range(-r, r + 1):
                if dy == 0 and dx == 0:
                    continue
                zt = zp[r + dy:r + dy + h, r + dx:r + dx + w]
                k = np.abs(own - gp[r + dy:r + dy + h, r + dx:r + dx + w]).sum(-1)
                wt = space[dy + r, dx + r] * range_[k]
                assert wt.dtype == np.float32
                ws.append(wt)
                zs.append(zt)
                present.append((zt != F(0)) & (wt > F(0)))
        support = np.sum(present, axis=0)
        if max_gap > 0:
            zref = np.zeros((h, w), np.float32)
            if gap_rule == 0:
                best = np.zeros((h, w), np.float32)
                for wt, zt, p in zip(ws, zs, present):
                    better = p & (wt > best)
                    best = np.where(better, wt, best)
                    zref = np.where(better, zt, zref)
            else:
                for zt, p in zip(zs, present):
                    zref = np.where(p & (zt > zref), zt, zref)
            present = [p & ~(np.abs(zt - zref) > max_gap) for zt, p in zip(zs, present)]
        num = np.zeros((h, w), np.float32)
        den = np.zeros((h, w), np.float32)
        for wt, zt, p in zip(ws, zs, present):
            num = np.where(p, num + wt * zt, num)
            den = np.where(p, den + wt, den)
        assert num.dtype == np.float32 and den.dtype == np.float32
        v = num / den
        fill = (z == F(0)) & (support >= int(min_taps)) & (v > F(0))
    return np.where(fill, v, z).astype(np.float32), fill


def fill_parts(depth, bgr, space, range_, radius=2, iterations=8, min_taps=3, max_gap=F(0), gap_rule=0, z_min=F(0), z_max=FLT_MAX):
    """one frame: depth [h, w] float32 / uint16, bgr [h, w, 3] uint8 -> dict(z float32, pass_of uint8, filled, remaining)"""
    z = sanitise(depth, z_min, z_max)
    pass_of = np.where(z > 0, 0, 255).astype(np.uint8)
    for p in range(1, int(iterations) + 1):
        z, fill = one_pass(z, bgr, space, range_, radius, min_taps, max_gap, gap_rule)
        if not fill.any():
            break                                               # the state did not change: neither will any later pass
        pass_of[fill] = p
    return dict(z=z, pass_of=pass_of, filled=int(((pass_of >= 1) & (pass_of != 255)).sum()), remaining=int((z == 0).sum()))


def fill(depth, bgr, space, range_, out_dtype=np.float32, **kw):
    """one frame: (filled depth [h, w] of out_dtype, pass_of, filled, remaining)"""
    p = fill_parts(depth, bgr, space, range_, **kw)
    return (p["z"] if out_dtype == np.float32 else depth_to_u16(p["z"])), p["pass_of"], p["filled"], p["remaining"]


# ---- the cases -------------------------------------------------------------------------------------------------------
# The kernel (holefill_kernels.hip) gives a workgroup of 256 threads one tile of 32 x 16 pixels; a launch stages the tile and a
# halo of k * r pixels and performs k <= 4 passes on it in LDS; a tile without a hole does no pass and copies its pixels.
TILE = (32, 16)
Case = namedtuple("Case", "name size radii params why")
CASES = {c.name: c for c in (
    Case("identity", (37, 21), (2,), {}, "no hole: every tile takes the copy path, partial tiles right and below; the output is the sanitised input"),
    Case("one_pixel", (1, 1), (1, 2, 3), {}, "a 1 x 1 hole: every tap is outside the frame, the hole stays, remaining is 1"),
    Case("speck", (70, 45), (1, 2, 3), dict(min_taps=1, sigma_color=1e6),
         "one valid pixel: the front crosses tile borders, partial tiles and launch boundaries; pass_of = ceil(chessboard distance / r), "
         "255 above N; tiles whose staged window holds no valid pixel at all"),
    Case("band", (48, 24), (1, 2, 3), {}, "an 8-pixel vertical hole band, columns 28 .. 35 across the tile border at 32, between two surfaces of "
         "different colour and depth; the colour edge at column 32: each side fills up to it; a partial tile row"),
    Case("island", (52, 50), (2,), {}, "a 36 x 36 hole, wider than 2 N r = 32: the inside stays, remaining > 0; tiles that are all hole"),
    Case("border", (35, 19), (1, 2, 3), {}, "holes along all four frame borders and in all four corners, odd sizes: taps outside the frame on every "
         "side, halo cells outside the frame that must not be filled"),
    Case("blocks", (101, 53), (1, 2, 3), {}, "4 x 4 tiles, 10 % salt plus rectangles: several workgroups, holes at tile corners, every launch count"),
    Case("twins", (44, 20), (2,), dict(sigma_color=30.0), "two surfaces of one colour 500 mm apart with a 6-pixel band between them across the tile "
         "border: the guard off blends them, gap_rule 0 and 1 at max_gap 100 do not, and differ"),
)}
IDS = list(CASES)
BASE = dict(iterations=8, min_taps=3, sigma_space=2.0, sigma_color=30.0)
Z_RANGE = (F(400.0), F(6000.0))
MAX_GAP = 100.0
GUARDS = ((0.0, 0), (MAX_GAP, 0), (MAX_GAP, 1))                # (max_gap, gap_rule)
BAND = (28, 36)                                                 # the hole columns of `band`
TWINS_BAND = (29, 35)
ISLAND = (slice(7, 43), slice(8, 44))                           # rows, columns
SPECKS = ((3, 2), (34, 17), (69, 44))                           # (x, y) of the valid pixel of each frame of `speck`
EDGE = {"band": 32, "twins": None}                              # the guide's colour edge; every other case: a little right of the middle


def params(name, **over):
    """the rule's parameters of a case: BASE, the case's own, then `over`"""
    p = dict(BASE)
    p.update(CASES[name].params)
    p.update(over)
    return p


def _salt(rng, z, integer, rate=0.1):
    bad = np.array([0.0, 65535.0, 100.0, 7000.0] if integer else [0.0, np.nan, np.inf, -np.inf, -5.0, 100.0, 7000.0, 399.99], np.float32)
    hit = rng.random(z.shape) < rate
    z[hit] = bad[rng.integers(0, bad.size, int(hit.sum()))]


def depth_frames(name, n=3, integer=False):
    """n frames [n, h, w] float32 (for `integer` whole millimetres, which a uint16 holds): a ramp with a block 1500 mm further on
    the right; where the case has salt, a tenth of the valid depth replaced by 0, NaN, +-inf, negatives and values outside
    Z_RANGE (for `integer` 0, 65535, 100, 7000)"""
    w, h = CASES[name].size
    rng = np.random.default_rng(sum(map(ord, name)) + (7 if integer else 0))
    y, x = np.mgrid[0:h, 0:w].astype(np.float32)
    out = np.empty((n, h, w), np.float32)
    for f in range(n):
        z = F(1000.0 + 30.0 * f) + F(7.0) * x + F(3.5) * y + (F(0) if integer else rng.uniform(0, 0.5, (h, w)).astype(np.float32))
        z[:, (w + 1) // 2:] += F(1500.0)
        if name in ("band", "twins"):                           # two nearly flat surfaces
            split, step = (EDGE["band"], 1500.0) if name == "band" else ((TWINS_BAND[0] + TWINS_BAND[1]) // 2, 500.0)
            z = F(1000.0 + 30.0 * f) + F(0.5) * y + (F(0) if integer else rng.uniform(0, 0.5, (h, w)).astype(np.float32))
            z[:, split:] += F(step)
        if integer:
            z = np.rint(z)
        if name == "one_pixel":
            z[...] = ([0.0, 100.0, 7000.0] if integer else [0.0, np.nan, -np.inf])[f % 3]
        elif name == "speck":
            sx, sy = SPECKS[f % 3]
            keep = z[sy, sx]
            z[...] = 0
            z[sy, sx] = keep
        elif name != "identity":
            _salt(rng, z, integer)
        if name == "band":
            z[:, BAND[0]:BAND[1]] = 0
        elif name == "twins":
            z[:, TWINS_BAND[0]:TWINS_BAND[1]] = 0
        elif name == "island":
            z[ISLAND] = 0
        elif name == "border":
            z[:2] = 0
            z[-3:] = 0
            z[:, :3] = 0
            z[:, -2:] = 0
        elif name == "blocks":
            z[10:20, 30:45] = 0
            z[35:50, 60:64] = 0
            z[0:6, 90:] = 0
            z[14:18, 0:3] = 0
        out[f] = z
    return out


def bgr_frames(name, n=3):
    """n guides [n, h, w, 3] uint8: two flat regions that meet at the case's colour edge, +-6 of noise per channel, so that k
    spreads over 0 .. 36 within a region and sits near 300 across; `twins`: one region"""
    w, h = CASES[name].size
    rng = np.random.default_rng(2000 + sum(map(ord, name)))
    img = np.empty((n, h, w, 3), np.int64)
    edge = EDGE.get(name, (w + 1) // 2 + 1)
    img[...] = (60, 90, 120)
    if edge is not None:
        img[:, :, edge:] = (180, 170, 200)
    img += rng.integers(-6, 7, img.shape)
    return np.clip(img, 0, 255).astype(np.uint8)


def stepped_guide(shape, seed=5):
    """a noisy guide whose colours differ by k = 0 or k >= 15: one grey level per pixel out of four, 5 apart in every channel.
    With sigma_color 1, range[15] is 0, so only taps of the pixel's exact colour weigh anything."""
    rng = np.random.default_rng(seed)
    level = rng.integers(0, 4, shape)
    return (100 + 5 * level)[..., None].repeat(3, -1).astype(np.uint8)
