"""DepthDecimation (kde_decimate_*): the rule in numpy, twice, and the named cases of the tests.

Every operation below is one IEEE binary32 operation in the order written (numpy float32 arithmetic rounds each result to
binary32 and never fuses a multiply with an add); the division is the correctly rounded `/`.

  frames   depth src_w x src_h, float32 or uint16 widened by (float)u; k = factor in 2..8; the output is ceil(src_w / k) by
           ceil(src_h / k).  Output pixel (i, j) stands for the source pixels qy = j*k .. min(j*k + k, src_h) - 1 (outer loop),
           qx = i*k .. min(i*k + k, src_w) - 1 (inner loop): the tap order.  A partial block uses the samples that exist.
  pixel    a sample is valid iff z > z_min and z < z_max (NaN and +-inf fail); m = the valid samples of the block
           m < min_valid: the pixel is 0
           zmed = the lower median of the valid samples: sorted ascending, v[(m - 1) / 2]
           MEDIAN: the pixel is zmed
           MEAN:   num = 0, cnt = 0; per valid sample in tap order with max_gap == 0 or |z - zmed| <= max_gap: num = num + z,
                   cnt = cnt + 1; the pixel is num / (float)cnt
           filled = the non-hole pixels (before any rounding to uint16)
           mixed  = the pixels with m >= 1 whose largest valid sample minus smallest exceeds max_gap; none when max_gap == 0
  guide    per channel s = the integer sum over the block's existing pixels, c their count: (2 s + c) / (2 c), integer division
  camera   fx / k, fy / k, (cx + 0.5) / k - 0.5, (cy + 0.5) / k - 0.5 in doubles

decimate() states it vectorised over the pixels of a frame, decimate_scalar() as a plain loop that follows the header line by
line; tests/test_decimate_cases.py holds them against each other, the GPU tests hold the library against decimate().
"""
from collections import namedtuple

import numpy as np

F = np.float32
FLT_MAX = np.finfo(np.float32).max
MEDIAN, MEAN = 0, 1
Z_RANGE = (F(400), F(4000))        # not the default range: both range tests bite
MAX_GAP = F(50)                    # against surfaces at 1000 and 2000
NEAR, FAR = 1000.0, 2000.0
FRAMES = 3

Case = namedtuple("Case", "name size factors f32 u16 bgr why")


def out_size(size, k):
    w, h = size
    return -(-w // k), -(-h // k)


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


def _blocks(a, k, fill):
    """a [h, w, ...] -> [oh, ow, k * k, ...] in tap order, `fill` where the source has no pixel"""
    h, w = a.shape[:2]
    ow, oh = out_size((w, h), k)
    p = np.full((oh * k, ow * k) + a.shape[2:], fill, a.dtype)
    p[:h, :w] = a
    p = p.reshape((oh, k, ow, k) + a.shape[2:])
    p = np.moveaxis(p, 1, 2)                                   # [oh, ow, k (qy), k (qx), ...]
    return p.reshape((oh, ow, k * k) + a.shape[2:])


def decimate(depth, k, mode=MEDIAN, min_valid=1, max_gap=F(0), z_min=F(0), z_max=FLT_MAX):
    """one frame [h, w] float32 / uint16 -> dict(z float32 [oh, ow], m, zmed, filled bool, mixed bool), vectorised"""
    z_min, z_max, max_gap = F(z_min), F(z_max), F(max_gap)
    z = _blocks(widen(depth), k, F(0))
    exists = _blocks(np.ones(np.shape(depth), bool), k, False)
    with np.errstate(invalid="ignore"):
        valid = exists & (z > z_min) & (z < z_max)
    m = valid.sum(-1)
    keyed = np.where(valid, z, F(np.inf))
    srt = np.sort(keyed, axis=-1)
    zmed = np.take_along_axis(srt, np.maximum((m - 1) // 2, 0)[..., None], -1)[..., 0]
    zmed = np.where(m >= 1, zmed, F(0)).astype(np.float32)
    filled = m >= min_valid
    vmin = srt[..., 0]
    vmax = np.where(valid, z, F(-np.inf)).max(-1)
    with np.errstate(invalid="ignore"):
        mixed = (m >= 1) & ((vmax - vmin) > max_gap) if max_gap > 0 else np.zeros(m.shape, bool)
    if mode == MEDIAN:
        res = zmed
    else:
        num = np.zeros(m.shape, np.float32)
        cnt = np.zeros(m.shape, np.int64)
        for t in range(k * k):                                  # the tap order
            zt = z[..., t]
            with np.errstate(invalid="ignore"):
                ok = valid[..., t] & ((np.abs(zt - zmed) <= max_gap) if max_gap > 0 else True)
            num = num + np.where(ok, zt, F(0))                  # + 0 leaves a sum of positive depths as it is
            cnt += ok
        assert num.dtype == np.float32
        with np.errstate(all="ignore"):
            res = num / cnt.astype(np.float32)
    out = np.where(filled, res, F(0)).astype(np.float32)
    return dict(z=out, m=m, zmed=zmed, filled=filled, mixed=mixed)


def decimate_scalar(depth, k, mode=MEDIAN, min_valid=1, max_gap=F(0), z_min=F(0), z_max=FLT_MAX):
    """the same, pixel by pixel and line by line as include/kde_hip.h states it"""
    z_min, z_max, max_gap = F(z_min), F(z_max), F(max_gap)
    src = widen(depth)
    src_h, src_w = src.shape
    out_w, out_h = out_size((src_w, src_h), k)
    out = np.zeros((out_h, out_w), np.float32)
    ms = np.zeros((out_h, out_w), np.int64)
    zmeds = np.zeros((out_h, out_w), np.float32)
    filled = np.zeros((out_h, out_w), bool)
    mixed = np.zeros((out_h, out_w), bool)
    for j in range(out_h):
        for i in range(out_w):
            taps = [src[qy, qx] for qy in range(j * k, min(j * k + k, src_h)) for qx in range(i * k, min(i * k + k, src_w))]
            valid = [z for z in taps if z > z_min and z < z_max]                       # 1: a NaN fails both comparisons
            m = len(valid)                                                              # 2
            ms[j, i] = m
            if m >= 1 and max_gap > 0 and F(max(valid) - min(valid)) > max_gap:         # 9
                mixed[j, i] = True
            if m < min_valid:                                                           # 3
                continue
            zmed = sorted(valid)[(m - 1) // 2]                                          # 4
            zmeds[j, i] = zmed
            filled[j, i] = True                                                         # 8
            if mode == MEDIAN:                                                          # 5
                out[j, i] = zmed
                continue
            num, cnt = F(0), 0                                                          # 6
            for z in valid:
                if max_gap == 0 or np.abs(F(z - zmed)) <= max_gap:
                    num = F(num + z)
                    cnt += 1
            out[j, i] = F(num / F(cnt))
    return dict(z=out, m=ms, zmed=zmeds, filled=filled, mixed=mixed)


def decimate_batch(frames, k, **kw):
    """frames [n, h, w] -> (float32 [n, oh, ow], filled uint32 [n], mixed uint32 [n])"""
    parts = [decimate(f, k, **kw) for f in frames]
    return (np.stack([p["z"] for p in parts]), np.array([p["filled"].sum() for p in parts], np.uint32),
            np.array([p["mixed"].sum() for p in parts], np.uint32))


def decimate_color(bgr, k):
    """one guide [h, w, 3] uint8 -> uint8 [oh, ow, 3]: the block's mean per channel, rounded half up, in integers"""
    assert bgr.dtype == np.uint8 and bgr.ndim == 3 and bgr.shape[2] == 3
    s = _blocks(bgr.astype(np.int64), k, 0).sum(2)
    c = _blocks(np.ones(bgr.shape[:2], np.int64), k, 0).sum(2)[..., None]
    return ((2 * s + c) // (2 * c)).astype(np.uint8)


def decimate_color_scalar(bgr, k):
    src_h, src_w = bgr.shape[:2]
    out_w, out_h = out_size((src_w, src_h), k)
    out = np.zeros((out_h, out_w, 3), np.uint8)
    for j in range(out_h):
        for i in range(out_w):
            for ch in range(3):
                px = [int(bgr[qy, qx, ch]) for qy in range(j * k, min(j * k + k, src_h)) for qx in range(i * k, min(i * k + k, src_w))]
                s, c = sum(px), len(px)
                out[j, i, ch] = (2 * s + c) // (2 * c)
    return out


def intrinsics(K, k):
    """the camera matrix of the small image, float64 [3, 3]"""
    K = np.asarray(K, np.float64).reshape(3, 3)
    r = K.copy()
    r[0, 0], r[0, 1], r[0, 2] = K[0, 0] / k, K[0, 1] / k, (K[0, 2] + 0.5) / k - 0.5
    r[1, 0], r[1, 1], r[1, 2] = K[1, 0] / k, K[1, 1] / k, (K[1, 2] + 0.5) / k - 0.5
    return r


# ---- the cases -------------------------------------------------------------------------------------------------------------
# what an invalid sample looks like, per source format
BAD_F32 = (F(0), F(np.nan), F(np.inf), F(-np.inf), F(-5), Z_RANGE[0], Z_RANGE[1], F(5000))
BAD_U16 = (0, 300, int(Z_RANGE[0]), int(Z_RANGE[1]), 60000)


def _surface(rng, w, h):
    """[FRAMES, h, w] float64: a slanted near surface, a far one right of a slanted line, a few millimetres of noise"""
    x, y = np.meshgrid(np.arange(w, dtype=np.float64), np.arange(h, dtype=np.float64))
    frames = []
    for f in range(FRAMES):
        far = x * 2 + y > (w + h / 2) * (0.9 + 0.2 * f)
        z = np.where(far, FAR, NEAR) + 0.37 * x + 0.21 * y + rng.uniform(-3, 3, (h, w))
        frames.append(z)
    return np.stack(frames)


def _with_invalid(rng, z, fraction=0.1):
    """(float32 frames with a tenth of BAD_F32, uint16 integer-valued frames with a tenth of BAD_U16), the same pixels"""
    f32 = z.astype(np.float32)
    u16 = np.rint(z).astype(np.uint16)
    bad = rng.random(z.shape) < fraction
    f32[bad] = rng.choice(np.array(BAD_F32, np.float32), int(bad.sum()))
    u16[bad] = rng.choice(np.array(BAD_U16, np.uint16), int(bad.sum()))
    return f32, u16


def _guide(rng, w, h):
    g = rng.integers(0, 256, (FRAMES, h, w, 3), dtype=np.uint8)
    g[:, : h // 2, : w // 2] |= 0xF0                               # a bright quarter: sums that round up and saturate
    g[0, h // 2:, : max(w // 3, 1)] = 255
    return g


def _plain(name, size, factors, why, seed):
    rng = np.random.default_rng(seed)
    w, h = size
    f32, u16 = _with_invalid(rng, _surface(rng, w, h))
    return Case(name, size, factors, f32, u16, _guide(rng, w, h), why)


def _holes(seed=7):
    """64 x 64: the 4 x 4 block b (raster order) has b % 17 invalid samples at places of its own, so m takes every value
    0 .. 16 at k = 4 and every value 0 .. 4 at k = 2; depths are a few quantised levels, so duplicates and ties abound"""
    rng = np.random.default_rng(seed)
    w = h = 64
    z = NEAR + 8.0 * rng.integers(0, 4, (FRAMES, h, w))
    f32, u16 = z.astype(np.float32), z.astype(np.uint16)
    for f in range(FRAMES):
        for b in range(256):
            by, bx = divmod(b, 16)
            for s in rng.permutation(16)[: (b + f) % 17]:
                y, x = by * 4 + s // 4, bx * 4 + s % 4
                f32[f, y, x] = BAD_F32[(b + s) % len(BAD_F32)]
                u16[f, y, x] = BAD_U16[(b + s) % len(BAD_U16)]
    return Case("holes", (w, h), (2, 4), f32, u16, _guide(rng, w, h),
                "m takes every value 0..k^2; min_valid 1, 2, k^2; even m and duplicate values")


def _edge(seed=8):
    """64 x 32: a diagonal step NEAR / FAR that cuts blocks at every offset, +-3 of noise, no invalid sample"""
    rng = np.random.default_rng(seed)
    w, h = 64, 32
    x, y = np.meshgrid(np.arange(w), np.arange(h))
    z = np.stack([np.where(x > y + 16 - 5 * f, FAR, NEAR) + rng.uniform(-3, 3, (h, w)) for f in range(FRAMES)])
    return Case("edge", (w, h), (2, 3, 4), z.astype(np.float32), np.rint(z).astype(np.uint16), _guide(rng, w, h),
                "a diagonal step: the median is a sample, the guarded mean never between the surfaces, mixed counts those blocks")


def _build():
    cases = [
        _plain("one_pixel", (1, 1), (2, 8), "a block with one existing sample; a grid of one workgroup", 1),
        _plain("one_block", (8, 8), (2, 3, 4, 5, 6, 7, 8), "k = 8 is one full block; k = 3, 5, 6, 7 give partial blocks of every width", 2),
        _plain("exact", (96, 48), (2, 3, 4, 6, 8), "no partial block; several tiles each way; rows on vector-load boundaries", 3),
        _plain("ragged", (101, 37), (2, 3, 4, 5, 6, 7, 8), "odd width: frames 1 and 2 and every row misaligned; partial blocks on both edges", 4),
        _plain("wide", (515, 9), (2, 3, 7), "many workgroups across, one down", 5),
        _plain("tall", (9, 260), (2, 3, 7), "the transpose", 6),
        _holes(),
        _edge(),
    ]
    # a valid sample in the one-pixel frames, so that their one block is not always a hole
    cases[0].f32[0, 0, 0], cases[0].u16[0, 0, 0] = F(1234.5), 1234
    cases[0].f32[1, 0, 0], cases[0].u16[1, 0, 0] = F(np.nan), 0
    return {c.name: c for c in cases}


CASES = _build()
CASE_FACTORS = [(name, k) for name, c in CASES.items() for k in c.factors]
GUARDS = (F(0), MAX_GAP)
