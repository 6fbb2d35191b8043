"""DepthTemporalFilter (kde_temporal_*): the rule in numpy, sequential over the frames and vectorised over the pixels, and the
crafted sequences of the tests.

Every operation below is one IEEE binary32 operation in the order written (numpy float32 arithmetic rounds each result to
binary32 and never fuses a multiply with an add).  State per pixel: value (float32, 0 = none) and hist (uint32: bits 0-7 the raw
validity of the last eight frames, bit 0 the newest; bits 8-31 the guide colour b | g << 8 | r << 16 of the previous frame).
For every frame, in time order:

  sample     z = (d > z_min && d < z_max) ? (float)d : 0 (NaN and +-inf become 0, uint16 is widened)
  scene      with a guide and color_thresh < 765: where |b - b'| + |g - g'| + |r - r'| > color_thresh against the stored
             colour, value = 0 and hist &= ~0xFF (changed counts the pixels whose value was > 0)
  valid      z > 0: prev = value; linked iff prev > 0 and |z - prev| <= max_diff + rel_diff * min(z, prev); out = prev +
             alpha * (z - prev) where linked (smoothed), else z (jumped where prev > 0); hist[7:0] = (hist[7:0] << 1 | 1) & 0xFF
  hole       z == 0: out = prev where prev > 0, persist_min >= 1 and popcount(hist[7:0]) >= persist_min (held), else 0;
             hist[7:0] = (hist[7:0] << 1) & 0xFF
  store      value = out (the float); the colour bits become this frame's colour (unchanged without a guide); the output is out,
             or depth_to_u16(out)
"""
from collections import namedtuple

import numpy as np

F = np.float32
U = np.uint32
FLT_MAX = np.finfo(np.float32).max
DEFAULTS = dict(alpha=0.4, max_diff=10.0, rel_diff=0.02, persist_min=3, color_thresh=48, z_min=0.0, z_max=float(FLT_MAX))
COUNTS = ("smoothed", "jumped", "held", "changed")
POP8 = np.array([bin(i).count("1") for i in range(256)], np.int64)


def depth_to_u16(z):
    """kde::depth_to_u16: rounded half to even; 0 for what the format does not hold"""
    with np.errstate(all="ignore"):
        r = np.rint(np.asarray(z, np.float32))
        ok = (r >= 1) & (r <= 65535)
    return np.where(ok, r, 0).astype(np.uint16)


def sanitise(depth, z_min, z_max):
    d = np.asarray(depth)
    assert d.dtype in (np.float32, np.uint16)
    d = d.astype(np.float32)
    with np.errstate(invalid="ignore"):
        return np.where((d > F(z_min)) & (d < F(z_max)), d, F(0)).astype(np.float32)


def pack_bgr(c):
    c = np.asarray(c)
    assert c.dtype == np.uint8 and c.shape[-1] == 3
    return c[..., 0].astype(U) | (c[..., 1].astype(U) << U(8)) | (c[..., 2].astype(U) << U(16))


def empty_state(h, w):
    return np.zeros((h, w), np.float32), np.zeros((h, w), np.uint32)


def step(value, hist, d, c, alpha, max_diff, rel_diff, persist_min, color_thresh, z_min, z_max):
    """one frame d [h, w] (float32 / uint16) with its guide c [h, w, 3] uint8 or None on the state (value, hist):
    (out float32, value, hist, (smoothed, jumped, held, changed))"""
    assert value.dtype == np.float32 and hist.dtype == np.uint32
    z = sanitise(d, z_min, z_max)
    changed = 0
    col = None
    if c is not None:
        col = pack_bgr(c)
        if color_thresh < 765:
            s = hist >> U(8)
            sad = sum(np.abs(((col >> U(k)) & U(255)).astype(np.int64) - ((s >> U(k)) & U(255)).astype(np.int64)) for k in (0, 8, 16))
            fire = sad > int(color_thresh)
            changed = int((fire & (value > 0)).sum())
            value = np.where(fire, F(0), value)
            hist = np.where(fire, hist & ~U(0xFF), hist)
    prev = value
    low = hist & U(0xFF)
    valid, has = z > 0, prev > 0
    with np.errstate(all="ignore"):
        m = F(rel_diff) * np.minimum(z, prev)
        t = F(max_diff) + m
        diff = z - prev
        link = valid & has & (np.abs(diff) <= t)
        scaled = F(alpha) * diff
        blend = prev + scaled
    assert m.dtype == t.dtype == diff.dtype == scaled.dtype == blend.dtype == np.float32
    hold = ~valid & has & (int(persist_min) >= 1) & (POP8[low] >= int(persist_min))
    out = np.where(valid, np.where(link, blend, z), np.where(hold, prev, F(0))).astype(np.float32)
    colour = (col << U(8)) if col is not None else (hist & ~U(0xFF))
    hist = (colour | (((low << U(1)) | valid.astype(U)) & U(0xFF))).astype(np.uint32)
    counts = (int(link.sum()), int((valid & has & ~link).sum()), int(hold.sum()), changed)
    return out, out.copy(), hist, counts


Result = namedtuple("Result", "out value hist smoothed jumped held changed")


def filter_sequence(depth, bgr=None, out_dtype=np.float32, state=None, **kw):
    """frames [n, h, w] (and guide [n, h, w, 3] or None) from `state` (value, hist; None: empty):
    Result(out [n, h, w] of out_dtype, value, hist, smoothed, jumped, held, changed -- uint32 [n] each)"""
    p = dict(DEFAULTS, **kw)
    n, h, w = depth.shape
    value, hist = empty_state(h, w) if state is None else (state[0].copy(), state[1].copy())
    outs, counts = [], []
    for t in range(n):
        out, value, hist, cnt = step(value, hist, depth[t], None if bgr is None else bgr[t], **p)
        outs.append(out if out_dtype == np.float32 else depth_to_u16(out))
        counts.append(cnt)
    counts = np.array(counts, np.uint32).reshape(n, 4)
    return Result(np.stack(outs), value, hist, *(counts[:, k].copy() for k in range(4)))


def scalar_pixel(d_seq, c_seq, alpha, max_diff, rel_diff, persist_min, color_thresh, z_min, z_max, value=F(0), hist=0):
    """the rule for ONE pixel as a plain Python loop over numpy float32 scalars: d_seq the samples, c_seq the (b, g, r) per
    frame or None.  Returns (outs, value, hist, [(smoothed, jumped, held, changed) per frame])."""
    value, hist = F(value), int(hist)
    outs, counts = [], []
    for t, d in enumerate(d_seq):
        d = F(d)
        z = d if (d > F(z_min) and d < F(z_max)) else F(0)
        sm = ju = he = ch = 0
        if c_seq is not None:
            b, g, r = (int(x) for x in c_seq[t])
            if color_thresh < 765:
                s = hist >> 8
                if abs(b - (s & 255)) + abs(g - ((s >> 8) & 255)) + abs(r - (s >> 16)) > color_thresh:
                    ch = int(value > 0)
                    value = F(0)
                    hist &= ~0xFF
        prev, low = value, hist & 0xFF
        if z > 0:
            if prev > 0 and abs(F(z - prev)) <= F(F(max_diff) + F(F(rel_diff) * min(z, prev))):
                out = F(prev + F(F(alpha) * F(z - prev)))
                sm = 1
            else:
                out = z
                ju = int(prev > 0)
            low = (low << 1 | 1) & 0xFF
        else:
            if prev > 0 and persist_min >= 1 and bin(low).count("1") >= persist_min:
                out = prev
                he = 1
            else:
                out = F(0)
            low = (low << 1) & 0xFF
        value = out
        colour = (b | g << 8 | r << 16) << 8 if c_seq is not None else hist & ~0xFF
        hist = colour | low
        outs.append(out)
        counts.append((sm, ju, he, ch))
    return outs, value, hist, counts


# ---- the cases -------------------------------------------------------------------------------------------------------
# A case is a sequence with a guide and the parameters it is run with.  Every case runs with and without its guide, as float32
# and as uint16 (`as_u16`: what a sensor could deliver of it -- whole millimetres, 0 for what uint16 does not hold).
Case = namedtuple("Case", "size n why params make")
SIZES = dict(odd=(37, 19), tiny=(3, 1), even=(64, 8))       # odd: every frame starts at another alignment; tiny: one partial group


def _rng(name):
    return np.random.default_rng(sum(ord(ch) * (i + 1) for i, ch in enumerate(name)))


def _guide(name, n, h, w, static=True):
    """a guide that never fires at a threshold >= 8: one random colour per pixel and +-2 levels of noise per frame"""
    r = _rng(name + "guide")
    base = r.integers(20, 230, (1, h, w, 3))
    noise = r.integers(-2, 3, (n, h, w, 3))
    return (base + noise).astype(np.uint8)


def _plane(h, w):
    y, x = np.mgrid[0:h, 0:w]
    return (1500.0 + 7.0 * x + 3.0 * y).astype(np.float32)


def _noise(name, n, size):
    w, h = size
    r = _rng(name)
    d = _plane(h, w)[None] + r.uniform(-6.0, 6.0, (n, h, w)).astype(np.float32)
    # The first rows lie at 7 .. 17 mm.  Samples and running value share one binade on the far plane, where alpha = 0.4 times a
    # difference never comes near half a unit of the result; here they span three, and a fused blend rounds differently.
    near = min(4, h // 2)
    d[:, :near] = F(12.0) + r.uniform(-5.0, 5.0, (n, near, w)).astype(np.float32)
    d[r.random((n, h, w)) < 0.1] = 0.0
    return d.astype(np.float32), _guide(name, n, h, w)


def _threshold(name, n, size):
    w, h = size
    d = np.zeros((n, h, w), np.float32)
    d[0] = 1024.0
    d[1, 0, :] = (1288.0, 1289.0, 1287.5)                   # 264 = 8 + 0.25 * 1024 exactly: linked; 265: not; 263.5: linked
    d[2:] = d[1]
    d[3, 0, :] = (1024.0, 1024.0, 0.0)
    return d, _guide(name, n, h, w)


def _step(name, n, size):
    w, h = size
    d, g = _noise(name, n, size)
    d[n // 2:, :, :w // 2] += 700.0                         # the left half moves back by 0.7 m and stays there
    d[d == 700.0] = 0.0
    return d, g


def _spike(name, n, size):
    w, h = size
    d, g = _noise(name, n, size)
    d[3, ::2, 1::3] = 400.0                                 # one frame of outlier, then back
    return d, g


def _dropout(name, n, size):
    """pixel k < 80: a = k % 8 + 1 valid frames, then b = k // 8 + 1 invalid ones, then valid again"""
    w, h = size
    d = np.zeros((n, h * w), np.float32)
    t = np.arange(n)[:, None]
    k = np.arange(h * w)[None, :] % 80
    a, b = k % 8 + 1, k // 8 + 1
    d[:] = np.where((t < a) | (t >= a + b), 2000.0 + (np.arange(h * w)[None, :] % 7) + 0.25 * t, 0.0)
    return d.reshape(n, h, w), _guide(name, n, h, w)


def _colour(name, n, size):
    """rows 0 .. h/2 - 1 a steady surface, the rows below a hole in frames 3 .. 5; at frame 4 the guide of column x changes
    by x % 4: nothing, 15 per channel (45 <= 48), 17 per channel (51 > 48), to white from black (765)"""
    w, h = size
    d = np.full((n, h, w), 1800.0, np.float32) + np.arange(n, dtype=np.float32)[:, None, None]
    d[3:6, h // 2:, :] = 0.0
    g = np.empty((n, h, w, 3), np.uint8)
    x = np.arange(w)
    before = np.where(x % 4 == 3, 0, 100)
    after = before + np.choose(x % 4, [0, 15, 17, 255])
    g[:4] = before[None, None, :, None]
    g[4:] = after[None, None, :, None]
    flicker = (x >= w // 2) & (x % 4 == 0)
    g[:, :, flicker, 0] += (np.arange(n) % 2).astype(np.uint8)[:, None, None]     # one level in b: fires at threshold 0 only
    return d, g


def _invalid(name, n, size):
    w, h = size
    d, g = _noise(name, n, size)
    r = _rng(name + "bad")
    bad = np.array([np.nan, np.inf, -np.inf, -1500.0, -0.0, 100.0, 500.0, 4000.0, 5000.0, FLT_MAX], np.float32)
    pick = r.random((n, h, w)) < 0.3
    d[pick] = bad[r.integers(0, len(bad), int(pick.sum()))]
    d[2] = np.nan                                           # all-invalid frames
    d[5] = 0.0
    return d, g


def _u16_edges(name, n, size):
    w, h = size
    d = np.zeros((n, h, w), np.float32)
    d[:, 0, 0] = (65535.0, 65535.0, 0.0, 65535.0, 1.0, 0.0, 65534.0)[:n]
    d[:, 0, 1] = (0.0, 1.0, 1.0, 0.0, 0.0, 0.0, 2.0)[:n]
    d[:, 0, 2] = (65000.0, 65535.0, 65535.0, 0.0, 65535.0, 64000.0, 65535.0)[:n]
    return d, _guide(name, n, h, w)


CASES = {
    "noise": Case(SIZES["odd"], 17, "the rounding of the three-step blend; a contracted fma differs on some samples", dict(), _noise),
    "threshold": Case(SIZES["tiny"], 7, "the link bound met exactly and missed by one", dict(alpha=0.5, max_diff=8.0, rel_diff=0.25), _threshold),
    "step": Case(SIZES["even"], 9, "a surface change: jumped, and no blend across it", dict(), _step),
    "spike": Case(SIZES["even"], 7, "one frame of outlier, then back", dict(), _spike),
    "colour_t0": Case(SIZES["even"], 9, "the guide changes inside a hole and a steady surface", dict(color_thresh=0), _colour),
    "colour_t48": Case(SIZES["even"], 9, "the same at the default threshold", dict(color_thresh=48), _colour),
    "colour_t764": Case(SIZES["even"], 9, "only black to white fires", dict(color_thresh=764), _colour),
    "colour_t765": Case(SIZES["even"], 9, "the guide is never consulted", dict(color_thresh=765), _colour),
    "invalid": Case(SIZES["odd"], 7, "NaN, +-inf, negatives, outside z_min .. z_max, all-invalid frames", dict(z_min=500.0, z_max=4000.0), _invalid),
    "alpha1": Case(SIZES["odd"], 9, "pass-through plus hold", dict(alpha=1.0), _noise),
    "u16_edges": Case(SIZES["tiny"], 7, "0 and 65535", dict(), _u16_edges),
    "single": Case(SIZES["odd"], 1, "a sequence of one frame", dict(), _noise),
}
for _p in (0, 1, 3, 8):
    CASES[f"dropout_p{_p}"] = Case(SIZES["odd"], 17, "hold, its expiry at eight, the popcount before the shift", dict(persist_min=_p), _dropout)
IDS = sorted(CASES)

_made = {}


def frames(name):
    """(depth float32 [n, h, w], guide uint8 [n, h, w, 3]) of a case: made once, never written to"""
    if name not in _made:
        c = CASES[name]
        d, g = c.make(name, c.n, c.size)
        assert d.shape == (c.n, c.size[1], c.size[0]) and g.shape == d.shape + (3,) and d.dtype == np.float32 and g.dtype == np.uint8
        d.setflags(write=False)
        g.setflags(write=False)
        _made[name] = (d, g)
    return _made[name]


def as_u16(depth):
    """what a sensor's uint16 holds of float frames: whole millimetres, 0 for NaN, +-inf, negatives and what lies above 65535"""
    with np.errstate(invalid="ignore"):
        ok = np.isfinite(depth) & (depth >= 0) & (depth <= 65535)
        return np.where(ok, np.rint(np.where(ok, depth, 0)), 0).astype(np.uint16)


def params(name, **kw):
    return dict(DEFAULTS, **{**CASES[name].params, **kw})
