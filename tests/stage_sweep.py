"""A seeded draw of cases for the seven depth-in / depth-out stages (kde_reg_*, kde_undist_*, kde_upsample_*, kde_holefill_*,
kde_speckle_*, kde_temporal_*, kde_decimate_*), and the comparison of the library with the numpy statements of their rules.

    case(kind, seed, index)   one self-contained case: sizes, formats, placement, constructor arguments, inputs, call plan, want
    run_case(torch, F_, c)    builds the object, runs the plan on the device and returns the violations (strings); none: equal

A case is drawn from np.random.default_rng([seed, kind number, index]) alone, so any case can be made again without the ones
before it.  Every parameter is drawn from the whole domain kde_*_create admits (the KDE_REQUIREs of csrc/kde_api_*.cpp and the
constants of csrc/kde_internal.h), so a refusal is a violation.  `want` comes from the statements of the *_cases.py files;
no rule is restated here.  The bar is byte equality and equal counts.

What every kind draws: width 1 .. 200 and height 1 .. 150 with weight on 1, on multiples of the tile and on those +- 1; n in
1 .. 4 frames in an object for n or n + 1; float32 or uint16 in and, independently, out; input and output 0 or 1 element past a
16-byte boundary; a caller-owned output inside sentinel bytes, or the object's own; a share of 0 .. 0.6 of invalid samples
(denser towards one side of the frame, so that blocks and windows with few, some and all samples valid occur) out of 0, -0, NaN,
+-inf, negatives, z_min and z_max with their float neighbours, 65535 and 65535.5; index 0 holds a frame without an invalid
sample and index 1 a frame of nothing else; planes with a step around the stage's threshold, exactly on it where the plane is
flat; a guide that is flat, noisy or has a colour edge.  test_stage_sweep.py holds the conditions on the draw.

This module needs no GPU: torch and the filters module are handed to run_case().
"""
from types import SimpleNamespace

import numpy as np

import decimate_cases as DC
import holefill_cases as HC
import reg_cases as RC
import speckle_cases as SC
import temporal_cases as TC
import undist_cases as UD
import upsample_cases as UC

F = np.float32
FLT_MAX = np.finfo(np.float32).max
SENTINEL = 0xA5
KINDS = ("reg", "undist", "upsample", "holefill", "speckle", "temporal", "decimate")
PAIRS = ((np.float32, np.float32), (np.float32, np.uint16), (np.uint16, np.float32), (np.uint16, np.uint16))
MAX_W, MAX_H = 200, 150

# the bounds of the library (csrc/kde_internal.h, csrc/kde_api_decimate.cpp:20); test_stage_sweep.py checks that create admits them
REG_MAX_SPLAT = 16
UPSAMPLE_MAX_RADIUS = 4
HOLEFILL_MAX_RADIUS, HOLEFILL_MAX_FUSE = 3, 4
DECIMATE_FACTORS = tuple(range(2, 9))
SPECKLE_MAX_SIZE = 1 << 24

# the budget of tests/test_gpu_stage_sweep.py; tests/test_stage_sweep.py holds the conditions on the draw over exactly this
SEEDS = (1, 2)
CASES_PER_KIND = 40


def kinds():
    return KINDS


def tile_of(kind, params=None):
    """(width, height) in output pixels of the tile a workgroup takes; the stages that walk a frame as a line count as 32 x 8"""
    if kind in ("holefill", "speckle"):
        return 32, 16
    if kind == "decimate" and params is not None and params["factor"] >= 5:
        return 32, 4
    return 32, 8


# ---- the draws every kind shares --------------------------------------------------------------------------------------
def _side(rng, tile, hi):
    """1 .. hi: 1, a multiple of the tile, a multiple +- 1, or anything"""
    u = rng.random()
    if u < 0.02:
        return 1
    if u < 0.40:
        return int(np.clip(tile * rng.integers(1, max(hi // tile, 1) + 1) + rng.integers(-1, 2), 1, hi))
    return int(rng.integers(1, hi + 1))


def _size(rng, kind):
    tw, th = tile_of(kind)
    if rng.random() < 0.08:                                   # a frame of one tile
        return _side(rng, tw, tw), _side(rng, th, th)
    return _side(rng, tw, MAX_W), _side(rng, th, MAX_H)


def _z_range(rng):
    return F(rng.choice([0.0, 400.0, 500.0])), F(rng.choice([float(FLT_MAX), 4000.0, 6000.0]))


def _specials(z_min, z_max, integer):
    """what an invalid sample, or one on the border of being one, looks like"""
    if integer:
        v = [0, 0, 65535, 1, 65534] + [int(b) + d for b in (z_min, z_max) if b <= 65535 for d in (-1, 0, 1)]
        return np.array([x for x in v if 0 <= x <= 65535], np.uint16)
    with np.errstate(over="ignore"):
        near = [np.nextafter(F(b), F(s)) for b in (z_min, z_max) for s in (-np.inf, np.inf)]
    return np.array([0.0, 0.0, -0.0, np.nan, np.inf, -np.inf, -5.0, -1e30, z_min, z_max, 65535.0, 65535.5] + near, np.float32)


def _line(rng, w, h):
    """a boolean [h, w]: one side of a random line through the frame, and the unit ramp 0 .. 1 across it"""
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    a = rng.uniform(0, 2 * np.pi)
    t = (x - (w - 1) / 2) * np.cos(a) + (y - (h - 1) / 2) * np.sin(a)
    span = max(np.abs(t).max(), 1.0)
    return t > rng.uniform(-0.5, 0.5) * span, (t / span + 1) / 2


def _step_height(rng, thr):
    """a step around the threshold thr: below, on, one float above, above, far above; thr == 0: a step of some size"""
    if thr <= 0:
        return float(rng.choice([0.0, 1.0, 40.0, 700.0]))
    thr = F(thr)
    return float(rng.choice([thr * F(0.5), np.nextafter(thr, F(0)), thr, np.nextafter(thr, F(np.inf)), thr * F(1.5), thr * F(4), thr * F(20)]))


def _planes(rng, n, w, h, thr):
    """[n, h, w] float64: per frame a plane -- flat in a third of the draws, without noise in a third -- with a step around thr
    along a line that moves from frame to frame, and mostly a box in front of it"""
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    flat, quiet = rng.random() < 0.33, rng.random() < 0.33
    sx, sy = (0.0, 0.0) if flat else rng.uniform(-2.5, 2.5, 2)
    base = float(rng.integers(900, 2400))
    step = _step_height(rng, thr)
    out = np.empty((n, h, w))
    for f in range(n):
        far, _ = _line(rng, w, h)
        out[f] = base + 32 * f + sx * x + sy * y + np.where(far, step, 0.0) + (0 if quiet else rng.uniform(-1.5, 1.5, (h, w)))
        if rng.random() < 0.85:                               # a box well in front of the plane: a step far above any threshold
            x0, y0 = rng.integers(0, w), rng.integers(0, h)
            out[f, y0:y0 + rng.integers(1, h // 2 + 2), x0:x0 + rng.integers(1, w // 2 + 2)] = float(rng.integers(620, 800)) + 2 * f
    return out


def _depth(rng, dt, z, z_min, z_max, share, index, rect=0.5):
    """the frames z [n, h, w] as dt with `share` of their samples replaced by specials, denser towards one side, and (rect: how
    often) a rectangle of nothing else; index 0: frame 0 keeps every sample, index 1: frame 0 is all specials.  Returns
    (frames, the mask of the replaced samples)"""
    n, h, w = z.shape
    integer = dt == np.uint16
    out = TC.as_u16(z.astype(np.float32)) if integer else z.astype(np.float32)
    sp = _specials(z_min, z_max, integer)
    bad = np.zeros(z.shape, bool)
    for f in range(n):
        _, ramp = _line(rng, w, h)
        bad[f] = rng.random((h, w)) < np.clip(share * (ramp - 0.25) / 0.28, 0, 1)    # none in a quarter of the frame; `share` overall
        if rng.random() < rect and share > 0:
            x0, y0 = rng.integers(0, w), rng.integers(0, h)
            bad[f, y0:y0 + rng.integers(1, h // 2 + 2), x0:x0 + rng.integers(1, w // 2 + 2)] = True
    if index == 0:
        bad[0] = False
    elif index == 1:
        bad[0] = True
    out[bad] = sp[rng.integers(0, sp.size, int(bad.sum()))]
    if index == 1:                                            # nothing but what the range test fails
        with np.errstate(invalid="ignore"):
            sp = sp[~((sp.astype(np.float32) > z_min) & (sp.astype(np.float32) < z_max))]
        out[0] = sp[rng.integers(0, sp.size, (h, w))]
    if index == 0:                                            # no invalid sample: inside the range, whatever it is
        out[0] = np.clip(out[0], 600, 3900).astype(out.dtype)
    return out, bad


def _guide(rng, n, w, h, moving=True):
    """[n, h, w, 3] uint8: flat, noisy, or with a colour edge along a line; `moving`: frames differ"""
    img = np.empty((n, h, w, 3), np.int64)
    img[...] = rng.integers(30, 220, 3)
    if rng.random() < 0.6:
        side, _ = _line(rng, w, h)
        img[:, side] = rng.integers(0, 256, 3)
    amp = int(rng.choice([0, 0, 3, 6, 40]))
    if amp:
        noise = rng.integers(-amp, amp + 1, img.shape if moving else (1,) + img.shape[1:])
        img = img + noise
    return np.clip(img, 0, 255).astype(np.uint8)


def _common(rng, kind, seed, index):
    n = int(rng.integers(1, 5))
    dt, ot = PAIRS[rng.integers(0, 4)]
    c = SimpleNamespace(kind=kind, seed=seed, index=index, n=n, max_batch=n + int(rng.integers(0, 2)), dt=dt, ot=ot,
                        in_by=int(rng.integers(0, 2)), out_by=int(rng.integers(0, 2)), owner=("caller", "object")[rng.integers(0, 2)],
                        in_place=False, share=float(rng.uniform(0, 0.6)), params={}, inputs={}, want={})
    c.z_min, c.z_max = _z_range(rng)
    return c


def _u16(a, ot):
    return a if ot == np.float32 else DC.depth_to_u16(a)


# ---- one draw per kind ------------------------------------------------------------------------------------------------
def _draw_reg(rng, c):
    c.size, c.out_size = _size(rng, "reg"), _size(rng, "reg")             # depth camera, colour camera
    (wd, hd), (wc, hc) = c.size, c.out_size
    fd = max(wd, hd) * rng.uniform(0.7, 1.4)
    fc = fd * (0.7 + 0.6 * rng.random() ** 2)                 # within 30 % of each other, more often the smaller of the two
    deg = rng.uniform(-3, 3, 2) * rng.choice([0.0, 1.0])
    t = rng.uniform(-80, 80, 3) * rng.choice([0.0, 1.0, 1.0, 1.0], 3)
    c.params = dict(max_splat=int(rng.integers(0, REG_MAX_SPLAT + 1)), z_min=c.z_min, z_max=c.z_max)
    c.calib = (RC.camera(wd, hd, fd), RC.camera(wc, hc, fc, rng.uniform(-2, 2), rng.uniform(-2, 2)), RC.rotation(*deg), t)
    c.bgr_frames = int(rng.choice([1, c.n]))
    z = _planes(rng, c.n, wd, hd, 400.0)
    c.inputs["depth"], c.bad = _depth(rng, c.dt, z, c.z_min, c.z_max, c.share, c.index)
    c.inputs["bgr"] = _guide(rng, c.bgr_frames, wc, hc)
    c.plan = [("depth",), ("color",)]


def _want_reg(c, tables=None):
    cal, p, d, g = RC.calib(*c.calib), c.params, c.inputs["depth"], c.inputs["bgr"]
    got = [RC.statement(f, cal, c.out_size, p["z_min"], p["z_max"], p["max_splat"], c.ot) for f in d]
    c.want = dict(out=np.stack([a for a, _ in got]), counts=dict(filled=[k for _, k in got]),
                  color=np.stack([RC.color_to_depth(f, g[i % len(g)], cal, p["z_min"], p["z_max"]) for i, f in enumerate(d)]))


def _draw_undist(rng, c):
    c.size, c.out_size = _size(rng, "undist"), _size(rng, "undist")       # source, output
    (sw, sh), (ow, oh) = c.size, c.out_size
    f = max(sw, sh) * rng.uniform(0.6, 1.3)
    K = UD.K3(f, f * rng.uniform(0.97, 1.03), (sw - 1) / 2 + rng.uniform(-2, 2), (sh - 1) / 2 + rng.uniform(-2, 2))
    dist = [rng.uniform(-0.3, 0.3), rng.uniform(-0.1, 0.1), rng.uniform(-0.005, 0.005), rng.uniform(-0.005, 0.005), rng.uniform(-0.05, 0.05)]
    Knew = None
    if rng.random() < 0.75:
        fn = f * rng.uniform(0.4, 1.0) * max(ow, oh) / max(sw, sh)        # mostly a wider view than the source's
        Knew = UD.K3(fn, fn * rng.uniform(0.97, 1.03), (ow - 1) / 2 + rng.uniform(-2, 2), (oh - 1) / 2 + rng.uniform(-2, 2))
    interp = int(rng.integers(0, 2))
    gap = float(rng.choice([5.0, 50.0, 300.0])) if interp or rng.random() < 0.5 else 0.0
    c.params = dict(z_min=c.z_min, z_max=c.z_max, depth_interp=interp, max_gap=gap)
    c.calib = (K, dist, Knew)
    c.bgr_frames = int(rng.choice([1, c.n]))
    z = _planes(rng, c.n, sw, sh, gap)
    c.inputs["depth"], c.bad = _depth(rng, c.dt, z, c.z_min, c.z_max, c.share, c.index)
    c.inputs["bgr"] = _guide(rng, c.bgr_frames, sw, sh)
    c.plan = [("depth",), ("color",)]


def _want_undist(c, tables=None):
    cal, p, d, g = UD.calib(*c.calib), c.params, c.inputs["depth"], c.inputs["bgr"]
    got = [UD.depth(f, cal, c.out_size, p["z_min"], p["z_max"], p["depth_interp"], p["max_gap"], c.ot) for f in d]
    c.want = dict(out=np.stack([a for a, _ in got]), counts=dict(filled=[k for _, k in got]),
                  color=np.stack([UD.color(g[i % len(g)], cal, c.out_size) for i in range(c.n)]))


def _draw_upsample(rng, c):
    ow, oh = c.out_size = _size(rng, "upsample")
    ratio = lambda: float(rng.choice([1.0, 2.0, 3.0, 4.0, 8.0, rng.uniform(1, 8)]))
    c.size = (int(np.clip(round(ow / ratio()), 1, ow)), int(np.clip(round(oh / ratio()), 1, oh)))
    gap = float(rng.choice([0.0, 10.0, 100.0]))
    c.params = dict(radius=int(rng.integers(1, UPSAMPLE_MAX_RADIUS + 1)), sigma_color=float(rng.choice([1.0, 30.0, 200.0])), max_gap=gap,
                    z_min=c.z_min, z_max=c.z_max)
    c.bgr_frames = int(rng.choice([1, c.n]))
    z = _planes(rng, c.n, *c.size, gap if gap else 100.0)
    c.inputs["depth"], c.bad = _depth(rng, c.dt, z, c.z_min, c.z_max, c.share, c.index)
    c.inputs["bgr"] = _guide(rng, c.bgr_frames, ow, oh)
    c.plan = [("depth",)]


def upsample_frame(c, f, tables=None, max_gap=None):
    """upsample_parts of frame f (max_gap: instead of the case's)"""
    p, g = c.params, c.inputs["bgr"]
    t = UC.tables(c.size, c.out_size, p["sigma_color"], None if tables is None else tables["range"])
    return UC.upsample_parts(c.inputs["depth"][f], g[f % len(g)], t, c.out_size, p["radius"], p["max_gap"] if max_gap is None else max_gap,
                             p["z_min"], p["z_max"])


def _want_upsample(c, tables=None):
    parts = [upsample_frame(c, f, tables) for f in range(c.n)]
    c.want = dict(out=np.stack([_u16(q["z"], c.ot) for q in parts]), counts=dict(filled=[int(q["kept"].sum()) for q in parts]))


def _draw_holefill(rng, c):
    c.size = c.out_size = _size(rng, "holefill")
    r = int(rng.integers(1, HOLEFILL_MAX_RADIUS + 1))
    taps = (2 * r + 1) ** 2 - 1
    gap = float(rng.choice([0.0, 10.0, 100.0]))
    c.params = dict(radius=r, iterations=int(rng.integers(1, 13)), min_taps=1 + int(taps * rng.random() ** 3), sigma_space=float(rng.choice([0.7, 2.0, 6.0])),
                    sigma_color=float(rng.choice([1.0, 30.0, 200.0])), max_gap=gap, gap_rule=int(rng.integers(0, 2)), z_min=c.z_min, z_max=c.z_max,
                    passes_per_launch=int(rng.integers(0, HOLEFILL_MAX_FUSE + 1)))
    c.bgr_frames = int(rng.choice([1, c.n]))
    c.with_pass_of = bool(rng.integers(0, 2))
    z = _planes(rng, c.n, *c.size, gap if gap else 100.0)
    c.inputs["depth"], c.bad = _depth(rng, c.dt, z, c.z_min, c.z_max, c.share, c.index)
    c.inputs["bgr"] = _guide(rng, c.bgr_frames, *c.size)
    c.plan = [("depth",)]


def _want_holefill(c, tables=None):
    p, g = c.params, c.inputs["bgr"]
    space = HC.space_table(p["radius"], p["sigma_space"]) if tables is None else tables["space"]
    range_ = HC.range_table(p["sigma_color"]) if tables is None else tables["range"]
    kw = {k: p[k] for k in ("radius", "iterations", "min_taps", "max_gap", "gap_rule", "z_min", "z_max")}
    parts = [HC.fill_parts(f, g[i % len(g)], space, range_, **kw) for i, f in enumerate(c.inputs["depth"])]
    c.want = dict(out=np.stack([_u16(q["z"], c.ot) for q in parts]), pass_of=np.stack([q["pass_of"] for q in parts]),
                  counts=dict(filled=[q["filled"] for q in parts], remaining=[q["remaining"] for q in parts]))


def _draw_speckle(rng, c):
    w, h = c.size = c.out_size = _size(rng, "speckle")
    u = rng.random()
    min_size = 1 if u < 0.03 else int(rng.integers(w * h + 1, min(4 * w * h + 2, SPECKLE_MAX_SIZE) + 1)) if u < 0.06 else \
        int(np.clip(np.exp(rng.uniform(np.log(2), np.log(max(w * h / 10, 3)))), 2, SPECKLE_MAX_SIZE))
    md = float(rng.choice([0.0, 2.0, 10.0]))
    c.params = dict(min_size=min_size, max_diff=md, rel_diff=float(rng.choice([0.0, 0.004, 0.02])), connectivity=int(rng.choice([4, 8])),
                    z_min=c.z_min, z_max=c.z_max)
    c.with_labels = bool(rng.integers(0, 2))
    c.in_place = bool(rng.integers(0, 2)) and c.dt == c.ot
    z = _planes(rng, c.n, w, h, md)
    if md == 0 and c.params["rel_diff"] == 0:                 # only equal depths link: terraces
        z = np.rint(z / 64) * 64
    fly = rng.random(z.shape) < rng.uniform(0.01, 0.1)        # flying pixels and speckles
    z[fly] = rng.uniform(600, 3900, int(fly.sum()))
    c.inputs["depth"], c.bad = _depth(rng, c.dt, z, c.z_min, c.z_max, c.share, c.index)
    c.plan = [("depth",)]


def _want_speckle(c, tables=None):
    out, labels, removed, comps = SC.filter_batch(c.inputs["depth"], c.ot, **c.params)
    c.want = dict(out=out, labels=labels, counts=dict(removed=removed.tolist(), components=comps.tolist(), capped=[0] * c.n))


def _draw_temporal(rng, c):
    w, h = c.size = c.out_size = _size(rng, "temporal")
    T = int(rng.integers(2, 9))
    md = float(rng.choice([0.0, 2.0, 10.0]))
    c.params = dict(alpha=float(rng.choice([1.0, 0.5, F(rng.uniform(0.01, 1.0))])), max_diff=md, rel_diff=float(rng.choice([0.0, 0.004, 0.02])),
                    persist_min=int(rng.integers(0, 9)), color_thresh=int(rng.choice([0, 48, 764, 765, rng.integers(0, 766)])), z_min=c.z_min, z_max=c.z_max)
    c.guide = ("absent", "static", "moving")[rng.integers(0, 3)]
    c.in_place = bool(rng.integers(0, 2)) and c.dt == c.ot
    cuts = []
    while sum(cuts) < T:                                      # the sequence cut into calls of 1 .. 4 frames
        cuts.append(int(min(rng.integers(1, 5), T - sum(cuts))))
    c.n = T
    c.reset_at = int(rng.integers(1, T)) if rng.random() < 1 / 3 else None
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    flat = rng.random() < 0.33
    sx, sy = (0.0, 0.0) if flat else rng.uniform(-2.5, 2.5, 2)
    plane = float(rng.integers(900, 2400)) + sx * x + sy * y
    thr = md + c.params["rel_diff"] * 1500
    z = np.empty((T, h, w))
    moved, _ = _line(rng, w, h)
    for t in range(T):                                        # jitter around the link bound; one side moves away half way through
        jitter = 0.0 if thr == 0 else rng.uniform(-0.7, 0.7, (h, w)) * thr * rng.choice([0.2, 1.0, 2.0])
        z[t] = plane + jitter + np.where(moved & (t >= T // 2), _step_height(rng, thr), 0.0)
    if flat and rng.random() < 0.5:
        z = np.rint(z)
    c.inputs["depth"], c.bad = _depth(rng, c.dt, z, c.z_min, c.z_max, c.share * 0.6, c.index, rect=0.3)
    if c.guide != "absent":
        g = _guide(rng, T, w, h, moving=c.guide == "moving")
        if c.guide == "moving":                               # a colour change of a region at some frame
            side, _ = _line(rng, w, h)
            g[int(rng.integers(1, T)):, side] = rng.integers(0, 256, 3, dtype=np.uint8)
        c.inputs["bgr"] = g
    c.plan, t = [], 0
    for k in cuts:
        if c.reset_at is not None and t < c.reset_at < t + k:             # a reset falls between calls
            c.plan += [("filter", t, c.reset_at), ("reset",), ("filter", c.reset_at, t + k)]
        else:
            c.plan += ([("reset",)] if c.reset_at == t else []) + [("filter", t, t + k)]
        t += k
    c.max_batch = max(s[2] - s[1] for s in c.plan if s[0] == "filter") + int(rng.integers(0, 2))


def _want_temporal(c, tables=None):
    d, g = c.inputs["depth"], c.inputs.get("bgr")
    parts = [(0, c.n)] if c.reset_at is None else [(0, c.reset_at), (c.reset_at, c.n)]
    rs = [TC.filter_sequence(d[a:b], None if g is None else g[a:b], c.ot, **c.params) for a, b in parts]
    c.want = dict(out=np.concatenate([r.out for r in rs]), value=rs[-1].value, hist=rs[-1].hist,
                  counts={k: np.concatenate([getattr(r, k) for r in rs]).tolist() for k in TC.COUNTS})


def _draw_decimate(rng, c):
    k = int(rng.choice(DECIMATE_FACTORS))
    tw, th = tile_of("decimate", dict(factor=k))
    w, h = c.size = (int(np.clip(_side(rng, tw, MAX_W // k + 1) * k + rng.integers(1 - k, 1), 1, MAX_W)),
                     int(np.clip(_side(rng, th, MAX_H // k + 1) * k + rng.integers(1 - k, 1), 1, MAX_H)))
    c.out_size = DC.out_size(c.size, k)
    gap = float(rng.choice([0.0, 10.0, 50.0]))
    c.params = dict(factor=k, mode=int(rng.integers(0, 2)), min_valid=int(rng.choice([1, k * k, 1 + int((k * k - 1) * rng.random() ** 2)], p=[0.25, 0.1, 0.65])), max_gap=gap, z_min=c.z_min, z_max=c.z_max)
    z = _planes(rng, c.n, w, h, gap if gap else 50.0)
    d, c.bad = _depth(rng, c.dt, z, c.z_min, c.z_max, c.share, c.index, rect=0.8)
    if c.index > 1 or c.n > 1:                                # a rectangle without a sample that holds a whole block where the frame has room
        x0, y0 = rng.integers(0, max(w - 2 * k, 0) + 1), rng.integers(0, max(h - 2 * k, 0) + 1)
        d[-1, y0:y0 + 2 * k, x0:x0 + 2 * k] = 0
    c.inputs["depth"] = d
    c.inputs["bgr"] = _guide(rng, c.n, w, h)
    c.plan = [("depth",), ("color",)]


def _want_decimate(c, tables=None):
    p = c.params
    z, filled, mixed = DC.decimate_batch(c.inputs["depth"], p["factor"], mode=p["mode"], min_valid=p["min_valid"], max_gap=p["max_gap"],
                                         z_min=p["z_min"], z_max=p["z_max"])
    c.want = dict(out=_u16(z, c.ot), counts=dict(filled=filled.tolist(), mixed=mixed.tolist()),
                  color=np.stack([DC.decimate_color(b, p["factor"]) for b in c.inputs["bgr"]]))


_DRAW = dict(reg=_draw_reg, undist=_draw_undist, upsample=_draw_upsample, holefill=_draw_holefill, speckle=_draw_speckle,
             temporal=_draw_temporal, decimate=_draw_decimate)
_WANT = dict(reg=_want_reg, undist=_want_undist, upsample=_want_upsample, holefill=_want_holefill, speckle=_want_speckle,
             temporal=_want_temporal, decimate=_want_decimate)


def draw(kind, seed, index):
    """the case without `want`"""
    rng = np.random.default_rng([seed, KINDS.index(kind), index])
    c = _common(rng, kind, seed, index)
    _DRAW[kind](rng, c)
    return c


def want(c, tables=None):
    """fills c.want from the statements; tables: the library's own (dict: range, space) for upsample and holefill, else numpy's"""
    with np.errstate(all="ignore"):                           # a sum of samples next to FLT_MAX overflows on both sides alike
        _WANT[c.kind](c, tables)
    return c


def case(kind, seed, index, tables=None):
    return want(draw(kind, seed, index), tables)


def describe(c):
    """what regenerates and explains a case"""
    fmt = lambda v: float(v) if isinstance(v, (float, np.floating)) else v
    d = dict(size=c.size, out_size=c.out_size, n=c.n, max_batch=c.max_batch, dt=np.dtype(c.dt).name, ot=np.dtype(c.ot).name, in_by=c.in_by,
             out_by=c.out_by, owner=c.owner, in_place=c.in_place, share=round(c.share, 3), **{k: fmt(v) for k, v in c.params.items()})
    for k in ("bgr_frames", "guide", "reset_at", "with_labels", "with_pass_of"):
        if hasattr(c, k):
            d[k] = getattr(c, k)
    if c.kind == "temporal":
        d["plan"] = c.plan
    return f"({c.kind!r}, seed {c.seed}, index {c.index}) {d}"


# ---- the device side: torch and kinectdepthmapenhancement_amd.filters are handed in ---------------------------------------
def new_object(F_, c):
    """the object of a case: the constructor and the calibration"""
    N, p = F_._native, c.params
    if c.kind == "reg":
        o = F_.DepthRegistration(c.size, c.out_size, c.max_batch, N.RegParams(p["z_min"], p["z_max"], p["max_splat"]))
        o.set_calibration(*c.calib)
    elif c.kind == "undist":
        o = F_.LensUndistortion(c.size, c.out_size, c.max_batch, N.UndistParams(p["z_min"], p["z_max"], p["depth_interp"], p["max_gap"]))
        o.set_calibration(*c.calib)
    elif c.kind == "upsample":
        o = F_.GuidedDepthUpsampling(c.size, c.out_size, c.max_batch, N.UpsampleParams(p["radius"], p["sigma_color"], p["max_gap"], p["z_min"], p["z_max"]))
    elif c.kind == "holefill":
        o = F_.DepthHoleFilling(c.size, c.max_batch, N.HolefillParams(p["radius"], p["iterations"], p["min_taps"], p["sigma_space"], p["sigma_color"],
                                                                      p["max_gap"], p["gap_rule"], p["z_min"], p["z_max"], p["passes_per_launch"]))
    elif c.kind == "speckle":
        o = F_.DepthSpeckleFilter(c.size, c.max_batch, N.SpeckleParams(p["min_size"], p["max_diff"], p["rel_diff"], p["connectivity"], p["z_min"], p["z_max"]))
    elif c.kind == "temporal":
        o = F_.DepthTemporalFilter(c.size, c.max_batch, N.TemporalParams(p["alpha"], p["max_diff"], p["rel_diff"], p["persist_min"], p["color_thresh"],
                                                                        p["z_min"], p["z_max"]))
    else:
        o = F_.DepthDecimation(c.size, c.max_batch, N.DecimateParams(p["factor"], p["mode"], p["min_valid"], p["max_gap"], p["z_min"], p["z_max"]))
    return o


def library_tables(o, c):
    """the tables the kernels read, from the object (no device needed); None for the kinds that have none"""
    if c.kind == "upsample":
        return dict(range=o.range_table())
    if c.kind == "holefill":
        return dict(range=o.range_table(), space=o.space_table())
    return None


def _tdt(torch, dtype):
    return {np.float32: torch.float32, np.uint16: torch.int16, np.uint8: torch.uint8, np.int32: torch.int32}[np.dtype(dtype).type]


def _placed(torch, a, by, fill, room=0):
    """the array on the device `by` elements past a 16-byte boundary in a buffer of `fill` bytes with `room` more elements
    behind it; (view, buffer)"""
    a = np.ascontiguousarray(a)
    flat = torch.empty(by + a.size + room + 16, dtype=_tdt(torch, a.dtype), device="cuda")
    flat.view(torch.uint8).fill_(fill)
    assert flat.data_ptr() % 16 == 0
    view = flat[by:by + a.size].view(a.shape)
    view.copy_(torch.from_numpy(a.view(np.int16) if a.dtype == np.uint16 else a).cuda())
    return view, flat


def _around_untouched(torch, buf, by, count):
    b = buf.view(torch.uint8)
    e = buf.element_size()
    return bool((b[:by * e] == SENTINEL).all()) and bool((b[(by + count) * e:] == SENTINEL).all())


def _host(t, dtype):
    a = t.cpu().numpy()
    return a.view(np.uint16) if np.dtype(dtype) == np.uint16 else a


def differs(got, want_, what):
    """None, or what differs between two arrays compared on their bytes"""
    if got.shape != want_.shape or got.dtype != want_.dtype:
        return f"{what}: {got.dtype} {got.shape} against {want_.dtype} {want_.shape}"
    if got.tobytes() != want_.tobytes():
        bits = {4: np.uint32, 2: np.uint16, 1: np.uint8}[got.dtype.itemsize]
        bad = np.argwhere(got.view(bits) != want_.view(bits))
        i = tuple(bad[0])
        return f"{what}: {len(bad)} elements differ, first at {i}: got {got[i]!r}, want {want_[i]!r}"
    return None


def run_case(torch, F_, c):
    """Builds the object of the drawn case c, fills c.want with the library's tables, runs the plan and compares.  Returns
    (violations, got): a list of strings -- empty: every byte, count and sentinel is as the statement says -- and the arrays the
    device gave (for a dump)."""
    bad, got = [], {}

    def check(msg):
        if msg:
            bad.append(msg)

    try:
        o = new_object(F_, c)
    except F_._native.KdeError as e:
        return [f"create refused an admitted configuration: {e}"], got
    try:
        want(c, library_tables(o, c))
        w_ = c.want
        frame = c.out_size[0] * c.out_size[1]
        src, src_buf = _placed(torch, c.inputs["depth"], c.in_by, SENTINEL if c.in_place else 0)
        src_before = src.clone()
        bgr = None
        if "bgr" in c.inputs:
            bgr, _ = _placed(torch, c.inputs["bgr"], c.in_by, 0)
            bgr_before = bgr.clone()
        outs = []

        def call(fn, lo, hi):
            """one batch call on frames lo .. hi - 1 of the input; its output frames, checked for what lies around them"""
            k = hi - lo
            if c.in_place:
                r = fn(src[lo:hi], src[lo:hi], None)
                check(None if r.data_ptr() == src[lo:hi].data_ptr() else "in place: another buffer was returned")
            elif c.owner == "caller":
                out, buf = _placed(torch, np.zeros((k,) + c.out_size[::-1], c.ot), c.out_by, SENTINEL, room=(c.max_batch - k) * frame)
                out.view(torch.uint8).fill_(SENTINEL)
                r = fn(src[lo:hi], out, None)
                check(None if _around_untouched(torch, buf, c.out_by, k * frame) else f"frames {lo}..{hi - 1}: bytes around the output were written")
            else:
                r = fn(src[lo:hi], None, _tdt(torch, c.ot))
            outs.append(_host(r, c.ot).copy())

        counts = {k: [] for k in w_["counts"]}

        def take_counts():
            for k in counts:
                counts[k] += getattr(o, k)().tolist()

        for step in c.plan:
            if c.kind == "reg" and step[0] == "depth":
                call(lambda d, out, fmt: o.register(d, out, **({} if fmt is None else dict(out_format=fmt))), 0, c.n)
                take_counts()
            elif c.kind == "reg":
                got["color"] = o.color_to_depth(src, bgr).cpu().numpy()
            elif c.kind == "undist" and step[0] == "depth":
                call(lambda d, out, fmt: o.depth(d, out, **({} if fmt is None else dict(out_format=fmt))), 0, c.n)
                take_counts()
            elif c.kind == "undist":
                got["color"] = o.color(bgr, c.n).cpu().numpy()
            elif c.kind == "upsample":
                call(lambda d, out, fmt: o.upsample(d, bgr, out, **({} if fmt is None else dict(out_format=fmt))), 0, c.n)
                take_counts()
            elif c.kind == "holefill":
                po = torch.full((c.n,) + c.size[::-1], 77, dtype=torch.uint8, device="cuda") if c.with_pass_of else None
                call(lambda d, out, fmt: o.fill(d, bgr, out, pass_of=po, **({} if fmt is None else dict(out_format=fmt))), 0, c.n)
                take_counts()
                if po is not None:
                    got["pass_of"] = po.cpu().numpy()
            elif c.kind == "speckle":
                lab = None
                if c.with_labels:
                    lab, lab_buf = _placed(torch, np.zeros((c.n,) + c.size[::-1], np.int32), 0, SENTINEL, room=frame)
                call(lambda d, out, fmt: o.filter(d, out, labels=lab, **({} if fmt is None else dict(out_format=fmt))), 0, c.n)
                take_counts()
                if lab is not None:
                    got["labels"] = lab.cpu().numpy()
                    check(None if _around_untouched(torch, lab_buf, 0, c.n * frame) else "bytes behind the labels were written")
            elif c.kind == "temporal" and step[0] == "reset":
                o.reset()
            elif c.kind == "temporal":
                lo, hi = step[1], step[2]
                call(lambda d, out, fmt: o.filter(d, None if bgr is None else bgr[lo:hi], out, **({} if fmt is None else dict(out_format=fmt))), lo, hi)
                take_counts()
            elif step[0] == "depth":
                call(lambda d, out, fmt: o.decimate(d, out, **({} if fmt is None else dict(out_format=fmt))), 0, c.n)
                take_counts()
            else:
                got["color"] = o.decimate_color(bgr).cpu().numpy()
        got["out"] = np.concatenate(outs)
        check(differs(got["out"], w_["out"], "depth"))
        for k in ("color", "labels", "pass_of"):
            if k in got:
                check(differs(got[k], w_[k], k))
        if c.kind == "temporal":
            value, hist = o.state()
            got["value"], got["hist"] = value.cpu().numpy(), hist.cpu().numpy().view(np.uint32)
            check(differs(got["value"], w_["value"], "state value"))
            check(differs(got["hist"], w_["hist"], "state hist"))
        for k, v in counts.items():
            got[k] = v
            check(None if v == [int(x) for x in w_["counts"][k]] else f"{k}: got {v}, want {list(w_['counts'][k])}")
        if c.in_place:
            check(None if _around_untouched(torch, src_buf, c.in_by, src.numel()) else "in place: bytes around the frames were written")
        else:
            check(None if torch.equal(src.view(torch.uint8), src_before.view(torch.uint8)) else "the input depth was written")
        if bgr is not None:
            check(None if torch.equal(bgr, bgr_before) else "the guide was written")
    except F_._native.KdeError as e:
        bad.append(f"a call refused an admitted configuration: {e}")
    finally:
        o.close()
    return bad, got
