"""A seeded draw of cases for the plane chain NormalMapGenerator -> NormalAdaptiveSuperpixel -> LabelEquivalenceSeg ->
PlaneProjection (kde_normals_*, kde_nasp_*, kde_les_*, kde_proj_*) and the KinectDepthEnhancement object that composes them, and the
comparison of the library with the CPU restatements tools/normals_ref.c, nasp_ref.c, les_ref.c and proj_ref.c.

    case(kind, seed, index)   one self-contained case: sizes, constructor arguments, one or two calls with their inputs, want
    run_case(torch, F_, c)    builds the object, runs the calls on the device and returns the violations (strings); none: equal

A case is drawn from np.random.default_rng([seed, kind number, index]) alone, so any case can be made again without the ones
before it.  Every parameter is drawn from the whole domain create, SetParametor and the call admit (the KDE_REQUIREs of
csrc/kde_api_normals.cpp, kde_api_nasp.cpp, kde_api_les.cpp, kde_api_proj.cpp and superpixel_geometry in csrc/kde_handles.h), so a
refusal is a violation.  `want` comes from the four tools/*_ref modules; no rule is restated here, and the bars are those of the
stages' own GPU tests: normals_cases.check_cm / assert_nan_equal_bits, nasp_cases.assert_identical, les_cases.diff_counts all
zero, tools/proj_ref.compare with plane_fitted, strict, hole, band and xy all 0 (window 1: bit for bit).

What every kind draws: n in 1 .. 4 frames on an object for n or n + 1; the single-frame or the batch entry point; for about half
the cases a second call on the same object with other content and another n and, where the API takes them per call, another
cluster count, other sigmas or another method.  The second call is compared against the restatement, never against the first,
and a batch is compared frame by frame.  The kind `chain` runs the six stages of KinectDepthEnhancement by hand, compares each of
normals, NASP, LES and projection against its restatement fed with the DEVICE's output of the stage before (so no tolerance
compounds), and then holds KinectDepthEnhancement to the by-hand bytes.  test_plane_sweep.py holds the conditions on the draw.

This module needs no GPU: torch and the filters module are handed to run_case().
"""
from types import SimpleNamespace

import numpy as np

import les_cases as LC
import nasp_cases as NC
import normals_cases as NM
import proj_cases as PC
from stage_sweep import _guide, _line

F = np.float32
KINDS = ("normals", "nasp", "les", "proj", "chain")

# the bounds of the library (csrc/kde_internal.h, csrc/normal_kernels.hip, csrc/nasp_kernels.hip)
DT_CAP_C = 47.0                     # kDtCapC: a frame whose largest DDSA exceeds it takes the serial distance transform
DT_BAND_ROWS = 64                   # kBandRows
NASP_MIN_WINDOW = 8
NASP_MAX_LDS_CLUSTERS = 1536        # kNaspMaxLdsClusters
NASP_SPATIAL_CAP_MAX = 1 << 20      # kde_nasp::kSpatialCapMax (csrc/kde_handles.h): entries of the spatial weight table
LES_MAX_CLUSTERS = 2048             # kLesMaxClusters
PROJ_MAX_WINDOW = 15                # kProjMaxWindow
PROJ_TILE = (64, 16)
CM, BILATERAL = 1, 2

NORMALS_H_CLASSES = (63, 64, 65, 127, 128, 129)
NORMALS_W_CLASSES = (255, 256, 257)
NORMALS_FACTORS = (0.05, 0.02, 0.2)
NORMALS_SMOOTHING = (20.0, 10.0, 5.0, 30.0, -2.0, 46.5)      # the default; one non-positive; 46.5: C just under 47 at near depth
NORMALS_HOLES = ("none", "one", 1e-4, 1e-3, 0.03, 0.3)
NASP_REF_CALL = (10.0, 50.0, 50.0, 150.0)                      # KinectDepthEnhancement.cpp:67
NASP_SIGMAS = ("ref", "color0", "spatial0", "depth0", "normal0", "depth0normal0", "other")
NASP_GRIDS = ("1x1", "1xN", "Nx1", "small", "big", "window")
NASP_WINDOWS = (8, 55, 56, 63, 64)
NASP_PINNED = ((384, 256, 32, 48), (392, 256, 32, 49))         # W, H, rows, cols: exactly 1536 and 1568 clusters of 8 x 8
LES_STYLES = ("grid", "blobs", "stripes")
LES_ANGLES = (float(LC.MAX_ANGLE), 0.1, 1.2, 0.0, 4.0, -1.0)
LES_DISTANCES = (float(LC.MAX_DIST), 30.0, 0.0, 1e9)
PROJ_ANGLES = (float(PC.MAX_ANGLE), 0.1, 1.2, 0.0)

# the budget of tests/test_gpu_plane_sweep.py; tests/test_plane_sweep.py holds the conditions on the draw over exactly this
SEEDS = (1, 2)
CASES_PER_KIND = dict(normals=40, nasp=16, les=40, proj=30, chain=10)

_refs = {}


def kinds():
    return KINDS


def budget(kind):
    return [(seed, index) for seed in SEEDS for index in range(CASES_PER_KIND[kind])]


def refs():
    """the four restatements, built once: .normals, .nasp, .les, .proj"""
    if not _refs:
        from tools import les_ref, nasp_ref, normals_ref, proj_ref
        for name, m in (("normals", normals_ref), ("nasp", nasp_ref), ("les", les_ref), ("proj", proj_ref)):
            m.build()
            _refs[name] = m
    return SimpleNamespace(**_refs)


# ---- the draws the kinds share ----------------------------------------------------------------------------------------
def _common(rng, kind, seed, index):
    n = int(rng.integers(1, 5))
    return SimpleNamespace(kind=kind, seed=seed, index=index, n=n, max_batch=n + int(rng.integers(0, 2)), params={}, calls=[])


def _entry(rng, n):
    return "single" if n == 1 and rng.random() < 0.6 else "batch"


def _second_n(rng, c):
    """a second call half the time: its n, mostly another one"""
    if rng.random() >= 0.5:
        return None
    other = [k for k in range(1, min(c.max_batch, 4) + 1) if k != c.n]
    return int(rng.choice(other)) if other and rng.random() < 0.8 else c.n


def _camera_points(z, W, H, f=575.8):
    """millimetre points [H, W, 3] of the depths z on the rays of a pinhole camera, as DimensionConvertor writes them"""
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float32)
    f = F(f)
    z = z.astype(np.float32)
    with np.errstate(all="ignore"):
        return np.stack([(xx - W / 2) / f * z, (H / 2 - yy) / f * z, z], -1).astype(np.float32)


def camera_matrix(W, H):
    f = 575.8 * W / 640.0
    return np.array([[f, 0.0, W / 2.0], [0.0, f, H / 2.0], [0.0, 0.0, 1.0]], np.float64)


def _surface(rng, W, H, z_top, shape=None, noise=None, step=None):
    """float64 [H, W]: a flat, tilted or wavy surface, mostly with 2 mm of noise, half the time with a depth step of 30 % along a
    line, scaled so that its largest depth is z_top"""
    y, x = np.mgrid[0:H, 0:W].astype(np.float64)
    shape = rng.choice(["flat", "tilted", "wavy"]) if shape is None else shape
    noise = rng.random() < 0.6 if noise is None else noise
    step = rng.random() < 0.5 if step is None else step
    if shape == "flat":
        rel = np.zeros((H, W))
    elif shape == "tilted":
        a, b = rng.uniform(-0.15, 0.15, 2)
        rel = a * x / max(W, 1) + b * y / max(H, 1)
    else:
        rel = 0.1 * np.sin(x / 9.0 + rng.uniform(0, 6)) + 0.05 * np.cos(y / 7.0 + rng.uniform(0, 6))
    z = 1.0 + rel
    if step:
        side, _ = _line(rng, W, H)
        z = np.where(side, z * 1.3, z)
    z = z * (z_top / z.max())
    if noise:
        z = z + rng.normal(0.0, 2.0, z.shape)
    return z, dict(shape=str(shape), noise=bool(noise), step=bool(step))


# ---- normals ----------------------------------------------------------------------------------------------------------
def _normals_side(rng, classes, lo, hi):
    """lo .. hi with weight on the classes, on multiples of 64 +- 1 and on sides >= 48"""
    u = rng.random()
    if u < 0.03:
        return 1
    if u < 0.30:
        return int(rng.choice(classes))
    if u < 0.45:
        return int(np.clip(64 * rng.integers(1, hi // 64 + 1) + rng.integers(-1, 2), lo, hi))
    if u < 0.85:
        return int(rng.integers(48, hi + 1))
    return int(rng.integers(lo, hi + 1))


def frame_C(points, smoothing):
    """the frame's largest DDSA as normals_prep_kernel forms it (NaN where a depth is NaN: such a frame is not capped)"""
    with np.errstate(all="ignore"):
        return float(np.max(F(smoothing) + (points[..., 2] / F(1000.0)) / F(10.0)))


def is_capped(points, smoothing):
    return frame_C(points, smoothing) <= DT_CAP_C


def _normals_frame(rng, W, H, smoothing, scale):
    if scale == "near":
        z_top = rng.uniform(700, 1500)
    elif scale == "mid":
        z_top = rng.uniform(2500, 5000)
    else:                                                     # C = smoothing + z_top / 10000 within 1 of 47, either side
        z_top = (DT_CAP_C + float(rng.choice([-0.9, -0.1, -0.01, 0.01, 0.1, 0.9])) - smoothing) * 10000.0
        if z_top < 500:
            z_top = rng.uniform(700, 1500)
    # On an exactly planar neighbourhood the sign of the smallest eigenvalue is a matter of rounding, and the checker's band
    # grows with every hole and step next to it; 2 mm of noise at 270 m is as good as none.  So that the band stays the sliver
    # test_plane_sweep.py asks for, a surface without noise or far away has at most one hole in 1000 pixels, and one without
    # noise has a step a quarter of the time only.
    noise = bool(rng.random() < 0.8)
    z, what = _surface(rng, W, H, z_top, noise=noise, step=None if noise else bool(rng.random() < 0.25))
    p_holes = np.array([0.22, 0.18, 0.15, 0.15, 0.18, 0.12])
    if not noise or scale == "far":
        p_holes[4:] = 0
    holes = NORMALS_HOLES[rng.choice(len(NORMALS_HOLES), p=p_holes / p_holes.sum())]
    if holes == "none":
        hit = np.zeros((H, W), bool)
    elif holes == "one":
        hit = np.zeros((H, W), bool)
        hit[rng.integers(0, H), rng.integers(0, W)] = True
    else:
        hit = rng.random((H, W)) < holes
    special = bool(rng.random() < 0.3)                        # holes of 0 only, or of every special depth
    values = np.array([0.0, np.nan, np.inf, -np.inf, -500.0]) if special else np.array([0.0])
    z[hit] = values[rng.integers(0, len(values), int(hit.sum()))]
    what.update(scale=scale, holes=holes, special=special)
    return _camera_points(z, W, H), what


def _normals_call(rng, c, n, method):
    p = c.params
    scales = [str(rng.choice(["near", "mid", "far"], p=[0.4, 0.25, 0.35])) for _ in range(n)]
    if n > 1 and rng.random() < 0.5:                          # a batch that mixes a capped and an uncapped frame
        scales[0], scales[1] = "near", "far"
    frames = [_normals_frame(rng, *c.size, p["normal_smoothing_size"], s) for s in scales]
    return SimpleNamespace(n=n, entry=_entry(rng, n), method=method, owner=("caller", "object")[rng.integers(0, 2)],
                           inputs=dict(points=np.stack([f[0] for f in frames])), what=[f[1] for f in frames], want=None)


def _draw_normals(rng, c):
    c.size = (_normals_side(rng, NORMALS_W_CLASSES, 1, 260), _normals_side(rng, NORMALS_H_CLASSES, 1, 200))
    c.params = dict(max_depth_change_factor=float(rng.choice(NORMALS_FACTORS, p=[0.6, 0.2, 0.2])),
                    normal_smoothing_size=float(rng.choice(NORMALS_SMOOTHING, p=[0.4, 0.12, 0.12, 0.12, 0.12, 0.12])))
    method = lambda: CM if rng.random() < 0.7 else BILATERAL
    c.calls.append(_normals_call(rng, c, c.n, method()))
    n2 = _second_n(rng, c)
    if n2 is not None:
        c.calls.append(_normals_call(rng, c, n2, method()))


def _want_normals(c):
    R, p = refs().normals, c.params
    for call in c.calls:
        kw = dict(factor=p["max_depth_change_factor"], smoothing=p["normal_smoothing_size"])
        call.want = [R.normals(f, R.CM, return_rest=True, **kw) if call.method == CM else R.normals(f, R.BILATERAL, **kw)
                     for f in call.inputs["points"]]


# ---- nasp -------------------------------------------------------------------------------------------------------------
def _nasp_geometry(rng, grid, seed=0, index=0):
    """(W, H, rows, cols) of a grid class: W = wx * cols + r with r < min(cols, wx), so that W / cols = wx and W / wx = cols"""
    cmax, rmax = 260 // NASP_MIN_WINDOW, 200 // NASP_MIN_WINDOW
    rows, cols = dict([("1x1", (1, 1)), ("1xN", (1, int(rng.integers(2, cmax + 1)))), ("Nx1", (int(rng.integers(2, rmax + 1)), 1)),
                       ("small", (int(rng.integers(2, 9)), int(rng.integers(2, 9)))),
                       ("big", (int(rng.integers(9, rmax + 1)), int(rng.integers(9, cmax + 1)))),
                       ("window", (int(rng.integers(1, 4)), int(rng.integers(1, 5))))])[grid]
    wx, wy = int(rng.integers(NASP_MIN_WINDOW, 260 // cols + 1)), int(rng.integers(NASP_MIN_WINDOW, 200 // rows + 1))
    if grid == "window":                                      # both windows out of NASP_WINDOWS, dealt by the index so that each occurs
        fit = [w for w in NASP_WINDOWS if w * cols <= 260], [w for w in NASP_WINDOWS if w * rows <= 200]
        wx, wy = fit[0][index % len(fit[0])], fit[1][(2 * index + seed) % len(fit[1])]
    W = wx * cols + int(rng.integers(0, min(cols, wx, 260 - wx * cols + 1)))
    H = wy * rows + int(rng.integers(0, min(rows, wy, 200 - wy * rows + 1)))
    return W, H, rows, cols


def _nasp_sigmas(rng, which):
    c, s, d, n = NASP_REF_CALL if which != "other" else [float(v) for v in rng.choice([1.0, 5.0, 10.0, 50.0, 150.0, 400.0], 4)]
    return dict(ref=(c, s, d, n), other=(c, s, d, n), color0=(0.0, s, d, n), spatial0=(c, 0.0, d, n), depth0=(c, s, 0.0, n),
                normal0=(c, s, d, 0.0), depth0normal0=(c, s, 0.0, 0.0))[which]


def _nasp_frame(rng, W, H, light=False):
    """(bgr, points, normals) of one frame; light: no restatement of the normals (random unit vectors only)"""
    z, what = _surface(rng, W, H, rng.uniform(700, 3500))
    for _ in range(int(rng.integers(0, 4))):                  # patches below, on and above the z > 50 tests, and NaN
        x0, y0 = rng.integers(0, W), rng.integers(0, H)
        v = float(rng.choice([0.0, 20.0, np.nextafter(F(50), F(0)), 50.0, np.nextafter(F(50), F(100)), np.nan]))
        z[y0:y0 + rng.integers(1, H // 3 + 2), x0:x0 + rng.integers(1, W // 3 + 2)] = v
    hit = rng.random((H, W)) < float(rng.choice([0.0, 0.01, 0.05]))
    z[hit] = rng.choice(np.array([0.0, 49.0, 50.0, np.nan]), int(hit.sum()))
    pts = _camera_points(z, W, H)
    source = "random" if light else str(rng.choice(["cm", "bilateral", "random"]))
    if source == "random":
        v = rng.normal(size=(H, W, 3)) + np.array([0.0, 0.0, -2.0])
        nrm = (v / np.linalg.norm(v, axis=-1, keepdims=True)).astype(np.float32)
    else:
        R = refs().normals
        nrm = np.ascontiguousarray(R.normals(pts, R.CM if source == "cm" else R.BILATERAL, want_band=False)[0])
    damage = str(rng.choice(["none", "bad", "partial", "nan", "all"], p=[0.2, 0.2, 0.3, 0.2, 0.1]))
    nans = bool(rng.random() < 0.5)                           # and, independently, NaN components in 2 % of the normals
    if damage == "bad":                                       # whole (-1, -1, -1): a rectangle and 2 % of the pixels
        x0, y0 = rng.integers(0, W), rng.integers(0, H)
        nrm[y0:y0 + rng.integers(1, H // 2 + 2), x0:x0 + rng.integers(1, W // 2 + 2)] = -1
        nrm[rng.random((H, W)) < 0.02] = -1
    elif damage == "partial":                                 # one or two components -1: ok3_and and ok3_or disagree
        hit = np.argwhere(rng.random((H, W)) < 0.1)
        for (y, x), k in zip(hit, rng.integers(1, 7, len(hit))):
            nrm[y, x, [i for i in range(3) if k >> i & 1]] = -1
    elif damage == "nan":
        hit = rng.random((H, W)) < 0.02
        nrm[hit, rng.integers(0, 3, int(hit.sum()))] = np.nan
    elif damage == "all":
        nrm[...] = -1
    if nans and damage != "nan":
        hit = rng.random((H, W)) < 0.02
        nrm[hit, rng.integers(0, 3, int(hit.sum()))] = np.nan
    what.update(normals=source, damage=damage, nans=nans)
    return _guide(rng, 1, W, H)[0], pts, nrm, what


def _nasp_call(rng, c, n, sigmas, iteration, light=False):
    frames = [_nasp_frame(rng, *c.size, light) for _ in range(n)]
    return SimpleNamespace(n=n, entry=_entry(rng, n), sigmas=sigmas, sig=_nasp_sigmas(rng, sigmas), iteration=iteration,
                           inputs=dict(bgr=np.stack([f[0] for f in frames]), points=np.stack([f[1] for f in frames]),
                                       normals=np.stack([f[2] for f in frames])), what=[f[3] for f in frames], want=None)


def _draw_nasp(rng, c):
    if c.index < len(NASP_PINNED):                            # both sides of the LDS cluster table: one frame, one call
        W, H, rows, cols = NASP_PINNED[c.index]
        c.grid, c.n, c.max_batch = "pinned", 1, 1 + int(rng.integers(0, 2))
        c.size, c.rows, c.cols = (W, H), rows, cols
        c.calls.append(_nasp_call(rng, c, 1, "ref", int(rng.integers(1, 3)), light=True))
        return
    deal = NASP_GRIDS + ("window",)                           # the grid classes in turn, the windows twice
    c.grid = deal[(c.index - len(NASP_PINNED)) % len(deal)]
    W, H, c.rows, c.cols = _nasp_geometry(rng, c.grid, c.seed, c.index)
    c.size = (W, H)
    first = str(rng.choice(NASP_SIGMAS))
    c.calls.append(_nasp_call(rng, c, c.n, first, int(rng.integers(0, 6))))
    n2 = _second_n(rng, c)
    if n2 is not None:                                        # other sigmas; a third of the time one sigma alone changes
        second = str(rng.choice([s for s in NASP_SIGMAS if s != first]))
        call = _nasp_call(rng, c, n2, second, int(rng.integers(0, 6)))
        if rng.random() < 0.35:
            k = int(rng.integers(0, 2))                       # the colour or the spatial sigma: one cached table stays valid
            sig = list(c.calls[0].sig)
            sig[k] = float(rng.choice([v for v in (3.0, 20.0, 80.0) if v != sig[k]]))
            call.sigmas, call.sig = "one changed", tuple(sig)
        c.calls.append(call)


def _want_nasp(c):
    """a restatement object per frame slot of the handle: a call's result may depend on the slot's history (iteration 0 leaves
    the labels of the call before)"""
    R = refs().nasp
    K = camera_matrix(*c.size)
    slots = [R.State(*c.size, c.rows, c.cols, K) for _ in range(c.max_batch)]
    for call in c.calls:
        i = call.inputs
        call.want = [slots[f].segmentation(i["bgr"][f], i["points"][f], i["normals"][f], *call.sig, call.iteration) for f in range(call.n)]


def nasp_iteration_zero_case():
    """The smallest input of what the sweep found first: Segmentation with iteration = 0 must leave the initial LD of
    initLD_NASP (own grid cell, 999999.9) and not touch the labels, on a fresh handle and on a used one.  16 x 8, two 8 x 8
    superpixels, a flat wall at 1 m; call 0 runs no iteration, call 1 two, call 2 none again (on LD and labels call 1 left)."""
    W, H = 16, 8
    c = SimpleNamespace(kind="nasp", seed=0, index=-1, n=1, max_batch=1, params={}, calls=[], size=(W, H), rows=1, cols=2, grid="named")
    bgr = np.full((1, H, W, 3), 90, np.uint8)
    bgr[:, :, W // 2:] = 160
    pts = _camera_points(np.full((H, W), 1000.0), W, H)[None]
    nrm = np.zeros((1, H, W, 3), np.float32)
    nrm[..., 2] = -1.0                                        # (0, 0, -1): facing the camera
    for it in (0, 2, 0):
        c.calls.append(SimpleNamespace(n=1, entry="single", sigmas="ref", sig=NASP_REF_CALL, iteration=it,
                                       inputs=dict(bgr=bgr, points=pts, normals=nrm), what=[{}], want=None))
    return c


# ---- les --------------------------------------------------------------------------------------------------------------
def _les_frame(rng, W, H, nc, style, thr, max_dist):
    y, x = np.mgrid[0:H, 0:W]
    if style == "grid":
        bw, bh = int(rng.integers(1, max(W // 3, 1) + 1)), int(rng.integers(1, max(H // 3, 1) + 1))
        labels = ((y // bh) * (-(-W // bw)) + x // bw) % nc
    elif style == "blobs":
        bw, bh = max(1, W // int(rng.integers(2, 9))), max(1, H // int(rng.integers(2, 9)))
        coarse = rng.integers(0, nc, (-(-H // bh), -(-W // bw)))
        labels = np.kron(coarse, np.ones((bh, bw), np.int64))[:H, :W]
        r = rng.random((H, W)) < 0.1
        labels[r] = rng.integers(0, nc, int(r.sum()))
    else:                                                     # one-pixel stripes: a chain as long as the frame is wide or high
        labels = (x if rng.random() < 0.5 else y) % nc
        if rng.random() < 0.5:
            labels = nc - 1 - labels
    labels = labels.astype(np.int32)
    r = rng.random((H, W))
    out = float(rng.choice([0.0, 0.0, 1.0]))                  # a third of the frames with every label in the table
    labels[r < 0.03 * out] = -1
    labels[(r >= 0.03) & (r < 0.03 + 0.02 * out)] = nc + rng.integers(0, 3)
    labels[(r >= 0.05) & (r < 0.05 + 0.01 * out)] = rng.choice([-7, 1 << 20, np.iinfo(np.int32).min])
    # normals: exactly z, z with a small tilt, at the angle threshold by a float step of the dot product, or far off
    kind = rng.random(nc)
    normals = np.zeros((nc, 3), np.float64)
    normals[:, 2] = 1.0
    tilt = (kind >= 0.4) & (kind < 0.65)
    normals[tilt] += 0.05 * rng.normal(size=(int(tilt.sum()), 3))
    off = kind >= 0.9
    normals[off] = rng.normal(size=(int(off.sum()), 3))
    normals = (normals / np.linalg.norm(normals, axis=1, keepdims=True)).astype(np.float32)
    edge = np.flatnonzero((kind >= 0.65) & (kind < 0.9))
    if -1 < thr < 1:                                          # (sqrt(1 - c^2), 0, c) . (0, 0, 1) = c exactly
        cth = np.full(len(edge), thr, np.float32)
        for i, s in enumerate(rng.integers(-3, 4, len(edge))):
            for _ in range(abs(int(s))):
                cth[i] = np.nextafter(cth[i], F(1) if s > 0 else F(-1))
        normals[edge] = np.stack([np.sqrt(1 - cth.astype(np.float64) ** 2), np.zeros(len(edge)), cth], -1).astype(np.float32)
    md = F(max_dist if 0 < max_dist < 1e6 else 100.0)         # plane distances on either side of max_plane_distance
    steps = np.array([0.0, 0.0, 0.0, md * F(0.5), np.nextafter(md, F(0)), md, np.nextafter(md, F(np.inf)), md * F(2)], np.float32)
    centers = (normals * (F(1000) + steps[rng.integers(0, len(steps), nc)])[:, None]).astype(np.float32)
    flaw = rng.random(nc)
    normals[flaw < 0.06] = -1
    normals[(flaw >= 0.06) & (flaw < 0.09), rng.integers(0, 3)] = np.nan
    normals[(flaw >= 0.09) & (flaw < 0.13), :2] = -1          # L7
    return normals, labels, centers


def _les_call(rng, c, n, nc):
    p = c.params
    style = str(rng.choice(LES_STYLES, p=[0.3, 0.3, 0.4]))
    frames = [_les_frame(rng, *c.size, nc, style, LC.acos_threshold(p["max_angle"]), p["max_plane_distance"]) for _ in range(n)]
    return SimpleNamespace(n=n, entry=_entry(rng, n), nc=nc, style=style, want=None,
                           inputs=dict(normals=np.stack([f[0] for f in frames]), labels=np.stack([f[1] for f in frames]),
                                       centers=np.stack([f[2] for f in frames])))


def _les_nc(rng, W, H):
    cap = min(W * H, LES_MAX_CLUSTERS)
    u = rng.random()
    return 1 if u < 0.05 else cap if u < 0.15 else int(np.clip(np.exp(rng.uniform(0, np.log(cap + 1))), 1, cap))


def _draw_les(rng, c):
    side = lambda hi: 1 if rng.random() < 0.04 else int(rng.integers(1, hi + 1))
    W, H = c.size = (side(200), side(200))
    c.params = dict(iterations=int(rng.integers(0, 13)), max_angle=float(rng.choice(LES_ANGLES, p=[0.5, 0.1, 0.1, 0.1, 0.1, 0.1])),
                    max_plane_distance=float(rng.choice(LES_DISTANCES, p=[0.55, 0.15, 0.15, 0.15])))
    c.calls.append(_les_call(rng, c, c.n, _les_nc(rng, W, H)))
    n2 = _second_n(rng, c)
    if n2 is not None:                                        # a smaller or a larger table than the call before, where there is one
        nc = _les_nc(rng, W, H)
        if nc == c.calls[0].nc and min(W * H, LES_MAX_CLUSTERS) > 1:
            nc = nc - 1 if nc > 1 else nc + 1
        c.calls.append(_les_call(rng, c, n2, nc))


def _want_les(c, extra_iterations=0):
    R, p = refs().les, c.params
    for call in c.calls:
        i = call.inputs
        call.want = [R.label_image(i["normals"][f], i["labels"][f], i["centers"][f], p["iterations"] + extra_iterations, p["max_angle"],
                                   p["max_plane_distance"]) for f in range(call.n)]


# ---- proj -------------------------------------------------------------------------------------------------------------
def _proj_side(rng, tile, hi):
    u = rng.random()
    if u < 0.5:
        return int(np.clip(tile * rng.integers(1, hi // tile + 1) + rng.integers(-1, 2), 1, hi))
    return 1 if u < 0.53 else int(rng.integers(1, hi + 1))


def _proj_frame(rng, c, nc, deep):
    W, H = c.size
    p = c.params
    holes = float(rng.choice([0.0, 0.02] if p["window_size"] == 1 and W * H >= 1000 else [0.0] if p["window_size"] == 1 else
                             [0.0, 0.02, 0.04, 0.08])) if not c.no_holes else 0.0
    seed = int(rng.integers(0, 2 ** 31))
    make = PC.deep_case if deep and holes and p["window_size"] > 1 else PC.synthetic_case
    nd, labels, variance, points, size, K = make(seed, W, H, nc) if make is PC.deep_case else make(seed, W, H, nc, hole_frac=holes)
    variance, size, nd = variance.copy(), size.copy(), nd.copy()
    thr = LC.acos_threshold(p["max_angle"])
    for k in rng.integers(0, nc, min(nc, 6)):                 # variances on the angle threshold and a float step to either side
        variance[k] = [thr, np.nextafter(thr, F(2)), np.nextafter(thr, F(-2)), np.nextafter(F(1), F(0))][rng.integers(0, 4)]
    if rng.random() < 0.5:                                    # a region whose ray denominator is 0
        nd[labels == labels[rng.integers(0, H), rng.integers(0, W)], :3] = 0
    if p["min_size"] != PC.min_size_for(W, H):                # a size table on both sides of the drawn min_size
        size = np.clip(np.int64(p["min_size"]) + rng.integers(0, 2, nc), -2 ** 31, 2 ** 31 - 1).astype(np.int32)
    return nd, labels, variance, points, size


def _proj_call(rng, c, n, nc):
    # up to 4000 mm in a fifth of the calls: BAND pixels, with depth_sigma 150 or spatial_sigma 0.5 also holes whose tap weights are
    # float32 denormals (exp arguments of -87 .. -103), where the quotient leaves the window's range by up to half a millimetre
    # (tools/proj_ref.BAND_SLACK_MM; proj_cases.denormal_weight_case is the smallest such input)
    deep = rng.random() < 0.2
    frames = [_proj_frame(rng, c, nc, deep) for _ in range(n)]
    names = ("nd", "labels", "variance", "points", "size")
    return SimpleNamespace(n=n, entry=_entry(rng, n), nc=nc, deep=bool(deep), want=None,
                           inputs={k: np.stack([f[j] for f in frames]) for j, k in enumerate(names)})


def _proj_nc(rng):
    u = rng.random()
    return 1 if u < 0.06 else 4096 if u < 0.12 else int(np.clip(np.exp(rng.uniform(0, np.log(4097))), 1, 4096))


def _draw_proj(rng, c):
    W, H = c.size = (_proj_side(rng, PROJ_TILE[0], 200), _proj_side(rng, PROJ_TILE[1], 150))
    window = int(rng.choice(np.arange(1, PROJ_MAX_WINDOW + 1, 2)))
    # a hole sums exp(-z^2 / (2 depth_sigma^2)) over its window: below depth_sigma = 100 at 1250 mm every hole would be a BAND
    # pixel, so the small depth sigmas go with frames without holes
    c.no_holes = bool(rng.random() < 0.35)
    c.params = dict(window_size=window, spatial_sigma=float(rng.choice([20.0, 3.0, 0.5, -4.0, 200.0])),
                    depth_sigma=float(rng.choice([10.0, 40.0, 100.0] if c.no_holes else [100.0, 150.0, 400.0])),
                    max_angle=float(rng.choice(PROJ_ANGLES, p=[0.55, 0.15, 0.15, 0.15])),
                    min_size=int(rng.choice([PC.min_size_for(W, H)] * 5 + [0, PC.MIN_SIZE, 2 ** 31 - 1, -5])))
    c.calls.append(_proj_call(rng, c, c.n, _proj_nc(rng)))
    n2 = _second_n(rng, c)
    if n2 is not None:
        c.calls.append(_proj_call(rng, c, n2, _proj_nc(rng)))


def _want_proj(c):
    R = refs().proj
    K = PC.intrinsics(*c.size)
    for call in c.calls:
        i = call.inputs
        call.want = [R.plane_projection(i["nd"][f], i["labels"][f], i["variance"][f], i["points"][f], i["size"][f], K, **c.params)
                     for f in range(call.n)]


# ---- chain ------------------------------------------------------------------------------------------------------------
def _chain_call(rng, c, n):
    from kinectdepthmapenhancement_amd import synth
    W, H = c.size
    source = str(rng.choice(["synth", "surface"]))
    if source == "synth":
        frames = [synth.make_frame(int(rng.integers(0, 2 ** 31)), W, H) for _ in range(n)]
        bgr, depth = np.stack([f[0] for f in frames]), np.stack([f[1] for f in frames])
    else:
        depth = np.stack([_surface(rng, W, H, rng.uniform(900, 3500))[0] for _ in range(n)]).astype(np.float32)
        depth[rng.random(depth.shape) < float(rng.choice([0.0, 1e-3, 0.03]))] = 0
        bgr = _guide(rng, n, W, H)
    return SimpleNamespace(n=n, entry=_entry(rng, n), source=source, inputs=dict(depth=np.ascontiguousarray(depth, np.float32),
                                                                               bgr=np.ascontiguousarray(bgr, np.uint8)), want=None)


def _draw_chain(rng, c):
    while True:                                               # a grid the geometry admits on a frame of 48 .. 200 x 48 .. 150
        W, H, c.rows, c.cols = _nasp_geometry(rng, str(rng.choice(["small", "big", "1xN", "Nx1"])))
        if 48 <= W <= 200 and 48 <= H <= 150:
            break
    c.size = (W, H)
    c.calls.append(_chain_call(rng, c, c.n))
    n2 = _second_n(rng, c)
    if n2 is not None:
        c.calls.append(_chain_call(rng, c, n2))


_DRAW = dict(normals=_draw_normals, nasp=_draw_nasp, les=_draw_les, proj=_draw_proj, chain=_draw_chain)
_WANT = dict(normals=_want_normals, nasp=_want_nasp, les=_want_les, proj=_want_proj, chain=lambda c: None)


def draw(kind, seed, index):
    """the case without `want`"""
    rng = np.random.default_rng([seed, KINDS.index(kind), index])
    c = _common(rng, kind, seed, index)
    _DRAW[kind](rng, c)
    return c


def want(c):
    """fills every call's want (a list, one entry per frame) from the restatements; the chain's restatements read the device's own
    intermediate results and run in run_case()"""
    _WANT[c.kind](c)
    return c


def case(kind, seed, index):
    return want(draw(kind, seed, index))


def describe(c):
    """what regenerates and explains a case"""
    d = dict(size=c.size, max_batch=c.max_batch, **c.params)
    for k in ("rows", "cols", "grid", "no_holes"):
        if hasattr(c, k):
            d[k] = getattr(c, k)
    keys = ("n", "entry", "method", "owner", "sigmas", "sig", "iteration", "nc", "style", "deep", "source", "what")
    d["calls"] = [{k: getattr(call, k) for k in keys if hasattr(call, k)} for call in c.calls]
    return f"({c.kind!r}, seed {c.seed}, index {c.index}) {d}"


# ---- the device side: torch and kinectdepthmapenhancement_amd.filters are handed in ---------------------------------------
def _dev(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _frames(t, n, shape):
    """a getter's tensor ([...] after a single call, [n, ...] after a batch of n > 1) as a host array [n, ...]"""
    return t.reshape((n,) + tuple(shape)).cpu().numpy()


def _asserted(bad, what, fn, *a, **kw):
    """runs a bar written as assertions; a failure becomes a violation"""
    try:
        return fn(*a, **kw)
    except AssertionError as e:
        bad.append(f"{what}: {e}")
        return None


def new_object(F_, c):
    """the object of a case; raises KdeError on a refusal"""
    N, p, (W, H) = F_._native, c.params, c.size
    if c.kind == "normals":
        return F_.NormalMapGenerator(W, H, c.max_batch, N.NormalsParams(c.calls[0].method, p["max_depth_change_factor"], p["normal_smoothing_size"]))
    if c.kind == "nasp":
        o = F_.NormalAdaptiveSuperpixel(W, H, c.max_batch)
        o.SetParametor(c.rows, c.cols, camera_matrix(W, H))
        return o
    if c.kind == "les":
        return F_.LabelEquivalenceSeg(W, H, c.max_batch, N.LesParams(p["iterations"], p["max_angle"], p["max_plane_distance"]))
    if c.kind == "proj":
        return F_.PlaneProjection(W, H, PC.intrinsics(W, H), c.max_batch,
                                  N.ProjParams(p["window_size"], p["spatial_sigma"], p["depth_sigma"], p["max_angle"], p["min_size"]))
    o = F_.KinectDepthEnhancement(W, H, c.max_batch)
    o.SetParametor(c.rows, c.cols, camera_matrix(W, H))
    return o


def _run_normals(torch, o, c, call, tag, bad, got):
    R, (W, H), n = refs().normals, c.size, call.n
    pts = _dev(torch, call.inputs["points"])
    before = pts.clone()
    o.setNormalEstimationMethods(call.method)
    if call.entry == "single":
        o.generateNormalMap(pts[0])
        out = o.getNormalMap()
    elif call.owner == "caller":
        out = o.generateNormalMapBatch(n, pts, torch.full_like(pts, 7.0))
    else:
        o.generateNormalMapBatch(n, pts)
        out = o.getNormalMap()
    nrm = _frames(out, n, (H, W, 3))
    fs = _frames(o.getSmoothingMap(), n, (H, W)) if call.method == CM else None
    got[tag] = dict(normals=nrm, fs=fs)
    kw = dict(factor=c.params["max_depth_change_factor"], smoothing=c.params["normal_smoothing_size"])
    for f in range(n):
        if call.method == CM:
            _asserted(bad, f"{tag} frame {f}", NM.check_cm, R, nrm[f], fs[f], call.inputs["points"][f], None, "CM", exp=call.want[f], **kw)
        else:
            _asserted(bad, f"{tag} frame {f}", NM.assert_nan_equal_bits, nrm[f], call.want[f][0], np.ones((H, W), bool), "bilateral")
    if not torch.equal(pts.view(torch.int32), before.view(torch.int32)):
        bad.append(f"{tag}: the points were written")


def _run_nasp(torch, o, c, call, tag, bad, got):
    R = refs().nasp
    i = {k: _dev(torch, v) for k, v in call.inputs.items()}
    if call.entry == "single":
        o.Segmentation(i["bgr"][0], i["points"][0], i["normals"][0], *call.sig, call.iteration)
    else:
        o.segmentation_batch(i["bgr"], i["points"], i["normals"], *call.sig, call.iteration)
    got[tag] = [NC.read_outputs(R, o, None if call.n == 1 else f) for f in range(call.n)]
    for f in range(call.n):
        _asserted(bad, f"{tag} frame {f}", NC.assert_identical, got[tag][f], call.want[f], "NASP")


def _les_outputs(o, n, size, nc):
    W, H = size
    return dict(merged_label=_frames(o.getMergedClusterLabel_Device(), n, (H, W)), merged_nd=_frames(o.getMergedClusterND_Device(), n, (H, W, 4)),
                size=_frames(o.getMergedClusterSize_Device(), n, (nc,)), variance=_frames(o.getMergedClusterVariance_Device(), n, (nc,)))


def _run_les(torch, o, c, call, tag, bad, got):
    i = {k: _dev(torch, v) for k, v in call.inputs.items()}
    if call.entry == "single":
        o.labelImage(i["normals"][0], i["labels"][0], i["centers"][0])
    else:
        o.label_image_batch(i["normals"], i["labels"], i["centers"])
    got[tag] = _les_outputs(o, call.n, c.size, call.nc)
    for f in range(call.n):
        counts = LC.diff_counts({k: v[f] for k, v in got[tag].items()}, call.want[f])
        if any(counts.values()):
            bad.append(f"{tag} frame {f}: differing elements {counts}")


def _proj_compare(R, bad, what, fitted, optimized, exp, window):
    cmp = R.compare(fitted, optimized, exp, window)
    if cmp["plane_fitted"] or cmp["strict"] or cmp["hole"] or cmp["band"] or cmp["xy"]:
        bad.append(f"{what}: {cmp}")
    if window == 1:
        k = int(R.differing(optimized, exp["optimized"]).sum())
        if k:
            bad.append(f"{what}: window 1, {k} optimized elements differ")


def _run_proj(torch, o, c, call, tag, bad, got):
    R, (W, H), n = refs().proj, c.size, call.n
    i = {k: _dev(torch, v) for k, v in call.inputs.items()}
    order = ("nd", "labels", "variance", "points", "size")
    if call.entry == "single":
        o.PlaneProjection(*[i[k][0] for k in order])
    else:
        o.plane_projection_batch(*[i[k] for k in order])
    got[tag] = dict(plane_fitted=_frames(o.GetPlaneFitted3D_Device(), n, (H, W, 3)), optimized=_frames(o.GetOptimized3D_Device(), n, (H, W, 3)))
    for f in range(n):
        _proj_compare(R, bad, f"{tag} frame {f}", got[tag]["plane_fitted"][f], got[tag]["optimized"][f], call.want[f], c.params["window_size"])


def _run_chain(torch, F_, o, c, call, tag, bad, got):
    """the six stages by hand on six objects (tests/test_gpu_enh.py::by_hand), each of the four plane stages against its
    restatement on the device's own output of the stage before; then KinectDepthEnhancement against the by-hand bytes"""
    R, (W, H), n, k = refs(), c.size, call.n, c.rows * c.cols
    K = camera_matrix(W, H)
    depth, bgr = _dev(torch, call.inputs["depth"]), _dev(torch, call.inputs["bgr"])
    made = []

    def new(obj):
        made.append(obj)
        return obj

    try:
        jbf = new(F_.JointBilateralFilter(W, H, max_batch=n))
        filtered = jbf.process_batch(depth, bgr)
        conv = new(F_.DimensionConvertor())
        conv.setCameraParameters(K, W, H)
        pts = torch.empty((n, H, W, 3), dtype=torch.float32, device="cuda")
        conv.projectiveToReal(filtered, pts)
        gen = new(F_.NormalMapGenerator(W, H, max_batch=n))
        gen.setNormalEstimationMethods(gen.CM)
        gen.generateNormalMapBatch(n, pts)
        h_pts, h_bgr = pts.cpu().numpy(), call.inputs["bgr"]
        h_nrm, h_fs = _frames(gen.getNormalMap(), n, (H, W, 3)), _frames(gen.getSmoothingMap(), n, (H, W))
        for f in range(n):
            _asserted(bad, f"{tag} normals frame {f}", NM.check_cm, R.normals, h_nrm[f], h_fs[f], h_pts[f], None, "CM")
        nasp = new(F_.NormalAdaptiveSuperpixel(W, H, max_batch=n))
        nasp.SetParametor(c.rows, c.cols, K)
        nasp.segmentation_batch(bgr, pts, gen.getNormalMap().reshape(n, H, W, 3), *NASP_REF_CALL, 1)
        seg = [NC.read_outputs(R.nasp, nasp, None if n == 1 else f) for f in range(n)]
        for f in range(n):
            exp = R.nasp.segmentation(h_bgr[f], h_pts[f], h_nrm[f], c.rows, c.cols, K, *NASP_REF_CALL, 1)
            _asserted(bad, f"{tag} NASP frame {f}", NC.assert_identical, seg[f], exp, "NASP")
        les = new(F_.LabelEquivalenceSeg(W, H, max_batch=n))
        les.label_image_batch(nasp.getNormalsDevice().reshape(n, k, 3), nasp.getLabelDevice().reshape(n, H, W),
                              nasp.getCentersDevice().reshape(n, k, 3), nasp.getNormalsVarianceDevice().reshape(n, k))
        merged = _les_outputs(les, n, c.size, k)
        for f in range(n):
            exp = R.les.label_image(seg[f]["normals"], seg[f]["labels"], seg[f]["centers"])
            counts = LC.diff_counts({key: v[f] for key, v in merged.items()}, exp)
            if any(counts.values()):
                bad.append(f"{tag} LES frame {f}: differing elements {counts}")
        proj = new(F_.PlaneProjection(W, H, K, max_batch=n))
        proj.plane_projection_batch(les.getMergedClusterND_Device().reshape(n, H, W, 4), les.getMergedClusterLabel_Device().reshape(n, H, W),
                                    les.getMergedClusterVariance_Device().reshape(n, k), pts, les.getMergedClusterSize_Device().reshape(n, k))
        fitted, opt = _frames(proj.GetPlaneFitted3D_Device(), n, (H, W, 3)), _frames(proj.GetOptimized3D_Device(), n, (H, W, 3))
        for f in range(n):
            exp = R.proj.plane_projection(merged["merged_nd"][f], merged["merged_label"][f], merged["variance"][f], h_pts[f], merged["size"][f], K)
            _proj_compare(R.proj, bad, f"{tag} projection frame {f}", fitted[f], opt[f], exp, R.proj.WINDOW_SIZE)
        torch.cuda.synchronize()
    finally:
        for obj in reversed(made):
            obj.close()
    if call.entry == "single":
        o.Process(depth[0], bgr[0])
    else:
        o.process_batch(depth, bgr)
    mine = dict(points=_frames(o.getEdgeEnhanced3DPoints_Device(), n, (H, W, 3)), labels=_frames(o.getLabelDevice(), n, (H, W)),
                merged=_frames(o.getMergedClusterLabel_Device(), n, (H, W)), optimized=_frames(o.getOptimizedPoints_Device(), n, (H, W, 3)))
    hand = dict(points=h_pts, labels=np.stack([s["labels"] for s in seg]), merged=merged["merged_label"], optimized=opt)
    got[tag] = mine
    for key in mine:
        k_ = int(R.proj.differing(mine[key], hand[key]).sum()) if mine[key].dtype == np.float32 else int((mine[key] != hand[key]).sum())
        if k_:
            bad.append(f"{tag}: KinectDepthEnhancement's {key} differ from the six stages by hand in {k_} elements")


def run_case(torch, F_, c):
    """Builds the object of the drawn case c, fills every call's want, runs the calls and compares.  Returns (violations, got):
    a list of strings -- empty: every bar holds -- and what the device gave per call (for a dump)."""
    bad, got = [], {}
    try:
        o = new_object(F_, c)
    except F_._native.KdeError as e:
        return [f"create refused an admitted configuration: {e}"], got
    try:
        want(c)
        for j, call in enumerate(c.calls):
            tag = f"call {j} ({call.entry}, n {call.n})"
            if c.kind == "chain":
                _run_chain(torch, F_, o, c, call, tag, bad, got)
            else:
                dict(normals=_run_normals, nasp=_run_nasp, les=_run_les, proj=_run_proj)[c.kind](torch, o, c, call, tag, bad, got)
    except F_._native.KdeError as e:
        bad.append(f"a call refused an admitted configuration: {e}")
    finally:
        o.close()
    return bad, got
