"""The numpy statement of LensUndistortion (undist_cases.py) and its named cases, checked from the statement alone.  No GPU."""
import numpy as np
import pytest

import undist_cases as UC

F = np.float32


def _modes(name):
    zr = UC.case_range(name)
    return [(zr, 0, F(0)), (zr, 1, F(UC.CASES[name].max_gap))]


def test_the_cases_are_what_their_reasons_say():
    assert UC.IDS == ["barrel", "rational_tangential", "identity", "half_ties", "one_pixel", "sliver", "tail", "blocks"]
    assert UC.CASES["blocks"].out[0] * UC.CASES["blocks"].out[1] > 8192
    shapes = {n: (c.src, c.out) for n, c in UC.CASES.items()}
    assert shapes["barrel"] == ((37, 23), (41, 19)) and shapes["rational_tangential"] == ((37, 23), (37, 23))
    assert shapes["one_pixel"] == ((1, 1), (1, 1)) and shapes["sliver"] == ((5, 3), (3, 5)) and shapes["tail"] == ((64, 4), (257, 1))
    assert all(c.why for c in UC.CASES.values())
    b = UC.CASES["barrel"]
    assert b.dist[0] < 0 and b.src[0] % 4 and b.out[0] % 4 and b.src != b.out
    assert all(v != 0 for v in UC.CASES["rational_tangential"].dist) and len(UC.CASES["rational_tangential"].dist) == 8
    rt = UC.case_calib("rational_tangential")
    assert all(float(v) != np.rint(float(v)) for v in (rt.cx, rt.cy, rt.cxn, rt.cyn))
    assert not any(UC.CASES["identity"].dist) and UC.CASES["identity"].Knew is None
    # barrel: an output pixel on each colour path, and corners that leave the source
    c = UC.case_calib("barrel")
    _, taps = UC.color_parts(UC.bgr_frames("barrel")[0], c, b.out)
    assert (taps == 0).any() and ((taps > 0) & (taps < 4)).any() and (taps == 4).any()
    ow, oh = b.out
    corners = taps.reshape(oh, ow)[[0, 0, -1, -1], [0, -1, 0, -1]]
    assert not corners.any()
    # the depth frames carry what the rule must not mishandle
    for name in ("barrel", "rational_tangential", "half_ties", "tail"):
        d = UC.depth_frames(name, 2)
        assert np.isnan(d).any() and np.isposinf(d).any() and np.isneginf(d).any() and (d < 0).any() and (d == 0).any()
        u = UC.depth_frames(name, 2, integer=True)
        assert (u == 0).any() and (u == 65535).any() and np.array_equal(u, np.rint(u)) and u.min() >= 0 and u.max() <= 65535
        gap = F(UC.CASES[name].max_gap)
        clean = UC.depth_frames(name, 1, specials=False)[0]
        dx = np.abs(np.diff(clean, axis=1))
        assert (dx > gap).any() and (dx < gap).any() and dx[dx < gap].max() < 3.0          # a step above, a ramp below max_gap
    # some depth case has a pixel on every branch of the guard (here: each of the two distorted 37 x 23 cases does)
    for name in ("barrel", "rational_tangential"):
        k = UC.CASES[name]
        zr = UC.case_range(name)
        for d in (UC.depth_frames(name)[0], UC.depth_frames(name, integer=True)[0].astype(np.uint16)):
            p = UC.depth_parts(d, UC.case_calib(name), k.out, *zr, interp=1, max_gap=k.max_gap)
            assert all(p[branch].any() for branch in ("blended", "hole", "gap", "border")), name
            assert 0 < p["kept"].sum() < p["kept"].size
    # half_ties: every even column and row is an exact tie, to even and to odd integers
    h = UC.CASES["half_ties"]
    us, vs = UC.source_points(UC.case_calib("half_ties"), h.out)
    ow, oh = h.out
    us, vs = us.reshape(oh, ow), vs.reshape(oh, ow)
    i = np.arange(ow, dtype=np.float32)
    assert np.array_equal(us[0], i / F(2) + F(0.5)) and np.array_equal(vs[:, 0], np.arange(oh, dtype=np.float32) / F(2) + F(0.5))
    ties = us[0][us[0] - np.floor(us[0]) == F(0.5)]
    assert ties.size == ow // 2
    down, up = np.floor(ties) % 2 == 0, np.floor(ties) % 2 == 1      # a tie goes down to an even floor, up from an odd one
    assert down.any() and up.any()
    assert np.array_equal(np.rint(ties)[down], np.floor(ties)[down]) and np.array_equal(np.rint(ties)[up], np.floor(ties)[up] + 1)
    p = UC.depth_parts(UC.depth_frames("half_ties", specials=False)[0], UC.case_calib("half_ties"), h.out, interp=1, max_gap=h.max_gap)
    assert p["blended"].any()


def test_identity_returns_the_source_bytes():
    """all coefficients zero and K_new NULL.  With the case's dyadic K the map is exact (us == i, vs == j), so every mode returns
    the source: colour byte for byte, depth wherever it is valid (0 elsewhere), and a frame without invalid samples whole.
    With a K that is not dyadic us differs from i by rounding only (a few units of 2^-24 times the coordinate), far below the
    half unit that could change a rounded uint8, the nearest pixel or a depth rounded to uint16: those results are the
    source's as well"""
    name = "identity"
    k = UC.CASES[name]
    c = UC.case_calib(name)
    ow, oh = k.out
    us, vs = UC.source_points(c, k.out)
    jj, ii = np.mgrid[0:oh, 0:ow]
    assert np.array_equal(us, ii.reshape(-1).astype(np.float32)) and np.array_equal(vs, jj.reshape(-1).astype(np.float32))
    bgr = UC.bgr_frames(name)[0]
    assert UC.color(bgr, c, k.out).tobytes() == bgr.tobytes()
    zr = UC.case_range(name)
    for interp in (0, 1):
        d = UC.depth_frames(name)[0]
        valid = (d > zr[0]) & (d < zr[1])
        assert 0 < valid.sum() < d.size
        got, filled = UC.depth(d, c, k.out, *zr, interp=interp, max_gap=k.max_gap)
        assert got.tobytes() == np.where(valid, d, F(0)).tobytes() and filled == int(valid.sum())
        whole = UC.depth_frames(name, specials=False)[0]
        got, filled = UC.depth(whole, c, k.out, *zr, interp=interp, max_gap=k.max_gap)
        assert got.tobytes() == whole.tobytes() and filled == whole.size
        u = UC.depth_frames(name, integer=True)[0].astype(np.uint16)
        got, filled = UC.depth(u, c, k.out, interp=interp, max_gap=k.max_gap, out_dtype=np.uint16)
        assert got.dtype == np.uint16 and got.tobytes() == u.tobytes() and filled == int((u > 0).sum())
    # a camera that is not dyadic
    K = UC.K3(11.7, 11.9, 6.3, 3.8)
    c2 = UC.calib(K, (0.0,) * 8)
    us, vs = UC.source_points(c2, k.out)
    err = max(np.abs(us - ii.reshape(-1)).max(), np.abs(vs - jj.reshape(-1)).max())
    assert 0 < err < 1e-5
    assert UC.color(bgr, c2, k.out).tobytes() == bgr.tobytes()
    d = UC.depth_frames(name)[0]
    valid = (d > zr[0]) & (d < zr[1])
    assert UC.depth(d, c2, k.out, *zr)[0].tobytes() == np.where(valid, d, F(0)).tobytes()
    u = UC.depth_frames(name, integer=True)[0].astype(np.uint16)
    for interp in (0, 1):
        assert UC.depth(u, c2, k.out, interp=interp, max_gap=k.max_gap, out_dtype=np.uint16)[0].tobytes() == u.tobytes()


def _model64(c, out_size):
    """the model from its definition (OpenCV's documentation of the rational model), in binary64, written on its own:
    x' = x (1 + k1 r^2 + k2 r^4 + k3 r^6) / (1 + k4 r^2 + k5 r^4 + k6 r^6) + 2 p1 x y + p2 (r^2 + 2 x^2), y' likewise with
    p1 (r^2 + 2 y^2) + 2 p2 x y; u = fx x' + cx, v = fy y' + cy"""
    ow, oh = out_size
    k1, k2, p1, p2, k3, k4, k5, k6 = (float(v) for v in c.k)
    v, u = np.mgrid[0:oh, 0:ow].astype(np.float64)
    x = (u - float(c.cxn)) / float(c.fxn)
    y = (v - float(c.cyn)) / float(c.fyn)
    r = np.hypot(x, y)
    radial = (1.0 + k1 * r ** 2 + k2 * r ** 4 + k3 * r ** 6) / (1.0 + k4 * r ** 2 + k5 * r ** 4 + k6 * r ** 6)
    xp = x * radial + 2.0 * p1 * x * y + p2 * (r ** 2 + 2.0 * x ** 2)
    yp = y * radial + p1 * (r ** 2 + 2.0 * y ** 2) + 2.0 * p2 * x * y
    return (float(c.fx) * xp + float(c.cx)).reshape(-1), (float(c.fy) * yp + float(c.cy)).reshape(-1)


MEASURED_MAP_ERROR = 1.4e-5      # pixels: the largest |float32 statement - binary64 model| over the cases, measured on the CPU


def test_the_float32_map_agrees_with_the_model_in_binary64():
    """a swapped p1 / p2 or a wrong power of r moves the map of the case with every coefficient by a tenth of a pixel to
    more than a pixel (the probes below: 0.40, 1.75 and 0.12 px); rounding moves it by MEASURED_MAP_ERROR.  The bound is eight
    times the measured value."""
    worst = 0.0
    for name in UC.IDS:
        c = UC.case_calib(name)
        us, vs = UC.source_points(c, UC.CASES[name].out)
        u64, v64 = _model64(c, UC.CASES[name].out)
        worst = max(worst, np.abs(us - u64).max(), np.abs(vs - v64).max())
    print("largest difference between the float32 map and the binary64 model:", worst)
    assert worst <= 8 * MEASURED_MAP_ERROR
    assert worst >= MEASURED_MAP_ERROR / 8          # the recorded figure is the measured one, not a loose guess
    # what the bound is there to catch, on the case with every coefficient: each mistake is far above it
    name = "rational_tangential"
    c = UC.case_calib(name)
    u64, v64 = _model64(c, UC.CASES[name].out)
    k = c.k.copy()
    for wrong in (k[[0, 1, 3, 2, 4, 5, 6, 7]], k[[1, 0, 2, 3, 4, 5, 6, 7]], k[[0, 1, 2, 3, 4, 6, 5, 7]]):   # p1 <-> p2, k1 <-> k2, k4 <-> k5
        us, vs = UC.source_points(c._replace(k=wrong), UC.CASES[name].out)
        assert max(np.abs(us - u64).max(), np.abs(vs - v64).max()) > 0.1                       # pixels: 7000 times the rounding


@pytest.mark.parametrize("name", UC.IDS)
def test_the_order_of_evaluation_changes_nothing(name):
    """every output pixel is a function of the source frame and its own coordinates: evaluated in any order, alone or together"""
    k = UC.CASES[name]
    c = UC.case_calib(name)
    ow, oh = k.out
    n = ow * oh
    rng = np.random.default_rng(5)
    bgr = UC.bgr_frames(name)[0]
    base_c = UC.color(bgr, c, k.out).reshape(n, 3)
    for perm in (np.arange(n)[::-1], rng.permutation(n)):
        assert np.array_equal(UC.color(bgr, c, k.out, pixels=perm), base_c[perm])
        for d in (UC.depth_frames(name)[0], UC.depth_frames(name, integer=True)[0].astype(np.uint16)):
            for zr, interp, gap in _modes(name):
                for out_dtype in (np.float32, np.uint16):
                    base, filled = UC.depth(d, c, k.out, *zr, interp=interp, max_gap=gap, out_dtype=out_dtype)
                    got, f2 = UC.depth(d, c, k.out, *zr, interp=interp, max_gap=gap, out_dtype=out_dtype, pixels=perm)
                    assert got.tobytes() == base.reshape(-1)[perm].tobytes() and f2 == filled
    one = UC.color(bgr, c, k.out, pixels=np.array([n - 1]))
    assert np.array_equal(one[0], base_c[n - 1])


def test_the_sampling_rules_on_cases_worked_out_by_hand():
    """half_ties: output pixel (i, j) shows the source point (i / 2 + 0.5, j / 2 + 0.5)"""
    name = "half_ties"
    k = UC.CASES[name]
    c = UC.case_calib(name)
    sw, sh = k.src
    ow, oh = k.out
    z = (F(1000) + F(4) * np.arange(sw, dtype=np.float32))[None, :].repeat(sh, 0)      # a ramp of 4 mm per column
    near, filled = UC.depth(z, c, k.out)
    # i = 0: us = 0.5 -> column 0 (even); i = 2: 1.5 -> 2; i = 4: 2.5 -> 2; i = 6: 3.5 -> 4; odd i: us = (i + 1) / 2 exactly
    assert near[0, :8].tolist() == [1000, 1004, 1008, 1008, 1008, 1012, 1016, 1016] and filled == ow * oh
    blend, _ = UC.depth(z, c, k.out, interp=1, max_gap=50.0)
    assert blend[0, :6].tolist() == [1002, 1004, 1006, 1008, 1010, 1012]              # ax = 0.5 halves the step
    # a step of 400 mm between columns 5 and 6: refused for the gap, the nearest sample instead (us = 5.5 ties to 6)
    zs = z.copy()
    zs[:, 6:] -= F(400)
    blend, _ = UC.depth(zs, c, k.out, interp=1, max_gap=50.0)
    assert blend[0, 10] == zs[0, 6] and blend[0, 8] == F(1018)
    # a hole at column 3: the pixels whose taps touch it take the nearest rule, and the hole itself stays 0
    zh = z.copy()
    zh[:, 3] = 0
    blend, filled = UC.depth(zh, c, k.out, interp=1, max_gap=50.0)
    assert blend[0, 4] == z[0, 2] and blend[0, 5] == 0 and blend[0, 6] == z[0, 4] and filled < ow * oh
    # colour: a tap outside the source is black, and us in (-1, 0) still blends with it
    bgr = np.full((sh, sw, 3), 200, np.uint8)
    cc = UC.calib(k.K, k.dist, UC.K3(16.0, 8.0, 1.5, 0.0))                                # us = (i - 1.5) / 2 + 0.5: i = 0 -> -0.25
    got = UC.color(bgr, cc, k.out)
    assert got[4, 0].tolist() == [150, 150, 150] and got[4, 2].tolist() == [200, 200, 200]
    assert UC.depth_to_u16(np.array([0.5, 1.5, 2.5, 65535.4, 65535.5, np.nan, -3.0], np.float32)).tolist() == [0, 2, 2, 65535, 0, 0, 0]
    # filled counts before the rounding to uint16: 0.3 mm is a valid depth that rounds to 0
    d, filled = UC.depth(np.full((sh, sw), 0.3, np.float32), c, k.out, out_dtype=np.uint16)
    assert filled == ow * oh and not d.any()
