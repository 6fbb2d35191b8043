"""The numpy statement of DepthRegistration (reg_cases.py, Kinect.cpp:71-75) on cases worked out by hand.  No GPU."""
import numpy as np

import reg_cases as RC

F = np.float32
I3 = np.eye(3)


def _K(f, cx, cy):
    return np.array([[f, 0, cx], [0, f, cy], [0, 0, 1]], np.float64)


def test_identity_returns_the_input_where_it_is_valid():
    """R = I, t = 0, equal cameras (with a principal point that is no integer): every valid pixel lands on itself with its
    own z, in point mode and with a one-pixel splat; every invalid pixel leaves a 0.  The range is 400 .. 3000: with the
    default range a denormal z is valid, and its X = xn * z is rounded to the denormal grid, so it need not land on itself"""
    w, h = 13, 9
    K = RC.camera(w, h, 11.7)
    c = RC.calib(K, K, I3, (0, 0, 0))
    for seed in (1, 2):
        lo, hi = F(400), F(3000)
        z = RC.depth_maps(seed, 1, h, w, lo, hi)[0]
        valid = (z > lo) & (z < hi)
        assert 0 < valid.sum() < w * h and np.isnan(z).any() and np.isinf(z).any() and (z < 0).any()
        want = np.where(valid, z, F(0))
        for splat in (0, 1):
            got, filled = RC.statement(z, c, (w, h), lo, hi, max_splat=splat)
            assert got.dtype == np.float32 and got.tobytes() == want.tobytes(), splat
            assert filled == int(valid.sum())
        zi = RC.depth_maps(seed, 1, h, w, integer=True)[0].astype(np.uint16)
        assert (zi == 0).any() and (zi == 65535).any()
        for splat in (0, 1):
            got, filled = RC.statement(zi, c, (w, h), max_splat=splat, out_dtype=np.uint16)
            assert got.dtype == np.uint16 and np.array_equal(got, zi) and filled == int((zi > 0).sum())


def test_a_plane_shifts_by_twelve_and_a_half_pixels_and_ties_go_to_even():
    """z = 1000, t = (25, 0, 0), fx = 500: every pixel moves by 500 * 25 / 1000 = 12.5 columns exactly, so every uc is a tie:
    an even u goes to u + 12, an odd u to u + 13 -- only even columns are reached, each by two sources of the same depth"""
    w, h = 40, 3
    K = _K(500.0, 8.0, 1.0)
    c = RC.calib(K, K, I3, (25, 0, 0))
    z = np.full((h, w), 1000, np.float32)
    u = np.arange(w, dtype=np.float32)
    uc, vc, Zc, ok = RC.project(u, np.zeros(w, np.float32), z[0], c, F(0), RC.FLT_MAX)
    assert np.array_equal(uc, u + F(12.5)) and ok.all() and np.all(Zc == 1000)        # the ties are exact
    got, filled = RC.statement(z, c, (w, h))
    cols = np.arange(w)
    want = np.where((cols >= 12) & (cols % 2 == 0), F(1000), F(0))
    assert np.array_equal(got, np.broadcast_to(want, (h, w)))
    assert filled == h * 14
    kept, iu, iv, _ = RC.centre_targets(z, c, (w, h))
    assert iu[0, :6].tolist() == [12, 14, 14, 16, 16, 18] and kept[0, :27].all() and not kept[0, 28:].any()
    # rows tie too when the shift is vertical: t = (0, 25, 0)
    zt = np.full((w, h), 1000, np.float32)
    gt, _ = RC.statement(zt, RC.calib(_K(500.0, 1.0, 8.0), _K(500.0, 1.0, 8.0), I3, (0, 25, 0)), (h, w))
    assert np.array_equal(gt, got.T)


def test_the_near_surface_wins_in_any_order():
    """a square at 1000 in front of a plane at 2000, t = (40, 0, 0), fx = 500: the square moves by 20 columns, the plane by 10,
    so the square's columns 10..15 and the plane's columns 20..25 land on the targets 30..35, where the square wins"""
    w, h = 48, 8
    K = _K(500.0, 24.0, 4.0)
    c = RC.calib(K, K, I3, (40, 0, 0))
    z = np.full((h, w), 2000, np.float32)
    z[2:6, 10:16] = 1000
    kept, iu, _, _ = RC.centre_targets(z, c, (w, h))
    assert iu[3, 10:16].tolist() == iu[3, 20:26].tolist() == list(range(30, 36))
    base = RC.keys(z, c, (w, h))
    got, filled = RC.finalise(base)
    assert np.all(got[2:6, 30:36] == 1000) and np.all(got[0:2, 30:36] == 2000) and np.all(got[:, :10] == 0)
    # the square's old place shows the plane from columns 0..5, which nothing hides; columns 20..25 of its rows stay empty
    assert np.all(got[2:6, 10:16] == 2000) and np.all(got[2:6, 20:26] == 0)
    n = w * h
    rng = np.random.default_rng(3)
    for order in (np.arange(n)[::-1], rng.permutation(n), rng.permutation(n)):
        assert np.array_equal(RC.keys(z, c, (w, h), order=order), base)
        assert np.array_equal(RC.keys(z, c, (w, h), max_splat=2, order=order), RC.keys(z, c, (w, h), max_splat=2))
    # a plain store in arrival order would not do: the plane offered last overwrites the square
    last = np.full(n, RC.EMPTY, np.uint32)
    kept, iu, iv, Zc = RC.centre_targets(z, c, (w, h))
    last[(iv * w + iu)[kept]] = Zc.view(np.uint32)[kept]
    assert not np.array_equal(last.reshape(h, w), base)


def _upscale():
    wd, hd, wc, hc = 8, 6, 16, 12
    Kd = _K(10.0, 3.5, 2.5)
    Kc = _K(20.0, 7.5, 5.5)                      # pixel centre u of the depth camera is seen at 2 u + 0.5
    return wd, hd, wc, hc, RC.calib(Kd, Kc, I3, (0, 0, 0))


def test_a_2x_upscale_in_point_mode_leaves_holes():
    wd, hd, wc, hc, c = _upscale()
    z = np.full((hd, wd), 1500, np.float32)
    got, filled = RC.statement(z, c, (wc, hc))
    assert filled == wd * hd and filled < wc * hc          # one target per source: three quarters of the targets are holes
    assert ((got == 0).sum(), (got == 1500).sum()) == (wc * hc - wd * hd, wd * hd)


def test_a_2x_upscale_with_splat_4_leaves_no_hole_on_a_plane():
    """the footprint of source pixel u is [2 u - 0.5, 2 u + 1.5): the columns 2 u and 2 u + 1; abutting footprints tile the
    line, so every target inside the warped footprint of the frame is reached"""
    wd, hd, wc, hc, c = _upscale()
    z = np.full((hd, wd), 1500, np.float32)
    zb = RC.keys(z, c, (wc, hc), max_splat=4)
    # the warped footprint of the whole frame, from the statement's own projection of its outer corners
    ua, va, _, _ = RC.project(F(-0.5), F(-0.5), F(1500), c, F(0), RC.FLT_MAX)
    ub, vb, _, _ = RC.project(F(wd - 0.5), F(hd - 0.5), F(1500), c, F(0), RC.FLT_MAX)
    i0, i1 = max(int(np.ceil(ua)), 0), min(int(np.ceil(ub)) - 1, wc - 1)
    j0, j1 = max(int(np.ceil(va)), 0), min(int(np.ceil(vb)) - 1, hc - 1)
    assert (i0, i1, j0, j1) == (0, wc - 1, 0, hc - 1)
    box = zb[j0:j1 + 1, i0:i1 + 1]
    share = (box != RC.EMPTY).sum() / box.size
    assert share == 1
    assert RC.finalise(zb)[1] == wc * hc
    # a splat cut to one column and one row is the first of each span: holes again
    assert RC.finalise(RC.keys(z, c, (wc, hc), max_splat=1))[1] == wd * hd
    # and the same on a tilted frame with a shifted camera: every target inside the footprint of the valid region is reached
    wd, hd, wc, hc = 32, 24, 80, 60
    c = RC.calib(RC.camera(wd, hd, 30.0), RC.camera(wc, hc, 75.0), I3, (0, 0, 0))
    z = np.full((hd, wd), 1200, np.float32)
    zb = RC.keys(z, c, (wc, hc), max_splat=4)
    ua, va, _, _ = RC.project(F(-0.5), F(-0.5), F(1200), c, F(0), RC.FLT_MAX)
    ub, vb, _, _ = RC.project(F(wd - 0.5), F(hd - 0.5), F(1200), c, F(0), RC.FLT_MAX)
    i0, i1 = max(int(np.ceil(ua)), 0), min(int(np.ceil(ub)) - 1, wc - 1)
    j0, j1 = max(int(np.ceil(va)), 0), min(int(np.ceil(vb)) - 1, hc - 1)
    box = zb[j0:j1 + 1, i0:i1 + 1]
    assert box.size > 0.9 * wc * hc and (box != RC.EMPTY).sum() / box.size == 1
    assert RC.finalise(RC.keys(z, c, (wc, hc)))[1] == wd * hd < box.size


def test_the_validity_rule_at_its_edges_and_the_rounding_to_uint16():
    z_min, z_max = F(400), F(3000)
    K = _K(50.0, 6.0, 0.0)
    c = RC.calib(K, K, I3, (0, 0, 0))
    z = RC.special_z(z_min, z_max)[None, :]
    got, filled = RC.statement(z, c, (z.size, 1), z_min, z_max)
    # NaN, +-inf, 0, -0, negatives, z_min, its upper neighbour (valid), its lower, z_max, its lower neighbour (valid), its upper
    want_valid = [False] * 8 + [True, False, False, True, False]
    assert (got != 0).reshape(-1).tolist() == want_valid and filled == 2
    assert RC.depth_to_u16(np.array([0.5, 1.5, 2.5, 0.49, 65535.4, 65535.5, np.nan, np.inf, -3.0], np.float32)).tolist() == \
        [0, 2, 2, 0, 65535, 0, 0, 0, 0]
    # the count is taken on the keys: a depth that rounds to 0 as uint16 still counts
    zs = np.full((1, 13), 0.3, np.float32)
    d, filled = RC.statement(zs, c, (13, 1), out_dtype=np.uint16)
    assert filled == 13 and not d.any()


def test_color_to_depth_has_no_occlusion_test():
    w, h = 48, 8
    K = _K(500.0, 24.0, 4.0)
    c = RC.calib(K, K, I3, (40, 0, 0))
    z = np.full((h, w), 2000, np.float32)
    z[2:6, 10:16] = 1000
    z[0, 0] = 0
    bgr = RC.bgr_images(1, 1, h, w)[0]
    got = RC.color_to_depth(z, bgr, c)
    assert got.shape == (h, w, 3) and got.dtype == np.uint8
    assert np.array_equal(got[3, 10:16], bgr[3, 30:36]) and np.array_equal(got[3, 20:26], bgr[3, 30:36])   # hidden, coloured alike
    assert not got[0, 0].any() and not got[:, 38:].any() and np.array_equal(got[0, 1:38], bgr[0, 11:48])
