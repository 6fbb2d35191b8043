"""The rule of GuidedDepthUpsampling as stated in numpy (upsample_cases.py), without a GPU: the properties the issue measured
on its prototype, the tables, the absent taps and the formats.  tests/test_gpu_upsample.py compares the kernel with this
statement byte for byte, so what holds here holds for the kernel."""
import numpy as np

import upsample_cases as UC

F = np.float32


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def test_radius_one_at_equal_sizes_returns_the_input_holes_included():
    name = "identity"
    k = UC.CASES[name]
    t = UC.tables(k.src, k.out, 30.0)
    assert t.sx == 1 and t.sy == 1 and t.gx_of.tolist() == list(range(13)) and t.gy_of.tolist() == list(range(9))
    for d in UC.depth_frames(name, 3):
        b = UC.bgr_frames(name, 1)[0]
        z, filled = UC.upsample(d, b, t, k.out, radius=1)
        with np.errstate(invalid="ignore"):
            valid = (d > 0) & (d < UC.FLT_MAX)
        assert 0 < (~valid).sum() < valid.sum()
        assert np.array_equal(_bits(z), _bits(np.where(valid, d, F(0)).astype(np.float32)))
        assert filled == int(valid.sum())


def test_the_depth_edge_lands_on_the_colour_edge():
    src, out, depth, img = UC.step_scene()
    t = UC.tables(src, out, 10.0)
    for r in (1, 2, 3):
        z, filled = UC.upsample(depth, img, t, out, radius=r)
        assert int(((z > 1100) & (z < 2900)).sum()) == 0, r
        assert filled == 41 * 29 and not (z == 0).any(), r
        assert (z[:, :20] < 1100).all() and (z[:, 20:] > 2900).all(), r


def test_the_guard_removes_the_flying_pixels_of_a_flat_guide():
    src, out, depth, img = UC.step_scene(flat_colour=True)
    t = UC.tables(src, out, 10.0)
    z, filled = UC.upsample(depth, img, t, out, radius=2)
    assert int(((z > 1100) & (z < 2900)).sum()) == 203 and filled == 41 * 29
    z, filled = UC.upsample(depth, img, t, out, radius=2, max_gap=100.0)
    assert int(((z > 1100) & (z < 2900)).sum()) == 0 and filled == 41 * 29
    assert (np.minimum(np.abs(z - 1000), np.abs(z - 3000)) < 0.01).all()    # a mean of equal depths, to the rounding of its sums


def test_the_range_table():
    for sigma in (30.0, 10.0, 1.0, 1e6):
        r = UC.range_table(sigma)
        assert r.dtype == np.float32 and r.shape == (766,)
        assert r[0] == 1
        assert (np.diff(r.astype(np.float64)) <= 0).all()
    r = UC.range_table(1.0)
    zero = np.flatnonzero(r == 0)
    assert zero.size and zero[0] == 15 and (r[zero[0]:] == 0).all()      # exp(-112.5) is below half the smallest denormal, exp(-98) is not
    assert (UC.range_table(1e6) > 0.9999).all()


def test_sigma_one_leaves_holes_where_the_only_similar_taps_are_invalid():
    """two colours 90 apart per channel (k = 270: range is 0 at sigma 1): the right half of the source is invalid, so the right
    half of the output, whose colour only its own taps share, stays empty, and filled says so"""
    src, out = (8, 6), (16, 12)
    t = UC.tables(src, out, 1.0)
    depth = np.full((6, 8), 1500.0, np.float32)
    depth[:, 4:] = 0.0
    img = np.empty((12, 16, 3), np.uint8)
    img[:, :8] = 40
    img[:, 8:] = 130
    z, filled = UC.upsample(depth, img, t, out, radius=2)
    assert (np.abs(z[:, :8] - 1500) < 0.01).all() and (z[:, 8:] == 0).all() and filled == 12 * 8
    t30 = UC.tables(src, out, 200.0)                      # a wide sigma lets the left half's depth leak across
    z, filled = UC.upsample(depth, img, t30, out, radius=2)
    assert (np.abs(z[:, 8:10] - 1500) < 0.01).all() and filled > 12 * 8


def test_invalid_taps_are_absent():
    src, out = (6, 5), (12, 10)
    t = UC.tables(src, out, 30.0)
    img = np.full((10, 12, 3), 99, np.uint8)
    base = np.full((5, 6), 2000.0, np.float32)
    want, filled = UC.upsample(base, img, t, out, radius=1, z_min=400.0, z_max=6000.0)
    assert (np.abs(want - 2000) < 0.01).all() and filled == 120
    for bad in (np.nan, np.inf, -np.inf, 0.0, -0.0, -5.0, 399.0, 400.0, 6000.0, 6500.0):
        d = base.copy()
        d[2, 3] = bad
        z, filled = UC.upsample(d, img, t, out, radius=1, z_min=400.0, z_max=6000.0)
        assert np.isfinite(z).all() and (np.abs(z[z != 0] - 2000) < 0.01).all(), bad   # an absent tap moves no mean of equal depths
        assert filled == int((z != 0).sum()) == 120, bad                     # r = 1 at ratio 2: every pixel has a second tap
    d = base.copy()
    d[:, :] = np.nan
    d[4, 5] = 2000.0
    z, filled = UC.upsample(d, img, t, out, radius=1)          # one sample reaches 2 r / sx = 4 pixels along an axis at most
    assert filled == int((z != 0).sum()) and 0 < filled <= 16 and (np.abs(z[z != 0] - 2000) < 0.01).all()


def test_a_one_pixel_source():
    k = UC.CASES["one_pixel"]
    t = UC.tables(k.src, k.out, 30.0)
    assert t.gx_of.tolist() == [2] and t.gy_of.tolist() == [1]
    img = UC.bgr_frames("one_pixel", 1)[0]
    for r in (1, 2, 4):
        z, filled = UC.upsample(np.array([[1234.5]], np.float32), img, t, k.out, radius=r)
        assert filled == 15 and (z == F(1234.5)).all()
        z, filled = UC.upsample(np.array([[0.0]], np.float32), img, t, k.out, radius=r)
        assert filled == 0 and (z == 0).all()


def test_uint16_in_and_out():
    name = "fraction"
    k = UC.CASES[name]
    t = UC.tables(k.src, k.out, 30.0)
    d = UC.depth_frames(name, 1, integer=True)[0]
    img = UC.bgr_frames(name, 1)[0]
    d16 = d.astype(np.uint16)
    assert np.array_equal(d16.astype(np.float32), d)
    zf, ff = UC.upsample(d, img, t, k.out, z_min=UC.Z_RANGE[0], z_max=UC.Z_RANGE[1])
    zu, fu = UC.upsample(d16, img, t, k.out, z_min=UC.Z_RANGE[0], z_max=UC.Z_RANGE[1])
    assert np.array_equal(_bits(zf), _bits(zu)) and ff == fu                 # (float)u widens exactly
    o16, f16 = UC.upsample(d16, img, t, k.out, z_min=UC.Z_RANGE[0], z_max=UC.Z_RANGE[1], out_dtype=np.uint16)
    assert o16.dtype == np.uint16 and f16 == ff                              # counted before the rounding
    assert np.array_equal(o16, UC.depth_to_u16(zf))
    assert np.abs(o16.astype(np.float64) - zf)[zf != 0].max() <= 0.5
    assert UC.depth_to_u16(np.array([0.5, 1.5, 2.5, 65535.4, 65535.5, np.nan, -3.0], np.float32)).tolist() == [0, 2, 2, 65535, 0, 0, 0]


def test_the_nearest_pixel_tables_take_ties_to_even():
    t = UC.tables((20, 15), (40, 30), 30.0)               # (q + 0.5) * 2 - 0.5 = 2 q + 0.5: every entry is a tie
    assert t.gx_of.tolist() == [2 * q + (2 * q) % 2 for q in range(20)] == [2 * q for q in range(20)]
    t = UC.tables((10, 8), (40, 32), 30.0)                # 4 q + 1.5: between 4 q + 1 and 4 q + 2, to the even one
    assert t.gx_of.tolist() == [4 * q + 2 for q in range(10)] and t.gy_of.tolist() == [4 * q + 2 for q in range(8)]
    t = UC.tables((3, 2), (67, 45), 30.0)
    assert (np.diff(t.gx_of) > 0).all() and 0 <= t.gx_of.min() and t.gx_of.max() <= 66


def test_the_named_cases_cover_what_they_claim():
    for name, k in UC.CASES.items():
        d = UC.depth_frames(name, 3)
        assert d.shape == (3, k.src[1], k.src[0]) and UC.bgr_frames(name, 3).shape == (3, k.out[1], k.out[0], 3)
        assert k.out[0] >= k.src[0] and k.out[1] >= k.src[1]
        if k.src[0] * k.src[1] > 40:
            with np.errstate(invalid="ignore"):
                bad = ~((d > UC.Z_RANGE[0]) & (d < UC.Z_RANGE[1]))
            assert 0.04 < bad.mean() < 0.2, (name, bad.mean())
            assert np.isnan(d).any() and np.isinf(d).any(), name
    tiles = lambda k: -(-k.out[0] // 32) * -(-k.out[1] // 8)
    assert tiles(UC.CASES["row"]) == 19 and tiles(UC.CASES["blocks"]) == 45 and tiles(UC.CASES["quad"]) == 8
