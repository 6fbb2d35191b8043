"""The statement of DepthHoleFilling's rule (holefill_cases.py) has the properties the rule promises.  No GPU, no library: the
GPU tests compare the kernels with this statement on bytes, so what is checked here is what they inherit."""
import numpy as np
import pytest

import holefill_cases as HC

F = np.float32
ZR = HC.Z_RANGE


def _tables(name, radius, **over):
    p = HC.params(name, **over)
    return HC.space_table(radius, p["sigma_space"]), HC.range_table(p["sigma_color"])


def _run(name, radius, depth, bgr, zr=ZR, **over):
    p = HC.params(name, **over)
    space, rng = HC.space_table(radius, p["sigma_space"]), HC.range_table(p["sigma_color"])
    kw = {k: v for k, v in p.items() if k not in ("sigma_space", "sigma_color")}
    return HC.fill_parts(depth, bgr, space, rng, radius=radius, z_min=zr[0], z_max=zr[1], **kw)


def test_the_tables():
    s = HC.space_table(2, 2.0)
    assert s.shape == (5, 5) and s.dtype == np.float32 and s[2, 2] == 1.0
    assert s[2, 3] == F(np.exp(-1.0 / 8.0)) and s[0, 0] == F(np.exp(-1.0)) and (s == s.T).all() and (s == s[::-1, ::-1]).all()
    r = HC.range_table(30.0)
    assert r.shape == (766,) and r[0] == 1.0 and r[30] == F(np.exp(-0.5)) and (np.diff(r.astype(np.float64)) <= 0).all()
    one = HC.range_table(1.0)
    assert one[14] > 0 and (one[15:] == 0).all()


def test_the_cases_are_what_their_names_say():
    for name, case in HC.CASES.items():
        w, h = case.size
        d, d16, g = HC.depth_frames(name), HC.depth_frames(name, integer=True), HC.bgr_frames(name)
        assert d.shape == d16.shape == (3, h, w) and g.shape == (3, h, w, 3) and g.dtype == np.uint8
        assert (d16[np.isfinite(d16)] == np.rint(d16[np.isfinite(d16)])).all() and np.isfinite(d16).all() and d16.min() >= 0 and d16.max() <= 65535
        assert not (d[0] == d[1]).all() and not (g[0] == g[1]).all()
        holes = [int((HC.sanitise(f, *ZR) == 0).sum()) for f in d]
        if name == "identity":
            assert holes == [0, 0, 0]
        elif name == "one_pixel":
            assert holes == [1, 1, 1] and not np.isfinite(d[1:]).any()
        elif name == "speck":
            assert holes == [w * h - 1] * 3
        else:
            assert all(0 < k < w * h for k in holes)
            assert not np.isfinite(d).all() and (d[np.isfinite(d)] < 0).any() and (d > ZR[1]).any()    # NaN, +-inf, out of range
            assert (d != np.rint(d))[np.isfinite(d)].any()                                              # fractional depths
    assert HC.BAND[0] < HC.TILE[0] < HC.BAND[1] and HC.TWINS_BAND[0] < HC.TILE[0] < HC.TWINS_BAND[1]     # across a tile border
    assert HC.ISLAND[1].stop - HC.ISLAND[1].start > 2 * HC.BASE["iterations"] * 2


@pytest.mark.parametrize("name", HC.IDS)
def test_valid_pixels_keep_their_bytes(name):
    case = HC.CASES[name]
    for integer in (False, True):
        d = HC.depth_frames(name, integer=integer)
        d = d.astype(np.uint16) if integer else d
        g = HC.bgr_frames(name)
        for radius in case.radii:
            for gap, rule in HC.GUARDS:
                for f in range(3):
                    r = _run(name, radius, d[f], g[f], max_gap=gap, gap_rule=rule)
                    z0 = HC.sanitise(d[f], *ZR)
                    held = z0 > 0
                    assert r["z"][held].tobytes() == z0[held].tobytes()
                    assert (r["pass_of"][held] == 0).all() and (r["pass_of"][~held] != 0).all()
                    assert np.isfinite(r["z"]).all() and (r["z"] >= 0).all()
                    assert ((r["z"] == 0) == (r["pass_of"] == 255)).all()
                    assert r["filled"] + r["remaining"] == int((~held).sum())
                    assert r["pass_of"][r["pass_of"] != 255].max(initial=0) <= HC.params(name)["iterations"]
                    if name == "identity":
                        assert r["z"].tobytes() == z0.tobytes() and r["filled"] == 0 and r["remaining"] == 0
                    if name == "one_pixel":
                        assert r["filled"] == 0 and r["remaining"] == 1 and r["pass_of"][0, 0] == 255
                    if name == "island":
                        assert r["remaining"] > 0 and (r["z"][HC.ISLAND][17:19, 17:19] == 0).all()


@pytest.mark.parametrize("radius", (1, 2, 3))
def test_pass_of_on_speck_is_the_chessboard_distance_over_r(radius):
    w, h = HC.CASES["speck"].size
    d, g = HC.depth_frames("speck"), HC.bgr_frames("speck")
    n = HC.params("speck")["iterations"]
    y, x = np.mgrid[0:h, 0:w]
    for f, (sx, sy) in enumerate(HC.SPECKS):
        r = _run("speck", radius, d[f], g[f])
        steps = -(-np.maximum(np.abs(x - sx), np.abs(y - sy)) // radius)            # ceil(distance / r)
        want = np.where(steps > n, 255, steps).astype(np.uint8)
        assert (r["pass_of"] == want).all()
        assert r["filled"] == int(((want >= 1) & (want != 255)).sum()) and r["remaining"] == int((want == 255).sum()) > 0


@pytest.mark.parametrize("name", ("blocks", "border", "band"))
def test_n_passes_then_m_more_are_n_plus_m(name):
    """at the default z_min / z_max: validity is z > 0 on the state and nothing else"""
    d, g = HC.depth_frames(name), HC.bgr_frames(name)
    zr = (F(0), HC.FLT_MAX)
    for radius in (1, 2):
        for gap, rule in HC.GUARDS:
            whole = _run(name, radius, d[0], g[0], zr, iterations=8, max_gap=gap, gap_rule=rule)
            for first in (1, 3, 5):
                a = _run(name, radius, d[0], g[0], zr, iterations=first, max_gap=gap, gap_rule=rule)
                b = _run(name, radius, a["z"], g[0], zr, iterations=8 - first, max_gap=gap, gap_rule=rule)
                assert b["z"].tobytes() == whole["z"].tobytes()
                assert a["filled"] + b["filled"] == whole["filled"] and b["remaining"] == whole["remaining"]
                later = np.where((b["pass_of"] >= 1) & (b["pass_of"] != 255), b["pass_of"] + first, b["pass_of"])
                assert (np.where(a["pass_of"] == 255, later, a["pass_of"]) == whole["pass_of"]).all()


def test_sigma_color_one_fills_nothing_without_a_tap_of_the_exact_colour():
    """a noisy guide whose colours are k = 0 or k >= 15 apart (HC.stepped_guide): range[15] == 0 at sigma_color 1, so a tap
    of another colour is absent by w > 0 although its depth is valid, and a hole with fewer than min_taps valid taps of its
    exact colour stays"""
    name, radius = "blocks", 2
    d = HC.depth_frames(name)[0]
    g = HC.stepped_guide(d.shape)
    one = _run(name, radius, d, g, sigma_color=1.0, iterations=1)
    z0 = HC.sanitise(d, *ZR)
    h, w = z0.shape
    zp = np.zeros((h + 4, w + 4), np.float32)
    zp[2:-2, 2:-2] = z0
    gp = np.full((h + 4, w + 4), -1)
    gp[2:-2, 2:-2] = g[..., 0]
    same = sum(((zp[2 + dy:2 + dy + h, 2 + dx:2 + dx + w] > 0) & (gp[2 + dy:2 + dy + h, 2 + dx:2 + dx + w] == g[..., 0])).astype(int)
               for dy in range(-2, 3) for dx in range(-2, 3) if (dy, dx) != (0, 0))
    holes = z0 == 0
    assert ((one["pass_of"] == 1) == (holes & (same >= 3))).all()
    assert (holes & (same == 0)).any() and (holes & (same >= 3)).any() and (one["pass_of"][holes & (same < 3)] == 255).all()
    full = _run(name, radius, d, g, iterations=1)                                   # sigma_color 30 fills more
    assert full["filled"] > one["filled"] > 0


def test_min_taps_at_its_threshold():
    """a hole with exactly four valid taps: filled at min_taps 4, left at 5; the guard does not recount support"""
    z = np.zeros((9, 9), np.float32)
    z[3, 3:6] = (1000.0, 1010.0, 1600.0)
    z[5, 4] = 1020.0
    g = np.full((9, 9, 3), 128, np.uint8)
    space, rng = HC.space_table(1, 2.0), HC.range_table(30.0)
    for taps, filled in ((1, True), (4, True), (5, False), (8, False)):
        out, fill = HC.one_pass(z, g, space, rng, 1, taps)
        assert bool(fill[4, 4]) == filled and (out[4, 4] > 0) == filled
    out, fill = HC.one_pass(z, g, space, rng, 1, 4, max_gap=F(100), gap_rule=0)     # 1600 leaves the sums, not the count
    assert fill[4, 4] and 1000 < out[4, 4] < 1020
    loose, _ = HC.one_pass(z, g, space, rng, 1, 4)
    assert loose[4, 4] > 1100


def test_the_two_gap_rules_differ_on_twins_as_intended():
    """guard off: the band's middle blends the surfaces; gap_rule 0 gives a pixel the surface of its heaviest tap, so the near
    surface comes half-way in; gap_rule 1 gives the whole band the far surface"""
    d, g = HC.depth_frames("twins"), HC.bgr_frames("twins")
    b0, b1 = HC.TWINS_BAND
    res = {(gap, rule): _run("twins", 2, d[0], g[0], max_gap=gap, gap_rule=rule) for gap, rule in HC.GUARDS}
    band = {k: v["z"][2:-2, b0:b1] for k, v in res.items()}
    near, far = F(1000.0), F(1500.0)
    assert all(v["remaining"] == 0 for v in res.values())

    def between(z):
        return (z > near + 110) & (z < far - 10)

    assert between(band[(0.0, 0)]).any()                                            # off: flying pixels
    assert not between(band[(HC.MAX_GAP, 0)]).any() and not between(band[(HC.MAX_GAP, 1)]).any()
    heaviest, farthest = band[(HC.MAX_GAP, 0)], band[(HC.MAX_GAP, 1)]
    assert (heaviest[:, 0] < near + 110).all() and (heaviest[:, -1] > far - 10).all()
    # pass 1 reaches two columns in from either side, where only one surface is in reach; pass 2 sees both
    assert (heaviest[:, 2] < near + 110).all() and (farthest[:, 2:] > far - 10).all()   # the background takes the shadow
    assert (farthest > far - 10).sum() > (heaviest > far - 10).sum()
    assert heaviest.tobytes() != farthest.tobytes()


def test_band_fills_each_side_up_to_the_colour_edge():
    d, g = HC.depth_frames("band"), HC.bgr_frames("band")
    b0, b1 = HC.BAND
    edge = HC.EDGE["band"]
    for radius in HC.CASES["band"].radii:
        r = _run("band", radius, d[0], g[0])
        assert r["remaining"] == 0
        assert (np.abs(r["z"][:, b0:edge] - 1006) < 30).all() and (np.abs(r["z"][:, edge:b1] - 2506) < 30).all()


def test_u16_output_and_counts_before_rounding():
    z = np.zeros((5, 5), np.float32)
    z[2, 1], z[2, 3] = 0.25, 0.25                                                   # fills of 0.25 round to the uint16 "invalid"
    g = np.full((5, 5, 3), 9, np.uint8)
    out, pass_of, filled, remaining = HC.fill(z, g, HC.space_table(1, 2.0), HC.range_table(30.0), np.uint16, radius=1, iterations=2, min_taps=1)
    assert out.dtype == np.uint16 and (out == 0).all() and filled == 23 and remaining == 0 and (pass_of != 255).all()
