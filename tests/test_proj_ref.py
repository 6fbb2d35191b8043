"""tools/proj_ref.c, the CPU checker of the five-argument Projection_GPU::PlaneProjection, pinned without a GPU: against the
independent numpy transcription in tests/proj_cases.py, against micro-cases worked by hand (one pixel per branch of
Projection_GPU.cu:38, :201-209 and :239-242), and against one golden.  DESIGN.md, "Plane projection (five-argument)"."""
import math
import os

import numpy as np
import pytest

import proj_cases as PC
from proj_cases import F


@pytest.fixture(scope="module")
def R():
    from tools import proj_ref
    proj_ref.build()
    return proj_ref


def bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def same(a, b):
    a, b = np.asarray(a, F), np.asarray(b, F)
    return bool(((bits(a) == bits(b)) | (np.isnan(a) & np.isnan(b))).all())


def test_threshold_is_derived_independently(R):
    """P3: t is the largest float whose acos is not below pi/8; three derivations agree (this file's, numpy's in
    les_cases.py, C's in proj_ref.c) and the boundary is where it should be"""
    c = PC.MAX_ANGLE
    t = R.acos_threshold(c)
    assert t == PC.acos_threshold(c)
    assert F(math.acos(float(t))) >= c and F(math.acos(float(np.nextafter(t, F(2))))) < c
    assert abs(float(t) - math.cos(math.pi / 8)) < 1e-6
    assert R.acos_threshold(F(np.nan)) == np.inf and R.acos_threshold(F(0)) == np.inf and R.acos_threshold(F(4)) < -1


def test_spatial_table_and_rays(R):
    t = R.spatial_filter()
    for i in range(7):
        for j in range(7):
            assert abs(float(t[i, j]) - math.exp(-((i - 3) ** 2 + (j - 3) ** 2) / 800.0)) < 1e-7
    assert t[3, 3] == 1 and same(t, t.T)
    K = PC.intrinsics(70, 50)                       # cx = 34.5 -> 34, cy = 24.5 -> 24
    rays = R.init_normalized(70, 50, K)
    rx, ry = PC.np_rays(70, 50, K)
    assert same(rays[..., 0], rx) and same(rays[..., 1], ry) and (rays[..., 2] == 1).all()
    assert rays[24, 34, 0] == 0 and rays[24, 34, 1] == 0 and rays[0, 0, 1] == F(24) / F(K[1, 1]) and rays[0, 0, 0] == F(-34) / F(K[0, 0])


def test_micro_cases_one_pixel_per_branch(R):
    nd, labels, variance, points, size, K = PC.micro_frame()
    o = R.plane_projection(nd, labels, variance, points, size, K, window_size=1)
    pf, z1, zo = o["plane_fitted"][0], o["prefilter"][0, :, 2], o["optimized"][0, :, 2]
    v = F(0.95)
    blend = F(F(1020) * v) + F(F(1000) * F(F(1) - v))
    assert pf[:, 2].tolist()[:7] == [1005, 1020, 1060, 1000, 1000, 1000, 1005]
    assert z1.tolist()[:7] == [1005, float(blend), 1000, 1000, 1000, 1000, 1000] and 1018 < blend < 1020
    for k in (0, 1, 2, 6):                                   # projected: x = z * ray.x, y = z * 0
        assert pf[k, 0] == F(pf[k, 2] * F(k)) and pf[k, 1] == 0
    for k in (3, 4, 5, 11, 12):                              # not projected: the input point, bit for bit
        assert same(pf[k], points[0, k])
    assert np.isinf(pf[7, 2]) and np.isinf(pf[7, 0]) and np.isnan(pf[7, 1]) and z1[7] == 1000
    assert pf[8, 2] == 40 and z1[8] == F(40.2)
    assert pf[9, 2] == 1000 and z1[9] == 0 and zo[9] == 0
    assert pf[10, 2] == 1020 and z1[10] == 1020
    assert z1[11] == 1000 and z1[12] == 1000
    # window 1: the centre weight is expf(0) * 1, so the filter returns the pre-filter z exactly (0 where it is <= 50)
    assert same(zo, np.where(z1 > 50, z1, F(0)))
    assert same(o["optimized"][0, :, 0], o["rays"][0, :, 0] * zo)
    assert same(o["prefilter"][0, :, :2], points[0, :, :2])  # x, y of Optimized3D are untouched before the filter
    n = PC.np_plane_projection(nd, labels, variance, points, size, K, window_size=1)
    assert same(n["plane_fitted"], o["plane_fitted"]) and same(n["prefilter"], o["prefilter"]) and same(n["optimized"], o["optimized"])


def test_micro_bilateral(R):
    """:224-242 by hand on 3 x 1, window 3, no labels: z = 1000, 1100, hole"""
    z = np.array([1000, 1100, 0], F)
    points = np.stack([np.zeros(3, F), np.zeros(3, F), z], -1)[None]
    args = (np.zeros((1, 3, 4), F), np.full((1, 3), -1, np.int32), np.zeros(1, F), points, np.zeros(1, np.int32), np.eye(3))
    o = R.plane_projection(*args, window_size=3)
    s1 = math.exp(-1 / 800.0)
    w01 = math.exp(-100.0 ** 2 / 20000.0) * s1
    exp0, exp1 = (1000 + 1100 * w01) / (1 + w01), (1100 + 1000 * w01) / (1 + w01)
    zo = o["optimized"][0, :, 2]
    assert abs(zo[0] - exp0) < 1e-6 * exp0 and abs(zo[1] - exp1) < 1e-6 * exp1
    # the hole sees one valid tap, weight exp(-1100^2 / 20000) s1 ~ 5e-27: the quotient is that tap's depth
    assert abs(zo[2] - 1100) < 1e-3 and abs(o["den64"][0, 2] - math.exp(-1100.0 ** 2 / 20000.0) * s1) < 1e-33
    assert abs(o["den64"][0, 0] - (1 + w01)) < 1e-7            # the table entry is a float32
    # no valid tap at all: denominator 0 -> 0 (:239-240); a hole beside a surface so far that the weight is below 2^-120 is BAND
    points[0, :, 2] = [0, 30, 50]
    assert (R.plane_projection(*args, window_size=3)["optimized"][0, :, 2] == 0).all()
    points[0, :, 2] = [0, 1400, 0]
    o = R.plane_projection(*args, window_size=3)
    assert o["optimized"][0, 1, 2] == 1400 and 0 < o["den64"][0, 0] < R.BAND_DEN and o["den64"][0, 1] == 1
    # snapshot semantics (P4): pixel 1's result does not feed pixel 2's window
    points[0, :, 2] = [1000, 1100, 1200]
    o = R.plane_projection(*args, window_size=3)
    w12 = w01
    assert abs(o["optimized"][0, 2, 2] - (1200 + 1100 * w12) / (1 + w12)) < 1e-6 * 1200


CASES = [("70x50 nc20", dict(seed=1, W=70, H=50, nc=20)), ("33x25 nc1", dict(seed=2, W=33, H=25, nc=1)),
         ("96x64 nc2048", dict(seed=3, W=96, H=64, nc=2048))]


@pytest.mark.parametrize("name,kw", CASES)
def test_checker_equals_numpy_transcription(R, name, kw):
    case = PC.synthetic_case(**kw)
    ms = PC.min_size_for(kw["W"], kw["H"])
    o = R.plane_projection(*case, min_size=ms)
    n = PC.np_plane_projection(*case, min_size=ms)
    assert same(o["plane_fitted"], n["plane_fitted"]) and same(o["prefilter"], n["prefilter"])
    cmp = R.compare(n["plane_fitted"], n["optimized"], o)
    b = PC.branch_counts(o, case[3], case[1], case[2], case[4], ms)
    print(name, cmp, b)
    assert cmp["plane_fitted"] == cmp["strict"] == cmp["hole"] == cmp["band"] == cmp["xy"] == 0
    assert cmp["max_rel_strict"] < 1e-6 and cmp["max_rel_hole"] < 1e-5
    assert np.allclose(o["den64"], n["den64"], rtol=1e-6, atol=0)
    # the inputs exercise what they claim: no BAND pixel by construction (depth <= 1250 mm), holes present, every branch taken
    assert cmp["n_band"] == 0 and cmp["n_hole"] > 0 and float(np.nanmax(o["prefilter"][..., 2])) <= 1250
    assert b["projected"] and b["kept"] and b["replaced"] and b["blended"] and (b["small_region"] or kw["nc"] == 1)


def test_deep_case_has_a_small_band(R):
    """depth up to 4000 mm: a hole whose window holds only far surfaces sums weights below 2^-120.  The same assertion the
    GPU test makes, here on the checker and the numpy transcription, so the inputs are proven before the GPU sees them"""
    case = PC.deep_case(5, 70, 50, 20)
    ms = PC.min_size_for(70, 50)
    o = R.plane_projection(*case, min_size=ms)
    n = PC.np_plane_projection(*case, min_size=ms)
    cmp = R.compare(n["plane_fitted"], n["optimized"], o)
    print(cmp)
    assert cmp["plane_fitted"] == cmp["strict"] == cmp["hole"] == cmp["band"] == 0
    holes = cmp["n_hole"] + cmp["n_band"]
    assert 0 < cmp["n_band"] < holes and cmp["n_band"] < 0.05 * 70 * 50 and cmp["n_hole"] > 0
    assert float(np.nanmax(case[3][..., 2])) > 3500


def test_denormal_weights_leave_the_window_range_by_half_a_millimetre_at_most(R):
    """found by the seeded sweep: where a hole's tap weights are float32 denormals the reference's own arithmetic leaves
    [min, max] of the window's valid z, so the BAND bar is that range widened by BAND_SLACK_MM (+ 2^-15 relative); the
    restatement and the numpy transcription meet it, and half a millimetre is not more than the arithmetic needs"""
    case, kw = PC.denormal_weight_case()
    o = R.plane_projection(*case, **kw)
    zo, unit = o["optimized"][0, :, 2], 2.0 ** -149
    assert 1.0 < o["den64"][0, 0] / unit < 1.1 and o["den64"][0, 1] == 1            # one unit: the weight is the grid's 1
    assert zo[1] == PC.DENORMAL_TAP and zo[0] == zo[2] == 2155                      # 2155 u / 1 u, below the only valid z
    cmp = R.compare(o["plane_fitted"], o["optimized"], o, 3)
    assert cmp["n_band"] == 2 and cmp["plane_fitted"] == cmp["strict"] == cmp["hole"] == cmp["band"] == cmp["xy"] == 0, cmp
    n = PC.np_plane_projection(*case, **kw)
    assert R.compare(n["plane_fitted"], n["optimized"], o, 3)["band"] == 0
    # the interval is not a licence: a millimetre off, or the far side of the slack, still fails; 0 (every weight flushed) passes
    for z, bad in ((2155.418 - 0.6, 1), (2155.418 + 0.6, 1), (2154.0, 1), (0.0, 0), (2155.5, 0), (2155.418, 0)):
        g = o["optimized"].copy()
        g[0, 0] = o["rays"][0, 0] * F(z)
        assert R.compare(o["plane_fitted"], g, o, 3)["band"] == bad, z
    # the bound is reached: a tap at k + 0.499 under a weight of one unit rounds down by 0.499
    worst = 0.0
    for zt in np.arange(2150.0, 2162.0, 0.0625, dtype=F) + F(0.499):
        case[3][0, 1, 2] = zt
        w = R.plane_projection(*case, **kw)
        if 0 < w["den64"][0, 0] < 1.5 * unit:
            worst = max(worst, abs(float(w["optimized"][0, 0, 2]) - float(zt)))
        assert R.compare(w["plane_fitted"], w["optimized"], w, 3)["band"] == 0, zt
    assert 0.49 < worst <= R.BAND_SLACK_MM


def test_golden(R):
    """tests/golden/proj_it1.npz (tests/golden/make_golden_proj.py): everything before the filter to the bit; the filter's
    result to 1e-6, because it goes through libm's expf"""
    g = np.load(os.path.join(PC.GOLDEN, "proj_it1.npz"))
    case = PC.golden_inputs()                     # the stored points with the LES golden's four outputs
    assert case[3].shape == (120, 160, 3) and 0.02 < float((case[3][..., 2] == 0).mean()) < 0.06
    o = R.plane_projection(*case)
    assert np.array_equal(bits(o["plane_fitted"]), g["plane_fitted"]) and np.array_equal(bits(o["prefilter"][..., 2]), g["prefilter_z"])
    gz = g["optimized_z"].view(F)
    assert np.array_equal(gz == 0, o["optimized"][..., 2] == 0)
    assert np.allclose(o["optimized"][..., 2], gz, rtol=1e-6, atol=0)
    b = PC.branch_counts(o, case[3], case[1], case[2], case[4], PC.MIN_SIZE)
    assert b["projected"] and b["kept"] and b["replaced"] and b["blended"] and b["small_region"], b
    assert g["branches"].tolist() == [b[k] for k in ("projected", "kept", "replaced", "blended", "small_region")]
