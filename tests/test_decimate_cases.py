"""The numpy statement of DepthDecimation (tests/decimate_cases.py) against itself, without a GPU: the vectorised statement
equals the scalar loop that follows the header on every case, and both have the properties the rule promises."""
import numpy as np
import pytest

import decimate_cases as DC
from decimate_cases import CASES, CASE_FACTORS, F, GUARDS, MAX_GAP, MEAN, MEDIAN, Z_RANGE

ZR = dict(z_min=Z_RANGE[0], z_max=Z_RANGE[1])


def _same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a.view(np.uint32) if a.dtype == np.float32 else a,
                                                                        b.view(np.uint32) if b.dtype == np.float32 else b)


@pytest.mark.parametrize("name,k", CASE_FACTORS)
def test_the_vectorised_statement_equals_the_scalar_loop(name, k):
    case = CASES[name]
    for frames in (case.f32, case.u16):
        for mode in (MEDIAN, MEAN):
            for gap in GUARDS:
                for f in (0, DC.FRAMES - 1):
                    a = DC.decimate(frames[f], k, mode, 1, gap, **ZR)
                    b = DC.decimate_scalar(frames[f], k, mode, 1, gap, **ZR)
                    for key in ("z", "m", "zmed", "filled", "mixed"):
                        assert _same(a[key], b[key]), (name, k, mode, gap, f, key)
    assert np.array_equal(DC.decimate_color(case.bgr[1], k), DC.decimate_color_scalar(case.bgr[1], k))


@pytest.mark.parametrize("min_valid", (1, 2, "all"))
@pytest.mark.parametrize("k", CASES["holes"].factors)
def test_holes_meets_every_count_and_min_valid_bites(k, min_valid):
    case = CASES["holes"]
    mv = k * k if min_valid == "all" else min_valid
    seen = set()
    for frames in (case.f32, case.u16):
        for f in range(DC.FRAMES):
            a = DC.decimate(frames[f], k, MEDIAN, mv, **ZR)
            b = DC.decimate_scalar(frames[f], k, MEDIAN, mv, **ZR)
            assert _same(a["z"], b["z"]) and _same(a["filled"], b["filled"])
            assert np.array_equal(a["filled"], a["m"] >= mv) and np.all(a["z"][~a["filled"]] == 0) and np.all(a["z"][a["filled"]] > 0)
            seen |= set(a["m"].ravel().tolist())
    assert seen == set(range(k * k + 1))                              # m takes every value 0 .. k^2
    # ties: some block with an even count of valid samples has the two middle samples different, and the lower one is taken
    z = DC._blocks(DC.widen(case.f32[0]), k, F(0))
    a = DC.decimate(case.f32[0], k, MEDIAN, 1, **ZR)
    lower_taken = 0
    for j, i in zip(*np.nonzero((a["m"] % 2 == 0) & (a["m"] >= 2))):
        v = np.sort([s for s in z[j, i] if s > Z_RANGE[0] and s < Z_RANGE[1]])
        assert a["z"][j, i] == v[(len(v) - 1) // 2]
        lower_taken += v[(len(v) - 1) // 2] < v[len(v) // 2]
    assert lower_taken > 0


@pytest.mark.parametrize("name,k", CASE_FACTORS)
def test_the_median_is_a_sample_and_the_guarded_mean_stays_with_it(name, k):
    case = CASES[name]
    for frames in (case.f32, case.u16):
        z = DC._blocks(DC.widen(frames[2]), k, F(0))
        med = DC.decimate(frames[2], k, MEDIAN, 1, MAX_GAP, **ZR)
        with np.errstate(invalid="ignore"):
            valid = (z > Z_RANGE[0]) & (z < Z_RANGE[1])
        is_sample = ((z == med["z"][..., None]) & valid).any(-1)
        assert np.array_equal(is_sample, med["filled"])
        mean = DC.decimate(frames[2], k, MEAN, 1, MAX_GAP, **ZR)
        f = mean["filled"]
        assert np.all(np.abs(mean["z"][f].astype(np.float64) - med["z"][f]) <= float(MAX_GAP))       # within max_gap of zmed
        # filled and mixed are their definitions
        assert np.array_equal(med["filled"], valid.sum(-1) >= 1)
        span = np.where(valid, z, -np.inf).max(-1) - np.where(valid, z, np.inf).min(-1)
        assert np.array_equal(med["mixed"], (valid.sum(-1) >= 1) & (span.astype(np.float32) > MAX_GAP))
        assert not DC.decimate(frames[2], k, MEAN, 1, F(0), **ZR)["mixed"].any()                      # no guard, nothing mixed
        if frames.dtype == np.uint16:                                                                 # uint16 to uint16 is exact
            assert np.array_equal(DC.depth_to_u16(med["z"]).astype(np.float32), med["z"])


@pytest.mark.parametrize("k", CASES["edge"].factors)
def test_edge_the_guarded_mean_is_never_between_the_surfaces(k):
    case = CASES["edge"]
    straddling = 0
    for f in range(DC.FRAMES):
        guarded = DC.decimate(case.f32[f], k, MEAN, 1, MAX_GAP, **ZR)
        plain = DC.decimate(case.f32[f], k, MEAN, 1, F(0), **ZR)
        z = guarded["z"]
        assert np.all((np.abs(z - DC.NEAR) <= 3) | (np.abs(z - DC.FAR) <= 3))
        between = (plain["z"] > DC.NEAR + 3) & (plain["z"] < DC.FAR - 3)
        assert np.array_equal(between, guarded["mixed"])              # the plain mean invents a depth exactly in the mixed blocks
        straddling += int(guarded["mixed"].sum())
    assert straddling > 0
    # the step cuts corners of several sizes off the blocks, so the median falls on either side of it
    far = np.concatenate([(DC._blocks(case.f32[f], k, F(0)) > 1500).sum(-1).ravel() for f in range(DC.FRAMES)])
    cut = {c for c in far.tolist() if 0 < c < k * k}
    assert len(cut) >= 2 and min(cut) < k * k / 2 < max(cut)          # k = 2: a corner of one sample, or of three


@pytest.mark.parametrize("k", (2, 3, 5, 8))
def test_a_constant_frame_decimates_to_the_constant(k):
    for dtype, value in ((np.float32, 1234.5), (np.uint16, 1234)):
        frame = np.full((19, 23), value, dtype)
        for mode in (MEDIAN, MEAN):
            for gap in GUARDS:
                a = DC.decimate(frame, k, mode, 1, gap, **ZR)
                assert a["filled"].all() and not a["mixed"].any() and np.all(a["z"] == F(value)), (k, mode, gap)


@pytest.mark.parametrize("name,k", CASE_FACTORS)
def test_the_guide_mean_is_round_half_up_inside_the_block(name, k):
    case = CASES[name]
    got = DC.decimate_color(case.bgr[0], k).astype(np.int64)
    b = DC._blocks(case.bgr[0].astype(np.int64), k, -1)              # -1: no pixel
    lo = np.where(b >= 0, b, 255).min(2)
    hi = b.max(2)
    assert np.all(got >= lo) and np.all(got <= hi)
    s, c = np.where(b >= 0, b, 0).sum(2), (b >= 0).sum(2)
    for j in range(got.shape[0]):
        for i in range(got.shape[1]):
            for ch in range(3):
                si, ci = int(s[j, i, ch]), int(c[j, i, ch])
                q, r = divmod(si, ci)                                 # round_half_up(s / c) in Python integers
                assert got[j, i, ch] == q + (1 if 2 * r >= ci else 0)


@pytest.mark.parametrize("k", range(2, 9))
def test_intrinsics_map_a_block_centre_to_its_pixel(k):
    K = np.array([[525.0, 0.0, 319.5], [0.0, 530.0, 239.5], [0.0, 0.0, 1.0]])
    Ks = DC.intrinsics(K, k)
    for i, j in ((0, 0), (3, 7), (79, 59)):
        cx, cy = i * k + (k - 1) / 2.0, j * k + (k - 1) / 2.0         # the centre of block (i, j) in source pixels
        for Z in (500.0, 3000.0):
            X, Y = (cx - K[0, 2]) / K[0, 0] * Z, (cy - K[1, 2]) / K[1, 1] * Z
            assert abs(Ks[0, 0] * X / Z + Ks[0, 2] - i) < 1e-9 and abs(Ks[1, 1] * Y / Z + Ks[1, 2] - j) < 1e-9
    assert np.array_equal(Ks[2], K[2])
