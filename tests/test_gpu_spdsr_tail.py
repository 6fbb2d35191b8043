"""The tail of SPDepthSuperResolution::Process (csrc/spdsr_kernels.hip: cluster_moments_kernel<false/true>,
cluster_planes_kernel, set_pseudo_depth_kernel, mrf_sweep_kernel, mrf_expand_kernel) on crafted inputs, through
kde_stage_spdsr_tail of the stage build (include/kde_test_hooks.h), against the binary64 references of
tests/spdsr_tail_cases.py.  tests/test_spdsr_tail_cases.py proves the cases and the references on the CPU.

Bars (none fitted to the GPU's output):
  normals        each component within 2 * 2^-23 of planes64's            (SC.planes_compare)
  d              within 2 float32 ulps of |n_gpu . mean_64|
  markers, unprojected pixels of plane_fitted: to the bit
  plane_fitted   z within 8 float32 ulps of |d / (a rx + b ry + c)| in binary64 from the same float32 planes and rays (two
                 products, two sums and a division, |denominator| >= 0.5); x, y = ray * z in float32 to the bit
  sweeps         z within 8 * e32 of sweeps64, e32 = the largest relative error of the float32 restatement
                 (okde_projection_plane) against sweeps64 on the same case: the GPU does the same 25 float32 accumulations
                 in another order with a 1-ulp reciprocal; one misplaced tap out of 25 moves a pixel by ~7e-5.  Rewritten mask
                 and NaN mask equal to sweeps64's, x, y = ray * z to the bit.  Pixels within 1e-5 of a decision (and what they
                 reach) are exempt from the value bar alone; the cases have none."""
import ctypes
import functools
import subprocess

import numpy as np
import pytest

import spdsr_tail_cases as SC
from conftest import PARITY_LOG
from gpu_util import dev, host, pts_as_f32

pytestmark = pytest.mark.gpu


def tail(c, **kw):
    from tools.hooks import stage
    return stage.spdsr_tail_run(c["w"], c["h"], c["rows"], c["cols"], c["K"], kw.pop("labels", c["labels"]),
                                kw.pop("points", c["points"]), **kw)


def f3(oracle, pts):
    return np.ascontiguousarray(pts, np.float32).view(oracle.FLOAT3).reshape(pts.shape[:-1])


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def check_fit(c, nd, pf, what, skip=(), nd_prev=None):
    """one frame of a plane-fit case against planes64 and the binary64 projection of the GPU's own planes"""
    ref = SC.planes64(c["labels"], c["points"], c["k"], nd_prev=nd_prev)
    dn, dd = SC.planes_compare(nd, ref, what, skip)
    z, proj, den = SC.plane_fitted64(nd, c["labels"], c["points"], c["tx"], c["ty"])
    assert np.array_equal(bits(pf[~proj]), bits(c["points"][~proj])), f"{what}: an unprojected pixel of plane_fitted is not the input point"
    ok = proj & ~np.isin(c["labels"], list(skip))
    assert den[ok].min() >= 0.5
    du = SC.ulps32(pf[..., 2][ok], z[ok]).max()
    assert du <= 8.0, f"{what}: plane_fitted z is {du:.1f} ulps from the binary64 projection"
    assert np.array_equal(pf[..., 0][proj], (c["tx"] * pf[..., 2])[proj]) and np.array_equal(pf[..., 1][proj], (c["ty"] * pf[..., 2])[proj])
    PARITY_LOG.append(f"SPDSR tail {what}: {int((ref['nd'][:, 0] == 5).sum())} markers of {c['k']} clusters, normals within "
                      f"{dn:.2f} x 2^-23, d within {dd:.2f} ulps, plane_fitted z within {du:.2f} ulps")


# ---- plane fit ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(SC.FIT_CASES))
def test_plane_fit(torch_cuda, name):
    """odd-8: register runs across row ends in one partly filled block; lds-1024: the largest table in LDS; global-1056: the
    global-atomics path.  Each with starved clusters (0..3 points), labels outside the table, a band of labels alternating at
    every pixel and a cluster poisoned by one NaN."""
    c = SC.fit_case(name)
    nd, pf, opt = tail(c, sweeps=1)
    check_fit(c, nd, pf, name)


def test_plane_fit_micro_clusters(torch_cuda):
    c = SC.fit_micro_case()
    nd, pf, opt = tail(c, sweeps=1)
    check_fit(c, nd, pf, "micro clusters", skip=[5])
    ref = SC.planes64(c["labels"], c["points"], c["k"])
    # the exact patches: z = const, x = const of either sign (normal exactly (+-1, 0, 0): |nx| < 1 fails, pixels unprojected)
    assert np.array_equal(nd[2], np.float32([0, 0, 1, 1250]))
    assert np.array_equal(nd[3], np.float32([1, 0, 0, 750])) and np.array_equal(nd[4], np.float32([-1, 0, 0, 750]))
    for l in (3, 4):
        m = c["labels"] == l
        assert np.array_equal(bits(pf[m]), bits(c["points"][m]))
    # collinear points: any unit normal across the line
    n = nd[5, :3].astype(np.float64)
    assert abs(np.linalg.norm(n) - 1.0) <= 1e-6 and abs(n @ c["direction"]) <= 1e-6
    assert SC.ulps32(nd[5, 3], abs(n @ ref["mean"][5])) <= 2.0


@pytest.mark.parametrize("name", ["odd-8", "global-1056"])
def test_marker_keeps_w_of_the_previous_call(torch_cuda, name):
    """a cluster that loses its plane keeps the distance its slot held: (5, 5, 5, d of the first call), bit for bit"""
    c = SC.fit_case(name)
    first = {"labels": c["full_labels"], "points": c["full_points"]}
    nd, pf, opt = tail(c, sweeps=1, nd_prev_call=first)
    assert (np.abs(first["nd"][:, 0]) < 1.0).all()
    check_fit(c, nd, pf, f"{name} second call", nd_prev=first["nd"])
    marker = [l for l, left in c["starved"].items() if left < 3]
    assert len(marker) >= 3
    assert np.array_equal(bits(nd[marker, :3]), bits(np.full((len(marker), 3), 5.0)))
    assert np.array_equal(bits(nd[marker, 3]), bits(first["nd"][marker, 3]))


@pytest.mark.parametrize("name", ["odd-8", "global-1056"])
def test_plane_fit_batch(torch_cuda, name):
    """three frames with their own label maps on a max_batch = 4 handle: every frame meets the bars of a single call"""
    cs = [SC.fit_case(name, f) for f in range(3)]
    nd, pf, opt = tail(cs[0], labels=np.stack([c["labels"] for c in cs]), points=np.stack([c["points"] for c in cs]), sweeps=1,
                       max_batch=4)
    assert nd.shape == (3, cs[0]["k"], 4)
    for f, c in enumerate(cs):
        check_fit(c, nd[f], pf[f], f"{name} batch frame {f}")


# ---- sweeps -------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def float32_restatement(oracle, name, item, frame, sweeps):
    """okde_projection_plane on a sweep case: (plane_fitted, optimized), shared and left unchanged"""
    c = SC.sweep_micro(item) if name == "micro" else SC.sweep_case(name, frame)
    pf, opt = oracle.projection_plane(c["nd"], c["labels"], f3(oracle, c["points"]), c["K"], sweeps)
    return pts_as_f32(pf), pts_as_f32(opt)


def check_sweeps(oracle, c, key, sweeps, pf, opt, what):
    """-> (e32, the GPU's largest relative error, flagged pixels)"""
    pf32, opt32 = float32_restatement(oracle, *key, sweeps)
    z, proj, den = SC.plane_fitted64(c["nd"], c["labels"], c["points"], c["tx"], c["ty"])
    assert np.array_equal(bits(pf[~proj]), bits(c["points"][~proj]))
    with np.errstate(all="ignore"):
        ok = proj & (den >= 0.5)
        assert SC.ulps32(pf[..., 2][ok], z[ok]).max() <= 8.0
        assert np.array_equal(np.isfinite(pf), np.isfinite(pf32)) and np.array_equal(np.isnan(pf), np.isnan(pf32))
    e32 = SC.sweep_compare(opt32, SC.sweeps64(pf32[..., 2], c["points"][..., 2], sweeps), c["points"], c["tx"], c["ty"], f"{what} (float32 restatement)")
    ref = SC.sweeps64(pf[..., 2], c["points"][..., 2], sweeps)          # from the GPU's own plane-fitted z: the sweeps alone
    err = SC.sweep_compare(opt, ref, c["points"], c["tx"], c["ty"], what)
    assert np.array_equal(np.isnan(opt), np.isnan(opt32)) and np.array_equal(np.isinf(opt), np.isinf(opt32)), f"{what}: NaN / inf masks differ from okde_projection_plane's"
    flagged = int(ref["flagged"].sum())
    PARITY_LOG.append(f"SPDSR tail {what}: e32 {e32:.2e}, GPU max rel err {err:.2e} (bar {8 * e32:.2e}), flagged {flagged} of {ref['flagged'].size}, "
                      f"rewritten {ref['rewritten'].mean():.2f}")
    print(PARITY_LOG[-1])
    assert err <= 8.0 * e32, f"{what}: optimized z is {err:.3e} from sweeps64 (> 8 x e32 = {8 * e32:.3e})"
    return e32, err, flagged


@pytest.mark.parametrize("sweeps", SC.SWEEP_COUNTS)
@pytest.mark.parametrize("name", list(SC.SWEEP_CASES))
def test_sweeps(torch_cuda, oracle, name, sweeps):
    """odd and small widths (has1 == false, ragged last LDS pair, narrower than a tile), heights off the tile, fewer than 8
    tiles; 0, 1, 2 and 20 sweeps end in either ping-pong buffer"""
    c = SC.sweep_case(name)
    nd, pf, opt = tail(c, nd=c["nd"], sweeps=sweeps)
    assert np.array_equal(bits(nd), bits(c["nd"]))
    e32, err, flagged = check_sweeps(oracle, c, (name, None, 0), sweeps, pf, opt, f"{name} x{sweeps}")
    assert flagged <= (SC.MAX_FLAGGED * opt[..., 2].size if sweeps > 1 else 0)
    if sweeps == 0:
        assert np.array_equal(bits(opt), bits(c["points"]))


@pytest.mark.parametrize("sweeps", (1, 20))
def test_sweeps_batch_is_bit_identical_to_single_frames(torch_cuda, oracle, sweeps):
    """sweep-67x21 x 3 frames: 18 tiles in one grid, walked through the band mapping"""
    name = "sweep-67x21"
    cs = [SC.sweep_case(name, f) for f in range(3)]
    st = lambda key: np.stack([c[key] for c in cs])
    nd, pf, opt = tail(cs[0], labels=st("labels"), points=st("points"), nd=st("nd"), sweeps=sweeps)
    for f, c in enumerate(cs):
        nd1, pf1, opt1 = tail(c, nd=c["nd"], sweeps=sweeps)
        assert np.array_equal(bits(pf[f]), bits(pf1)) and np.array_equal(bits(opt[f]), bits(opt1)), f"frame {f}"
        check_sweeps(oracle, c, (name, None, f), sweeps, pf[f], opt[f], f"{name} batch frame {f} x{sweeps}")


def test_sweep_micro_taps(torch_cuda, oracle):
    """a tap at exactly 50.0f is none, one at nextafter(50.0f) is"""
    c = SC.sweep_micro()
    h, w = c["h"], c["w"]
    nd, pf, opt = tail(c, nd=c["nd"], sweeps=1)
    z = opt[..., 2]
    assert (z[SC.window_of(SC.TAP_INVALID, h, w)] == 50.25).all()
    assert (z[SC.window_of(SC.TAP_VALID, h, w)] < 50.245).all()
    assert (z[:, :6] == 1000.0).all()
    check_sweeps(oracle, c, ("micro", None, 0), 1, pf, opt, "micro taps")


@pytest.mark.parametrize("item", SC.MICRO_ITEMS)
def test_sweep_micro_non_finite(torch_cuda, oracle, item):
    """one +inf / -inf / NaN / 3e38 / negative z, or a plane whose denominator is 0, in a flat frame: NaN and inf land where
    okde_projection_plane puts them (a +inf tap makes its 24 neighbours NaN for good), everything finite meets the sweep bar"""
    c = SC.sweep_micro(item)
    for sweeps in (1, 2, 20):
        nd, pf, opt = tail(c, nd=c["nd"], sweeps=sweeps)
        check_sweeps(oracle, c, ("micro", item, 0), sweeps, pf, opt, f"micro {item} x{sweeps}")
        if item == "plus_inf":
            nan = np.isnan(opt[..., 2])
            assert nan.sum() == 24 and np.array_equal(nan, SC.window_of(SC.MICRO_AT, c["h"], c["w"]))


# ---- the hook runs what Process runs --------------------------------------------------------------------------------------------
def test_hook_is_the_tail_of_process(torch_cuda, oracle, synth, frame):
    from kinectdepthmapenhancement_amd import _native, filters
    from tools.hooks import stage
    w, h = 160, 120
    bgr, depth = frame(720, w, h)
    K = synth.intrinsics(w, h)
    pts = pts_as_f32(oracle.p2r_depth(depth, K))
    t = torch_cuda

    def process():
        sp = filters.SPDepthSuperResolution(w, h)
        try:
            sp.SetParametor(6, 8, K)
            sp.Process(dev(t, depth), dev(t, pts), dev(t, bgr))
            return [host(g()).copy() for g in (sp.getRefinedLabels_Device, sp.getEdgeEnhanced3DPoints_Device, sp.getClusterND_Device,
                                               sp.getOptimizedPoints_Device)]
        finally:
            sp.close()

    prod = process()
    with stage.stage_library():
        staged = process()
    assert np.array_equal(prod[0], staged[0]) and np.array_equal(bits(prod[1]), bits(staged[1]))
    nd, pf, opt = stage.spdsr_tail_run(w, h, 6, 8, K, staged[0], staged[1])
    for other in (staged, prod):
        live = np.abs(other[2][:, 0]) < 1.0
        assert np.array_equal(nd[~live, :3], other[2][~live, :3], equal_nan=True)
        assert SC.ulps32(nd[live], other[2][live].astype(np.float64)).max() <= 1.0
        assert np.array_equal(np.isfinite(opt), np.isfinite(other[3]))
        fin = np.isfinite(opt)
        assert np.allclose(opt[fin], other[3][fin], rtol=1e-4, atol=1e-2)
    assert "kde_stage_spdsr_tail" not in subprocess.run(["nm", "-D", "--defined-only", _native.LIB_PATH], capture_output=True, text=True).stdout
    assert not hasattr(ctypes.CDLL(_native.LIB_PATH), "kde_stage_spdsr_tail")


def test_hook_refusals(torch_cuda):
    from kinectdepthmapenhancement_amd import _native, filters
    from tools.hooks import stage
    c = SC.sweep_micro()
    t = torch_cuda
    lab, pts = dev(t, c["labels"]), dev(t, c["points"])
    with stage.stage_library():
        l = stage.lib()
        call = lambda sp, n=1, la=lab, p=pts, sw=1: l.kde_stage_spdsr_tail(sp, n, None if la is None else la.data_ptr(),
                                                                          None if p is None else p.data_ptr(), None, sw, None)
        sp = filters.SPDepthSuperResolution(c["w"], c["h"], max_batch=2)
        try:
            assert call(sp._h) == _native.KDE_ERR_INVALID and b"SetParametor" in l.kde_last_error_string()
            sp.SetParametor(c["rows"], c["cols"], c["K"])
            assert call(None) == _native.KDE_ERR_INVALID and b"null" in l.kde_last_error_string()
            assert call(sp._h, la=None) == _native.KDE_ERR_INVALID and call(sp._h, p=None) == _native.KDE_ERR_INVALID
            for n in (0, -1, 3):
                assert call(sp._h, n=n) == _native.KDE_ERR_INVALID and b"max_batch" in l.kde_last_error_string()
            assert call(sp._h, sw=-1) == _native.KDE_ERR_INVALID and b"sweeps" in l.kde_last_error_string()
            assert call(sp._h) == _native.KDE_OK
            t.cuda.synchronize()
        finally:
            sp.close()
