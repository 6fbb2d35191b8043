"""NormalAdaptiveSuperpixel on the GPU (nasp_kernels.hip) against the CPU restatement tools/nasp_ref.c, through the Python
class.  The bar is bit-identity of EVERY output -- labels, (distance, label) records, mean records including size, centres,
normals, variance; equal NaN positions for floats -- with no pixel or cluster excluded ("Normal-adaptive
superpixels": with NA3 and NA4 every float operation left is + - * / sqrt in a fixed order)."""
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from nasp_cases import assert_identical, differing, read_outputs, ubits

pytestmark = pytest.mark.gpu

REF_CALL = (10.0, 50.0, 50.0, 150.0)        # KinectDepthEnhancement.cpp:67


@pytest.fixture(scope="module")
def R():
    from tools import nasp_ref
    nasp_ref.build()
    return nasp_ref


@pytest.fixture(scope="module")
def NR():
    from tools import normals_ref
    normals_ref.build()
    return normals_ref


@pytest.fixture(scope="module")
def T(torch_cuda):
    import torch
    torch.cuda.set_device(0)
    return torch


def intrinsics(W, H):
    from kinectdepthmapenhancement_amd import synth
    return synth.intrinsics(W, H)


_cache = {}


def synth_inputs(NR, seed, W, H, method):
    """synth.make_frame -> oracle p2r_depth -> tools/normals_ref normals (so a normals bug cannot hide here)"""
    key = (seed, W, H, method)
    if key not in _cache:
        from kinectdepthmapenhancement_amd import synth
        from oracle import oracle as O
        bgr, depth = synth.make_frame(seed, W, H)
        pts = O.p2r_depth(depth, synth.intrinsics(W, H)).view(np.float32).reshape(H, W, 3).copy()
        nrm, _, _ = NR.normals(pts, method, want_band=False)
        _cache[key] = (np.ascontiguousarray(bgr), pts, np.ascontiguousarray(nrm))
    return _cache[key]


def ragged_inputs(NR, seed, W, H, method=2, nans=False):
    """a wavy surface with 3 % holes and noisy colour, as tests/test_gpu_normals.py's ragged_points.  nans=True: 0.5 % of
    the depths are NaN (the checker's BILATERAL normals are then NaN there and at the neighbours that difference against
    them) and a further 1 % of the normals are overwritten with NaN components"""
    key = ("ragged", seed, W, H, method, nans)
    if key not in _cache:
        rng = np.random.default_rng(seed)
        yy, xx = np.mgrid[0:H, 0:W].astype(np.float32)
        z = (800.0 + 3000.0 * (0.3 + 0.2 * np.sin(xx / 9.0) + 0.1 * np.cos(yy / 7.0))).astype(np.float32)
        z += rng.normal(0.0, 2.0, z.shape).astype(np.float32)
        z[rng.random(z.shape) < 0.03] = 0.0
        if nans:
            z[rng.random(z.shape) < 0.005] = np.nan
        f = np.float32(575.8)
        pts = np.stack([(xx - W / 2) / f * z, (H / 2 - yy) / f * z, z], -1).astype(np.float32)
        bgr = (128 + 100 * np.sin(xx[..., None] / np.array([11.0, 17.0, 23.0]) + yy[..., None] / 13.0)).astype(np.int64)
        bgr = np.clip(bgr + rng.integers(-20, 21, bgr.shape), 0, 255).astype(np.uint8)
        nrm, _, _ = NR.normals(pts, method, want_band=False)
        if nans:
            hit = rng.random(z.shape) < 0.01
            nrm[hit, rng.integers(0, 3, int(hit.sum()))] = np.nan
        _cache[key] = (np.ascontiguousarray(bgr), pts, np.ascontiguousarray(nrm))
    return _cache[key]


def gpu_segmentation(T, R, bgr, pts, nrm, rows, cols, K, sig, it, sp=None):
    from kinectdepthmapenhancement_amd import filters
    H, W = bgr.shape[:2]
    own = sp is None
    if own:
        sp = filters.NormalAdaptiveSuperpixel(W, H)
        sp.SetParametor(rows, cols, K)
    sp.Segmentation(T.from_numpy(bgr).cuda(), T.from_numpy(pts).cuda(), T.from_numpy(nrm).cuda(), *sig, it)
    out = read_outputs(R, sp)
    T.cuda.synchronize()
    if own:
        sp.close()
    return out


def check(T, R, inputs, rows, cols, sig, it, what):
    bgr, pts, nrm = inputs
    H, W = bgr.shape[:2]
    K = intrinsics(W, H)
    exp = R.segmentation(bgr, pts, nrm, rows, cols, K, *sig, it)
    got = gpu_segmentation(T, R, bgr, pts, nrm, rows, cols, K, sig, it)
    assert_identical(got, exp, what)
    return exp


@pytest.mark.parametrize("method", [1, 2], ids=["CM", "BILATERAL"])
@pytest.mark.parametrize("it", [1, 3, 5])
def test_vga_reference_call(T, R, NR, method, it):
    inp = synth_inputs(NR, 1, 640, 480, method)
    exp = check(T, R, inp, 15, 20, REF_CALL, it, f"VGA 15x20 method {method} it {it}")
    assert len(np.unique(exp["labels"])) > 250


@pytest.mark.parametrize("it", [1, 3, 5])
def test_vga_nan_normals_through_tree_and_sums(T, R, NR, it):
    """NaN normals (and NaN depths): NaN distances go through the 64-way tree (a NaN neither replaces nor is replaced), NaN
    sums through analyzeClusters_NASP into the cluster normals the weighted pass reads"""
    inp = ragged_inputs(NR, 12, 640, 480, 2, nans=True)
    assert np.isnan(inp[2]).any(-1).sum() > 4000 and np.isnan(inp[1][..., 2]).sum() > 1000
    exp = check(T, R, inp, 15, 20, REF_CALL, it, f"VGA NaN normals it {it}")
    # (a cluster that owns a NaN normal has a NaN average after analyzeClusters_NASP; the weighted pass then rejects all its
    # pixels -- a NaN normal_diff fails the NA3 test -- and stores the bad normal (-1,-1,-1) with centre 0)
    assert np.isnan(exp["ld"]["d"]).sum() > 1000 and (exp["normals"] == -1).all(-1).sum() > 20


def test_vga_depth_sigma_zero_normal_sigma_on(T, R, NR):
    exp = check(T, R, synth_inputs(NR, 2, 640, 480, 1), 15, 20, (10.0, 50.0, 0.0, 150.0), 2, "VGA depth_sigma 0")
    assert (exp["labels"] == -1).any()                     # the reset still runs (normal_sigma != 0)
    check(T, R, synth_inputs(NR, 2, 640, 480, 1), 15, 20, (10.0, 50.0, 0.0, 0.0), 2, "VGA colour + space only")


def test_vga_all_bad_normals(T, R, NR):
    bgr, pts, _ = synth_inputs(NR, 3, 640, 480, 1)
    nrm = np.full_like(pts, -1.0)
    exp = check(T, R, (bgr, pts, nrm), 15, 20, REF_CALL, 2, "VGA all-bad normals")
    assert (exp["normals"] == -1).all() and (exp["variance"] == 0).all()


@pytest.mark.parametrize("W,H,rows,cols", [(320, 240, 7, 9), (70, 50, 3, 5)])
def test_ragged_windows(T, R, NR, W, H, rows, cols):
    for it in (1, 3):
        check(T, R, synth_inputs(NR, 4, W, H, 1), rows, cols, REF_CALL, it, f"{W}x{H} {rows}x{cols} it {it}")
        check(T, R, ragged_inputs(NR, 5, W, H), rows, cols, REF_CALL, it, f"ragged {W}x{H} {rows}x{cols} it {it}")


def test_more_clusters_than_fit_in_lds(T, R, NR):
    """40 x 40 = 1600 clusters of 16 x 12 pixels: the assignment kernel reads its cluster table from global memory (the LDS
    form holds 1536 records)"""
    check(T, R, synth_inputs(NR, 1, 640, 480, 1), 40, 40, REF_CALL, 2, "VGA 40x40 clusters")
    check(T, R, ragged_inputs(NR, 12, 640, 480, 2, nans=True), 40, 40, REF_CALL, 2, "VGA 40x40 clusters, NaN normals")


def test_vga_ragged_points_with_holes(T, R, NR):
    for method in (1, 2):
        check(T, R, ragged_inputs(NR, 6, 640, 480, method), 15, 20, REF_CALL, 3, f"ragged VGA method {method}")


def test_1080p(T, R, NR):
    check(T, R, synth_inputs(NR, 1, 1920, 1080, 2), 15, 20, REF_CALL, 1, "1080p 15x20 it 1")


def test_batch_equals_single_calls_and_second_call_equals_fresh_handle(T, R, NR):
    from kinectdepthmapenhancement_amd import filters
    W, H, rows, cols, n = 320, 240, 7, 9, 5
    frames = [synth_inputs(NR, 4, W, H, 1), ragged_inputs(NR, 5, W, H), synth_inputs(NR, 7, W, H, 2),
              ragged_inputs(NR, 8, W, H, 1), ragged_inputs(NR, 9, W, H, 2, nans=True)]
    assert np.isnan(frames[4][2]).any()
    frames[3] = (frames[3][0], frames[3][1], np.full_like(frames[3][2], -1.0))          # one frame without normals
    K = intrinsics(W, H)
    singles = [gpu_segmentation(T, R, *f, rows, cols, K, REF_CALL, 3) for f in frames]
    sp = filters.NormalAdaptiveSuperpixel(W, H, max_batch=n)
    sp.SetParametor(rows, cols, K)
    for order in ([0, 1, 2, 3, 4], [3, 0, 4, 2, 1]):
        dev = [T.from_numpy(np.stack([frames[k][j] for k in order])).cuda() for j in range(3)]
        sp.segmentation_batch(*dev, *REF_CALL, 3)
        for pos, k in enumerate(order):
            assert_identical(read_outputs(R, sp, pos), singles[k], f"batch order {order} position {pos}")
    # NA5: a later single-frame call on the handle that just served a batch equals a fresh handle's
    got = gpu_segmentation(T, R, *frames[2], rows, cols, K, REF_CALL, 1, sp=sp)
    assert_identical(got, gpu_segmentation(T, R, *frames[2], rows, cols, K, REF_CALL, 1), "second call on a used handle")
    assert_identical(got, R.segmentation(*frames[2], rows, cols, K, *REF_CALL, 1), "second call vs checker")
    # the pinned host copies
    assert np.array_equal(sp.getLabelsHost(), got["labels"]) and np.array_equal(sp.getMeanDataHost().view(R.SUPERPIXEL).reshape(-1), got["mean"])
    assert differing(sp.getCentersHost(), got["centers"]) == 0 and differing(sp.getNormalsHost(), got["normals"]) == 0
    assert differing(sp.getNormalsVarianceHost(), got["variance"]) == 0
    img = sp.getNormalImg()
    assert img.shape == (H, W, 3) and (img[got["labels"] == -1] == 0).all() and img.any()
    sp.close()


def test_chain_normal_map_generator_feeds_nasp_on_the_device(T, R):
    from kinectdepthmapenhancement_amd import filters, synth
    from oracle import oracle as O
    W, H = 640, 480
    bgr, depth = synth.make_frame(11, W, H)
    K = synth.intrinsics(W, H)
    conv = filters.DimensionConvertor()
    conv.setCameraParameters(K, W, H)
    pts = T.empty((H, W, 3), dtype=T.float32, device="cuda")
    conv.projectiveToReal(T.from_numpy(depth).cuda(), pts)
    g = filters.NormalMapGenerator(W, H)
    g.setNormalEstimationMethods(g.CM)
    g.generateNormalMap(pts)
    sp = filters.NormalAdaptiveSuperpixel(W, H)
    sp.SetParametor(15, 20, K)
    sp.Segmentation(T.from_numpy(bgr).cuda(), pts, g.getNormalMap(), *REF_CALL, 1)
    got = read_outputs(R, sp)
    exp = R.segmentation(bgr, pts.cpu().numpy(), g.getNormalMap().cpu().numpy(), 15, 20, K, *REF_CALL, 1)
    assert_identical(got, exp, "NormalMapGenerator -> NASP")
    sp.close()
    g.close()


def test_geometry_rejection_and_argument_checks(T, R):
    from kinectdepthmapenhancement_amd import filters, _native
    sp = filters.NormalAdaptiveSuperpixel(640, 480)
    K = intrinsics(640, 480)
    for rows, cols in ((15, 81), (61, 20), (0, 20)):          # 7-pixel windows, no rows
        assert not R.check_geometry(640, 480, rows, cols)
        with pytest.raises(_native.KdeError):
            sp.SetParametor(rows, cols, K)
    z = T.zeros((480, 640, 3), dtype=T.uint8, device="cuda")
    f = T.zeros((480, 640, 3), dtype=T.float32, device="cuda")
    with pytest.raises(_native.KdeError):
        sp.Segmentation(z, f, f, *REF_CALL, 1)                 # SetParametor never succeeded
    sp.SetParametor(15, 20, K)
    with pytest.raises(_native.KdeError):
        sp.Segmentation(z, f, f, 0.0, 0.0, 0.0, 0.0, 1)        # the sigmas sum to zero
    with pytest.raises(_native.KdeError):
        sp.Segmentation(z, f, f, *REF_CALL, -1)
    sp.close()


def test_normals_on_both_sides_of_the_acos_threshold(T, R, NR):
    """NA3: library and checker derive the acos threshold independently (compared directly in tests/test_nasp_sanitize.py);
    here the kernel's use of it: cluster normal (0, 0, -1), pixel normals at 60 degrees +- a few ulp"""
    W, H, rows, cols = 64, 64, 2, 2
    bgr = np.full((H, W, 3), 90, np.uint8)
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float32)
    z = np.full((H, W), 1000.0, np.float32)
    pts = np.stack([(xx - W / 2) * z / 575.8, (H / 2 - yy) * z / 575.8, z], -1).astype(np.float32)
    t = R.acos_threshold()
    steps = ((np.arange(W * H) % 9) - 4).reshape(H, W)
    c = np.full((H, W), t, np.float32)
    for _ in range(4):
        c = np.where(steps > 0, np.nextafter(c, np.float32(1)), np.where(steps < 0, np.nextafter(c, np.float32(0)), c))
        steps = steps - np.sign(steps)
    nrm = np.stack([np.sqrt(1 - c.astype(np.float64) ** 2).astype(np.float32), np.zeros_like(c), -c], -1).astype(np.float32)
    nrm[::2] = np.array([0, 0, -1], np.float32)                # half the pixels pull the cluster normal to (0, 0, -1)
    exp = check(T, R, (bgr, pts, nrm), rows, cols, REF_CALL, 2, "normals around the NA3 threshold")
    assert (exp["variance"] > 0).all()


def test_graph_capture_replays_the_same_bytes(T, R, NR):
    from kinectdepthmapenhancement_amd import filters
    W, H, rows, cols, n = 320, 240, 7, 9, 3
    frames = [synth_inputs(NR, 4, W, H, 1), ragged_inputs(NR, 9, W, H, 2, nans=True), synth_inputs(NR, 7, W, H, 2)]
    dev = [T.from_numpy(np.stack([f[j] for f in frames])).cuda() for j in range(3)]
    sp = filters.NormalAdaptiveSuperpixel(W, H, max_batch=n)
    sp.SetParametor(rows, cols, intrinsics(W, H))
    sp.segmentation_batch(*dev, *REF_CALL, 2)                  # eager; also builds the weight tables of these sigmas
    eager = [read_outputs(R, sp, k) for k in range(n)]
    T.cuda.synchronize()
    s = T.cuda.Stream()
    graph = T.cuda.CUDAGraph()
    with T.cuda.graph(graph, stream=s):                        # all captured work on the one capture stream
        sp.segmentation_batch(*dev, *REF_CALL, 2)
    for _ in range(2):
        for name in ("getLabelDevice", "getLDDevice", "getMeanDataDevice", "getCentersDevice", "getNormalsDevice", "getNormalsVarianceDevice"):
            getattr(sp, name)().zero_()
        T.cuda.synchronize()
        graph.replay()
        T.cuda.synchronize()
        for k in range(n):
            assert_identical(read_outputs(R, sp, k), eager[k], f"replay frame {k}")
    del graph
    sp.close()


def test_nasp_demo_runs(T, tmp_path):
    exe = os.path.join(ROOT, "examples", "nasp_demo")
    assert os.path.exists(exe), "examples/nasp_demo is built by __graft_entry__.build()"
    r = subprocess.run([exe, str(tmp_path)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "nasp_demo ok 640x480" in r.stdout, r.stdout + r.stderr
    for name in ("nasp_random_color.ppm", "nasp_normals.ppm"):
        assert os.path.getsize(str(tmp_path / name)) > 640 * 480 * 3
