"""LabelEquivalenceSeg on the GPU (les_kernels.hip) against the CPU restatement tools/les_ref.c, through the Python class.
The bar is bit-identity of EVERY output -- merged label and merged (n, d) per pixel, size and variance per merged label;
equal NaN positions for floats -- with no pixel or cluster excluded ("Superpixel merging": under L4 and L6 every
float operation left is + - * / and fabsf in a fixed order)."""
import os
import subprocess
import zlib

import numpy as np
import pytest

import les_cases as LC
from conftest import ROOT
from gpu_util import dev
from les_cases import F

pytestmark = pytest.mark.gpu

NASP_CALL = (10.0, 50.0, 50.0, 150.0)        # KinectDepthEnhancement.cpp:67


@pytest.fixture(scope="module")
def R():
    from tools import les_ref
    les_ref.build()
    return les_ref


@pytest.fixture(scope="module")
def T(torch_cuda):
    import torch
    torch.cuda.set_device(0)
    return torch


def read_outputs(seg, frame=None):
    pick = (lambda t: t) if frame is None else (lambda t: t[frame])
    return {"merged_label": pick(seg.getMergedClusterLabel_Device()).cpu().numpy(),
            "merged_nd": pick(seg.getMergedClusterND_Device()).cpu().numpy(),
            "size": pick(seg.getMergedClusterSize_Device()).cpu().numpy(),
            "variance": pick(seg.getMergedClusterVariance_Device()).cpu().numpy()}


def params(**kw):
    from kinectdepthmapenhancement_amd import filters
    p = filters.LabelEquivalenceSeg.default_params()
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def gpu_label_image(T, case, seg=None, **kw):
    from kinectdepthmapenhancement_amd import filters
    normals, labels, centers = case
    own = seg is None
    if own:
        seg = filters.LabelEquivalenceSeg(labels.shape[1], labels.shape[0], params=params(**kw) if kw else None)
    seg.labelImage(dev(T, np.ascontiguousarray(normals, F)), dev(T, np.ascontiguousarray(labels, np.int32)),
                   dev(T, np.ascontiguousarray(centers, F)))
    out = read_outputs(seg)
    T.cuda.synchronize()
    if own:
        seg.close()
    return out


def assert_identical(got, exp, what):
    counts = LC.diff_counts(got, exp)
    print(f"{what}: differing elements {counts}; pixels with label -1 {int((exp['merged_label'] == -1).sum())}, regions "
          f"{len(set(np.unique(exp['merged_label']).tolist()) - {-1})}, NaN variances {int(np.isnan(exp['variance']).sum())}")
    assert not any(counts.values()), f"{what}: {counts}"


def check(T, R, case, what, **kw):
    exp = R.label_image(*case, **kw)
    assert_identical(gpu_label_image(T, case, **kw), exp, what)
    return exp


@pytest.mark.parametrize("it", (1, 3))
def test_goldens(T, R, it):
    exp = check(T, R, LC.golden_inputs(it), f"golden it{it}")
    g = np.load(os.path.join(LC.GOLDEN, f"les_it{it}.npz"))
    assert np.array_equal(exp["merged_label"], g["merged_label"].astype(np.int32)) and np.array_equal(LC.ubits(exp["merged_nd"]), g["merged_nd"])


_nasp = {}


def nasp_outputs(T, W, H, rows, cols, seeds=(1,)):
    """full NASP output computed on the device (normals by NormalMapGenerator), kept on the device: labels [n,H,W],
    centres and normals [n, rows*cols, 3]"""
    key = (W, H, rows, cols, seeds)
    if key not in _nasp:
        from kinectdepthmapenhancement_amd import filters, synth
        K = synth.intrinsics(W, H)
        n = len(seeds)
        frames = [synth.make_frame(s, W, H) for s in seeds]
        bgr = dev(T, np.stack([f[0] for f in frames]))
        depth = dev(T, np.stack([f[1] for f in frames]))
        conv = filters.DimensionConvertor()
        conv.setCameraParameters(K, W, H)
        pts = T.empty((n, H, W, 3), dtype=T.float32, device="cuda")
        conv.projectiveToReal(depth, pts)
        g = filters.NormalMapGenerator(W, H, max_batch=n)
        g.setNormalEstimationMethods(g.CM)
        nrm = T.empty((n, H, W, 3), dtype=T.float32, device="cuda")
        g.generateNormalMapBatch(n, pts, nrm)
        sp = filters.NormalAdaptiveSuperpixel(W, H, max_batch=n)
        sp.SetParametor(rows, cols, K)
        sp.segmentation_batch(bgr, pts, nrm, *NASP_CALL, 1)
        k = rows * cols
        out = (sp.getNormalsDevice().reshape(n, k, 3).clone(), sp.getLabelDevice().reshape(n, H, W).clone(),
               sp.getCentersDevice().reshape(n, k, 3).clone())
        T.cuda.synchronize()
        sp.close(); g.close(); conv.close()
        _nasp[key] = out
    return _nasp[key]


@pytest.mark.parametrize("W,H,rows,cols", [(640, 480, 15, 20), (1920, 1080, 15, 20), (1920, 1080, 40, 40), (333, 250, 7, 9)])
def test_nasp_output_fed_straight_in(T, R, W, H, rows, cols):
    """NASP's four cluster outputs on the device -> labelImage; 333 x 250 is divisible by neither 32 nor 24"""
    from kinectdepthmapenhancement_amd import filters
    normals, labels, centers = [t[0] for t in nasp_outputs(T, W, H, rows, cols)]
    seg = filters.LabelEquivalenceSeg(W, H)
    seg.labelImage(normals, labels, centers, None)
    got = read_outputs(seg)
    exp = R.label_image(normals.cpu().numpy(), labels.cpu().numpy(), centers.cpu().numpy())
    assert_identical(got, exp, f"NASP {W}x{H} {rows}x{cols}")
    nreg = len(set(np.unique(exp["merged_label"]).tolist()) - {-1})
    assert 1 < nreg < rows * cols and exp["changed"][0] > 0
    assert np.array_equal(seg.getMergedClusterLabel_Host(), got["merged_label"]) and LC.differing(seg.getMergedClusterND_Host(), got["merged_nd"]) == 0
    img, segimg = seg.getNormalImg(), seg.getSegmentResult()
    assert img.shape == (H, W, 3) and (img[got["merged_label"] == -1] == 0).all() and img.any() and segimg.shape == (H, W, 3)
    seg.close()


def test_micro_cases(T, R):
    for deg, extra in ((10, 0.0), (30, 0.0), (10, 200.0), (0, 0.0)):
        check(T, R, LC.two_halves(deg, extra), f"two halves {deg} deg, +{extra} mm")
    exp = check(T, R, LC.wrap_case(False), "wrap")
    assert exp["merged_label"][2, 15] == 1
    exp = check(T, R, LC.wrap_case(True), "wrap swapped")
    assert exp["merged_label"][2, 15] == 1 and exp["merged_label"][3, 0] == 2
    normals = np.stack([LC.tilted(0), LC.tilted(10)])
    centers = (F(1000) * normals).astype(F)
    for fill, (yy, xx), val in ((1, (3, 7), 0), (0, (3, 7), 1), (0, (3, slice(None)), 1)):
        labels = np.full((4, 8), fill, np.int32)
        labels[yy, xx] = val
        check(T, R, (normals, labels, centers), "last row / last column")
    for W, H in ((1, 9), (9, 1)):
        check(T, R, (normals, (np.arange(W * H).reshape(H, W) >= 4).astype(np.int32), centers), f"{W}x{H}")
    check(T, R, (normals[:1], np.zeros((1, 1), np.int32), centers[:1]), "1x1")


def test_unconverged_chain(T, R):
    exp = check(T, R, LC.chain_case(False), "chain, 10 rounds")
    assert [int(exp["merged_label"][1, 4 * k]) for k in range(16)] == [max(k - 10, 0) for k in range(16)]
    exp = check(T, R, LC.chain_case(False), "chain, 15 rounds", iterations=15)
    assert (exp["merged_label"][1:] == 0).all()
    check(T, R, LC.chain_case(False), "chain, 14 rounds", iterations=14)
    exp = check(T, R, LC.chain_case(True), "chain with a valid row 0")
    assert (exp["merged_label"][1:] == 0).all()


def test_pixels_without_superpixel_bad_normals_and_a_used_handle(T, R):
    """L1, L7, and L5: a second call with other inputs on the same handle leaves no trace of the first"""
    from kinectdepthmapenhancement_amd import filters
    normals = np.stack([LC.tilted(0), np.full(3, -1, F), LC.tilted(10), np.array([-1, -1, 0.5], F)])
    centers = (F(1000) * normals).astype(F)
    labels = np.zeros((6, 16), np.int32)
    labels[:, 4:8], labels[:, 8:12], labels[:, 12:] = 1, 2, 3
    labels[0, 0], labels[5, 9], labels[2, 2] = -1, 4, 1 << 20
    exp = check(T, R, (normals, labels, centers), "no superpixel / bad normals")
    assert (exp["merged_nd"][exp["merged_label"] == -1] == 0).all() and (exp["merged_label"][:, 12:] == -1).all()
    seg = filters.LabelEquivalenceSeg(16, 6)
    first = gpu_label_image(T, LC.two_halves(10), seg=seg)
    assert (first["merged_label"] == 0).all()
    assert_identical(gpu_label_image(T, (normals, labels, centers), seg=seg), exp, "second call on a used handle")
    assert_identical(gpu_label_image(T, LC.random_case(9, 16, 6, 30), seg=seg), R.label_image(*LC.random_case(9, 16, 6, 30)),
                     "third call, more superpixels")
    seg.close()


@pytest.mark.parametrize("seed,W,H,nc", LC.RANDOM_SHAPES + [(11, 160, 120, 700), (12, 97, 61, 2048)])
def test_random_label_maps(T, R, seed, W, H, nc):
    nc = min(nc, W * H)
    case = LC.random_case(seed, W, H, nc)
    check(T, R, case, f"random {W}x{H} nc {nc}")
    for kw in ({"iterations": 0}, {"iterations": 1}, {"max_angle": 1.2, "max_plane_distance": 30.0},
               {"max_angle": 4.0, "max_plane_distance": 1e9, "iterations": 3}):
        check(T, R, case, f"random {W}x{H} nc {nc} {kw}", **kw)


def batch_inputs(T):
    W, H, rows, cols = 320, 240, 7, 9
    normals, labels, centers = [t.clone() for t in nasp_outputs(T, W, H, rows, cols, seeds=(4, 5, 7))]
    rnd = LC.random_case(21, W, H, rows * cols)
    extra = [dev(T, np.ascontiguousarray(a))[None] for a in rnd]
    return W, H, T.cat([normals, extra[0]]), T.cat([labels, extra[1]]), T.cat([centers, extra[2]])


def test_batch_equals_single_calls_on_a_side_stream(T, R):
    from kinectdepthmapenhancement_amd import filters
    W, H, normals, labels, centers = batch_inputs(T)
    n = normals.shape[0]
    singles = [gpu_label_image(T, (normals[k].cpu().numpy(), labels[k].cpu().numpy(), centers[k].cpu().numpy())) for k in range(n)]
    for k in range(n):
        assert_identical(singles[k], R.label_image(normals[k].cpu().numpy(), labels[k].cpu().numpy(), centers[k].cpu().numpy()), f"single {k}")
    seg = filters.LabelEquivalenceSeg(W, H, max_batch=n + 1)
    T.cuda.synchronize()
    s = T.cuda.Stream()
    for order in (list(range(n)), [3, 0, 2, 1]):
        idx = T.tensor(order, device="cuda")
        a, b, c = normals[idx].contiguous(), labels[idx].contiguous(), centers[idx].contiguous()
        T.cuda.synchronize()
        with T.cuda.stream(s):
            seg.label_image_batch(a, b, c)
        s.synchronize()
        for pos, k in enumerate(order):
            assert_identical(read_outputs(seg, pos), singles[k], f"batch order {order} position {pos}")
    seg.close()


def test_graph_capture_replays_the_same_bytes(T, R):
    from kinectdepthmapenhancement_amd import filters
    W, H, normals, labels, centers = batch_inputs(T)
    n = normals.shape[0]
    seg = filters.LabelEquivalenceSeg(W, H, max_batch=n)
    seg.label_image_batch(normals, labels, centers)
    eager = [read_outputs(seg, k) for k in range(n)]
    T.cuda.synchronize()
    s = T.cuda.Stream()
    graph = T.cuda.CUDAGraph()
    with T.cuda.graph(graph, stream=s):
        seg.label_image_batch(normals, labels, centers)
    for _ in range(2):
        for name in ("getMergedClusterLabel_Device", "getMergedClusterND_Device", "getMergedClusterSize_Device", "getMergedClusterVariance_Device"):
            getattr(seg, name)().fill_(7)
        T.cuda.synchronize()
        graph.replay()
        T.cuda.synchronize()
        for k in range(n):
            assert_identical(read_outputs(seg, k), eager[k], f"replay frame {k}")
    del graph
    seg.close()


def test_argument_checks(T):
    from kinectdepthmapenhancement_amd import filters, _native
    seg = filters.LabelEquivalenceSeg(64, 48)
    lab = T.zeros((48, 64), dtype=T.int32, device="cuda")
    for k in (0, 2049):
        with pytest.raises((_native.KdeError, ValueError)):
            seg.labelImage(T.zeros((k, 3), device="cuda"), lab, T.zeros((k, 3), device="cuda"))
    with pytest.raises(_native.KdeError):
        seg.label_image_batch(T.zeros((2, 4, 3), device="cuda"), T.zeros((2, 48, 64), dtype=T.int32, device="cuda"), T.zeros((2, 4, 3), device="cuda"))
    seg.close()
    small = filters.LabelEquivalenceSeg(4, 3)
    with pytest.raises(_native.KdeError):                      # n_clusters > W*H
        small.labelImage(T.zeros((13, 3), device="cuda"), T.zeros((3, 4), dtype=T.int32, device="cuda"), T.zeros((13, 3), device="cuda"))
    small.close()
    with pytest.raises(_native.KdeError):
        filters.LabelEquivalenceSeg(64, 48, params=params(iterations=-1))


def test_les_demo_agrees_with_the_python_path(T, tmp_path):
    """examples/les_demo = nasp_demo plus kde::LabelEquivalenceSeg::labelImage on the same synthetic frame; it prints the
    number of merged regions and the CRC-32 of the merged label image"""
    from kinectdepthmapenhancement_amd import filters
    exe = os.path.join(ROOT, "examples", "les_demo")
    assert os.path.exists(exe), "examples/les_demo is built by __graft_entry__.build()"
    r = subprocess.run([exe, str(tmp_path)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "les_demo ok 640x480" in r.stdout, r.stdout + r.stderr
    tok = r.stdout.split("les_demo ok 640x480")[1].split()
    regions, crc = int(tok[tok.index("regions") + 1]), int(tok[tok.index("crc32") + 1], 16)
    for name in ("les_segments.ppm", "les_normals.ppm"):
        assert os.path.getsize(str(tmp_path / name)) > 640 * 480 * 3
    # the same chain in Python, on the demo's inputs (it writes them next to the images)
    raw = lambda name, dt, shape: dev(T, np.fromfile(str(tmp_path / name), dt).reshape(shape))
    normals, labels, centers = raw("les_in_normals.bin", F, (300, 3)), raw("les_in_labels.bin", np.int32, (480, 640)), raw("les_in_centers.bin", F, (300, 3))
    seg = filters.LabelEquivalenceSeg(640, 480)
    seg.labelImage(normals, labels, centers)
    m = seg.getMergedClusterLabel_Host()
    assert len(set(np.unique(m).tolist()) - {-1}) == regions and (zlib.crc32(m.tobytes()) & 0xFFFFFFFF) == crc
    assert 1 < regions < 300
    seg.close()
