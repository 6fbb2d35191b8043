"""The shipped library above the cache threshold: one call per size-selected launch site (csrc/kde_internal.h: CacheSite) that
moves just over 256 MiB by that site's own formula, against the same frames made by calls that each stay under it.

tests/test_gpu_streaming_forms.py holds the streaming kernel forms to the references at small shapes, on the stage build with
its threshold at 0.  This file ties libkde_hip.so itself to that: a call past the threshold takes the streaming forms, the
split calls the cached forms that every other test compares with a reference, and the bytes must be the same.  The split is
chosen so that the stage's definition gives the same answer: frames are independent everywhere but in the temporal filter,
whose sequence continues on the same kind of handle from call to call.  No CPU reference runs at these sizes.

Inputs are made on the device by a seeded generator: a tenth of the samples are holes (0), float sources carry NaN and inf,
the depth-in stages take a uint16 source.  Outputs are prefilled with 0xA5 and compared as bytes, slack included.

  site (formula of the bytes a call moves)                                    the call here                 split into
  launch_p2r_any        px n 16                                               64 x VGA, depth and interp    4 x 16
  launch_points_any     px n 24                                               40 x VGA, p2r and r2p         4 x 10
  points_to_depth       n (12 + 2 or 4)            tests/test_gpu_points_to_depth.py::test_streaming_variant_above_the_cache_size
  launch_cloud          px n (source + 16) + px images 3                      64 x VGA uint16, dense;       4 x 16
                                                                              32 x VGA float3, organised    4 x 8
  launch_mesh           the cloud's + n 2 (W-1) (H-1) 12                      24 x VGA uint16 (its cloud    3 x 8
                                                                              call stays under: 155 MB)
  launch_error3d        px (truth frames truth + n sum of candidates)         64 x VGA, float3 + uint16     4 x 16
                                                                              against a float map
  launch_undist_color   (images spx + n opx) 3                                150 x VGA                     3 x 50
  launch_undist_depth   n (spx in + opx out)                                  150 x VGA uint16 to float     3 x 50
  launch_reg            n (pxd in + pxc out)                                  150 x VGA uint16 to float     3 x 50
  launch_reg_gather     n pxd (in + 3) + images pxc 3                         150 x VGA uint16              3 x 50
  kde_temporal_filter_batch   n px (in + out + 3 with a guide)                100 x VGA uint16 to float,    4 x 25 on a
                                                                              guided (1 pixel per thread)   second handle
                                                                              16 x 1080p, the same (8)      4 x 4

Every test asserts that its call is above and its pieces are below the threshold by the formula.  Each allocates less than 2 GB
and frees it.  On an MI355X: 0.01 - 0.4 s a test, 1.2 s together."""
import numpy as np
import pytest

import reg_cases as RC
import undist_cases as UD

pytestmark = pytest.mark.gpu

W, H = 640, 480
PX = W * H
CACHE = 256 << 20                                             # csrc/kde_internal.h: kCacheBytes
SENTINEL = 0xA5


@pytest.fixture
def torch(torch_cuda):
    yield torch_cuda
    torch_cuda.cuda.synchronize()
    torch_cuda.cuda.empty_cache()


def _gen(torch, seed):
    g = torch.Generator(device="cuda")
    g.manual_seed(seed)
    return g


def _out(torch, shape, dtype):
    """a tensor of the shape whose every byte is the sentinel"""
    t = torch.empty(shape, dtype=dtype, device="cuda")
    t.view(torch.uint8).fill_(SENTINEL)
    return t


def _same(torch, a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))


def _depth(torch, g, n, u16=False, w=W, h=H):
    """[n, h, w]: 600 .. 3600 mm, a tenth holes; float32 with a few NaN, inf, -0 and negatives, or int16 holding uint16"""
    z = 600.0 + 3000.0 * torch.rand((n, h, w), generator=g, device="cuda")
    z[torch.rand((n, h, w), generator=g, device="cuda") < 0.1] = 0.0
    if u16:
        return torch.round(z).to(torch.int16)
    flat = z.view(-1)
    flat[5::1009] = float("nan")
    flat[7::2003] = float("inf")
    flat[11::4001] = -0.0
    flat[13::8009] = -1000.0
    return z


def _bgr(torch, g, n, w=W, h=H):
    return torch.randint(0, 256, (n, h, w, 3), generator=g, device="cuda", dtype=torch.uint8)


def _K(w=W, h=H):
    return np.array([[525.0, 0.0, w / 2 + 0.4], [0.0, 526.5, h / 2 - 0.3], [0.0, 0.0, 1.0]])


def _pieces(n, k):
    assert n % k == 0
    return [(a, a + k) for a in range(0, n, k)]


def _split_is_right(whole, piece):
    assert piece <= CACHE < whole, (piece, CACHE, whole)


def test_p2r_depth_and_interp(torch):
    from kinectdepthmapenhancement_amd import filters as F
    n, k = 64, 16
    _split_is_right(PX * n * 16, PX * k * 16)
    depth = _depth(torch, _gen(torch, 1), n)
    conv = F.DimensionConvertor()
    conv.setCameraParameters(_K(), W, H)
    try:
        for fn in (conv.projectiveToReal, conv.projectiveToRealInterp):
            whole, parts = _out(torch, (n, H, W, 3), torch.float32), _out(torch, (n, H, W, 3), torch.float32)
            fn(depth, whole)
            for a, b in _pieces(n, k):
                fn(depth[a:b], parts[a:b])
            assert _same(torch, whole, parts), fn.__name__
            assert not bool((whole.view(torch.uint8) == SENTINEL).all(-1).any())                # every pixel was written
            del whole, parts
    finally:
        conv.close()


def test_p2r_points_and_r2p(torch):
    from kinectdepthmapenhancement_amd import filters as F
    n, k = 40, 10
    _split_is_right(PX * n * 24, PX * k * 24)
    g = _gen(torch, 2)
    pts = torch.empty((n, H, W, 3), dtype=torch.float32, device="cuda")
    pts[..., 0] = W * torch.rand((n, H, W), generator=g, device="cuda")
    pts[..., 1] = H * torch.rand((n, H, W), generator=g, device="cuda")
    pts[..., 2] = _depth(torch, g, n)
    conv = F.DimensionConvertor()
    conv.setCameraParameters(_K(), W, H)
    try:
        real = None
        for fn in (conv.projectiveToReal, conv.realToProjective):
            src = pts if real is None else real                # r2p of the cloud the first call made
            whole, parts = _out(torch, (n, H, W, 3), torch.float32), _out(torch, (n, H, W, 3), torch.float32)
            fn(src, whole)
            for a, b in _pieces(n, k):
                fn(src[a:b], parts[a:b])
            assert _same(torch, whole, parts), fn.__name__
            real = whole
    finally:
        conv.close()


@pytest.mark.parametrize("fmt,organized,n,k", [("u16", False, 64, 16), ("points", True, 32, 8)], ids=["u16-dense", "float3-organised"])
def test_cloud(torch, fmt, organized, n, k):
    from kinectdepthmapenhancement_amd import filters as F
    esz = 2 if fmt == "u16" else 12
    _split_is_right(PX * n * (esz + 16) + PX * n * 3, PX * k * (esz + 16) + PX * k * 3)
    g = _gen(torch, 3)
    z = _depth(torch, g, n, u16=fmt == "u16")
    if fmt == "points":
        src = torch.empty((n, H, W, 3), dtype=torch.float32, device="cuda")
        src[..., 0] = 4000.0 * torch.rand((n, H, W), generator=g, device="cuda") - 2000.0
        src[..., 1] = 3000.0 * torch.rand((n, H, W), generator=g, device="cuda") - 1500.0
        src[..., 2] = z
    else:
        src = z
    bgr = _bgr(torch, g, n)
    C = F.PointCloudXYZRGB(W, H, max_batch=n, organized=organized)
    try:
        C.set_camera(_K())
        whole, parts = _out(torch, (n, PX, 16), torch.uint8), _out(torch, (n, PX, 16), torch.uint8)
        C.build(src, bgr, whole)
        counts = C.counts()
        got = []
        for a, b in _pieces(n, k):
            C.build(src[a:b], bgr[a:b], parts[a:b])
            got.append(C.counts())
        assert np.array_equal(counts, np.concatenate(got))
        assert 0.8 * PX < counts.min() and counts.max() < 0.95 * PX           # holes, and a dense frame leaves slack behind its records
        assert _same(torch, whole, parts)
    finally:
        C.close()


def test_mesh(torch):
    from kinectdepthmapenhancement_amd import filters as F
    n, k = 24, 8
    slot = 2 * (W - 1) * (H - 1)
    bytes_of = lambda m: PX * m * (2 + 16) + PX * m * 3 + slot * m * 12
    _split_is_right(bytes_of(n), bytes_of(k))
    g = _gen(torch, 4)
    # a surface smooth enough that most quads are linked: a ramp with 8 mm of noise (the link is 10 mm + 2 %), a tenth holes
    y, x = torch.meshgrid(torch.arange(H, device="cuda"), torch.arange(W, device="cuda"), indexing="ij")
    z = 1200.0 + 0.8 * x + 0.5 * y + 16.0 * torch.rand((n, H, W), generator=g, device="cuda")
    z[torch.rand((n, H, W), generator=g, device="cuda") < 0.1] = 0.0
    src = torch.round(z).to(torch.int16)
    bgr = _bgr(torch, g, n)
    M = F.OrganizedMesh(W, H, max_batch=n)
    try:
        M.set_camera(_K())
        vw, tw = _out(torch, (n, PX, 16), torch.uint8), _out(torch, (n, slot, 12), torch.uint8)
        vp, tp = _out(torch, (n, PX, 16), torch.uint8), _out(torch, (n, slot, 12), torch.uint8)
        M.build(src, bgr, vw, tw)
        counts, tri = M.counts(), M.tri_counts()
        gc, gt = [], []
        for a, b in _pieces(n, k):
            M.build(src[a:b], bgr[a:b], vp[a:b], tp[a:b])
            gc.append(M.counts())
            gt.append(M.tri_counts())
        assert np.array_equal(counts, np.concatenate(gc)) and np.array_equal(tri, np.concatenate(gt))
        assert 0.2 * slot < tri.min() and tri.max() < 0.9 * slot
        assert _same(torch, vw, vp) and _same(torch, tw, tp)
    finally:
        M.close()


def test_error3d(torch):
    from kinectdepthmapenhancement_amd import filters as F
    n, k = 64, 16
    _split_is_right(PX * n * (4 + 12 + 2), PX * k * (4 + 12 + 2))
    g = _gen(torch, 5)
    truth = _depth(torch, g, n)
    E = F.MeanError3D(W, H, max_batch=n, max_candidates=2)
    try:
        E.set_camera(_K())
        cloud = torch.empty((n, H, W, 3), dtype=torch.float32, device="cuda")
        conv = F.DimensionConvertor()
        conv.setCameraParameters(_K(), W, H)
        for a, b in _pieces(n, k):                                # calls under the threshold: the candidate is an input here
            conv.projectiveToReal(truth[a:b] + 3.0, cloud[a:b])
        conv.close()
        cloud[torch.rand((n, H, W), generator=g, device="cuda") < 0.05] = 0.0
        u16 = torch.round(torch.nan_to_num(truth, 0.0, 0.0, 0.0).clamp(0.0, 60000.0) + 2.0 * torch.rand((n, H, W), generator=g, device="cuda")).to(torch.int16)
        E.compare([cloud, u16], truth)
        whole = E.results_host()
        parts = []
        for a, b in _pieces(n, k):
            E.compare([cloud[a:b], u16[a:b]], truth[a:b])
            parts.append(E.results_host())
        parts = np.concatenate(parts)
        assert whole.shape == (n, 2) and whole.tobytes() == parts.tobytes()
        assert whole["count"].min() > 0.6 * PX and whole["count"].max() < PX and np.all(whole["mean"] > 0.0) and np.all(whole["mean"] < 50.0)
    finally:
        E.close()


def _undist(F, n):
    o = F.LensUndistortion((W, H), (W, H), n, F._native.UndistParams(400.0, 6000.0, 1, 50.0))
    o.set_calibration(UD.K3(520.0, 523.0, W / 2 - 1.3, H / 2 + 0.8), [-0.25, 0.08, 0.001, -0.002, 0.01], UD.K3(400.0, 402.0, W / 2 + 0.7, H / 2 - 0.4))
    return o


def test_undist_color(torch):
    from kinectdepthmapenhancement_amd import filters as F
    n, k = 150, 50
    _split_is_right((n * PX + n * PX) * 3, (k * PX + k * PX) * 3)
    bgr = _bgr(torch, _gen(torch, 6), n)
    o = _undist(F, n)
    try:
        whole, parts = _out(torch, (n, H, W, 3), torch.uint8), _out(torch, (n, H, W, 3), torch.uint8)
        o.color(bgr, out=whole)
        for a, b in _pieces(n, k):
            o.color(bgr[a:b], out=parts[a:b])
        assert _same(torch, whole, parts)
        assert bool((whole[0] != SENTINEL).any()) and bool((whole[0] == 0).all(-1).any())       # a wider view: black outside the source
    finally:
        o.close()


def test_undist_depth(torch):
    from kinectdepthmapenhancement_amd import filters as F
    n, k = 150, 50
    _split_is_right(n * PX * (2 + 4), k * PX * (2 + 4))
    z = _depth(torch, _gen(torch, 7), n, u16=True)
    o = _undist(F, n)
    try:
        whole, parts = _out(torch, (n, H, W), torch.float32), _out(torch, (n, H, W), torch.float32)
        o.depth(z, whole)
        filled = o.filled()
        got = []
        for a, b in _pieces(n, k):
            o.depth(z[a:b], parts[a:b])
            got.append(o.filled())
        assert np.array_equal(filled, np.concatenate(got)) and 0 < filled.min() and filled.max() < PX
        assert _same(torch, whole, parts)
    finally:
        o.close()


def _reg(F, n):
    o = F.DepthRegistration((W, H), (W, H), n, F._native.RegParams(400.0, 6000.0, 3))
    o.set_calibration(RC.camera(W, H, 580.0), RC.camera(W, H, 525.0, 1.1, -0.7), RC.rotation(1.2, -0.6), (25.0, -1.5, 4.0))
    return o


def test_reg(torch):
    from kinectdepthmapenhancement_amd import filters as F
    n, k = 150, 50
    _split_is_right(n * PX * (2 + 4), k * PX * (2 + 4))
    z = _depth(torch, _gen(torch, 8), n, u16=True)
    o = _reg(F, n)
    try:
        whole, parts = _out(torch, (n, H, W), torch.float32), _out(torch, (n, H, W), torch.float32)
        o.register(z, whole)
        filled = o.filled()
        got = []
        for a, b in _pieces(n, k):
            o.register(z[a:b], parts[a:b])
            got.append(o.filled())
        assert np.array_equal(filled, np.concatenate(got)) and 0 < filled.min() and filled.max() < PX
        assert _same(torch, whole, parts)
    finally:
        o.close()


def test_reg_color_to_depth(torch):
    from kinectdepthmapenhancement_amd import filters as F
    n, k = 150, 50
    _split_is_right(n * PX * (2 + 3) + n * PX * 3, k * PX * (2 + 3) + k * PX * 3)
    g = _gen(torch, 9)
    z, bgr = _depth(torch, g, n, u16=True), _bgr(torch, g, n)
    o = _reg(F, n)
    try:
        whole, parts = _out(torch, (n, H, W, 3), torch.uint8), _out(torch, (n, H, W, 3), torch.uint8)
        o.color_to_depth(z, bgr, whole)
        for a, b in _pieces(n, k):
            o.color_to_depth(z[a:b], bgr[a:b], parts[a:b])
        assert _same(torch, whole, parts)
        assert bool((whole[0] != 0).any()) and bool((whole[0] == 0).all(-1).any())
    finally:
        o.close()


@pytest.mark.parametrize("W,H,n,k,pixels", [(640, 480, 100, 25, 1), (1920, 1080, 16, 4, 8)], ids=["100xVGA", "16x1080p"])
def test_temporal(torch, W, H, n, k, pixels):
    """the sequence in one call past the threshold on one handle, and in four calls on another, which carries its state from
    call to call: the frames, the four counts and the final state.  A thread owns one pixel at VGA and eight at 1080p
    (temporal_shape): the element stores and the 16-byte stores of the streaming form"""
    from kinectdepthmapenhancement_amd import filters as F
    PX = W * H
    _split_is_right(n * PX * (2 + 4 + 3), k * PX * (2 + 4 + 3))
    g = _gen(torch, 10)
    # a static scene with 6 mm of jitter (the link is 10 mm + 2 %), a tenth holes, a region that steps away half way through
    scene = 900.0 + 2500.0 * torch.rand((1, H, W), generator=g, device="cuda")
    z = scene + 12.0 * torch.rand((n, H, W), generator=g, device="cuda")
    z[n // 2:, :, W // 2:] += 400.0
    z[torch.rand((n, H, W), generator=g, device="cuda") < 0.1] = 0.0
    z = torch.round(z).to(torch.int16)
    bgr = _bgr(torch, g, 1, W, H).expand(n, H, W, 3).contiguous()
    bgr[n // 3:, : H // 4] = 255 - bgr[n // 3:, : H // 4]       # a colour change the guide reports
    params = F._native.TemporalParams(0.4, 10.0, 0.02, 2, 48, 400.0, 6000.0)
    a_, b_ = F.DepthTemporalFilter((W, H), n, params), F.DepthTemporalFilter((W, H), k, params)
    try:
        assert a_.shape(n)[0] == pixels and b_.shape(k)[0] == pixels
        whole, parts = _out(torch, (n, H, W), torch.float32), _out(torch, (n, H, W), torch.float32)
        a_.filter(z, bgr, whole)
        counts = {name: getattr(a_, name)() for name in ("smoothed", "jumped", "held", "changed")}
        got = {name: [] for name in counts}
        for a, b in _pieces(n, k):
            b_.filter(z[a:b], bgr[a:b], parts[a:b])
            for name in got:
                got[name].append(getattr(b_, name)())
        for name in counts:
            assert np.array_equal(counts[name], np.concatenate(got[name])), name
            assert counts[name].sum() > 0, name
        assert _same(torch, whole, parts)
        for sa, sb in zip(a_.state(), b_.state()):
            assert _same(torch, sa, sb)
    finally:
        a_.close()
        b_.close()
