"""DepthRegistration on the GPU (filters.DepthRegistration, kde_reg_*) against the numpy statement of the rule (reg_cases.py).
Every comparison is on bytes.

Shapes, and the property of the kernels each is there for (a wave of the scatter owns 256 consecutive source pixels, four per
lane, a workgroup 1024; a source frame that starts on a 16-byte (float) or 8-byte (uint16) boundary is read with vector loads by
every wave whose 256 pixels lie inside it, any other frame and the wave with the frame's end with element loads; a thread of
the finalise owns eight keys and writes them with 16-byte stores where the output frame starts on a 16-byte boundary):
  7x5 -> 7x5, 3 frames       35 pixels: one partial wave; 35 * 4 and 35 * 2 are no multiples of 16 (or 8), so the later frames of
                             every format are misaligned: element loads, element stores, a partial last octet of keys
  64x48 -> 64x48, 3 frames   3072 pixels: three workgroups, every wave whole, every frame of every format aligned: vector
                             loads and 16-byte stores only
  67x35 -> 61x37, 3 frames   ragged rows on both sides (a wave's 256 pixels span rows); the colour camera's longer focal length
                             sends source pixels out of the target on every edge
  32x24 -> 80x60, 2 frames   upscale 2.5 x: max_splat 0, 2 (spans cut), 3 and 16; splats clipped at the frame edge
  80x60 -> 32x24, 2 frames   downscale: many sources per target, empty spans in splat mode
  64x48 -> 8x8, 1 frame      a colour camera whose focal length sends every source pixel to ONE target pixel: the min of 3072
                             keys on one address, the contention case at a size that takes microseconds
  640x480 -> 640x480         one frame, 300 workgroups; Kinect-like: baseline 25 mm, a rotation of 1 degree, focal lengths 2 % apart
"""
import numpy as np
import pytest

import reg_cases as RC
from gpu_util import dev

pytestmark = pytest.mark.gpu

F = np.float32
SENTINEL = 0xA5
RANGE = (F(400), F(3000))
#        name       depth     colour     n  fd     fc      t (mm)            rotation (deg)  z range  splats
CASES = {
    "7x5":      ((7, 5), (7, 5), 3, 6.0, 6.3, (150.0, -90.0, 15.0), (2.0, 1.0), RANGE, (0, 3)),
    "64x48":    ((64, 48), (64, 48), 3, 58.0, 59.0, (120.0, -40.0, 10.0), (1.0, 0.5), None, (0, 3)),
    "67x35":    ((67, 35), (61, 37), 3, 60.0, 84.0, (60.0, 30.0, -20.0), (-1.5, 1.0), RANGE, (0, 3)),
    "up":       ((32, 24), (80, 60), 2, 30.0, 78.0, (40.0, 25.0, 5.0), (1.0, -1.0), None, (0, 2, 3, 16)),
    "down":     ((80, 60), (32, 24), 2, 75.0, 30.0, (40.0, 25.0, 5.0), (1.0, -1.0), RANGE, (0, 3)),
    "one":      ((64, 48), (8, 8), 1, 58.0, 1e-3, (25.0, 0.0, 0.0), (0.0, 0.0), RANGE, (0, 4)),
    "vga":      ((640, 480), (640, 480), 1, 575.8, 575.8 * 1.02, (25.0, 0.0, 0.0), (1.0, 0.0), None, (0, 2)),
}
IDS = list(CASES)
FIRST = IDS[:3]

_cache = {}


def _case(name):
    """the calibration and the inputs of a case, computed once and shared (nothing writes to them)"""
    if name not in _cache:
        (wd, hd), (wc, hc), n, fd, fc, t, rot, zr, splats = CASES[name]
        c = RC.calib(RC.camera(wd, hd, fd), RC.camera(wc, hc, fc, 0.4, -0.3), RC.rotation(*rot), t)
        zr = zr or (F(0), RC.FLT_MAX)
        seed = 7 * wd + hd
        df = RC.depth_maps(seed, n, hd, wd, *zr)
        du = RC.depth_maps(seed + 1, n, hd, wd, *zr, integer=True).astype(np.uint16)
        _cache[name] = dict(wd=wd, hd=hd, wc=wc, hc=hc, n=n, c=c, zr=zr, splats=splats, depth={np.float32: df, np.uint16: du}, keys={})
    return _cache[name]


def _keys(name, dtype, splat):
    """the statement's z-buffers [n, Hc, Wc] of a case's frames"""
    k = _case(name)
    key = (dtype, splat)
    if key not in k["keys"]:
        k["keys"][key] = np.stack([RC.keys(d, k["c"], (k["wc"], k["hc"]), *k["zr"], max_splat=splat) for d in k["depth"][dtype]])
    return k["keys"][key]


def _want(name, dtype, splat, out_dtype):
    zb = _keys(name, dtype, splat)
    fin = [RC.finalise(z, out_dtype) for z in zb]
    return np.stack([f[0] for f in fin]), [f[1] for f in fin]


def _object(F_, name, splat, max_batch=None):
    k = _case(name)
    R = F_.DepthRegistration((k["wd"], k["hd"]), (k["wc"], k["hc"]), max_batch or k["n"] + 1,
                             F_._native.RegParams(float(k["zr"][0]), float(k["zr"][1]), splat))
    R.set_calibration(k["c"].Kd, k["c"].Kc, k["c"].R, k["c"].T)
    return R


def _tensor(torch, a):
    """a float32 or uint16 array on the device (uint16 as the int16 tensor that holds its bits)"""
    return dev(torch, a.view(np.int16) if a.dtype == np.uint16 else a)


def _host(t, dtype):
    a = t.cpu().numpy()
    return a.view(np.uint16) if dtype == np.uint16 else a


def _sentinel(torch, shape, dtype):
    t = torch.empty(shape, dtype=torch.float32 if dtype == np.float32 else torch.int16, device="cuda")
    t.view(torch.uint8).fill_(SENTINEL)
    return t


def _untouched(t):
    return bool((t.contiguous().view(-1).view(__import__("torch").uint8) == SENTINEL).all())


def _shifted(torch, a, by=1):
    """the array on the device, `by` elements past a 16-byte boundary"""
    tdt = torch.float32 if a.dtype == np.float32 else (torch.uint8 if a.dtype == np.uint8 else torch.int16)
    flat = torch.zeros(a.size + 16, dtype=tdt, device="cuda")
    assert flat.data_ptr() % 16 == 0
    view = flat[by:by + a.size].view(a.shape)
    view.copy_(_tensor(torch, a))
    assert view.data_ptr() % 16 == by * flat.element_size()
    return view


def _assert_equal(got, want, what):
    if got.tobytes() != want.tobytes():
        bad = np.argwhere(got.view(np.uint32 if got.dtype == np.float32 else np.uint16) !=
                          want.view(np.uint32 if want.dtype == np.float32 else np.uint16))
        i = tuple(bad[0])
        raise AssertionError((what, "pixels differing", len(bad), "first", i, got[i], want[i]))


def test_the_cases_are_what_their_reasons_say():
    """no GPU needed for this, but it guards what the GPU cases are for"""
    for name in IDS:
        k = _case(name)
        px = k["wc"] * k["hc"]
        for dtype in (np.float32, np.uint16):
            d = k["depth"][dtype]
            if dtype == np.float32:
                assert np.isnan(d).any() and np.isinf(d).any() and (d < 0).any() and (d == 0).any()
                assert all((d == v).any() for v in k["zr"])
            else:
                assert (d == 0).any() and (d == 65535).any()
            filled = [RC.finalise(z)[1] for z in _keys(name, dtype, 0)]
            assert all(f > 0 for f in filled)
            if name == "one":
                assert filled == [1]
            if name == "up":
                f = {s: RC.finalise(_keys(name, dtype, s)[0])[1] for s in k["splats"]}
                assert f[0] < f[2] < f[3] <= f[16] and f[0] < 0.2 * px and f[16] > 0.6 * px
            if name == "67x35":
                kept = RC.centre_targets(np.full((k["hd"], k["wd"]), 2000, np.float32), k["c"], (k["wc"], k["hc"]))[0]
                assert not kept[0].any() and not kept[-1].any() and not kept[:, 0].any() and not kept[:, -1].any() and kept.any()


@pytest.mark.parametrize("name", IDS)
def test_register(torch_cuda, name):
    """both input formats x both output formats x the case's splat sizes: the frames, filled[f], nothing written behind the
    frames; then the object-owned buffer and the host getters"""
    from kinectdepthmapenhancement_amd import filters as F_
    torch = torch_cuda
    k = _case(name)
    n, shape = k["n"], (k["n"] + 1, k["hc"], k["wc"])
    for splat in k["splats"]:
        R = _object(F_, name, splat)
        for dtype in (np.float32, np.uint16):
            src = _tensor(torch, k["depth"][dtype])
            for out_dtype in (np.float32, np.uint16):
                want, filled = _want(name, dtype, splat, out_dtype)
                out = _sentinel(torch, shape, out_dtype)
                got = R.register(src, out[:n])
                assert got.data_ptr() == out.data_ptr() and R.depth_device().data_ptr() == out.data_ptr()
                _assert_equal(_host(out[:n], out_dtype), want, (name, splat, dtype, out_dtype))
                assert _untouched(out[n]), (name, splat, "written behind the frames")
                f = R.filled()
                assert f.dtype == np.uint32 and f.tolist() == filled, (name, splat, f, filled)
                assert R.filled_device().cpu().numpy().view(np.uint32).reshape(-1).tolist() == filled
                assert R.depth_host().tobytes() == want.tobytes()
                # the object-owned buffer, in either format
                own = R.register(src, out_format=torch.float32 if out_dtype == np.float32 else torch.int16)
                assert own.data_ptr() != out.data_ptr() and tuple(own.shape) == (n, k["hc"], k["wc"])
                _assert_equal(_host(own, out_dtype), want, (name, splat, dtype, out_dtype, "object-owned"))
                host = R.depth_host()
                assert host.dtype == out_dtype and host.tobytes() == want.tobytes() and R.filled().tolist() == filled
        R.close()


@pytest.mark.parametrize("name", IDS)
def test_a_frame_gives_the_same_bytes_anywhere(torch_cuda, name):
    """alone, at another place of a longer batch, from pointers that are no 16-byte boundary (element loads and stores); and a
    second call with a smaller n shows nothing of the first: the z-buffer starts empty in every call"""
    from kinectdepthmapenhancement_amd import filters as F_
    torch = torch_cuda
    k = _case(name)
    n = k["n"]
    splat = k["splats"][1]
    R = _object(F_, name, splat, max_batch=n + 2)
    for dtype, out_dtype in ((np.float32, np.float32), (np.uint16, np.uint16), (np.float32, np.uint16)):
        d = k["depth"][dtype]
        want, filled = _want(name, dtype, splat, out_dtype)
        order = list(range(n))[::-1] + [0, n - 1]
        got = R.register(_tensor(torch, d[order]), out_format=torch.float32 if out_dtype == np.float32 else torch.int16)
        _assert_equal(_host(got, out_dtype), want[order], (name, dtype, "reordered"))
        assert R.filled().tolist() == [filled[f] for f in order]
        for f in range(n):                                          # a smaller n straight after a larger one
            got = R.register(_tensor(torch, d[f:f + 1]), out_format=torch.float32 if out_dtype == np.float32 else torch.int16)
            _assert_equal(_host(got, out_dtype), want[f:f + 1], (name, dtype, f, "alone"))
            assert R.filled().tolist() == [filled[f]]
        for by in (1, 2):
            out = _shifted(torch, np.zeros((n, k["hc"], k["wc"]), out_dtype), by)
            R.register(_shifted(torch, d, by), out)
            _assert_equal(_host(out, out_dtype), want, (name, dtype, "shifted by", by))
            assert R.filled().tolist() == filled
    # an all-invalid frame straight after a full one: zeros and filled == 0
    for bad in (np.zeros((1, k["hd"], k["wd"]), np.float32), np.full((1, k["hd"], k["wd"]), np.nan, np.float32),
                np.full((1, k["hd"], k["wd"]), -700.0, np.float32), np.zeros((1, k["hd"], k["wd"]), np.uint16)):
        R.register(_tensor(torch, k["depth"][np.float32][:1]))
        out = _sentinel(torch, (2, k["hc"], k["wc"]), np.float32)
        R.register(_tensor(torch, bad), out[:1])
        assert not out[0].cpu().numpy().view(np.uint32).any() and _untouched(out[1]) and R.filled().tolist() == [0]
    R.close()


def test_graph_capture_replays_to_the_same_bytes(torch_cuda):
    """three kernel nodes (reset, scatter, finalise): no allocation, no synchronisation, nothing the capture refuses; the reset
    is a kernel because a memset node in its place was not kept in front of the scatter when the graph was replayed"""
    from kinectdepthmapenhancement_amd import filters as F_
    torch = torch_cuda
    name, splat = "67x35", 3
    k = _case(name)
    n = k["n"]
    want, filled = _want(name, np.float32, splat, np.uint16)
    R = _object(F_, name, splat)
    src = _tensor(torch, k["depth"][np.float32])
    out = _sentinel(torch, (n, k["hc"], k["wc"]), np.uint16)
    R.register(src, out)                                            # eager
    _assert_equal(_host(out, np.uint16), want, "eager")
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=s):
        R.register(src, out)
    for _ in range(2):
        out.view(torch.uint8).fill_(SENTINEL)
        R.filled_device().fill_(SENTINEL)
        torch.cuda.synchronize()
        graph.replay()
        torch.cuda.synchronize()
        _assert_equal(_host(out, np.uint16), want, "replay")
        assert R.filled().tolist() == filled
    # new frames through the same device buffer
    src.copy_(_tensor(torch, k["depth"][np.float32][::-1].copy()))
    graph.replay()
    torch.cuda.synchronize()
    _assert_equal(_host(out, np.uint16), want[::-1], "replay on new frames")
    del graph
    R.close()


@pytest.mark.parametrize("name", FIRST)
def test_color_to_depth(torch_cuda, name):
    """the companion gather with one image for every frame and with one per frame, both depth formats, aligned and not"""
    from kinectdepthmapenhancement_amd import filters as F_
    torch = torch_cuda
    k = _case(name)
    n = k["n"]
    bgr = RC.bgr_images(5, n, k["hc"], k["wc"])
    R = _object(F_, name, 0)
    for dtype in (np.float32, np.uint16):
        d = k["depth"][dtype]
        src = _tensor(torch, d)
        for frames in (1, n):
            want = np.stack([RC.color_to_depth(d[f], bgr[f if frames == n else 0], k["c"], *k["zr"]) for f in range(n)])
            assert want.any() and not want.all()
            out = torch.full((n + 1, k["hd"], k["wd"], 3), SENTINEL, dtype=torch.uint8, device="cuda")
            got = R.color_to_depth(src, dev(torch, bgr[:frames]), out[:n])
            assert got.data_ptr() == out.data_ptr()
            assert out[:n].cpu().numpy().tobytes() == want.tobytes(), (name, dtype, frames)
            assert _untouched(out[n])
            assert R.color_to_depth(src, dev(torch, bgr[:frames])).cpu().numpy().tobytes() == want.tobytes()
            o2 = _shifted(torch, np.zeros((n, k["hd"], k["wd"], 3), np.uint8), 1)
            R.color_to_depth(_shifted(torch, d, 1), _shifted(torch, bgr[:frames], 3), o2)
            assert o2.cpu().numpy().tobytes() == want.tobytes(), (name, dtype, frames, "shifted")
    R.close()


def test_registered_depth_feeds_the_enhancement(torch_cuda):
    """the composition: the registered float frame of the 640 x 480 case goes into KinectDepthEnhancement as it is, and the
    result is the one the statement's output gives"""
    from kinectdepthmapenhancement_amd import filters as F_
    torch = torch_cuda
    name, splat = "vga", 2
    k = _case(name)
    want, _ = _want(name, np.float32, splat, np.float32)
    R = _object(F_, name, splat)
    reg = R.register(_tensor(torch, k["depth"][np.float32]))
    _assert_equal(reg.cpu().numpy(), want, "registered")
    bgr = dev(torch, RC.bgr_images(9, 1, k["hc"], k["wc"]))
    E = F_.KinectDepthEnhancement(k["wc"], k["hc"], max_batch=1)
    E.SetParametor(15, 20, k["c"].Kc)
    E.process_batch(reg, bgr)
    got = E.getOptimizedPoints_Device().cpu().numpy().copy()
    E.process_batch(dev(torch, want), bgr)
    ref = E.getOptimizedPoints_Device().cpu().numpy()
    assert got.shape[-3:] == (k["hc"], k["wc"], 3) and got.tobytes() == ref.tobytes()
    z = got[..., 2]
    assert ((z > 50) & (z < 15000)).mean() > 0.5
    E.close()
    R.close()
