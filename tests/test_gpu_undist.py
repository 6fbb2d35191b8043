"""LensUndistortion on the GPU (filters.LensUndistortion, kde_undist_*) against the numpy statement of the rule
(undist_cases.py).  Every comparison is on bytes: both sides perform the same IEEE binary32 operations in the same order.

The cases and the property of the kernels each is there for are listed in undist_cases.py (a thread owns four consecutive
output pixels, a wave 256, a workgroup 1024 in the colour kernel and eight such tiles in the depth kernel; the colour kernel
passes a whole wave's 768 bytes through LDS where the output frame starts on a 4-byte boundary and stores bytes elsewhere and
in the wave that holds the frame's end, and fetches the two taps of a row as 4 + 2 bytes where both are inside; the depth kernel
stores 16 (float) or 8 (uint16) bytes per thread where the output frame starts on such a boundary, elements elsewhere and in
the frame's last partial quad).  Three frames per case: with 41 x 19, 37 x 23, 13 x 9, 3 x 5, 257 x 1 and 131 x 67 pixels per
frame the later frames of a batch start off those boundaries, so these cases run the vector and the element stores."""
import numpy as np
import pytest

import reg_cases as RC
import undist_cases as UC
from gpu_util import dev

pytestmark = pytest.mark.gpu

F = np.float32
SENTINEL = 0xA5
N = 3
DTYPES = (np.float32, np.uint16)

_cache = {}


def _case(name):
    """the calibration, the inputs and the statement's results of a case, computed once and shared (nothing writes to them)"""
    if name not in _cache:
        k = UC.CASES[name]
        c = UC.case_calib(name)
        zr = UC.case_range(name)
        src = {np.float32: UC.depth_frames(name, N), np.uint16: UC.depth_frames(name, N, integer=True).astype(np.uint16)}
        bgr = UC.bgr_frames(name, N)
        want = {"color": np.stack([UC.color(b, c, k.out) for b in bgr]), "map": UC.undist_map(c, k.out)}
        for interp in (0, 1):
            for dt in DTYPES:
                for ot in DTYPES:
                    r = [UC.depth(d, c, k.out, *zr, interp=interp, max_gap=k.max_gap, out_dtype=ot) for d in src[dt]]
                    want[(interp, dt, ot)] = (np.stack([v for v, _ in r]), [f for _, f in r])
        _cache[name] = dict(k=k, c=c, zr=zr, src=src, bgr=bgr, want=want)
    return _cache[name]


def _object(F_, name, interp, max_batch=N + 1):
    s = _case(name)
    k = s["k"]
    U = F_.LensUndistortion(k.src, k.out, max_batch, F_._native.UndistParams(float(s["zr"][0]), float(s["zr"][1]), interp,
                                                                           float(k.max_gap) if interp else 0.0))
    U.set_calibration(k.K, k.dist, k.Knew)
    return U


def _tensor(torch, a):
    """a float32, uint8 or uint16 array on the device (uint16 as the int16 tensor that holds its bits)"""
    return dev(torch, a.view(np.int16) if a.dtype == np.uint16 else a)


def _host(t, dtype):
    a = t.cpu().numpy()
    return a.view(np.uint16) if dtype == np.uint16 else a


def _tdt(torch, dtype):
    return {np.float32: torch.float32, np.uint16: torch.int16, np.uint8: torch.uint8}[dtype]


def _sentinel(torch, shape, dtype):
    t = torch.empty(shape, dtype=_tdt(torch, dtype), device="cuda")
    t.view(torch.uint8).fill_(SENTINEL)
    return t


def _untouched(torch, t):
    return bool((t.contiguous().view(-1).view(torch.uint8) == SENTINEL).all())


def _shifted(torch, a, by=1):
    """the array on the device, `by` elements past a 16-byte boundary"""
    flat = torch.zeros(a.size + 16, dtype=_tdt(torch, a.dtype.type), device="cuda")
    assert flat.data_ptr() % 16 == 0
    view = flat[by:by + a.size].view(a.shape)
    view.copy_(_tensor(torch, a))
    assert view.data_ptr() % 16 == by * flat.element_size()
    return view


def _assert_equal(got, want, what):
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    if got.tobytes() != want.tobytes():
        bits = {4: np.uint32, 2: np.uint16, 1: np.uint8}[got.dtype.itemsize]
        bad = np.argwhere(got.view(bits) != want.view(bits))
        i = tuple(bad[0])
        raise AssertionError((what, "elements differing", len(bad), "first", i, got[i], want[i]))


@pytest.mark.parametrize("name", UC.IDS)
def test_byte_exact_against_the_statement(torch_cuda, name):
    """colour (one image per frame), the map, depth in both modes and all four format pairs, filled[f]; nothing is written
    behind the frames of the call"""
    from kinectdepthmapenhancement_amd import filters as F_
    torch = torch_cuda
    s = _case(name)
    ow, oh = s["k"].out
    for interp in (0, 1):
        U = _object(F_, name, interp)
        if interp == 0:
            out = torch.full((N + 1, oh, ow, 3), SENTINEL, dtype=torch.uint8, device="cuda")
            got = U.color(dev(torch, s["bgr"]), out=out[:N])
            assert got.data_ptr() == out.data_ptr()
            _assert_equal(out[:N].cpu().numpy(), s["want"]["color"], (name, "colour"))
            assert _untouched(torch, out[N]), (name, "colour written behind the frames")
            _assert_equal(U.map().cpu().numpy(), s["want"]["map"], (name, "map"))
        for dt in DTYPES:
            src = _tensor(torch, s["src"][dt])
            for ot in DTYPES:
                want, filled = s["want"][(interp, dt, ot)]
                out = _sentinel(torch, (N + 1, oh, ow), ot)
                got = U.depth(src, out[:N])
                assert got.data_ptr() == out.data_ptr()
                _assert_equal(_host(out[:N], ot), want, (name, interp, dt, ot))
                assert _untouched(torch, out[N]), (name, interp, "depth written behind the frames")
                f = U.filled()
                assert f.dtype == np.uint32 and f.tolist() == filled, (name, interp, dt, ot, f, filled)
        U.close()


@pytest.mark.parametrize("name", UC.IDS)
def test_a_frame_gives_the_same_bytes_anywhere(torch_cuda, name):
    """alone, as frame 0, 1 or 2 of n = 3 in a max_batch of 4, from source and output pointers one element past a 16-byte
    boundary, and with one colour image for every frame or one per frame"""
    from kinectdepthmapenhancement_amd import filters as F_
    torch = torch_cuda
    s = _case(name)
    ow, oh = s["k"].out
    U = _object(F_, name, 1, max_batch=4)
    for dt, ot in ((np.float32, np.float32), (np.uint16, np.uint16), (np.float32, np.uint16), (np.uint16, np.float32)):
        d = s["src"][dt]
        want, filled = s["want"][(1, dt, ot)]
        fmt = torch.float32 if ot == np.float32 else torch.int16
        for f in range(N):
            got = U.depth(_tensor(torch, d[f:f + 1]), out_format=fmt)                       # alone
            _assert_equal(_host(got, ot), want[f:f + 1], (name, dt, ot, f, "alone"))
            assert U.filled().tolist() == [filled[f]]
            order = [(f + r) % N for r in range(N)]                                           # at every place of a batch of 3
            got = U.depth(_tensor(torch, d[order]), out_format=fmt)
            _assert_equal(_host(got, ot), want[order], (name, dt, ot, order))
            assert U.filled().tolist() == [filled[g] for g in order]
        out = _shifted(torch, np.zeros((N, oh, ow), ot))
        U.depth(_shifted(torch, d), out)
        _assert_equal(_host(out, ot), want, (name, dt, ot, "shifted"))
        assert U.filled().tolist() == filled
    bgr, want = s["bgr"], s["want"]["color"]
    for f in range(N):
        _assert_equal(U.color(dev(torch, bgr[f:f + 1])).cpu().numpy(), want[f:f + 1], (name, "colour alone", f))
        order = [(f + r) % N for r in range(N)]
        _assert_equal(U.color(dev(torch, bgr[order])).cpu().numpy(), want[order], (name, "colour", order))
        one = U.color(dev(torch, bgr[f:f + 1]), n=N)                                          # bgr_frames 1, n 3
        _assert_equal(one.cpu().numpy(), np.stack([want[f]] * N), (name, "one image for every frame", f))
    out = _shifted(torch, np.zeros((N, oh, ow, 3), np.uint8))
    U.color(_shifted(torch, bgr, 3), out=out)
    _assert_equal(out.cpu().numpy(), want, (name, "colour shifted"))
    U.close()


def test_graph_capture_replays_to_the_same_bytes(torch_cuda):
    """a colour call and a depth call captured on one stream: three kernel nodes in a line, no allocation, no synchronisation"""
    from kinectdepthmapenhancement_amd import filters as F_
    torch = torch_cuda
    name = "barrel"
    s = _case(name)
    ow, oh = s["k"].out
    want, filled = s["want"][(1, np.float32, np.uint16)]
    U = _object(F_, name, 1)
    src, bgr = _tensor(torch, s["src"][np.float32]), dev(torch, s["bgr"])
    out = _sentinel(torch, (N, oh, ow), np.uint16)
    cout = torch.full((N, oh, ow, 3), SENTINEL, dtype=torch.uint8, device="cuda")
    U.color(bgr, out=cout)                                          # eager
    U.depth(src, out)
    _assert_equal(_host(out, np.uint16), want, "eager")
    _assert_equal(cout.cpu().numpy(), s["want"]["color"], "eager colour")
    torch.cuda.synchronize()
    stream = torch.cuda.Stream()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=stream):
        U.color(bgr, out=cout)
        U.depth(src, out)
    out.view(torch.uint8).fill_(SENTINEL)
    cout.fill_(SENTINEL)
    U.filled_device().fill_(SENTINEL)
    torch.cuda.synchronize()
    graph.replay()
    torch.cuda.synchronize()
    _assert_equal(_host(out, np.uint16), want, "replay")
    _assert_equal(cout.cpu().numpy(), s["want"]["color"], "replay colour")
    assert U.filled().tolist() == filled
    del graph
    U.close()


def test_undistorted_depth_feeds_the_registration(torch_cuda):
    """the chain: the undistorted float frames of a case go into filters.DepthRegistration as they are (its depth camera is the
    pinhole camera K_new), and the registered result is the two numpy statements chained"""
    from kinectdepthmapenhancement_amd import filters as F_
    torch = torch_cuda
    name = "rational_tangential"
    s = _case(name)
    k = s["k"]
    ow, oh = k.out
    wc, hc = 43, 29
    U = _object(F_, name, 1)
    flat = U.depth(_tensor(torch, s["src"][np.uint16]))                                       # uint16 in, float out
    want_flat, _ = s["want"][(1, np.uint16, np.float32)]
    _assert_equal(flat.cpu().numpy(), want_flat, "undistorted")
    rc = RC.calib(k.Knew, RC.camera(wc, hc, 33.0), RC.rotation(1.0, 0.5), (25.0, -5.0, 3.0))
    R = F_.DepthRegistration(k.out, (wc, hc), N, F_._native.RegParams(float(s["zr"][0]), float(s["zr"][1]), 2))
    R.set_calibration(rc.Kd, rc.Kc, rc.R, rc.T)
    reg = R.register(flat)
    want = [RC.statement(z, rc, (wc, hc), *s["zr"], max_splat=2) for z in want_flat]
    _assert_equal(reg.cpu().numpy(), np.stack([w for w, _ in want]), "registered")
    assert R.filled().tolist() == [f for _, f in want] and all(f > 0 for _, f in want)
    R.close()
    U.close()


def test_python_mirrors(torch_cuda):
    """map(), the host getters and the object-owned output buffer (out_dev == NULL) agree with the device results; a new
    calibration gives a new map"""
    from kinectdepthmapenhancement_amd import filters as F_
    torch = torch_cuda
    name = "sliver"
    s = _case(name)
    k = s["k"]
    ow, oh = k.out
    U = _object(F_, name, 1)
    m = U.map()
    assert tuple(m.shape) == (oh, ow, 2) and m.dtype == torch.float32
    _assert_equal(m.cpu().numpy(), s["want"]["map"], "map")
    assert U.map().data_ptr() == m.data_ptr()
    for dt in DTYPES:
        src = _tensor(torch, s["src"][dt])
        for ot in DTYPES:
            want, filled = s["want"][(1, dt, ot)]
            out = _sentinel(torch, (N, oh, ow), ot)
            U.depth(src, out)
            assert U.depth_device().data_ptr() == out.data_ptr()
            own = U.depth(src, out_format=torch.float32 if ot == np.float32 else torch.int16)
            assert own.data_ptr() != out.data_ptr() and tuple(own.shape) == (N, oh, ow)
            _assert_equal(_host(own, ot), want, (dt, ot, "object-owned"))
            _assert_equal(_host(out, ot), want, (dt, ot, "caller's buffer"))
            host = U.depth_host()
            assert host.dtype == ot and host.tobytes() == want.tobytes()
            assert U.filled().tolist() == filled
            assert U.filled_device().cpu().numpy().view(np.uint32).reshape(-1).tolist() == filled
    # a second calibration: the map follows it
    U.set_calibration(k.K, (0.0,) * 8, k.Knew)
    _assert_equal(U.map().cpu().numpy(), UC.undist_map(UC.calib(k.K, (0.0,) * 8, k.Knew), k.out), "map after a new calibration")
    U.close()
