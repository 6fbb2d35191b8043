"""GuidedDepthUpsampling on the GPU (filters.GuidedDepthUpsampling, kde_upsample_*) against the numpy statement of the rule
(upsample_cases.py).  Every comparison is on bytes: both sides perform the same IEEE binary32 operations in the same order, and
the statement is fed the library's own range table, so a last-bit difference between two libm's exp cannot fail it.

The paths of the kernel (upsample_kernels.hip) and the case that is there for each -- the list of upsample_cases.CASES says why:
  a workgroup takes four consecutive tiles of 32 x 8 output pixels in raster order
      one workgroup with fewer than four tiles ....... identity, one_pixel, strip (1 or 2 tiles), row's last workgroup (3 tiles)
      several workgroups, the workgroup index in the tile index, a workgroup across two tile rows .... blocks (45 tiles), cell, row
      partial tiles on the right and at the bottom ... fraction, blocks, cell, row, identity
  the tap window of a tile staged in LDS
      a window of 31 + 2r columns (equal widths) ..... strip with r = 2 and 4, identity
      a window of 2r x 2r (a tile inside one cell) ... cell
      more taps than threads (39 x 11: a second pass of the staging loop) ... strip with r = 4
      taps outside the source on every side .......... one_pixel, row (above and below), every case at its border
  the radius: template instances r = 1, 2, 3, 4, the guard with weights kept (r <= 2) and recomputed (r >= 3) ... fraction
  ties of rintf in gx_of / gy_of ..................... double, quad
  vector stores (width a multiple of 4 and the frame on a 16 / 8-byte boundary) ... double, quad, strip, row, and element stores
      for the same frames one element off a boundary (test_a_frame_gives_the_same_bytes_anywhere); element stores ... fraction,
      identity, one_pixel, cell, blocks (odd widths: frames 1 and 2 of a batch start off a boundary as well)
  float and uint16 on both sides, bgr_frames 1 and n, n < max_batch, a tenth of the depth invalid with NaN and +-inf ... every case
  zero weights (sigma_color 1): taps that are valid but weigh nothing, holes with a matching filled ... test_sigma_one_...
Three frames per case."""
import numpy as np
import pytest

import reg_cases as RC
import upsample_cases as UC
from gpu_util import dev

pytestmark = pytest.mark.gpu

F = np.float32
SENTINEL = 0xA5
N = 3
DTYPES = (np.float32, np.uint16)
ZR = UC.Z_RANGE

_cache = {}
_range = {}


def _range_table(F_, sigma):
    """the library's own table for sigma_color"""
    if sigma not in _range:
        p = F_.GuidedDepthUpsampling.default_params()
        p.sigma_color = sigma
        U = F_.GuidedDepthUpsampling((2, 2), (2, 2), 1, p)
        _range[sigma] = U.range_table()
        U.close()
    return _range[sigma]


def _inputs(name):
    if name not in _cache:
        _cache[name] = dict(src={np.float32: UC.depth_frames(name, N), np.uint16: UC.depth_frames(name, N, integer=True).astype(np.uint16)},
                            bgr=UC.bgr_frames(name, N), want={})
    return _cache[name]


def _want(F_, name, radius, gap, dt, ot, sigma=30.0, one_guide=None):
    """the statement's frames and counts, computed once per setting and shared (nothing writes to them); one_guide: the index
    of the guide every frame uses (bgr_frames 1)"""
    s = _inputs(name)
    key = (radius, gap, dt, sigma, one_guide)
    if key not in s["want"]:
        k = UC.CASES[name]
        t = UC.tables(k.src, k.out, sigma, _range_table(F_, sigma))
        r = [UC.upsample_parts(d, s["bgr"][f if one_guide is None else one_guide], t, k.out, radius, gap, *ZR) for f, d in enumerate(s["src"][dt])]
        z = np.stack([p["z"] for p in r])
        s["want"][key] = (z, UC.depth_to_u16(z), [int(p["kept"].sum()) for p in r])
    z, z16, filled = s["want"][key]
    return (z if ot == np.float32 else z16), filled


def _object(F_, name, radius=2, gap=0.0, sigma=30.0, max_batch=N + 1):
    k = UC.CASES[name]
    return F_.GuidedDepthUpsampling(k.src, k.out, max_batch, F_._native.UpsampleParams(radius, sigma, gap, float(ZR[0]), float(ZR[1])))


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


def _shifted(torch, a, by=1, fill=0):
    """the array on the device, `by` elements past a 16-byte boundary, in a buffer of `fill` bytes; returns (view, buffer)"""
    flat = torch.empty(a.size + 16, dtype=_tdt(torch, a.dtype.type), device="cuda")
    flat.view(torch.uint8).fill_(fill)
    assert flat.data_ptr() % 16 == 0
    view = flat[by:by + a.size].view(a.shape)
    view.copy_(_tensor(torch, a))
    assert view.data_ptr() % 16 == by * flat.element_size()
    return view, flat


def _assert_equal(got, want, what):
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    if got.tobytes() != want.tobytes():
        bits = {4: np.uint32, 2: np.uint16, 1: np.uint8}[got.dtype.itemsize]
        bad = np.argwhere(got.view(bits) != want.view(bits))
        i = tuple(bad[0])
        raise AssertionError((what, "elements differing", len(bad), "first", i, got[i], want[i]))


@pytest.mark.parametrize("name", UC.IDS)
def test_byte_exact_against_the_statement(torch_cuda, name):
    """every radius of the case, without and with the guard, all four format pairs, n = 3 in an object for 4, filled[f]; nothing
    is written behind the frames of the call"""
    from kinectdepthmapenhancement_amd import filters as F_
    torch = torch_cuda
    s = _inputs(name)
    ow, oh = UC.CASES[name].out
    bgr = dev(torch, s["bgr"])
    for radius in UC.RADII.get(name, (2,)):
        for gap in (0.0, UC.MAX_GAP):
            U = _object(F_, name, radius, gap)
            for dt in DTYPES:
                src = _tensor(torch, s["src"][dt])
                for ot in DTYPES:
                    want, filled = _want(F_, name, radius, gap, dt, ot)
                    out = _sentinel(torch, (N + 1, oh, ow), ot)
                    got = U.upsample(src, bgr, out[:N])
                    assert got.data_ptr() == out.data_ptr()
                    _assert_equal(_host(out[:N], ot), want, (name, radius, gap, dt, ot))
                    assert _untouched(torch, out[N]), (name, radius, gap, "written behind the frames")
                    f = U.filled()
                    assert f.dtype == np.uint32 and f.tolist() == filled, (name, radius, gap, dt, ot, f, filled)
            U.close()
    if name == "identity":                                      # r = 1 at equal sizes: the valid input itself
        want, _ = _want(F_, name, 1, 0.0, np.float32, np.float32)
        d = s["src"][np.float32]
        with np.errstate(invalid="ignore"):
            _assert_equal(want, np.where((d > ZR[0]) & (d < ZR[1]), d, F(0)).astype(np.float32), "identity")


@pytest.mark.parametrize("name", UC.IDS)
def test_sigma_one_leaves_zero_weight_holes(torch_cuda, name):
    """sigma_color 1: range[k] is 0 from k = 15 on, so most taps across the guide's noise weigh nothing -- absent by w > 0, not by
    their depth -- and pixels without a remaining tap are holes that filled does not count"""
    from kinectdepthmapenhancement_amd import filters as F_
    torch = torch_cuda
    s = _inputs(name)
    table = _range_table(F_, 1.0)
    assert table[0] == 1 and table[14] > 0 and (table[15:] == 0).all()
    px = UC.CASES[name].out[0] * UC.CASES[name].out[1]
    for gap in (0.0, UC.MAX_GAP):
        U = _object(F_, name, 2, gap, sigma=1.0)
        want, filled = _want(F_, name, 2, gap, np.float32, np.float32, sigma=1.0)
        got = U.upsample(_tensor(torch, s["src"][np.float32]), dev(torch, s["bgr"]))
        _assert_equal(got.cpu().numpy(), want, (name, gap, "sigma 1"))
        assert U.filled().tolist() == filled == [int((w != 0).sum()) for w in want]
        U.close()
        if name in ("fraction", "blocks", "double"):
            _, full = _want(F_, name, 2, gap, np.float32, np.float32)
            assert all(a < b for a, b in zip(filled, full)) and all(a < px for a in filled), (name, filled, full)


@pytest.mark.parametrize("name", UC.IDS)
def test_a_frame_gives_the_same_bytes_anywhere(torch_cuda, name):
    """alone, as frame 0, 1 or 2 of n = 3 in a max_batch of 4, from source, guide and output pointers one element past a 16-byte
    boundary (with the bytes around the output untouched), and with one guide for every frame"""
    from kinectdepthmapenhancement_amd import filters as F_
    torch = torch_cuda
    s = _inputs(name)
    ow, oh = UC.CASES[name].out
    gap = UC.MAX_GAP
    U = _object(F_, name, 2, gap, max_batch=4)
    bgr = s["bgr"]
    for dt, ot in ((np.float32, np.float32), (np.uint16, np.uint16), (np.float32, np.uint16), (np.uint16, np.float32)):
        d = s["src"][dt]
        want, filled = _want(F_, name, 2, gap, dt, ot)
        fmt = torch.float32 if ot == np.float32 else torch.int16
        for f in range(N):
            got = U.upsample(_tensor(torch, d[f:f + 1]), dev(torch, bgr[f:f + 1]), out_format=fmt)      # alone
            _assert_equal(_host(got, ot), want[f:f + 1], (name, dt, ot, f, "alone"))
            assert U.filled().tolist() == [filled[f]]
            order = [(f + r) % N for r in range(N)]                                                       # at every place of a batch of 3
            got = U.upsample(_tensor(torch, d[order]), dev(torch, bgr[order]), out_format=fmt)
            _assert_equal(_host(got, ot), want[order], (name, dt, ot, order))
            assert U.filled().tolist() == [filled[g] for g in order]
        out, buf = _shifted(torch, np.zeros((N, oh, ow), ot), fill=SENTINEL)
        U.upsample(_shifted(torch, d)[0], _shifted(torch, bgr, 3)[0], out)
        _assert_equal(_host(out, ot), want, (name, dt, ot, "shifted"))
        assert U.filled().tolist() == filled
        assert _untouched(torch, buf[:1]) and _untouched(torch, buf[1 + out.numel():]), (name, dt, ot, "written around the frames")
    for g in range(N):                                                                                    # bgr_frames 1, n 3
        want, filled = _want(F_, name, 2, gap, np.float32, np.float32, one_guide=g)
        got = U.upsample(_tensor(torch, s["src"][np.float32]), dev(torch, bgr[g:g + 1]))
        _assert_equal(got.cpu().numpy(), want, (name, "one guide for every frame", g))
        assert U.filled().tolist() == filled
    U.close()


def test_graph_capture_replays_to_the_same_bytes(torch_cuda):
    """captured at the object's first call: two kernel nodes in a line, no allocation, no synchronisation, and no count left over
    from an earlier replay"""
    from kinectdepthmapenhancement_amd import filters as F_
    torch = torch_cuda
    name = "blocks"
    s = _inputs(name)
    ow, oh = UC.CASES[name].out
    want, filled = _want(F_, name, 2, UC.MAX_GAP, np.float32, np.uint16)
    U = _object(F_, name, 2, UC.MAX_GAP)
    src, bgr = _tensor(torch, s["src"][np.float32]), dev(torch, s["bgr"])
    out = _sentinel(torch, (N, oh, ow), np.uint16)
    torch.cuda.synchronize()
    stream = torch.cuda.Stream()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=stream):
        U.upsample(src, bgr, out)                                    # the first call of this object
    for _ in range(2):
        out.view(torch.uint8).fill_(SENTINEL)
        U.filled_device().fill_(SENTINEL)
        torch.cuda.synchronize()
        graph.replay()
        torch.cuda.synchronize()
        _assert_equal(_host(out, np.uint16), want, "replay")
        assert U.filled().tolist() == filled
    out.view(torch.uint8).fill_(SENTINEL)
    U.upsample(src, bgr, out)                                        # eager, after the graph
    _assert_equal(_host(out, np.uint16), want, "eager")
    assert U.filled().tolist() == filled
    del graph
    U.close()


def test_the_result_feeds_the_joint_bilateral_filter(torch_cuda):
    """the float frames go into kde_jbf_process_batch as they are: [n, H, W] back to back, 0 for a hole, nothing else that is not
    a depth of the range"""
    from kinectdepthmapenhancement_amd import filters as F_
    torch = torch_cuda
    name = "blocks"
    s = _inputs(name)
    ow, oh = UC.CASES[name].out
    U = _object(F_, name, 2, UC.MAX_GAP)
    up = U.upsample(_tensor(torch, s["src"][np.uint16]), dev(torch, s["bgr"]))
    assert tuple(up.shape) == (N, oh, ow) and up.dtype == torch.float32 and up.is_contiguous()
    z = up.cpu().numpy()
    assert np.isfinite(z).all() and ((z == 0) | ((z > ZR[0]) & (z < ZR[1]))).all()
    J = F_.JointBilateralFilter(ow, oh, max_batch=N)
    filtered = J.process_batch(up, dev(torch, s["bgr"])).cpu().numpy()
    assert filtered.shape == (N, oh, ow) and np.isfinite(filtered).all()
    held = z != 0
    assert held.mean() > 0.9 and (filtered >= 0).all() and (filtered < ZR[1]).all() and (filtered[held] > 0).all()
    _assert_equal(up.cpu().numpy(), z, "the filter left its input alone")
    J.close()
    U.close()


def test_registration_at_the_depth_resolution_then_upsampling(torch_cuda):
    """the chain of INTEGRATION.md: DepthRegistration warps the depth into the colour camera's view at the depth camera's
    resolution (Kc scaled by src / out, principal point by the pixel-centre rule), GuidedDepthUpsampling brings it to the colour
    image's size: equal to the two numpy statements composed"""
    from kinectdepthmapenhancement_amd import filters as F_
    torch = torch_cuda
    (sw, sh), (ow, oh) = (40, 30), (100, 75)
    ax, ay = sw / ow, sh / oh
    Kc = RC.camera(ow, oh, 95.0)
    Kc_low = np.array([[Kc[0, 0] * ax, 0.0, (Kc[0, 2] + 0.5) * ax - 0.5], [0.0, Kc[1, 1] * ay, (Kc[1, 2] + 0.5) * ay - 0.5], [0.0, 0.0, 1.0]])
    rc = RC.calib(RC.camera(sw, sh, 36.0), Kc_low, RC.rotation(1.0, 0.5), (25.0, -5.0, 3.0))
    depth = RC.depth_maps(5, N, sh, sw, *ZR)
    bgr = (RC.bgr_images(5, N, oh, ow) // 8 + 100).astype(np.uint8)  # a guide of little contrast, so that most taps weigh something
    R = F_.DepthRegistration((sw, sh), (sw, sh), N, F_._native.RegParams(float(ZR[0]), float(ZR[1]), 0))
    R.set_calibration(rc.Kd, rc.Kc, rc.R, rc.T)
    low = R.register(dev(torch, depth))
    want_low = np.stack([RC.statement(z, rc, (sw, sh), *ZR)[0] for z in depth])
    _assert_equal(low.cpu().numpy(), want_low, "registered")
    U = F_.GuidedDepthUpsampling((sw, sh), (ow, oh), N, F_._native.UpsampleParams(2, 30.0, UC.MAX_GAP, float(ZR[0]), float(ZR[1])))
    up = U.upsample(low, dev(torch, bgr))
    t = UC.tables((sw, sh), (ow, oh), 30.0, _range_table(F_, 30.0))
    want = [UC.upsample(z, b, t, (ow, oh), 2, UC.MAX_GAP, *ZR) for z, b in zip(want_low, bgr)]
    _assert_equal(up.cpu().numpy(), np.stack([w for w, _ in want]), "upsampled")
    assert U.filled().tolist() == [f for _, f in want] and all(f > 0.8 * ow * oh for _, f in want)
    U.close()
    R.close()


def test_python_mirrors(torch_cuda):
    """the host getters and the object-owned output buffer (out_dev == NULL) agree with the device results"""
    from kinectdepthmapenhancement_amd import filters as F_
    torch = torch_cuda
    name = "quad"
    s = _inputs(name)
    ow, oh = UC.CASES[name].out
    U = _object(F_, name, 2, 0.0)
    bgr = dev(torch, s["bgr"])
    for dt in DTYPES:
        src = _tensor(torch, s["src"][dt])
        for ot in DTYPES:
            want, filled = _want(F_, name, 2, 0.0, dt, ot)
            out = _sentinel(torch, (N, oh, ow), ot)
            U.upsample(src, bgr, out)
            assert U.depth_device().data_ptr() == out.data_ptr()
            own = U.upsample(src, bgr, out_format=torch.float32 if ot == np.float32 else torch.int16)
            assert own.data_ptr() != out.data_ptr() and tuple(own.shape) == (N, oh, ow)
            _assert_equal(_host(own, ot), want, (dt, ot, "object-owned"))
            _assert_equal(_host(out, ot), want, (dt, ot, "caller's buffer"))
            host = U.depth_host()
            assert host.dtype == ot and host.tobytes() == want.tobytes()
            assert U.filled().tolist() == filled
            assert U.filled_device().cpu().numpy().view(np.uint32).reshape(-1).tolist() == filled
    U.close()
