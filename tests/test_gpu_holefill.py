"""DepthHoleFilling on the GPU (filters.DepthHoleFilling, kde_holefill_*) against the numpy statement of the rule
(holefill_cases.py).  Every comparison is on bytes: both sides perform the same IEEE binary32 operations in the same order, and
the statement is fed the library's own tables, so a last-bit difference between two libm's exp cannot fail it.

The paths of the kernel (holefill_kernels.hip) and the case that is there for each -- the list of holefill_cases.CASES says why:
  a workgroup owns one tile of 32 x 16 pixels, a thread two of them
      the copy path of a tile without a hole ......... identity (every tile), blocks and band (some tiles), every case in the
                                                       launches after its holes are closed
      partial tiles on the right and at the bottom ... every case but one_pixel (1 x 1: one tile with one pixel)
      several workgroups ............................. blocks (4 x 4 tiles), speck (3 x 3), island (2 x 4)
  the tile and a halo of k * r pixels staged in LDS, k passes on it, the exact region shrinking by r per pass
      fronts that cross tile borders inside one launch and between launches ... speck (pass_of in closed form), band, twins
      halo cells outside the frame, which are never filled ... border, one_pixel, every case at its rim
      tiles that are all hole, windows without a valid pixel ... island, speck
      every k = 1 .. 4 and the default at iterations 1 .. 2k + 1: iterations < k, not a multiple of k, one, two and three
      launches, both state images ... test_the_same_bytes_for_every_passes_per_launch
      64 passes ...................................... test_sixty_four_iterations_close_the_island
  the radius: template instances r = 1, 2, 3; the guard: off, heaviest, farthest ... speck, band, border, blocks; twins
  pass_of in place between launches, in the caller's array or the object's (pass_of_dev == NULL) ... every case
  float and uint16 on both sides, bgr_frames 1 and n, n < max_batch, a tenth of the depth invalid with NaN and +-inf ... every case
Three frames per case."""
import numpy as np
import pytest

import holefill_cases as HC
import reg_cases as RC
from gpu_util import dev

pytestmark = pytest.mark.gpu

F = np.float32
SENTINEL = 0xA5
N = 3
DTYPES = (np.float32, np.uint16)
ZR = HC.Z_RANGE

_cache = {}
_tables = {}


def _params(F_, name, radius, gap=0.0, rule=0, fuse=0, zr=ZR, **over):
    p = HC.params(name, **over)
    return F_._native.HolefillParams(radius, p["iterations"], p["min_taps"], p["sigma_space"], p["sigma_color"], gap, rule, float(zr[0]),
                                     float(zr[1]), fuse)


def _object(F_, name, radius=2, gap=0.0, rule=0, fuse=0, max_batch=N + 1, **over):
    return F_.DepthHoleFilling(HC.CASES[name].size, max_batch, _params(F_, name, radius, gap, rule, fuse, **over))


def _lib_tables(F_, name, radius, **over):
    """the library's own tables for the case's sigmas"""
    p = HC.params(name, **over)
    key = (radius, p["sigma_space"], p["sigma_color"])
    if key not in _tables:
        H = F_.DepthHoleFilling((2, 2), 1, _params(F_, name, radius, **over))
        _tables[key] = (H.space_table(), H.range_table())
        H.close()
    return _tables[key]


def _inputs(name):
    if name not in _cache:
        _cache[name] = dict(src={np.float32: HC.depth_frames(name, N), np.uint16: HC.depth_frames(name, N, integer=True).astype(np.uint16)},
                            bgr=HC.bgr_frames(name, N), want={})
    return _cache[name]


def _want(F_, name, radius, gap, rule, dt, ot, one_guide=None, **over):
    """the statement's frames, pass_of and counts, computed once per setting and shared (nothing writes to them); one_guide:
    the index of the guide every frame uses (bgr_frames 1)"""
    s = _inputs(name)
    key = (radius, gap, rule, dt, one_guide, tuple(sorted(over.items())))
    if key not in s["want"]:
        p = HC.params(name, **over)
        space, rng = _lib_tables(F_, name, radius, **over)
        r = [HC.fill_parts(d, s["bgr"][f if one_guide is None else one_guide], space, rng, radius=radius, iterations=p["iterations"],
                           min_taps=p["min_taps"], max_gap=gap, gap_rule=rule, z_min=ZR[0], z_max=ZR[1]) for f, d in enumerate(s["src"][dt])]
        z = np.stack([q["z"] for q in r])
        s["want"][key] = (z, HC.depth_to_u16(z), np.stack([q["pass_of"] for q in r]), [q["filled"] for q in r], [q["remaining"] for q in r])
    z, z16, pass_of, filled, remaining = s["want"][key]
    return (z if ot == np.float32 else z16), pass_of, filled, remaining


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


def _counts(H):
    return H.filled().tolist(), H.remaining().tolist()


@pytest.mark.parametrize("name", HC.IDS)
def test_byte_exact_against_the_statement(torch_cuda, name):
    """every radius of the case, the guard off and on (both rules), all four format pairs, n = 3 in an object for 4, filled,
    remaining and pass_of; nothing is written behind the frames of the call; pass_of_dev == NULL; bgr_frames 1"""
    from kinectdepthmapenhancement_amd import filters as F_
    torch = torch_cuda
    s = _inputs(name)
    w, h = HC.CASES[name].size
    bgr = dev(torch, s["bgr"])
    for radius in HC.CASES[name].radii:
        for gap, rule in HC.GUARDS:
            H = _object(F_, name, radius, gap, rule)
            for dt in DTYPES:
                src = _tensor(torch, s["src"][dt])
                for ot in DTYPES:
                    what = (name, radius, gap, rule, dt, ot)
                    want, pass_of, filled, remaining = _want(F_, name, radius, gap, rule, dt, ot)
                    out = _sentinel(torch, (N + 1, h, w), ot)
                    po = _sentinel(torch, (N + 1, h, w), np.uint8)
                    got = H.fill(src, bgr, out[:N], pass_of=po[:N])
                    assert got.data_ptr() == out.data_ptr()
                    _assert_equal(_host(out[:N], ot), want, what)
                    _assert_equal(po[:N].cpu().numpy(), pass_of, what + ("pass_of",))
                    assert _untouched(torch, out[N]) and _untouched(torch, po[N]), what + ("written behind the frames",)
                    assert _counts(H) == (filled, remaining), what + (_counts(H), filled, remaining)
                    assert H.filled().dtype == np.uint32
            want, _, filled, remaining = _want(F_, name, radius, gap, rule, np.float32, np.float32)
            own = H.fill(_tensor(torch, s["src"][np.float32]), bgr)                  # pass_of_dev == NULL, the object's buffer
            _assert_equal(own.cpu().numpy(), want, (name, radius, gap, rule, "no pass_of"))
            assert _counts(H) == (filled, remaining)
            want, _, filled, remaining = _want(F_, name, radius, gap, rule, np.float32, np.float32, one_guide=1)
            got = H.fill(_tensor(torch, s["src"][np.float32]), bgr[1:2])            # bgr_frames 1
            _assert_equal(got.cpu().numpy(), want, (name, radius, gap, rule, "one guide"))
            assert _counts(H) == (filled, remaining)
            H.close()
    want, pass_of, filled, remaining = _want(F_, name, HC.CASES[name].radii[0], 0.0, 0, np.float32, np.float32)
    z0 = np.stack([HC.sanitise(d, *ZR) for d in s["src"][np.float32]])
    if name == "identity":
        _assert_equal(want, z0, "identity")
        assert filled == [0] * N and remaining == [0] * N and not pass_of.any()
    if name == "one_pixel":
        assert filled == [0] * N and remaining == [1] * N and (pass_of == 255).all()
    if name == "island":
        assert all(r > 0 for r in remaining)


@pytest.mark.parametrize("name", ("speck", "blocks"))
def test_the_same_bytes_for_every_passes_per_launch(torch_cuda, name):
    """k = 1 .. 4 and the default, at iterations 1 .. 2k + 1 (for the default 1 .. 9): iterations below k, not a multiple of k,
    one, two and three launches -- the statement's bytes every time, and so the same for every k"""
    from kinectdepthmapenhancement_amd import filters as F_
    torch = torch_cuda
    s = _inputs(name)
    w, h = HC.CASES[name].size
    bgr = dev(torch, s["bgr"])
    src = _tensor(torch, s["src"][np.float32])
    for radius in HC.CASES[name].radii:
        for fuse in (0, 1, 2, 3, 4):
            for iterations in range(1, 2 * (fuse or 4) + 2):
                gap, rule = ((0.0, 0), (HC.MAX_GAP, 0), (HC.MAX_GAP, 1))[iterations % 3]
                H = _object(F_, name, radius, gap, rule, fuse, iterations=iterations)
                k = H.passes_per_launch()
                assert 1 <= k <= 4 and (fuse == 0 or k == fuse)
                want, pass_of, filled, remaining = _want(F_, name, radius, gap, rule, np.float32, np.float32, iterations=iterations)
                po = _sentinel(torch, (N, h, w), np.uint8)
                got = H.fill(src, bgr, pass_of=po)
                what = (name, radius, fuse, iterations)
                _assert_equal(got.cpu().numpy(), want, what)
                _assert_equal(po.cpu().numpy(), pass_of, what + ("pass_of",))
                assert _counts(H) == (filled, remaining), what
                H.close()


@pytest.mark.parametrize("name", HC.IDS)
def test_a_frame_gives_the_same_bytes_anywhere(torch_cuda, name):
    """alone, as frame 0, 1 or 2 of n = 3 in a max_batch of 4, and from depth, guide, output and pass_of pointers one element
    past a 16-byte boundary (with the bytes around the outputs untouched)"""
    from kinectdepthmapenhancement_amd import filters as F_
    torch = torch_cuda
    s = _inputs(name)
    w, h = HC.CASES[name].size
    gap, rule = HC.MAX_GAP, 0
    H = _object(F_, name, 2, gap, rule, max_batch=4)
    bgr = s["bgr"]
    for dt, ot in ((np.float32, np.float32), (np.uint16, np.uint16), (np.float32, np.uint16), (np.uint16, np.float32)):
        d = s["src"][dt]
        want, pass_of, filled, remaining = _want(F_, name, 2, gap, rule, dt, ot)
        fmt = torch.float32 if ot == np.float32 else torch.int16
        for f in range(N):
            po = _sentinel(torch, (1, h, w), np.uint8)
            got = H.fill(_tensor(torch, d[f:f + 1]), dev(torch, bgr[f:f + 1]), out_format=fmt, pass_of=po)           # alone
            _assert_equal(_host(got, ot), want[f:f + 1], (name, dt, ot, f, "alone"))
            _assert_equal(po.cpu().numpy(), pass_of[f:f + 1], (name, dt, ot, f, "alone", "pass_of"))
            assert _counts(H) == ([filled[f]], [remaining[f]])
            order = [(f + r) % N for r in range(N)]                                                                   # at every place of a batch of 3
            got = H.fill(_tensor(torch, d[order]), dev(torch, bgr[order]), out_format=fmt)
            _assert_equal(_host(got, ot), want[order], (name, dt, ot, order))
            assert _counts(H) == ([filled[g] for g in order], [remaining[g] for g in order])
        out, buf = _shifted(torch, np.zeros((N, h, w), ot), fill=SENTINEL)
        po, pbuf = _shifted(torch, np.zeros((N, h, w), np.uint8), 1, fill=SENTINEL)
        H.fill(_shifted(torch, d)[0], _shifted(torch, bgr, 3)[0], out, pass_of=po)
        _assert_equal(_host(out, ot), want, (name, dt, ot, "shifted"))
        _assert_equal(po.cpu().numpy(), pass_of, (name, dt, ot, "shifted", "pass_of"))
        assert _counts(H) == (filled, remaining)
        assert _untouched(torch, buf[:1]) and _untouched(torch, buf[1 + out.numel():]), (name, dt, ot, "written around the frames")
        assert _untouched(torch, pbuf[:1]) and _untouched(torch, pbuf[1 + po.numel():]), (name, dt, ot, "written around pass_of")
    H.close()


def test_graph_capture_replays_to_the_same_bytes(torch_cuda):
    """captured at the object's first call -- three fill launches and the count in a line, no allocation, no synchronisation --
    and replayed twice on changed inputs: no state, pass_of or count left over from an earlier replay"""
    from kinectdepthmapenhancement_amd import filters as F_
    torch = torch_cuda
    name = "blocks"
    s = _inputs(name)
    w, h = HC.CASES[name].size
    gap, rule = HC.MAX_GAP, 1
    H = _object(F_, name, 2, gap, rule, fuse=3)
    src, bgr = _tensor(torch, s["src"][np.float32]).clone(), dev(torch, s["bgr"]).clone()
    out = _sentinel(torch, (N, h, w), np.uint16)
    po = _sentinel(torch, (N, h, w), np.uint8)
    torch.cuda.synchronize()
    stream = torch.cuda.Stream()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=stream):
        H.fill(src, bgr, out, pass_of=po)                            # the first call of this object
    for order in ([1, 2, 0], [2, 0, 1]):
        want, pass_of, filled, remaining = _want(F_, name, 2, gap, rule, np.float32, np.uint16)
        src.copy_(_tensor(torch, s["src"][np.float32][order]))
        bgr.copy_(dev(torch, s["bgr"][order]))
        out.view(torch.uint8).fill_(SENTINEL)
        po.fill_(SENTINEL)
        H.filled_device().fill_(SENTINEL)
        H.remaining_device().fill_(SENTINEL)
        torch.cuda.synchronize()
        graph.replay()
        torch.cuda.synchronize()
        _assert_equal(_host(out, np.uint16), want[order], ("replay", order))
        _assert_equal(po.cpu().numpy(), pass_of[order], ("replay", order, "pass_of"))
        assert _counts(H) == ([filled[g] for g in order], [remaining[g] for g in order])
    out.view(torch.uint8).fill_(SENTINEL)
    H.fill(src, bgr, out)                                            # eager, after the graph
    _assert_equal(_host(out, np.uint16), want[order], "eager")
    del graph
    H.close()


def test_sixty_four_iterations_close_the_island(torch_cuda):
    from kinectdepthmapenhancement_amd import filters as F_
    torch = torch_cuda
    name = "island"
    s = _inputs(name)
    w, h = HC.CASES[name].size
    for radius, fuse in ((1, 0), (2, 3)):
        H = _object(F_, name, radius, fuse=fuse, iterations=64)
        want, pass_of, filled, remaining = _want(F_, name, radius, 0.0, 0, np.float32, np.float32, iterations=64)
        po = _sentinel(torch, (N, h, w), np.uint8)
        got = H.fill(_tensor(torch, s["src"][np.float32]), dev(torch, s["bgr"]), pass_of=po)
        _assert_equal(got.cpu().numpy(), want, (name, radius, "64 passes"))
        _assert_equal(po.cpu().numpy(), pass_of, (name, radius, "64 passes", "pass_of"))
        assert _counts(H) == (filled, remaining) and remaining == [0] * N
        assert int(pass_of.max()) >= -(-18 // radius)                # the middle of the 36 x 36 hole is 18 pixels from its rim
        H.close()


def test_in_place_is_refused_and_results_before_a_call(torch_cuda):
    """kde_hip.h: out_dev must not overlap depth_dev"""
    from kinectdepthmapenhancement_amd import filters as F_
    torch = torch_cuda
    name = "blocks"
    s = _inputs(name)
    H = _object(F_, name)
    src, bgr = _tensor(torch, s["src"][np.float32]), dev(torch, s["bgr"])
    before = src.clone()
    with pytest.raises(F_._native.KdeError, match="in place"):
        H.fill(src, bgr, src)
    with pytest.raises(F_._native.KdeError, match="in place"):
        H.fill(src[:2], bgr[:2], src[1:])                            # a partial overlap
    with pytest.raises(F_._native.KdeError, match="was not called"):
        H.filled()
    assert torch.equal(src.view(torch.int32), before.view(torch.int32))
    H.fill(src[:1], bgr[:1], src[1:2].clone())
    H.close()
    # the object-owned buffer (out_dev == NULL) is an output like any other: feeding a call's result back without a buffer for
    # the new result is in place too, whatever the number of launches and whichever format the buffer held
    for fuse, iterations in ((0, 8), (4, 3), (1, 1)):
        H = _object(F_, name, fuse=fuse, iterations=iterations)
        for fmt in (torch.float32, torch.int16):
            own = H.fill(src, bgr, out_format=fmt)
            kept = own.clone()
            with pytest.raises(F_._native.KdeError, match="in place"):
                H.fill(own, bgr)
            with pytest.raises(F_._native.KdeError, match="in place"):
                H.fill(own, bgr, out_format=torch.int16)
            with pytest.raises(F_._native.KdeError, match="in place"):
                H.fill(H.depth_device()[1:], bgr[1:])                # a part of it
            assert torch.equal(own, kept)
            more = H.fill(own, bgr, torch.empty_like(own))           # with a buffer for the result it is an ordinary call
            assert more.data_ptr() != own.data_ptr() and torch.equal(own, kept)
        H.close()


def test_registration_then_fill_then_the_joint_bilateral_filter(torch_cuda):
    """the chain of INTEGRATION.md with device pointers passed along -- DepthRegistration (point mode, which leaves cracks and
    occlusion bands), DepthHoleFilling, JointBilateralFilter -- equals the three stages called by hand with copies through the
    host in between; the first two also equal their numpy statements composed"""
    from kinectdepthmapenhancement_amd import filters as F_
    torch = torch_cuda
    (sw, sh), (ow, oh) = (40, 30), (100, 75)
    rc = RC.calib(RC.camera(sw, sh, 36.0), RC.camera(ow, oh, 95.0), RC.rotation(1.0, 0.5), (25.0, -5.0, 3.0))
    depth = RC.depth_maps(5, N, sh, sw, *ZR)
    bgr = (RC.bgr_images(5, N, oh, ow) // 8 + 100).astype(np.uint8)
    params = F_._native.HolefillParams(2, 8, 3, 2.0, 30.0, HC.MAX_GAP, 1, float(ZR[0]), float(ZR[1]), 0)

    def stages():
        R = F_.DepthRegistration((sw, sh), (ow, oh), N, F_._native.RegParams(float(ZR[0]), float(ZR[1]), 0))
        R.set_calibration(rc.Kd, rc.Kc, rc.R, rc.T)
        return R, F_.DepthHoleFilling((ow, oh), N, params), F_.JointBilateralFilter(ow, oh, max_batch=N)

    R, H, J = stages()
    g = dev(torch, bgr)
    reg = R.register(dev(torch, depth))
    filled = H.fill(reg, g)
    chained = J.process_batch(filled, g).cpu().numpy()
    reg_np, filled_np = reg.cpu().numpy(), filled.cpu().numpy()
    counts = _counts(H)
    for x in (R, H, J):
        x.close()
    R, H, J = stages()                                               # by hand: every result through the host
    reg2 = R.register(dev(torch, depth)).cpu().numpy()
    filled2 = H.fill(dev(torch, reg2), dev(torch, bgr)).cpu().numpy()
    byhand = J.process_batch(dev(torch, filled2), dev(torch, bgr)).cpu().numpy()
    for x in (R, H, J):
        x.close()
    _assert_equal(reg_np, reg2, "registered")
    _assert_equal(filled_np, filled2, "filled")
    _assert_equal(chained, byhand, "filtered")
    want_reg = np.stack([RC.statement(z, rc, (ow, oh), *ZR)[0] for z in depth])
    _assert_equal(reg_np, want_reg, "registered against its statement")
    T = F_.DepthHoleFilling((2, 2), 1, params)
    space, rng = T.space_table(), T.range_table()
    T.close()
    parts = [HC.fill_parts(z, b, space, rng, radius=2, max_gap=HC.MAX_GAP, gap_rule=1, z_min=ZR[0], z_max=ZR[1]) for z, b in zip(want_reg, bgr)]
    _assert_equal(filled_np, np.stack([p["z"] for p in parts]), "filled against its statement")
    assert counts == ([p["filled"] for p in parts], [p["remaining"] for p in parts])
    holes_in = (want_reg == 0).sum()
    assert holes_in > 0.5 * want_reg.size and sum(counts[0]) > 0.5 * holes_in      # point mode at 2.5 x: mostly cracks, mostly closed
    assert np.isfinite(chained).all() and (chained[filled_np > 0] > 0).all()


def test_python_mirrors(torch_cuda):
    """the host getters and the object-owned output buffer (out_dev == NULL) agree with the device results"""
    from kinectdepthmapenhancement_amd import filters as F_
    torch = torch_cuda
    name = "border"
    s = _inputs(name)
    w, h = HC.CASES[name].size
    H = _object(F_, name, 2, 0.0)
    bgr = dev(torch, s["bgr"])
    for dt in DTYPES:
        src = _tensor(torch, s["src"][dt])
        for ot in DTYPES:
            want, _, filled, remaining = _want(F_, name, 2, 0.0, 0, dt, ot)
            out = _sentinel(torch, (N, h, w), ot)
            H.fill(src, bgr, out)
            assert H.depth_device().data_ptr() == out.data_ptr()
            own = H.fill(src, bgr, out_format=torch.float32 if ot == np.float32 else torch.int16)
            assert own.data_ptr() != out.data_ptr() and tuple(own.shape) == (N, h, w)
            _assert_equal(_host(own, ot), want, (dt, ot, "object-owned"))
            _assert_equal(_host(out, ot), want, (dt, ot, "caller's buffer"))
            host = H.depth_host()
            assert host.dtype == ot and host.tobytes() == want.tobytes()
            assert _counts(H) == (filled, remaining)
            assert H.filled_device().cpu().numpy().view(np.uint32).reshape(-1).tolist() == filled
            assert H.remaining_device().cpu().numpy().view(np.uint32).reshape(-1).tolist() == remaining
    H.close()
