"""DepthSpeckleFilter on the GPU (filters.DepthSpeckleFilter, kde_speckle_*) against the numpy statement of the rule
(speckle_cases.py): the bytes of the depth and of the labels and all three counts.  Labels are component minima and the counts
integer sums, so nothing depends on the order in which atomics land, and capped is 0 everywhere.

The paths of the kernels (speckle_kernels.hip) and the case that is there for each -- speckle_cases.CASES says why:
  S1 tile     the no-valid-pixel path ... all_invalid, comb, corner, snake's gaps;  the fully-linked path ... identity, stairs
              unions in LDS ... every other case; partial tiles right and below ... every case but comb and corner
              unions that meet on chains other threads are compressing ... lost_link, 200 runs (test_no_link_is_lost_...)
  S2 seam     column and row seams, 4 and 8 ... identity, snake, comb; diagonal pairs at seams and four-tile corners ... checker,
              corner; no seam at all (one tile: three launches) ... one_pixel
  S3 resolve  sizes summed over the local roots of four tiles ... corner; over many ... snake, comb
  S4 apply    float and uint16 on both sides, labels or none, in place ... every case
Three frames per case."""
import numpy as np
import pytest

import reg_cases as RC
import speckle_cases as SC
from gpu_util import dev

pytestmark = pytest.mark.gpu

SENTINEL = 0xA5
N = 3
DTYPES = (np.float32, np.uint16)

_cache = {}


def _params(F_, name, conn, min_size):
    p = SC.params(name, connectivity=conn, min_size=min_size)
    return F_._native.SpeckleParams(p["min_size"], p["max_diff"], p["rel_diff"], p["connectivity"], p["z_min"], p["z_max"])


def _object(F_, name, conn=4, min_size=None, max_batch=N + 1):
    return F_.DepthSpeckleFilter(SC.CASES[name].size, max_batch, _params(F_, name, conn, SC.min_size_of(name) if min_size is None else min_size))


def _inputs(name):
    if name not in _cache:
        _cache[name] = dict(src={np.float32: SC.depth_frames(name), np.uint16: SC.depth_frames(name, integer=True).astype(np.uint16)}, want={})
    return _cache[name]


def _want(name, conn, min_size, dt, ot):
    """the statement's frames, labels and counts, computed once per setting and shared (nothing writes to them)"""
    s = _inputs(name)
    key = (conn, min_size, dt)
    if key not in s["want"]:
        z, labels, removed, comps = SC.filter_batch(s["src"][dt], np.float32, **SC.params(name, connectivity=conn, min_size=min_size))
        s["want"][key] = (z, SC.depth_to_u16(z), labels, removed.tolist(), comps.tolist())
    z, z16, labels, removed, comps = s["want"][key]
    return (z if ot == np.float32 else z16), labels, removed, comps


def _tensor(torch, a):
    return dev(torch, a.view(np.int16) if a.dtype == np.uint16 else a)


def _host(t, dtype):
    a = t.cpu().numpy()
    return a.view(np.uint16) if dtype == np.uint16 else a


def _tdt(torch, dtype):
    return {np.float32: torch.float32, np.uint16: torch.int16, np.int32: torch.int32}[dtype]


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
    capped = H.capped().tolist()
    assert capped == [0] * len(capped), ("capped", capped)
    return H.removed().tolist(), H.components().tolist()


def _min_sizes(name):
    own = SC.min_size_of(name)
    return (1, own, own + 1, SC.HUGE) if name == "snake" else (1, own, SC.HUGE)


@pytest.mark.parametrize("name", SC.IDS)
def test_byte_exact_against_the_statement(torch_cuda, name):
    """connectivity 4 and 8, min_size 1, the case's own and a huge one, all four format pairs, n = 3 in an object for 4, depth,
    labels, removed, components, capped; nothing is written behind the frames of the call; labels_dev == NULL"""
    from kinectdepthmapenhancement_amd import filters as F_
    torch = torch_cuda
    s = _inputs(name)
    w, h = SC.CASES[name].size
    for conn in (4, 8):
        for min_size in _min_sizes(name):
            H = _object(F_, name, conn, min_size)
            for dt in DTYPES:
                src = _tensor(torch, s["src"][dt])
                for ot in DTYPES:
                    what = (name, conn, min_size, dt, ot)
                    want, labels, removed, comps = _want(name, conn, min_size, dt, ot)
                    out = _sentinel(torch, (N + 1, h, w), ot)
                    lab = _sentinel(torch, (N + 1, h, w), np.int32)
                    got = H.filter(src, out[:N], labels=lab[:N])
                    assert got.data_ptr() == out.data_ptr()
                    _assert_equal(_host(out[:N], ot), want, what)
                    _assert_equal(lab[:N].cpu().numpy(), labels, what + ("labels",))
                    assert _untouched(torch, out[N]) and _untouched(torch, lab[N]), what + ("written behind the frames",)
                    assert _counts(H) == (removed, comps), what + (_counts(H), removed, comps)
                    assert H.removed().dtype == np.uint32
            want, _, removed, comps = _want(name, conn, min_size, np.float32, np.float32)
            own = H.filter(_tensor(torch, s["src"][np.float32]))                   # labels_dev == NULL, the object's buffer
            _assert_equal(own.cpu().numpy(), want, (name, conn, min_size, "no labels"))
            assert _counts(H) == (removed, comps)
            if min_size == 1:                                                     # plain labelling: nothing removed
                assert removed == [0] * N
                _assert_equal(want, np.stack([SC.sanitise(d, SC.params(name)["z_min"], SC.params(name)["z_max"]) for d in s["src"][np.float32]]),
                              (name, "min_size 1"))
            if min_size == SC.HUGE:
                assert not want.any() and comps == [0] * N
            H.close()


def test_no_link_is_lost_between_concurrent_unions(torch_cuda):
    """`lost_link` 200 times over: 48 copies of the tile per run whose unions in LDS lost a link in about one run of fifty under
    the first path compression of kde_union.h (found by the randomised sweep, tests/stage_sweep.py: speckle, seed 1, index 234).
    The labels are component minima, so every run gives the statement's bytes whatever the order of the atomics."""
    from kinectdepthmapenhancement_amd import filters as F_
    torch = torch_cuda
    name = "lost_link"
    H = _object(F_, name, 4, 1)
    src = _tensor(torch, _inputs(name)["src"][np.uint16])
    want, labels, removed, comps = _want(name, 4, 1, np.uint16, np.uint16)
    lab = torch.empty((N,) + want.shape[1:], dtype=torch.int32, device="cuda")
    want_labels = torch.from_numpy(labels).cuda()
    wrong = []
    for run in range(200):
        out = H.filter(src, out_format=torch.int16, labels=lab)
        if not torch.equal(lab, want_labels) or _counts(H) != (removed, comps):
            wrong.append((run, int((lab != want_labels).sum()), H.components().tolist()))
    _assert_equal(_host(out, np.uint16), want, (name, "depth"))
    assert not wrong, (len(wrong), "runs of 200 differ: (run, labels differing, components)", wrong[:5], "want", comps)
    H.close()


@pytest.mark.parametrize("name", SC.IDS)
def test_a_frame_gives_the_same_bytes_anywhere_and_in_place(torch_cuda, name):
    """alone, as frame 0, 1 or 2 of n = 3 in a max_batch of 4, from depth, output and label pointers one element past a 16-byte
    boundary (with the bytes around the outputs untouched), and in place in both formats"""
    from kinectdepthmapenhancement_amd import filters as F_
    torch = torch_cuda
    s = _inputs(name)
    w, h = SC.CASES[name].size
    conn, min_size = 8, SC.min_size_of(name)
    H = _object(F_, name, conn, max_batch=4)
    for dt, ot in ((np.float32, np.float32), (np.uint16, np.uint16), (np.float32, np.uint16), (np.uint16, np.float32)):
        d = s["src"][dt]
        want, labels, removed, comps = _want(name, conn, min_size, dt, ot)
        fmt = torch.float32 if ot == np.float32 else torch.int16
        for f in range(N):
            lab = _sentinel(torch, (1, h, w), np.int32)
            got = H.filter(_tensor(torch, d[f:f + 1]), out_format=fmt, labels=lab)                                    # alone
            _assert_equal(_host(got, ot), want[f:f + 1], (name, dt, ot, f, "alone"))
            _assert_equal(lab.cpu().numpy(), labels[f:f + 1], (name, dt, ot, f, "alone", "labels"))
            assert _counts(H) == ([removed[f]], [comps[f]])
            order = [(f + r) % N for r in range(N)]                                                                   # at every place of a batch of 3
            got = H.filter(_tensor(torch, d[order]), out_format=fmt)
            _assert_equal(_host(got, ot), want[order], (name, dt, ot, order))
            assert _counts(H) == ([removed[g] for g in order], [comps[g] for g in order])
        out, buf = _shifted(torch, np.zeros((N, h, w), ot), fill=SENTINEL)
        lab, lbuf = _shifted(torch, np.zeros((N, h, w), np.int32), 1, fill=SENTINEL)
        H.filter(_shifted(torch, d)[0], out, labels=lab)
        _assert_equal(_host(out, ot), want, (name, dt, ot, "shifted"))
        _assert_equal(lab.cpu().numpy(), labels, (name, dt, ot, "shifted", "labels"))
        assert _counts(H) == (removed, comps)
        assert _untouched(torch, buf[:1]) and _untouched(torch, buf[1 + out.numel():]), (name, dt, ot, "written around the frames")
        assert _untouched(torch, lbuf[:1]) and _untouched(torch, lbuf[1 + lab.numel():]), (name, dt, ot, "written around the labels")
        if dt == ot:                                                                                                  # in place
            src = _tensor(torch, d).clone()
            lab = _sentinel(torch, (N, h, w), np.int32)
            got = H.filter(src, src, labels=lab)
            assert got.data_ptr() == src.data_ptr()
            _assert_equal(_host(src, ot), want, (name, dt, "in place"))
            _assert_equal(lab.cpu().numpy(), labels, (name, dt, "in place", "labels"))
            assert _counts(H) == (removed, comps)
    H.close()


def test_graph_capture_replays_to_the_same_bytes(torch_cuda):
    """captured at the object's first call -- five kernels in a line, no memset node, no allocation, no synchronisation -- and
    replayed twice on changed inputs: no parent, size or count left over from an earlier replay"""
    from kinectdepthmapenhancement_amd import filters as F_
    torch = torch_cuda
    name, conn = "frame", 8
    min_size = SC.min_size_of(name)
    s = _inputs(name)
    w, h = SC.CASES[name].size
    H = _object(F_, name, conn)
    src = _tensor(torch, s["src"][np.float32]).clone()
    out = _sentinel(torch, (N, h, w), np.uint16)
    lab = _sentinel(torch, (N, h, w), np.int32)
    torch.cuda.synchronize()
    stream = torch.cuda.Stream()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=stream):
        H.filter(src, out, labels=lab)                                # the first call of this object
    want, labels, removed, comps = _want(name, conn, min_size, np.float32, np.uint16)
    for order in ([1, 2, 0], [2, 0, 1]):
        src.copy_(_tensor(torch, s["src"][np.float32][order]))
        out.view(torch.uint8).fill_(SENTINEL)
        lab.view(torch.uint8).fill_(SENTINEL)
        for counts in (H.removed_device(), H.components_device(), H.capped_device()):
            counts.fill_(SENTINEL)
        torch.cuda.synchronize()
        graph.replay()
        torch.cuda.synchronize()
        _assert_equal(_host(out, np.uint16), want[order], ("replay", order))
        _assert_equal(lab.cpu().numpy(), labels[order], ("replay", order, "labels"))
        assert _counts(H) == ([removed[g] for g in order], [comps[g] for g in order])
    out.view(torch.uint8).fill_(SENTINEL)
    H.filter(src, out)                                                # eager, after the graph
    _assert_equal(_host(out, np.uint16), want[order], "eager")
    del graph
    H.close()


def test_the_in_place_rule_and_results_before_a_call(torch_cuda):
    """kde_hip.h: in place exactly when out_dev == depth_dev and out_format == depth_format; any other overlap is refused"""
    from kinectdepthmapenhancement_amd import filters as F_
    torch = torch_cuda
    name = "noise"
    s = _inputs(name)
    H = _object(F_, name)
    src = _tensor(torch, s["src"][np.float32])
    before = src.clone()
    with pytest.raises(F_._native.KdeError, match="was not called"):
        H.removed()
    with pytest.raises(F_._native.KdeError, match="in place"):
        H.filter(src[:2], src[1:])                                    # a partial overlap
    with pytest.raises(F_._native.KdeError, match="in place"):
        H.filter(src, src.view(torch.int16).view(-1)[:src.numel()].view(src.shape))     # the same pointer in another format
    with pytest.raises(F_._native.KdeError, match="labels_dev overlaps"):
        H.filter(src, labels=src.view(torch.int32))
    assert torch.equal(src.view(torch.int32), before.view(torch.int32))
    own = H.filter(src)
    kept = own.clone()
    with pytest.raises(F_._native.KdeError, match="in place"):
        H.filter(own)                                                 # out_dev == NULL selects the buffer `own` lies in
    with pytest.raises(F_._native.KdeError, match="in place"):
        H.filter(H.depth_device()[1:])
    assert torch.equal(own, kept)
    again = H.filter(own, own)                                        # named as the output it is an in-place call
    assert again.data_ptr() == own.data_ptr() and torch.equal(own, kept)      # and filtering twice changes nothing here
    with pytest.raises(AttributeError):
        H.filled()
    H.close()


def test_registration_then_speckle_then_fill_then_the_joint_bilateral_filter(torch_cuda):
    """the chain of INTEGRATION.md with device pointers passed along -- DepthRegistration (point mode, which lets the background
    show through the cracks of the foreground), DepthSpeckleFilter, DepthHoleFilling, JointBilateralFilter -- equals the four
    stages called by hand with copies through the host in between; the speckle stage also equals its statement"""
    from kinectdepthmapenhancement_amd import filters as F_
    torch = torch_cuda
    ZR = SC.Z_RANGE
    (sw, sh), (ow, oh) = (40, 30), (100, 75)
    rc = RC.calib(RC.camera(sw, sh, 36.0), RC.camera(ow, oh, 95.0), RC.rotation(1.0, 0.5), (25.0, -5.0, 3.0))
    depth = RC.depth_maps(5, N, sh, sw, *ZR)
    bgr = (RC.bgr_images(5, N, oh, ow) // 8 + 100).astype(np.uint8)
    sp = dict(min_size=6, max_diff=10.0, rel_diff=0.02, connectivity=8, z_min=ZR[0], z_max=ZR[1])

    def stages():
        R = F_.DepthRegistration((sw, sh), (ow, oh), N, F_._native.RegParams(float(ZR[0]), float(ZR[1]), 0))
        R.set_calibration(rc.Kd, rc.Kc, rc.R, rc.T)
        S = F_.DepthSpeckleFilter((ow, oh), N, F_._native.SpeckleParams(sp["min_size"], sp["max_diff"], sp["rel_diff"], sp["connectivity"],
                                                                        sp["z_min"], sp["z_max"]))
        H = F_.DepthHoleFilling((ow, oh), N, F_._native.HolefillParams(2, 8, 3, 2.0, 30.0, 100.0, 1, float(ZR[0]), float(ZR[1]), 0))
        return R, S, H, F_.JointBilateralFilter(ow, oh, max_batch=N)

    R, S, H, J = stages()
    g = dev(torch, bgr)
    reg = R.register(dev(torch, depth))
    clean = S.filter(reg)
    filled = H.fill(clean, g)
    chained = J.process_batch(filled, g).cpu().numpy()
    reg_np, clean_np, filled_np = reg.cpu().numpy(), clean.cpu().numpy(), filled.cpu().numpy()
    counts = _counts(S)
    for x in (R, S, H, J):
        x.close()
    R, S, H, J = stages()                                             # by hand: every result through the host
    reg2 = R.register(dev(torch, depth)).cpu().numpy()
    clean2 = S.filter(dev(torch, reg2)).cpu().numpy()
    filled2 = H.fill(dev(torch, clean2), dev(torch, bgr)).cpu().numpy()
    byhand = J.process_batch(dev(torch, filled2), dev(torch, bgr)).cpu().numpy()
    for x in (R, S, H, J):
        x.close()
    _assert_equal(reg_np, reg2, "registered")
    _assert_equal(clean_np, clean2, "speckle-filtered")
    _assert_equal(filled_np, filled2, "filled")
    _assert_equal(chained, byhand, "filtered")
    z, _, removed, comps = SC.filter_batch(reg_np, np.float32, **sp)
    _assert_equal(clean_np, z, "speckle-filtered against its statement")
    assert counts == (removed.tolist(), comps.tolist())


def test_vga_generator_frames(torch_cuda):
    """two frames of the generator at 640 x 480 with the injected outliers: 20 x 30 tiles, components that span hundreds of them"""
    from kinectdepthmapenhancement_amd import filters as F_
    torch = torch_cuda
    w, h = 640, 480
    d = np.stack([SC.injected_frame(seed, w, h)[0] for seed in (0, 1)])
    for conn in (4, 8):
        p = dict(SC.DEFAULTS, connectivity=conn, z_min=SC.Z_RANGE[0], z_max=SC.Z_RANGE[1])
        z, labels, removed, comps = SC.filter_batch(d, np.float32, **p)
        S = F_.DepthSpeckleFilter((w, h), 2, F_._native.SpeckleParams(p["min_size"], p["max_diff"], p["rel_diff"], conn, p["z_min"], p["z_max"]))
        lab = _sentinel(torch, (2, h, w), np.int32)
        got = S.filter(dev(torch, d), labels=lab)
        _assert_equal(got.cpu().numpy(), z, ("vga", conn))
        _assert_equal(lab.cpu().numpy(), labels, ("vga", conn, "labels"))
        assert _counts(S) == (removed.tolist(), comps.tolist()) and min(removed) > 0
        S.close()
