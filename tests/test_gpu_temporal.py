"""DepthTemporalFilter on the GPU (filters.DepthTemporalFilter, kde_temporal_*) against the numpy statement of the rule
(temporal_cases.py): the bytes of the depth, of the state (value, hist) and all four counts.  No tolerance anywhere: both sides
perform the same IEEE binary32 operations in the same order and the counts are integer sums.

The paths of the kernel (temporal_kernels.hip) and what runs them:
  frames of 37 x 19 (703 pixels: the frames of a call start at four different alignments, the last thread owns a partial group),
  3 x 1 (one partial group) and 64 x 8 (every group whole and aligned); sequences of 1, 7, 9 and 17 frames (whole chunks of the
  frames loaded ahead and the frames left over behind them); float and uint16 on both sides; with and without guide; every
  pixels-per-thread x load-ahead shape the library has."""
import numpy as np
import pytest

import holefill_cases as HC
import speckle_cases as SC
import temporal_cases as TC
from gpu_util import dev

pytestmark = pytest.mark.gpu

SENTINEL = 0xA5
DTYPES = (np.float32, np.uint16)
SHAPES = [(p, u) for p in (1, 2, 4, 8) for u in (1, 2, 4)]

_cache = {}


def _params(F_, name, **kw):
    p = TC.params(name, **kw)
    return F_._native.TemporalParams(p["alpha"], p["max_diff"], p["rel_diff"], p["persist_min"], p["color_thresh"], p["z_min"], p["z_max"])


def _object(F_, name, max_batch=None, **kw):
    c = TC.CASES[name]
    return F_.DepthTemporalFilter(c.size, c.n + 1 if max_batch is None else max_batch, _params(F_, name, **kw))


def _inputs(name):
    if name not in _cache:
        d, g = TC.frames(name)
        _cache[name] = dict(src={np.float32: d.copy(), np.uint16: TC.as_u16(d)}, bgr=g.copy(), want={})    # torch wants writable arrays
    return _cache[name]


def _want(name, guide, dt):
    """the statement on the whole sequence of a case, computed once per setting and shared (nothing writes to it)"""
    s = _inputs(name)
    key = (guide, dt)
    if key not in s["want"]:
        s["want"][key] = TC.filter_sequence(s["src"][dt], s["bgr"] if guide else None, **TC.params(name))
    return s["want"][key]


def _as(out, ot):
    return out if ot == np.float32 else TC.depth_to_u16(out)


def _tensor(torch, a):
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
    return [getattr(H, k)().tolist() for k in TC.COUNTS]


def _want_counts(r, sl=slice(None)):
    return [getattr(r, k)[sl].tolist() for k in TC.COUNTS]


def _assert_state(H, r, what):
    value, hist = H.state()
    _assert_equal(value.cpu().numpy(), r.value, what + ("value",))
    _assert_equal(hist.cpu().numpy().view(np.uint32), r.hist, what + ("hist",))


@pytest.mark.parametrize("name", TC.IDS)
def test_byte_exact_against_the_statement(torch_cuda, name):
    """every case as one call: with and without guide, all four format pairs, depth, state and counts; nothing is written
    behind the frames of the call (max_batch is n + 1)"""
    from kinectdepthmapenhancement_amd import filters as F_
    torch = torch_cuda
    s = _inputs(name)
    n, (w, h) = TC.CASES[name].n, TC.CASES[name].size
    for guide in (False, True):
        H = _object(F_, name)
        bgr = dev(torch, s["bgr"]) if guide else None
        for dt in DTYPES:
            src = _tensor(torch, s["src"][dt])
            r = _want(name, guide, dt)
            for ot in DTYPES:
                what = (name, guide, dt, ot)
                H.reset()
                out = _sentinel(torch, (n + 1, h, w), ot)
                got = H.filter(src, bgr, out[:n])
                assert got.data_ptr() == out.data_ptr()
                _assert_equal(_host(out[:n], ot), _as(r.out, ot), what)
                assert _untouched(torch, out[n]), what + ("written behind the frames",)
                _assert_state(H, r, what)
                assert _counts(H) == _want_counts(r), what + (_counts(H), _want_counts(r))
                assert H.smoothed().dtype == np.uint32
        H.reset()
        own = H.filter(_tensor(torch, s["src"][np.float32]), bgr)          # the object's buffer
        _assert_equal(own.cpu().numpy(), _want(name, guide, np.float32).out, (name, guide, "object-owned"))
        _assert_equal(H.depth_host(), _want(name, guide, np.float32).out, (name, guide, "depth_host"))
        H.close()


@pytest.mark.parametrize("name,cuts", [("step", (4, 1, 4)), ("colour_t48", (4, 1, 4)), ("noise", (1,) * 17), ("dropout_p3", (1,) * 17),
                                       ("dropout_p1", (8, 2, 7))])
def test_the_cut_of_the_sequence_does_not_matter(torch_cuda, name, cuts):
    """n = 9 in one call against 4 + 1 + 4, n = 17 against 17 calls of one: the same depth, counts per frame and final state"""
    from kinectdepthmapenhancement_amd import filters as F_
    torch = torch_cuda
    s = _inputs(name)
    assert sum(cuts) == TC.CASES[name].n
    for dt, ot in ((np.float32, np.float32), (np.uint16, np.uint16), (np.float32, np.uint16)):
        r = _want(name, True, dt)
        H = _object(F_, name)
        src, bgr = _tensor(torch, s["src"][dt]), dev(torch, s["bgr"])
        t = 0
        for c in cuts:
            got = H.filter(src[t:t + c], bgr[t:t + c], out_format=_tdt(torch, ot))
            _assert_equal(_host(got, ot), _as(r.out[t:t + c], ot), (name, dt, ot, "frames", t, c))
            assert _counts(H) == _want_counts(r, slice(t, t + c)), (name, dt, ot, t, c)
            t += c
        _assert_state(H, r, (name, dt, ot, cuts))
        H.close()


@pytest.mark.parametrize("name", ("noise", "colour_t0", "u16_edges"))
def test_every_shape_gives_the_same_bytes(torch_cuda, name):
    """the pixels a thread owns (1, 2, 4, 8) and the frames it loads ahead (1, 2, 4) change nothing: depth, state, counts"""
    from kinectdepthmapenhancement_amd import filters as F_
    torch = torch_cuda
    s = _inputs(name)
    H = _object(F_, name)
    bgr = dev(torch, s["bgr"])
    assert H.shape(TC.CASES[name].n) in SHAPES
    for dt in DTYPES:
        src = _tensor(torch, s["src"][dt])
        r = _want(name, True, dt)
        for shape in SHAPES:
            H.set_shape(*shape)
            assert H.shape(1) == shape
            H.reset()
            got = H.filter(src, bgr, out_format=_tdt(torch, dt))
            _assert_equal(_host(got, dt), _as(r.out, dt), (name, dt, shape))
            _assert_state(H, r, (name, dt, shape))
            assert _counts(H) == _want_counts(r), (name, dt, shape)
    with pytest.raises(F_._native.KdeError, match="kde_temporal_set_shape"):
        H.set_shape(3, 1)
    H.set_shape(0, 0)
    H.close()


@pytest.mark.parametrize("name", ("noise", "colour_t48", "invalid", "u16_edges"))
def test_alignment_sentinels_and_in_place(torch_cuda, name):
    """depth, guide and output one element past a 16-byte boundary, with the bytes in front of frame 0 and behind frame n - 1
    untouched in an object for more frames than the call has; then exactly in place in both formats"""
    from kinectdepthmapenhancement_amd import filters as F_
    torch = torch_cuda
    s = _inputs(name)
    n, (w, h) = TC.CASES[name].n, TC.CASES[name].size
    H = _object(F_, name, max_batch=n + 3)
    for dt, ot in ((np.float32, np.float32), (np.uint16, np.uint16), (np.float32, np.uint16), (np.uint16, np.float32)):
        r = _want(name, True, dt)
        for by in (1, 3):
            H.reset()
            out, buf = _shifted(torch, np.zeros((n, h, w), ot), by, fill=SENTINEL)
            H.filter(_shifted(torch, s["src"][dt], by)[0], _shifted(torch, s["bgr"], by)[0], out)
            _assert_equal(_host(out, ot), _as(r.out, ot), (name, dt, ot, "shifted", by))
            assert _untouched(torch, buf[:by]) and _untouched(torch, buf[by + out.numel():]), (name, dt, ot, "written around the frames")
            _assert_state(H, r, (name, dt, ot, "shifted", by))
            assert _counts(H) == _want_counts(r)
        if dt == ot:                                                      # in place
            for guide in (False, True):
                r = _want(name, guide, dt)
                H.reset()
                src = _tensor(torch, s["src"][dt]).clone()
                got = H.filter(src, dev(torch, s["bgr"]) if guide else None, src)
                assert got.data_ptr() == src.data_ptr()
                _assert_equal(_host(src, ot), _as(r.out, ot), (name, dt, guide, "in place"))
                _assert_state(H, r, (name, dt, guide, "in place"))
                assert _counts(H) == _want_counts(r)
    H.close()


def test_the_in_place_rule_and_results_before_a_call(torch_cuda):
    """kde_hip.h: in place exactly when out_dev == depth_dev and out_format == depth_format; any other overlap of the written
    frames with the depth or the guide is refused, and nothing is launched: the state stays empty"""
    from kinectdepthmapenhancement_amd import filters as F_
    torch = torch_cuda
    name = "step"
    s = _inputs(name)
    H = _object(F_, name)
    src = _tensor(torch, s["src"][np.float32])
    before = src.clone()
    with pytest.raises(F_._native.KdeError, match="was not called"):
        H.smoothed()
    with pytest.raises(F_._native.KdeError, match="in place"):
        H.filter(src[:2], None, src[1:3])                             # a partial overlap
    with pytest.raises(F_._native.KdeError, match="in place"):
        H.filter(src, None, src.view(torch.int16).view(-1)[:src.numel()].view(src.shape))      # the same pointer in another format
    n, h, w = src.shape
    raw = torch.zeros(n * h * w * 4, dtype=torch.uint8, device="cuda")
    with pytest.raises(F_._native.KdeError, match="overlaps bgr_dev"):
        H.filter(src, raw[:n * h * w * 3].view(n, h, w, 3), raw.view(torch.float32).view(n, h, w))
    assert torch.equal(src.view(torch.int32), before.view(torch.int32))
    value, hist = H.state()
    assert not value.any() and not hist.any()
    own = H.filter(src)
    with pytest.raises(F_._native.KdeError, match="in place"):
        H.filter(own)                                                 # out_dev == NULL selects the buffer `own` lies in
    with pytest.raises(AttributeError):
        H.filled()
    H.close()


def test_reset_in_the_middle_equals_a_fresh_object(torch_cuda):
    from kinectdepthmapenhancement_amd import filters as F_
    torch = torch_cuda
    name = "noise"
    s = _inputs(name)
    src, bgr = _tensor(torch, s["src"][np.float32]), dev(torch, s["bgr"])
    H = _object(F_, name)
    H.filter(src[:5], bgr[:5])
    H.reset()
    with pytest.raises(F_._native.KdeError, match="was not called"):
        H.held()                                                      # reset also clears what the getters report
    with pytest.raises(F_._native.KdeError, match="was not called"):
        H.depth_device()
    value, hist = H.state()
    assert not value.any() and not hist.any()
    r = TC.filter_sequence(s["src"][np.float32][5:], s["bgr"][5:], **TC.params(name))
    got = H.filter(src[5:], bgr[5:])
    _assert_equal(got.cpu().numpy(), r.out, "after reset")
    _assert_state(H, r, ("after reset",))
    assert _counts(H) == _want_counts(r)
    fresh = _object(F_, name)
    _assert_equal(fresh.filter(src[5:], bgr[5:]).cpu().numpy(), r.out, "fresh")
    fresh.close()
    H.close()


def test_state_copied_to_another_object_continues_the_sequence(torch_cuda):
    """kde_temporal_state_device: a checkpoint is two copies out, restoring it or moving the stream two copies in"""
    from kinectdepthmapenhancement_amd import filters as F_
    torch = torch_cuda
    name = "dropout_p3"
    s = _inputs(name)
    r = _want(name, True, np.uint16)
    src, bgr = _tensor(torch, s["src"][np.uint16]), dev(torch, s["bgr"])
    A, B = _object(F_, name), _object(F_, name)
    A.filter(src[:6], bgr[:6])
    checkpoint = [t.clone() for t in A.state()]
    for to, frm in zip(B.state(), A.state()):
        to.copy_(frm)
    got = B.filter(src[6:], bgr[6:])
    _assert_equal(got.cpu().numpy(), r.out[6:], "moved")
    _assert_state(B, r, ("moved",))
    assert _counts(B) == _want_counts(r, slice(6, None))
    A.filter(src[6:9], bgr[6:9])                                      # A goes on, is put back to the checkpoint and goes on again
    for to, frm in zip(A.state(), checkpoint):
        to.copy_(frm)
    _assert_equal(A.filter(src[6:], bgr[6:]).cpu().numpy(), r.out[6:], "restored")
    _assert_state(A, r, ("restored",))
    A.close()
    B.close()


def test_a_graph_captured_at_the_first_call_advances_the_stream(torch_cuda):
    """captured at the object's first call -- two kernels, no memset node, no allocation, no synchronisation -- and replayed once
    per chunk, with the next chunk copied into the same buffers: the statement on the whole sequence"""
    from kinectdepthmapenhancement_amd import filters as F_
    torch = torch_cuda
    name, k = "noise", 8
    s = _inputs(name)
    r = _want(name, True, np.float32)
    w, h = TC.CASES[name].size
    H = _object(F_, name)
    src = torch.zeros((k, h, w), dtype=torch.float32, device="cuda")
    bgr = torch.zeros((k, h, w, 3), dtype=torch.uint8, device="cuda")
    out = _sentinel(torch, (k, h, w), np.uint16)
    torch.cuda.synchronize()
    stream = torch.cuda.Stream()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=stream):
        H.filter(src, bgr, out)                                       # the first call of this object; nothing runs yet
    value, hist = H.state()
    assert not value.any() and not hist.any()
    for chunk in range(2):
        t = chunk * k
        src.copy_(_tensor(torch, s["src"][np.float32][t:t + k]))
        bgr.copy_(dev(torch, s["bgr"][t:t + k]))
        out.view(torch.uint8).fill_(SENTINEL)
        for name_ in TC.COUNTS:
            getattr(H, name_ + "_device")().fill_(SENTINEL)
        torch.cuda.synchronize()
        graph.replay()
        torch.cuda.synchronize()
        _assert_equal(_host(out, np.uint16), TC.depth_to_u16(r.out[t:t + k]), ("replay", chunk))
        assert _counts(H) == _want_counts(r, slice(t, t + k)), ("replay", chunk)
    last = H.filter(_tensor(torch, s["src"][np.float32][2 * k:]), dev(torch, s["bgr"][2 * k:]))      # eager, after the graph
    _assert_equal(last.cpu().numpy(), r.out[2 * k:], "eager")
    _assert_state(H, r, ("graph",))
    del graph
    H.close()


def test_speckle_then_temporal_then_hole_fill(torch_cuda):
    """the chain of INTEGRATION.md with device pointers passed along -- DepthSpeckleFilter, DepthTemporalFilter, DepthHoleFilling
    -- over a short moving sequence, cut into two calls, equals the three numpy statements composed"""
    from kinectdepthmapenhancement_amd import filters as F_
    from kinectdepthmapenhancement_amd import synth
    torch = torch_cuda
    n, w, h = 6, 72, 50
    bgr, depth, _, _ = synth.make_sequence(3, n, w, h, step=(4, 1), dropout=0.05)
    sp = dict(SC.DEFAULTS, min_size=6)
    tp = dict(TC.DEFAULTS)
    S = F_.DepthSpeckleFilter((w, h), n, F_._native.SpeckleParams(sp["min_size"], sp["max_diff"], sp["rel_diff"], sp["connectivity"], sp["z_min"], sp["z_max"]))
    T = F_.DepthTemporalFilter((w, h), n)
    hp = F_._native.HolefillParams(2, 8, 3, 2.0, 30.0, 100.0, 1, 0.0, float(TC.FLT_MAX), 0)
    H = F_.DepthHoleFilling((w, h), n, hp)
    space, rng = H.space_table(), H.range_table()
    g = dev(torch, bgr)
    d = dev(torch, depth)
    got_t, got_f, counts = [], [], []
    for a, b in ((0, 4), (4, 6)):
        clean = S.filter(d[a:b])
        smooth = T.filter(clean, g[a:b])
        got_t.append(smooth.cpu().numpy())
        counts.append(_counts(T))
        got_f.append(H.fill(smooth, g[a:b]).cpu().numpy())
    for x in (S, T, H):
        x.close()
    want_s = SC.filter_batch(depth, np.float32, **sp)[0]
    want_t = TC.filter_sequence(want_s, bgr, **tp)
    _assert_equal(np.concatenate(got_t), want_t.out, "temporal against the statements")
    assert [sum((c[k] for c in counts), []) for k in range(4)] == _want_counts(want_t)
    assert int(want_t.held.sum()) > 0 and int(want_t.smoothed.sum()) > 0 and int(want_t.changed.sum()) > 0
    parts = [HC.fill_parts(z, b, space, rng, radius=2, max_gap=F32(100.0), gap_rule=1) for z, b in zip(want_t.out, bgr)]
    _assert_equal(np.concatenate(got_f), np.stack([p["z"] for p in parts]), "filled against the statements")


F32 = np.float32
