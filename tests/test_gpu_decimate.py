"""DepthDecimation on the GPU (filters.DepthDecimation, kde_decimate_*) against the numpy statement of the rule
(decimate_cases.py).  Every comparison is on bytes: both sides perform the same IEEE binary32 operations in the same order.

The paths of the kernels (decimate_kernels.hip) and the case that is there for each -- decimate_cases.CASES says why:
  a workgroup takes a tile of 32 x 8 (k <= 4) or 32 x 4 (k >= 5) output pixels
      a grid of one workgroup, a block with one existing sample ....... one_pixel, one_block
      several tiles each way, none partial (k = 2, 3) ................. exact; tiles partial on the right and at the bottom:
      every other case (zeroed LDS in front of the staging); many across and one down ... wide; the transpose ... tall
  a source row is read as the aligned 16-byte pieces inside it and as elements at its ends
      every row on a 16-byte boundary: whole pieces only .............. exact (96 wide), holes, edge (64 wide), float and uint16
      rows off a boundary, a different offset per row and per frame ... ragged (101 wide), wide (515), tall, one_block (8 wide as
      uint16: a row is one piece), and every case from pointers one element past a boundary (test_a_frame_gives_the_same_...)
      a row shorter than a piece: elements only ....................... one_pixel, tall (9 wide), one_block as float at k >= 3
      more pieces than four per thread (a second pass of the staging loop) ... exact and ragged at k = 8
  the regrouping into k x k blocks through LDS, k = 3, 5, 6, 7 included ... one_block, ragged (every k), exact, wide, tall
  the selection: the sorting network of every k, padded to 4, 16, 16, 32, 64, 64, 64 values ... every case at its factors
      m = 0 .. k^2 in some block, even m, duplicates: the lower median's tie ... holes, with min_valid 1, 2, k^2
  the mean: without a guard no selection runs; with the guard a wavefront selects only if one of its blocks is mixed
      wavefronts with and without a mixed block ....................... edge, exact, ragged (a far surface in a part of the frame)
  float and uint16 on both sides, n < max_batch, a tenth of the samples invalid (0, NaN, +-inf, negative, z_min, >= z_max) ... all
  the colour kernel: the same tiles and pieces on bytes, partial blocks divided by their own count ... every case and factor
Three frames per case."""
import numpy as np
import pytest

import decimate_cases as DC
import upsample_cases as UC
from decimate_cases import CASES, CASE_FACTORS, GUARDS, MAX_GAP, MEAN, MEDIAN, Z_RANGE
from gpu_util import dev

pytestmark = pytest.mark.gpu

F = np.float32
SENTINEL = 0xA5
N = DC.FRAMES
DTYPES = (np.float32, np.uint16)
PAIRS = ((np.float32, np.float32), (np.uint16, np.uint16), (np.float32, np.uint16), (np.uint16, np.float32))

_want_cache = {}


def _src(name, dt):
    return CASES[name].f32 if dt == np.float32 else CASES[name].u16


def _want(name, k, mode, gap, dt, ot, min_valid=1):
    """the statement's frames and counts, computed once per setting and shared (nothing writes to them)"""
    key = (name, k, mode, float(gap), dt, min_valid)
    if key not in _want_cache:
        z, filled, mixed = DC.decimate_batch(_src(name, dt), k, mode=mode, min_valid=min_valid, max_gap=gap, z_min=Z_RANGE[0], z_max=Z_RANGE[1])
        _want_cache[key] = (z, DC.depth_to_u16(z), filled.tolist(), mixed.tolist())
    z, z16, filled, mixed = _want_cache[key]
    return (z if ot == np.float32 else z16), filled, mixed


def _object(F_, name, k, mode=MEDIAN, gap=0.0, min_valid=1, max_batch=N + 1):
    return F_.DepthDecimation(CASES[name].size, max_batch, F_._native.DecimateParams(k, mode, min_valid, float(gap), float(Z_RANGE[0]), float(Z_RANGE[1])))


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


@pytest.mark.parametrize("name,k", CASE_FACTORS)
def test_byte_exact_against_the_statement(torch_cuda, name, k):
    """both modes, without and with the guard, all four format pairs, n = 3 in an object for 4, filled[f] and mixed[f]; nothing
    is written behind the frames of the call"""
    from kinectdepthmapenhancement_amd import filters as F_
    torch = torch_cuda
    ow, oh = DC.out_size(CASES[name].size, k)
    for mode in (MEDIAN, MEAN):
        for gap in GUARDS:
            D = _object(F_, name, k, mode, gap)
            assert D.out_size == (ow, oh)
            for dt, ot in PAIRS:
                src = _tensor(torch, _src(name, dt))
                want, filled, mixed = _want(name, k, mode, gap, dt, ot)
                out = _sentinel(torch, (N + 1, oh, ow), ot)
                got = D.decimate(src, out[:N])
                assert got.data_ptr() == out.data_ptr()
                _assert_equal(_host(out[:N], ot), want, (name, k, mode, gap, dt, ot))
                assert _untouched(torch, out[N]), (name, k, mode, gap, "written behind the frames")
                f, m = D.filled(), D.mixed()
                assert f.dtype == np.uint32 and f.tolist() == filled, (name, k, mode, gap, dt, ot, f, filled)
                assert m.dtype == np.uint32 and m.tolist() == mixed, (name, k, mode, gap, dt, ot, m, mixed)
            D.close()


@pytest.mark.parametrize("min_valid", (1, 2, "all"))
@pytest.mark.parametrize("k", CASES["holes"].factors)
def test_holes_with_each_min_valid(torch_cuda, k, min_valid):
    from kinectdepthmapenhancement_amd import filters as F_
    torch = torch_cuda
    mv = k * k if min_valid == "all" else min_valid
    for mode, gap in ((MEDIAN, 0.0), (MEAN, MAX_GAP), (MEAN, 0.0)):
        D = _object(F_, "holes", k, mode, gap, mv)
        for dt, ot in PAIRS:
            want, filled, mixed = _want("holes", k, mode, gap, dt, ot, mv)
            got = D.decimate(_tensor(torch, _src("holes", dt)), out_format=_tdt(torch, ot))
            _assert_equal(_host(got, ot), want, ("holes", k, mv, mode, gap, dt, ot))
            assert D.filled().tolist() == filled and D.mixed().tolist() == mixed
        D.close()
    full, _, _ = _want("holes", k, MEDIAN, 0.0, np.float32, np.float32, 1)
    some, _, _ = _want("holes", k, MEDIAN, 0.0, np.float32, np.float32, mv)
    assert mv == 1 or (some != 0).sum() < (full != 0).sum()          # min_valid bites


@pytest.mark.parametrize("name,k", CASE_FACTORS)
def test_a_frame_gives_the_same_bytes_anywhere(torch_cuda, name, k):
    """alone, as frame 0, 1 or 2 of n = 3 in a max_batch of 4, and from source and output pointers one element past a 16-byte
    boundary, with the bytes around the output untouched"""
    from kinectdepthmapenhancement_amd import filters as F_
    torch = torch_cuda
    ow, oh = DC.out_size(CASES[name].size, k)
    D = _object(F_, name, k, MEAN, MAX_GAP, max_batch=4)
    for dt, ot in PAIRS:
        d = _src(name, dt)
        want, filled, mixed = _want(name, k, MEAN, MAX_GAP, dt, ot)
        fmt = _tdt(torch, ot)
        for f in range(N):
            got = D.decimate(_tensor(torch, d[f:f + 1]), out_format=fmt)                                   # alone
            _assert_equal(_host(got, ot), want[f:f + 1], (name, k, dt, ot, f, "alone"))
            assert D.filled().tolist() == [filled[f]] and D.mixed().tolist() == [mixed[f]]
            order = [(f + r) % N for r in range(N)]                                                        # at every place of a batch of 3
            got = D.decimate(_tensor(torch, np.ascontiguousarray(d[order])), out_format=fmt)
            _assert_equal(_host(got, ot), want[order], (name, k, dt, ot, order))
            assert D.filled().tolist() == [filled[g] for g in order] and D.mixed().tolist() == [mixed[g] for g in order]
        out, buf = _shifted(torch, np.zeros((N, oh, ow), ot), fill=SENTINEL)
        D.decimate(_shifted(torch, d)[0], out)
        _assert_equal(_host(out, ot), want, (name, k, dt, ot, "shifted"))
        assert D.filled().tolist() == filled and D.mixed().tolist() == mixed
        assert _untouched(torch, buf[:1]) and _untouched(torch, buf[1 + out.numel():]), (name, k, dt, ot, "written around the frames")
    D.close()


@pytest.mark.parametrize("name,k", CASE_FACTORS)
def test_the_colour_call(torch_cuda, name, k):
    """byte-exact on every case and factor, from aligned pointers and from pointers 1, 2 and 3 bytes past a 16-byte boundary, with
    nothing written around the output; the depth results of the object stay as they were"""
    from kinectdepthmapenhancement_amd import filters as F_
    torch = torch_cuda
    bgr = CASES[name].bgr
    ow, oh = DC.out_size(CASES[name].size, k)
    want = np.stack([DC.decimate_color(b, k) for b in bgr])
    D = _object(F_, name, k)
    depth = D.decimate(_tensor(torch, _src(name, np.float32))).cpu().numpy()
    out = _sentinel(torch, (N + 1, oh, ow, 3), np.uint8)
    D.decimate_color(dev(torch, bgr), out[:N])
    _assert_equal(out[:N].cpu().numpy(), want, (name, k, "colour"))
    assert _untouched(torch, out[N])
    _assert_equal(D.decimate_color(dev(torch, bgr[1:2])).cpu().numpy(), want[1:2], (name, k, "colour, one frame"))
    for by in (1, 2, 3):
        o, buf = _shifted(torch, np.zeros((N, oh, ow, 3), np.uint8), by, fill=SENTINEL)
        D.decimate_color(_shifted(torch, bgr, by)[0], o)
        _assert_equal(o.cpu().numpy(), want, (name, k, "colour shifted", by))
        assert _untouched(torch, buf[:by]) and _untouched(torch, buf[by + o.numel():])
    _assert_equal(D.depth_device().cpu().numpy(), depth, "the colour call left the depth results alone")
    D.close()


def test_graph_capture_replays_to_the_same_bytes(torch_cuda):
    """captured at the object's first call: two kernel nodes in a line, no allocation, no synchronisation, and no count left over
    from an earlier replay"""
    from kinectdepthmapenhancement_amd import filters as F_
    torch = torch_cuda
    name, k = "ragged", 3
    ow, oh = DC.out_size(CASES[name].size, k)
    want, filled, mixed = _want(name, k, MEAN, MAX_GAP, np.float32, np.uint16)
    D = _object(F_, name, k, MEAN, MAX_GAP)
    src = _tensor(torch, _src(name, np.float32))
    out = _sentinel(torch, (N, oh, ow), np.uint16)
    torch.cuda.synchronize()
    stream = torch.cuda.Stream()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=stream):
        D.decimate(src, out)                                         # the first call of this object
    for _ in range(2):
        out.view(torch.uint8).fill_(SENTINEL)
        D.filled_device().fill_(SENTINEL)
        D.mixed_device().fill_(SENTINEL)
        torch.cuda.synchronize()
        graph.replay()
        torch.cuda.synchronize()
        _assert_equal(_host(out, np.uint16), want, "replay")
        assert D.filled().tolist() == filled and D.mixed().tolist() == mixed
    out.view(torch.uint8).fill_(SENTINEL)
    D.decimate(src, out)                                             # eager, after the graph
    _assert_equal(_host(out, np.uint16), want, "eager")
    assert D.filled().tolist() == filled and D.mixed().tolist() == mixed
    del graph
    D.close()


def test_python_mirrors(torch_cuda):
    """the host getters and the object-owned output buffer (out_dev == NULL) agree with the device results"""
    from kinectdepthmapenhancement_amd import filters as F_
    torch = torch_cuda
    name, k = "edge", 4
    ow, oh = DC.out_size(CASES[name].size, k)
    D = _object(F_, name, k, MEAN, MAX_GAP)
    for dt, ot in PAIRS:
        src = _tensor(torch, _src(name, dt))
        want, filled, mixed = _want(name, k, MEAN, MAX_GAP, dt, ot)
        out = _sentinel(torch, (N, oh, ow), ot)
        D.decimate(src, out)
        assert D.depth_device().data_ptr() == out.data_ptr()
        own = D.decimate(src, out_format=_tdt(torch, ot))
        assert own.data_ptr() != out.data_ptr() and tuple(own.shape) == (N, oh, ow)
        _assert_equal(_host(own, ot), want, (dt, ot, "object-owned"))
        _assert_equal(_host(out, ot), want, (dt, ot, "caller's buffer"))
        host = D.depth_host()
        assert host.dtype == ot and host.tobytes() == want.tobytes()
        assert D.filled().tolist() == filled and D.mixed().tolist() == mixed and sum(mixed) > 0
        assert D.filled_device().cpu().numpy().view(np.uint32).reshape(-1).tolist() == filled
        assert D.mixed_device().cpu().numpy().view(np.uint32).reshape(-1).tolist() == mixed
        if dt == ot:                                                 # out_format None: the format of the input
            assert D.decimate(src).dtype == _tdt(torch, dt)
    with pytest.raises(F_._native.KdeError, match="overlaps depth_dev"):
        _in_place(D, torch, name)
    D.close()


def _in_place(D, torch, name):
    """a source whose first bytes are the output buffer's: refused"""
    w, h = CASES[name].size
    flat = torch.zeros(N * h * w, dtype=torch.float32, device="cuda")
    return D.decimate(flat.view(N, h, w), flat[: N * D.out_size[0] * D.out_size[1]].view(N, D.out_size[1], D.out_size[0]))


def _window_range(z, radius):
    """per pixel of [n, h, w]: (smallest, largest, number) of the samples the JBF counts as valid (> 50 mm) within `radius`"""
    n, h, w = z.shape
    lo, hi, cnt = np.full(z.shape, np.inf, np.float32), np.zeros(z.shape, np.float32), np.zeros(z.shape, np.int64)
    p = np.zeros((n, h + 2 * radius, w + 2 * radius), np.float32)
    p[:, radius:radius + h, radius:radius + w] = z
    for dy in range(2 * radius + 1):
        for dx in range(2 * radius + 1):
            t = p[:, dy:dy + h, dx:dx + w]
            ok = t > 50
            lo = np.where(ok, np.minimum(lo, t), lo)
            hi = np.where(ok, np.maximum(hi, t), hi)
            cnt += ok
    return lo, hi, cnt


def test_the_chain_decimate_filter_upsample(torch_cuda):
    """the recipe of INTEGRATION.md on `exact` with k = 2 and min_valid 4, which leaves a third of the small frame as holes:
    decimate and decimate_color feed JointBilateralFilter at the small size; GuidedDepthUpsampling takes the decimated depth back
    to 96 x 48 under the full-resolution guide, equal to the two numpy statements composed.
    Holes: a hole of the decimator is the bit pattern of +0 -- not a NaN, not a blend -- and stays that through the filter's call
    (the frames are compared with a snapshot taken before it).  The filter's OUTPUT at a hole is not 0: it averages the valid
    taps of its 5 x 5 window with weights >= 0, there as at every pixel, so what it may give is 0 (no valid tap, or every weight
    underflowed) or a value within the smallest .. largest valid sample of the window, up to the rounding of a 25-term weighted
    mean (25 * 2^-24 < 1e-5 relative)."""
    from kinectdepthmapenhancement_amd import filters as F_
    torch = torch_cuda
    name, k, mv = "exact", 2, 4
    case = CASES[name]
    (w, h), (ow, oh) = case.size, DC.out_size(case.size, k)
    D = _object(F_, name, k, MEDIAN, 0.0, mv)
    low = D.decimate(_tensor(torch, case.u16), out_format=torch.float32)
    guide = D.decimate_color(dev(torch, case.bgr))
    want_low, filled, _ = _want(name, k, MEDIAN, 0.0, np.uint16, np.float32, mv)
    before = low.cpu().numpy().copy()                                 # the snapshot, before the filter runs
    _assert_equal(before, want_low, "decimated")
    _assert_equal(guide.cpu().numpy(), np.stack([DC.decimate_color(b, k) for b in case.bgr]), "decimated guide")
    assert tuple(low.shape) == (N, oh, ow) and tuple(guide.shape) == (N, oh, ow, 3) and low.is_contiguous() and guide.is_contiguous()
    hole = before.view(np.uint32) == 0                                # +0 exactly
    assert D.filled().tolist() == filled == [int((~hm).sum()) for hm in hole]
    assert all(0.2 * ow * oh < hm.sum() < 0.5 * ow * oh for hm in hole)         # 1 - 0.9^4 = 0.34 of the blocks lack a sample
    assert np.isfinite(before).all() and ((before > Z_RANGE[0]) & (before < Z_RANGE[1]))[~hole].all()
    J = F_.JointBilateralFilter(ow, oh, max_batch=N)
    assert J.default_params().window_size == 5
    filtered = J.process_batch(low, guide).cpu().numpy()
    _assert_equal(low.cpu().numpy(), before, "holes stay 0: the filter left its input alone")
    assert filtered.shape == (N, oh, ow) and np.isfinite(filtered).all()
    lo, hi, cnt = _window_range(before, 2)
    zero = filtered == 0
    assert zero[cnt == 0].all() and (cnt[hole] > 0).any()
    inside = (filtered >= lo * F(1 - 1e-5)) & (filtered <= hi * F(1 + 1e-5))
    assert (zero | inside).all(), ("filter output outside its window", int((~(zero | inside)).sum()))
    assert (zero | inside)[hole].all() and (filtered[~hole] > 0).all()
    J.close()
    p = F_._native.UpsampleParams(2, 30.0, float(MAX_GAP), float(Z_RANGE[0]), float(Z_RANGE[1]))
    U = F_.GuidedDepthUpsampling((ow, oh), (w, h), N, p)
    up = U.upsample(low, dev(torch, case.bgr))
    t = UC.tables((ow, oh), (w, h), 30.0, U.range_table())
    want = [UC.upsample(zl, b, t, (w, h), 2, MAX_GAP, *Z_RANGE) for zl, b in zip(want_low, case.bgr)]
    _assert_equal(up.cpu().numpy(), np.stack([a for a, _ in want]), "upsampled")
    assert U.filled().tolist() == [f for _, f in want] and all(f > 0.9 * w * h for _, f in want)
    Ks = D.intrinsics([[100.0, 0.0, 47.5], [0.0, 100.0, 23.5], [0.0, 0.0, 1.0]])
    assert np.array_equal(Ks, DC.intrinsics([[100.0, 0.0, 47.5], [0.0, 100.0, 23.5], [0.0, 0.0, 1.0]], k))
    U.close()
    D.close()
