"""Host-fed JBF (kde_jbf_feed_*, filters.JointBilateralFilterFeed): frames in host memory, chunked copy-in / K0 + K1 /
copy-out on the feed's three streams.  The bar is the resident path: every output is bit-identical to
kde_jbf_process_batch on the same frames, whatever the chunking, the depth format or the kind of host memory."""
import ctypes as C
import json
import os
import subprocess
import sys
import threading

import numpy as np
import pytest

from conftest import ROOT
from gpu_util import dev, host

pytestmark = pytest.mark.gpu

W11 = (11, 3.0, 7.65, 20.0)          # bench.py's headline parameters
W19 = (19, 3.0, 7.65, 20.0)          # its 1080p leg


def _params(F, cfg):
    p = F.JointBilateralFilter.default_params()      # cfg None: the reference's constants (window 5, pre-smoothing on)
    if cfg is not None:
        p.window_size, p.spatial_sigma, p.color_sigma, p.depth_sigma = cfg
    return p


def _bits(a):
    return np.ascontiguousarray(np.asarray(a, np.float32)).view(np.uint32)


def _resident(torch, F, cfg, bgr, depth):
    n, h, w = depth.shape
    jbf = F.JointBilateralFilter(w, h, _params(F, cfg), max_batch=n)
    out = torch.empty((n, h, w), dtype=torch.float32, device="cuda")
    jbf.process_batch(dev(torch, depth), dev(torch, bgr), out)
    return host(out)


@pytest.fixture(scope="module")
def vga65(synth):
    """65 distinct 640x480 frames: 33 from the generator and 32 of them mirrored left to right"""
    bgr, depth = synth.make_batch(700, 33, 640, 480)
    bgr = np.ascontiguousarray(np.concatenate([bgr, bgr[:32, :, ::-1]]))
    depth = np.ascontiguousarray(np.concatenate([depth, depth[:32, :, ::-1]]))
    return bgr, depth


@pytest.mark.timeout(240)
@pytest.mark.parametrize("cfg", [W11, None], ids=["w11", "reference_constants"])
def test_bit_identical_to_the_resident_batch(torch_cuda, vga65, cfg):
    from kinectdepthmapenhancement_amd import filters as F
    bgr, depth = vga65
    ref = _resident(torch_cuda, F, cfg, bgr, depth)
    jbf = F.JointBilateralFilter(640, 480, _params(F, cfg))          # max_batch 1: the feed is not bounded by it
    for chunk, n in ((1, 64), (7, 64), (64, 64), (8, 65)):
        feed = F.JointBilateralFilterFeed(jbf, chunk)
        got = feed.process(depth[:n], bgr[:n])
        st = feed.last_stats()
        assert (st["frames"], st["chunk_frames"], st["chunks"]) == (n, min(chunk, n), -(-n // chunk))
        assert np.array_equal(_bits(got), _bits(ref[:n])), f"chunk {chunk}, n {n}"


@pytest.mark.timeout(180)
def test_bit_identical_at_1080p_window19_with_a_short_last_chunk(torch_cuda, synth):
    from kinectdepthmapenhancement_amd import filters as F
    bgr, depth = synth.make_batch(900, 4, 1920, 1080)
    ref = _resident(torch_cuda, F, W19, bgr, depth)
    feed = F.JointBilateralFilterFeed(F.JointBilateralFilter(1920, 1080, _params(F, W19)), 3)
    got = feed.process(depth, bgr)
    assert feed.last_stats()["chunks"] == 2
    assert np.array_equal(_bits(got), _bits(ref))


@pytest.mark.timeout(180)
def test_uint16_depth_is_widened_exactly(torch_cuda, synth, vga65):
    from kinectdepthmapenhancement_amd import filters as F
    bgr, depth = vga65
    bgr, depth = bgr[:64], depth[:64]
    d16 = np.where(depth > 0, np.rint(depth), 0).astype(np.uint16)
    d32 = d16.astype(np.float32)
    ref = _resident(torch_cuda, F, W11, bgr, d32)
    feed = F.JointBilateralFilterFeed(F.JointBilateralFilter(640, 480, _params(F, W11)), 8)
    got16 = feed.process(d16, bgr)
    assert feed.last_stats()["h2d_bytes"] == 64 * 640 * 480 * 5          # 2 B depth + 3 B colour per pixel over the link
    got32 = feed.process(d32, bgr)
    assert feed.last_stats()["h2d_bytes"] == 64 * 640 * 480 * 7
    assert np.array_equal(_bits(got16), _bits(got32))
    assert np.array_equal(_bits(got16), _bits(ref))
    # a geometry whose chunks are not a multiple of 8 samples: the widening kernel's scalar tail
    b, d = synth.make_batch(40, 3, 161, 121)
    d16 = np.where(d > 0, np.rint(d), 0).astype(np.uint16)
    ref = _resident(torch_cuda, F, None, b, d16.astype(np.float32))
    got = F.JointBilateralFilterFeed(F.JointBilateralFilter(161, 121), 2).process(d16, b)
    assert np.array_equal(_bits(got), _bits(ref))


@pytest.mark.timeout(180)
def test_pinned_and_pageable_buffers_give_the_same_bits(torch_cuda, vga65):
    torch = torch_cuda
    from kinectdepthmapenhancement_amd import filters as F
    bgr, depth = vga65[0][:16], vga65[1][:16]
    ref = _resident(torch, F, W11, bgr, depth)
    feed = F.JointBilateralFilterFeed(F.JointBilateralFilter(640, 480, _params(F, W11)), 4)
    pd = torch.empty(depth.shape, dtype=torch.float32, pin_memory=True)
    pc = torch.empty(bgr.shape, dtype=torch.uint8, pin_memory=True)
    pd.numpy()[...] = depth
    pc.numpy()[...] = bgr
    for pin_in in (False, True):
        for pin_out in (False, True):
            out = torch.full(depth.shape, -1.0, dtype=torch.float32, pin_memory=True) if pin_out else np.full(depth.shape, -1.0, np.float32)
            got = feed.process(pd if pin_in else depth, pc if pin_in else bgr, out)
            assert got is out
            st = feed.last_stats()
            assert (st["inputs_staged"], st["outputs_staged"]) == (int(not pin_in), int(not pin_out)), (pin_in, pin_out)
            arr = out.numpy() if pin_out else out
            assert np.array_equal(_bits(arr), _bits(ref)), (pin_in, pin_out)


_OVERLAP_CHILD = r"""
import json, sys
sys.path.insert(0, %r)
import numpy as np, torch
from kinectdepthmapenhancement_amd import filters as F, synth
bgr, depth = synth.make_batch(800, 8, 640, 480)
bgr, depth = np.ascontiguousarray(np.tile(bgr, (8, 1, 1, 1))), np.ascontiguousarray(np.tile(depth, (8, 1, 1)))
pd, pc = torch.from_numpy(depth).pin_memory(), torch.from_numpy(bgr).pin_memory()
out = torch.empty(depth.shape, dtype=torch.float32, pin_memory=True)
p = F.JointBilateralFilter.default_params()
p.window_size, p.spatial_sigma, p.color_sigma, p.depth_sigma = 11, 3.0, 7.65, 20.0
feed = F.JointBilateralFilterFeed(F.JointBilateralFilter(640, 480, p), 8)
feed.process(pd, pc, out)            # first call: sizes the device slots
feed.process(pd, pc, out)
print(json.dumps(feed.last_stats()))
"""


@pytest.mark.timeout(150)
def test_copies_overlap_the_kernels(torch_cuda):
    """pinned buffers, 64 x VGA, window 11, chunk 8: the wall time of ONE call is below the serial sum of its copy-in,
    compute and copy-out spans (measured once, never retried).  In a fresh process: which hardware queues the feed's
    three streams share depends on the streams the process already has (GPU_MAX_HW_QUEUES), and a stream that shares
    its queue with another of the feed's serialises with it."""
    r = subprocess.run([sys.executable, "-c", _OVERLAP_CHILD % ROOT], capture_output=True, text=True, timeout=140)
    assert r.returncode == 0, r.stdout + r.stderr[-3000:]
    st = json.loads(r.stdout.strip().splitlines()[-1])
    assert (st["inputs_staged"], st["outputs_staged"], st["chunks"]) == (0, 0, 8), st
    serial = st["h2d_ms"] + st["compute_ms"] + st["d2h_ms"]
    assert min(st["h2d_ms"], st["compute_ms"], st["d2h_ms"]) > 0, st
    assert st["wall_ms"] < serial, json.dumps(st)


@pytest.mark.timeout(120)
def test_the_borrowed_handle_is_left_untouched(torch_cuda, vga65):
    torch = torch_cuda
    from kinectdepthmapenhancement_amd import filters as F
    bgr, depth = vga65
    jbf = F.JointBilateralFilter(640, 480, _params(F, W11), max_batch=8)
    jbf.process_batch(dev(torch, depth[:8]), dev(torch, bgr[:8]))       # into the handle's own buffers
    torch.cuda.synchronize()
    filtered = jbf.getFiltered_Device(8).clone()
    smooth = jbf.getSmoothImage_Device(8).clone()
    mirrored = jbf.getFiltered_Host()
    F.JointBilateralFilterFeed(jbf, 4).process(depth[20:36], bgr[20:36])
    torch.cuda.synchronize()
    assert torch.equal(jbf.getFiltered_Device(8), filtered)
    assert torch.equal(jbf.getSmoothImage_Device(8), smooth)
    assert np.array_equal(_bits(jbf.getFiltered_Host()), _bits(mirrored))
    assert np.array_equal(_bits(mirrored), _bits(host(filtered[0])))


@pytest.mark.timeout(120)
def test_invalid_arguments_on_a_real_handle_launch_nothing(torch_cuda, vga65):
    from kinectdepthmapenhancement_amd import _native as N, filters as F
    lib = N.lib()
    bgr, depth = vga65[0][:2], vga65[1][:2]
    jbf = F.JointBilateralFilter(640, 480, _params(F, W11))
    h = C.c_void_p()
    for chunk in (0, 65536, -1):
        assert lib.kde_jbf_feed_create(C.byref(h), jbf._h, chunk) == N.KDE_ERR_INVALID
        assert h.value is None and b"chunk_frames" in lib.kde_last_error_string()
    feed = F.JointBilateralFilterFeed(jbf, 1)
    out = np.full(depth.shape, -7.0, np.float32)
    d, c, o = depth.ctypes.data, bgr.ctypes.data, out.ctypes.data
    for args in ((2, d, 2, c, o), (2, d, -1, c, o), (0, d, 0, c, o), (-3, d, 0, c, o),
                 (2, None, 0, c, o), (2, d, 0, None, o), (2, d, 0, c, None)):
        assert lib.kde_jbf_feed_process(feed._h, *args) == N.KDE_ERR_INVALID, args
        assert b"kde_jbf_feed_process" in lib.kde_last_error_string()
    assert np.all(out == -7.0)
    assert feed.last_stats()["frames"] == 0                     # no call got as far as the pipeline
    with pytest.raises(ValueError):
        feed.process(depth.astype(np.float64), bgr)
    with pytest.raises(ValueError):
        feed.process(np.asfortranarray(depth[0]), bgr[0])
    with pytest.raises(ValueError):
        feed.process(depth, bgr[:1])
    with pytest.raises(TypeError):
        feed.process(dev(torch_cuda, depth), bgr)
    assert np.all(out == -7.0) and feed.last_stats()["frames"] == 0


@pytest.mark.timeout(120)
def test_a_call_while_another_device_is_current_is_rejected(torch_cuda, vga65):
    from kinectdepthmapenhancement_amd import _native as N, filters as F
    lib = N.lib()
    cnt = C.c_int(0)
    N.check(lib.kde_device_count(C.byref(cnt)))
    if cnt.value < 2:
        pytest.skip("needs a second visible device to make current")
    bgr, depth = vga65[0][:1], vga65[1][:1]
    feed = F.JointBilateralFilterFeed(F.JointBilateralFilter(640, 480), 1)
    out = np.full(depth.shape, -7.0, np.float32)
    N.check(lib.kde_set_device(1))
    try:
        rc = lib.kde_jbf_feed_process(feed._h, 1, depth.ctypes.data, 0, bgr.ctypes.data, out.ctypes.data)
    finally:
        N.check(lib.kde_set_device(0))
    assert rc == N.KDE_ERR_INVALID and b"device" in lib.kde_last_error_string()
    assert np.all(out == -7.0)


@pytest.mark.timeout(180)
def test_two_threads_with_their_own_feeds_on_one_device(torch_cuda, vga65):
    from kinectdepthmapenhancement_amd import filters as F
    bgr, depth = vga65
    shards = [(depth[0:24], bgr[0:24]), (depth[30:54], bgr[30:54])]
    feeds = [F.JointBilateralFilterFeed(F.JointBilateralFilter(640, 480, _params(F, W11)), 4) for _ in shards]
    alone = [f.process(d, c) for f, (d, c) in zip(feeds, shards)]
    together, errors = [None, None], []

    def run(k):
        try:
            together[k] = feeds[k].process(*shards[k])
        except Exception as e:            # reported by the main thread
            errors.append(repr(e))

    threads = [threading.Thread(target=run, args=(k,)) for k in range(2)]
    for t in threads:
        t.start()
    for t in threads:
        t.join(timeout=90)
    assert not errors and not any(t.is_alive() for t in threads), errors
    for a, b in zip(alone, together):
        assert np.array_equal(_bits(a), _bits(b))


@pytest.mark.timeout(300)
@pytest.mark.parametrize("u16", [False, True], ids=["f32", "u16"])
def test_shard_replay_host_fed_matches_the_resident_run(torch_cuda, u16):
    exe = os.path.join(ROOT, "examples", "shard_replay")
    if not os.path.exists(exe):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "examples"), "-s"])
    common = ["--share-device", "2", "--frames", "16", "--steps", "2", "--warmup", "1"] + (["--u16"] if u16 else [])
    lines = {}
    for mode, extra in (("host-fed", ["--host-fed", "--verify"]), ("resident", [])):
        r = subprocess.run([exe] + common + extra, capture_output=True, text=True, timeout=240)
        assert r.returncode == 0, r.stdout + r.stderr
        lines[mode] = json.loads(r.stdout.strip().splitlines()[-1])
    hf, res = lines["host-fed"], lines["resident"]
    assert hf["verified"] is True and hf["mode"].startswith("host-fed") and res["mode"].startswith("resident")
    assert hf["checksum"] == res["checksum"]
    assert hf["hostfed_mpixels_per_s"] > 0 and res["hostfed_mpixels_per_s"] is None
    assert all(d["h2d_GBs"] > 0 and d["d2h_GBs"] > 0 for d in hf["per_device"])
