"""Host-fed KinectDepthEnhancement (kde_enh_feed_*, filters.KinectDepthEnhancementFeed): frames in host memory, chunked
copy-in / Process / output step / copy-out on the feed's three streams.  The bar is the resident path: every result is
bit-identical to kde_enh_process_batch on the same frames (followed by kde_points_to_depth for the two depth formats), whatever
the chunking, the depth format, the output format or the kind of host memory."""
import ctypes as C
import os
import subprocess
import zlib

import numpy as np
import pytest

from conftest import ROOT
from gpu_util import dev

pytestmark = pytest.mark.gpu

W, H, ROWS, COLS = 80, 64, 4, 5               # the shape of test_gpu_enh.py
SEEDS = (1, 2, 3, 4, 5, 6, 7)
ESIZE = {"points": 12, "depth": 4, "depth_u16": 2}


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def _pinned(torch, a):
    """a pinned copy of a numpy array as a numpy array (uint16 goes through an int16 tensor), and the tensor that owns it"""
    t = torch.from_numpy(a.view(np.int16) if a.dtype == np.uint16 else a).pin_memory()
    return t.numpy().view(a.dtype), t


@pytest.fixture(scope="module")
def scene(torch_cuda):
    """the 7 frames as float and as uint16 depth, and for each the resident result in the three output formats"""
    torch = torch_cuda
    from kinectdepthmapenhancement_amd import filters as F, synth
    torch.cuda.set_device(0)
    fr = [synth.make_frame(s, W, H) for s in SEEDS]
    bgr = np.ascontiguousarray(np.stack([f[0] for f in fr]))
    d32 = np.ascontiguousarray(np.stack([f[1] for f in fr]), np.float32)
    d16 = np.where(d32 > 0, np.rint(d32), 0).astype(np.uint16)
    K = synth.intrinsics(W, H)
    enh = F.KinectDepthEnhancement(W, H, max_batch=len(SEEDS))
    enh.SetParametor(ROWS, COLS, K)
    ref = {}
    for name, depth in (("f32", d32), ("u16", d16.astype(np.float32))):
        enh.process_batch(dev(torch, depth), dev(torch, bgr))
        pts = enh.getOptimizedPoints_Device().reshape(len(SEEDS), H, W, 3)
        ref[name] = {"points": pts.cpu().numpy(), "depth": F.points_to_depth(pts).cpu().numpy(),
                     "depth_u16": F.points_to_depth(pts, dtype=torch.int16).cpu().numpy().view(np.uint16)}
    torch.cuda.synchronize()
    enh.close()
    for r in ref.values():                    # the scene is worth the name: most pixels keep a depth, the formats agree
        assert (r["points"][..., 2] > 50).mean() > 0.5 and (r["depth_u16"] > 0).mean() > 0.5
        assert np.array_equal(_bits(r["depth"]), _bits(np.ascontiguousarray(r["points"][..., 2])))
    return {"bgr": bgr, "f32": d32, "u16": d16, "K": K, "ref": ref}


@pytest.fixture(scope="module")
def enh4(torch_cuda, scene):
    from kinectdepthmapenhancement_amd import filters as F
    enh = F.KinectDepthEnhancement(W, H, max_batch=4)
    enh.SetParametor(ROWS, COLS, scene["K"])
    yield enh
    enh.close()


CASES = [  # n, chunk, depth format, pinned inputs, pinned output, output format
    (7, 2, "f32", False, False, "points"),
    (7, 2, "u16", True, True, "depth_u16"),
    (7, 2, "u16", False, True, "depth"),
    (7, 2, "f32", True, False, "depth_u16"),
    (1, 4, "u16", False, False, "points"),
    (1, 4, "f32", True, True, "depth"),
]


@pytest.mark.parametrize("n,chunk,fmt,pin_in,pin_out,output", CASES,
                         ids=[f"n{c[0]}_chunk{c[1]}_{c[2]}_{'pin' if c[3] else 'page'}_{'pin' if c[4] else 'page'}_{c[5]}" for c in CASES])
def test_bit_identical_to_the_resident_batch(torch_cuda, scene, enh4, n, chunk, fmt, pin_in, pin_out, output):
    torch = torch_cuda
    from kinectdepthmapenhancement_amd import filters as F
    depth, bgr, ref = scene[fmt][:n], scene["bgr"][:n], scene["ref"][fmt][output][:n]
    keep = []
    if pin_in:
        (depth, t1), (bgr, t2) = _pinned(torch, depth), _pinned(torch, bgr)
        keep += [t1, t2]
    out = np.full(ref.shape, 0xAB, ref.dtype) if ref.dtype == np.uint16 else np.full(ref.shape, -7.0, np.float32)
    if pin_out:
        out, t3 = _pinned(torch, out)
        keep.append(t3)
    feed = F.KinectDepthEnhancementFeed(enh4, chunk)
    got = feed.process(depth, bgr, out, output=output)
    assert got is out
    st = feed.last_stats()
    cf = min(chunk, n)
    assert (st["frames"], st["chunk_frames"], st["chunks"]) == (n, cf, -(-n // cf))
    assert (st["inputs_staged"], st["outputs_staged"]) == (int(not pin_in), int(not pin_out))
    assert st["h2d_bytes"] == W * H * n * ((2 if fmt == "u16" else 4) + 3) and st["d2h_bytes"] == W * H * n * ESIZE[output]
    assert st["wall_ms"] > 0
    assert np.array_equal(_bits(got), _bits(ref)), f"{int((_bits(got) != _bits(ref)).sum())} elements differ"
    feed.close()


def test_one_feed_serves_every_format_and_leaves_the_object_usable(torch_cuda, scene, enh4):
    """a slot sized for 2-byte outputs is resized for 12-byte ones (and uint16 landing areas appear on demand); the default
    chunk is max_batch; afterwards the borrowed object's getters show the last chunk, and it still runs on its own"""
    torch = torch_cuda
    from kinectdepthmapenhancement_amd import filters as F
    feed = F.KinectDepthEnhancementFeed(enh4)
    assert feed.chunk_frames == 4
    n = len(SEEDS)
    for fmt, output in (("f32", "depth_u16"), ("u16", "points"), ("f32", "depth"), ("u16", "depth_u16")):
        got = feed.process(scene[fmt], scene["bgr"], output=output)
        ref = scene["ref"][fmt][output]
        assert got.dtype == ref.dtype and got.shape == ref.shape
        assert np.array_equal(_bits(got), _bits(ref)), (fmt, output)
        assert feed.last_stats()["d2h_bytes"] == W * H * n * ESIZE[output] and feed.last_stats()["chunks"] == 2
    # the last chunk of the last call: frames 4..6 of the uint16 run
    last = enh4.getOptimizedPoints_Device().reshape(3, H, W, 3).cpu().numpy()
    assert np.array_equal(_bits(last), _bits(scene["ref"]["u16"]["points"][4:]))
    enh4.process_batch(dev(torch, scene["f32"][:2]), dev(torch, scene["bgr"][:2]))
    own = enh4.getOptimizedPoints_Device().reshape(2, H, W, 3).cpu().numpy()
    assert np.array_equal(_bits(own), _bits(scene["ref"]["f32"]["points"][:2]))
    again = feed.process(scene["f32"][:3], scene["bgr"][:3], output="depth")
    assert np.array_equal(_bits(again), _bits(scene["ref"]["f32"]["depth"][:3]))
    feed.close()


def test_refusals(torch_cuda, scene, enh4):
    from kinectdepthmapenhancement_amd import _native as N, filters as F
    lib = N.lib()
    depth, bgr = scene["f32"][:2], scene["bgr"][:2]
    h = N.EnhFeedHandle()
    for chunk in (0, 5, -1, 65536):                                   # enh4.max_batch is 4
        assert lib.kde_enh_feed_create(C.byref(h), enh4._h, chunk) == N.KDE_ERR_INVALID
        assert h.value is None and b"kde_enh_feed_create" in lib.kde_last_error_string() and b"chunk_frames" in lib.kde_last_error_string()
    with pytest.raises(N.KdeError):
        F.KinectDepthEnhancementFeed(enh4, 5)
    feed = F.KinectDepthEnhancementFeed(enh4, 1)
    out = np.full((2, H, W, 3), -7.0, np.float32)
    d, c, o = depth.ctypes.data, bgr.ctypes.data, out.ctypes.data
    for args in ((2, d, 2, c, 0, o), (2, d, -1, c, 0, o), (2, d, 0, c, 3, o), (2, d, 0, c, -1, o), (0, d, 0, c, 0, o), (-3, d, 0, c, 0, o),
                 (2, None, 0, c, 0, o), (2, d, 0, None, 0, o), (2, d, 0, c, 0, None)):
        assert lib.kde_enh_feed_process(feed._h, *args) == N.KDE_ERR_INVALID, args
        assert b"kde_enh_feed_process" in lib.kde_last_error_string()
    assert np.all(out == -7.0) and feed.last_stats()["frames"] == 0   # no call got as far as the pipeline
    with pytest.raises(ValueError):
        feed.process(depth.astype(np.float64), bgr)
    with pytest.raises(ValueError):
        feed.process(depth, bgr[:1])
    with pytest.raises(ValueError):
        feed.process(depth, bgr, output="cloud")
    with pytest.raises(ValueError):
        feed.process(depth, bgr, np.empty((2, H, W), np.float32), output="depth_u16")
    with pytest.raises(TypeError):
        feed.process(dev(torch_cuda, depth), bgr)
    feed.close()
    # an object whose SetParametor was not called: the feed is created, process returns the object's own refusal
    unset = F.KinectDepthEnhancement(W, H, max_batch=2)
    f2 = F.KinectDepthEnhancementFeed(unset, 2)
    with pytest.raises(N.KdeError, match="SetParametor was not called"):
        f2.process(depth, bgr, out)
    assert np.all(out == -7.0) and f2.last_stats()["frames"] == 0
    unset.SetParametor(ROWS, COLS, scene["K"])
    got = f2.process(depth, bgr, out)                                 # and the feed works once it was
    assert np.array_equal(_bits(got), _bits(scene["ref"]["f32"]["points"][:2]))
    f2.close()
    unset.close()


def test_enh_feed_demo_agrees_with_the_python_path(torch_cuda, tmp_path):
    """examples/enh_feed_demo: uint16 VGA frames through kde::KinectDepthEnhancementFeed, uint16 depth out; it prints the frame
    count, the number of valid pixels and the CRC-32 of the result, and writes its inputs next to the result"""
    from kinectdepthmapenhancement_amd import filters as F
    exe = os.path.join(ROOT, "examples", "enh_feed_demo")
    assert os.path.exists(exe), "examples/enh_feed_demo is built by __graft_entry__.build()"
    r = subprocess.run([exe, str(tmp_path), "3"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "enh_feed_demo ok 640x480" in r.stdout, r.stdout + r.stderr
    tok = r.stdout.split("enh_feed_demo ok 640x480")[1].split()
    frames, valid, crc = int(tok[tok.index("frames") + 1]), int(tok[tok.index("valid") + 1]), int(tok[tok.index("crc32") + 1], 16)
    assert frames == 3
    w, h = 640, 480
    d16 = np.fromfile(str(tmp_path / "enh_feed_in_depth.bin"), np.uint16).reshape(frames, h, w)
    bgr = np.fromfile(str(tmp_path / "enh_feed_in_bgr.bin"), np.uint8).reshape(frames, h, w, 3)
    f = 575.8 * w / 640.0
    enh = F.KinectDepthEnhancement(w, h, max_batch=2)
    enh.SetParametor(15, 20, [[f, 0.0, w / 2.0], [0.0, f, h / 2.0], [0.0, 0.0, 1.0]])
    feed = F.KinectDepthEnhancementFeed(enh, 2)
    got = feed.process(d16, bgr, output="depth_u16")
    assert (zlib.crc32(got.tobytes()) & 0xFFFFFFFF) == crc and int((got != 0).sum()) == valid
    assert np.array_equal(np.fromfile(str(tmp_path / "enh_feed_depth.bin"), np.uint16).reshape(got.shape), got)
    feed.close()
    enh.close()
