"""DepthTemporalFilter (kde_temporal_*) at the ABI level, without a GPU: declared, exported and bound; the typed handle; the
defaults; every refusal that precedes a HIP call and its message; the in-place rule; getters before the first call; a
device-less create; the Python class, the C++ class and the demo.

On a host without a device kde_temporal_create makes the object without buffers, so the refusals that need a handle are checked
here as well."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

HEADER = os.path.join(ROOT, "include", "kde_hip.h")
COUNTS = ("smoothed", "jumped", "held", "changed")
DEVICE_GETTERS = ("kde_temporal_depth_device",) + tuple(f"kde_temporal_{c}_device" for c in COUNTS)
HOST_GETTERS = ("kde_temporal_depth_host",) + tuple(f"kde_temporal_{c}_host" for c in COUNTS)
FUNCS = ("kde_temporal_default_params", "kde_temporal_create", "kde_temporal_destroy", "kde_temporal_filter_batch", "kde_temporal_reset",
         "kde_temporal_state_device", "kde_temporal_set_shape", "kde_temporal_shape") + DEVICE_GETTERS + HOST_GETTERS
FLT_MAX = float(np.finfo(np.float32).max)
DEFAULTS = (float(np.float32(0.4)), 10.0, float(np.float32(0.02)), 3, 48, 0.0, FLT_MAX)
FIELDS = ["alpha", "max_diff", "rel_diff", "persist_min", "color_thresh", "z_min", "z_max"]


@pytest.fixture(scope="module")
def native():
    from kinectdepthmapenhancement_amd import _native
    if not os.path.exists(_native.LIB_PATH):
        _native.build()
    return _native


def _hipcc():
    return os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "bin", "hipcc")


def _fields(p):
    return tuple(getattr(p, name) for name, _ in p._fields_)


@pytest.mark.timeout(120)
def test_declared_exported_and_bound(native):
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    for name in FUNCS:
        assert re.search(r"\bint\s+" + name + r"\s*\(", text), name
    assert "#define KDE_ABI_VERSION 1" in text                     # the new entry points only add to the ABI
    lib = ctypes.CDLL(native.LIB_PATH)
    assert all(hasattr(lib, n) for n in FUNCS)
    assert {n for n in native.SIGNATURES if n.startswith("kde_temporal_")} == set(FUNCS)
    assert native.lib().kde_abi_version() == 1
    assert ctypes.sizeof(native.TemporalParams) == 28
    assert [n for n, _ in native.TemporalParams._fields_] == FIELDS
    # none of them is picked up by the enumeration of tools/abi_refusals.py, whose record is frozen
    frozen = (ctypes.c_void_p, ctypes.POINTER(ctypes.c_void_p))
    assert [n for n in FUNCS if native.SIGNATURES[n][1][0] in frozen] == []
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "abi_refusals.py")], capture_output=True, text=True, timeout=100)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "kde_temporal" not in r.stdout
    p = native.TemporalParams(9.0, 1.0, 2.0, 3, 4, 5.0, 6.0)
    assert native.lib().kde_temporal_default_params(ctypes.byref(p)) == native.KDE_OK
    assert _fields(p) == DEFAULTS


def test_the_header_states_the_rule():
    raw = re.sub(r"\s*\n \*\s*", " ", open(HEADER).read())                  # comment lines joined
    for must in ("The frames of a call are consecutive in time, and the object carries state from one call to the next",
                 "bits 0-7 hold the raw validity of the last eight frames, bit 0 the newest",
                 "b | g << 8 | r << 16 of the previous frame",
                 "kde_temporal_create and kde_temporal_reset set both words to 0",
                 "no fused multiply-add",
                 "z = (d > z_min && d < z_max) ? (float)d : 0",
                 "only with a guide and color_thresh < 765",
                 "value = 0 and hist &= ~0xFF",
                 "prev > 0 && fabsf(z - prev) <= max_diff + rel_diff * fminf(z, prev)",
                 "out = prev + alpha * (z - prev)",
                 "the difference, the product and the sum each rounded on its own",
                 "hist[7:0] = (hist[7:0] << 1 | 1) & 0xFF",
                 "prev > 0 && persist_min >= 1 && popcount(hist[7:0]) >= persist_min",
                 "the history before this frame's shift",
                 "held for at most eight frames after the last valid sample",
                 "value = out (the float, never the uint16 rounding)",
                 "integer sums taken before the uint16 rounding",
                 "a function of the sequence since the last reset and nothing else",
                 "how the sequence is cut into calls",
                 "In place is allowed exactly when out_dev == depth_dev and out_format == depth_format",
                 "each thread reads its pixel of frame t before it writes it",
                 "no memset node: capturable from the first call",
                 "Replaying a captured graph advances the stream by n frames",
                 "A launch on `stream`, not a memset node; capturable",
                 "writing to it between calls is allowed and is the way to restore a checkpoint",
                 "frames of height S * H",
                 "A sequence does not shard across GPUs"):
        assert must in raw, must


@pytest.mark.timeout(120)
def test_the_typed_handle_refuses_a_plain_void_pointer(native):
    lib = native.lib()
    assert issubclass(native.TemporalHandle, ctypes.c_void_p)
    assert lib.kde_temporal_destroy(None) == native.KDE_OK
    assert lib.kde_temporal_destroy(native.TemporalHandle()) == native.KDE_OK
    out = ctypes.c_void_p()
    for plain in (ctypes.c_void_p(), ctypes.c_void_p(16)):
        with pytest.raises(ctypes.ArgumentError):
            lib.kde_temporal_destroy(plain)
        with pytest.raises(ctypes.ArgumentError):
            lib.kde_temporal_filter_batch(plain, 1, None, 0, None, 0, None, None)
        with pytest.raises(ctypes.ArgumentError):
            lib.kde_temporal_reset(plain, None)
        with pytest.raises(ctypes.ArgumentError):
            lib.kde_temporal_state_device(plain, ctypes.byref(out), ctypes.byref(out))
        with pytest.raises(ctypes.ArgumentError):
            lib.kde_temporal_set_shape(plain, 0, 0)
        for name in DEVICE_GETTERS:
            with pytest.raises(ctypes.ArgumentError):
                getattr(lib, name)(plain, ctypes.byref(out))
        for name in HOST_GETTERS:
            with pytest.raises(ctypes.ArgumentError):
                getattr(lib, name)(plain, None, ctypes.byref(out))
        with pytest.raises(ctypes.ArgumentError):
            lib.kde_temporal_create(ctypes.byref(plain), 8, 8, 1, None)
    for other in (native.CloudHandle(), native.RegHandle(), native.UndistHandle(), native.UpsampleHandle(), native.HolefillHandle(),
                  native.SpeckleHandle()):
        with pytest.raises(ctypes.ArgumentError):
            lib.kde_temporal_destroy(other)
    from kinectdepthmapenhancement_amd import filters
    assert filters.DepthTemporalFilter._handle_type is native.TemporalHandle
    assert _fields(filters.DepthTemporalFilter.default_params()) == DEFAULTS


@pytest.mark.timeout(120)
def test_refusals_name_their_function(native):
    lib = native.lib()
    INVALID = native.KDE_ERR_INVALID
    Params = native.TemporalParams
    DF, DU = native.KDE_DEPTH_F32, native.KDE_DEPTH_U16
    nan, inf = float("nan"), float("inf")

    def refused(name, rc, *words):
        assert rc == INVALID, (name, rc, lib.kde_last_error_string())
        assert name.encode() in lib.kde_last_error_string(), (name, lib.kde_last_error_string())
        for word in words:
            assert word.encode() in lib.kde_last_error_string(), (word, lib.kde_last_error_string())

    def create(out, size=(8, 6), batch=1, params=None):
        return lib.kde_temporal_create(out if out is None else ctypes.byref(out), *size, batch, None if params is None else ctypes.byref(params))

    def with_(**kw):
        p = Params(*DEFAULTS)
        for k, v in kw.items():
            setattr(p, k, v)
        return p

    out = native.TemporalHandle()
    refused("kde_temporal_default_params", lib.kde_temporal_default_params(None))
    refused("kde_temporal_create", create(None))
    for size in ((0, 6), (8, 0), (-1, 6), (8, -3), (1 << 16, 1 << 15), (1 << 30, 2)):
        refused("kde_temporal_create", create(out, size), "bad size")
    for batch in (0, -1, 65536):
        refused("kde_temporal_create", create(out, batch=batch), "max_batch")
    bad = dict(alpha=(0.0, -0.5, 1.0000001, 2.0, nan, inf, -inf), max_diff=(-1.0, -1e-30, nan, inf, -inf), rel_diff=(-1.0, -1e-30, nan, inf, -inf),
               persist_min=(-1, 9, 100), color_thresh=(-1, 766, 1 << 20), z_min=(nan, inf, -inf, -1.0, -1e-30))
    for field, values in bad.items():
        for v in values:
            refused("kde_temporal_create", create(out, params=with_(**{field: v})), field)
    for zmin, zmax in ((100.0, 100.0), (200.0, 100.0), (FLT_MAX, FLT_MAX), (inf, inf), (0.0, nan), (0.0, 0.0), (0.0, -1.0)):
        refused("kde_temporal_create", create(out, params=with_(z_min=zmin, z_max=zmax)))
    assert out.value is None
    for params in (with_(alpha=1.0, max_diff=0.0, rel_diff=0.0, persist_min=0, color_thresh=0, z_max=inf),
                   with_(alpha=1e-30, max_diff=1e30, rel_diff=1e30, persist_min=8, color_thresh=765, z_min=5.0, z_max=6.0),
                   with_(max_diff=-0.0, rel_diff=-0.0)):          # the limits are inside
        for size in ((8, 6), (1, 1), (1 << 24, 1)):
            assert create(out, size, params=params) == native.KDE_OK, lib.kde_last_error_string()
            assert lib.kde_temporal_destroy(out) == native.KDE_OK
            out = native.TemporalHandle()
    # null handles
    p, q = ctypes.c_void_p(), ctypes.c_void_p()
    P, U = ctypes.c_int(), ctypes.c_int()
    refused("kde_temporal_filter_batch", lib.kde_temporal_filter_batch(None, 1, 4096, DF, None, DF, None, None))
    refused("kde_temporal_reset", lib.kde_temporal_reset(None, None))
    refused("kde_temporal_state_device", lib.kde_temporal_state_device(None, ctypes.byref(p), ctypes.byref(q)))
    refused("kde_temporal_set_shape", lib.kde_temporal_set_shape(None, 0, 0))
    refused("kde_temporal_shape", lib.kde_temporal_shape(None, 1, ctypes.byref(P), ctypes.byref(U)))
    for name in DEVICE_GETTERS:
        refused(name, getattr(lib, name)(None, ctypes.byref(p)))
    for name in HOST_GETTERS:
        refused(name, getattr(lib, name)(None, None, ctypes.byref(p)))
    assert lib.kde_temporal_destroy(None) == native.KDE_OK

    h = native.TemporalHandle()
    assert create(h, (20, 13), 4, Params(0.5, 3.0, 0.5, 2, 100, 100.0, 5000.0)) == native.KDE_OK, lib.kde_last_error_string()
    assert h.value
    try:
        for name in DEVICE_GETTERS:
            refused(name, getattr(lib, name)(h, None))
            refused(name, getattr(lib, name)(h, ctypes.byref(p)), "kde_temporal_filter_batch was not called")      # getters before the first call
        for name in HOST_GETTERS:
            refused(name, getattr(lib, name)(h, None, None))
            refused(name, getattr(lib, name)(h, None, ctypes.byref(p)), "kde_temporal_filter_batch was not called")
        refused("kde_temporal_state_device", lib.kde_temporal_state_device(h, None, ctypes.byref(q)))
        refused("kde_temporal_state_device", lib.kde_temporal_state_device(h, ctypes.byref(p), None))
        for shape in ((3, 1), (4, 3), (16, 1), (4, 8), (0, 1), (1, 0), (-1, -1)):
            refused("kde_temporal_set_shape", lib.kde_temporal_set_shape(h, *shape), "pixels_per_thread")
        refused("kde_temporal_shape", lib.kde_temporal_shape(h, 1, None, ctypes.byref(U)))
        refused("kde_temporal_shape", lib.kde_temporal_shape(h, 5, ctypes.byref(P), ctypes.byref(U)), "outside 1..max_batch=4")
        for n in (1, 2, 4):
            assert lib.kde_temporal_shape(h, n, ctypes.byref(P), ctypes.byref(U)) == native.KDE_OK
            assert P.value in (1, 2, 4, 8) and U.value in (1, 2, 4) and U.value <= n                 # never frames ahead of the call's last
        assert lib.kde_temporal_set_shape(h, 8, 2) == native.KDE_OK
        assert lib.kde_temporal_shape(h, 1, ctypes.byref(P), ctypes.byref(U)) == native.KDE_OK and (P.value, U.value) == (8, 2)
        assert lib.kde_temporal_set_shape(h, 0, 0) == native.KDE_OK

        def call(n, src=4096, dfmt=DF, bgr=None, ofmt=DF, out_dev=1 << 20):
            return lib.kde_temporal_filter_batch(h, n, src, dfmt, bgr, ofmt, out_dev, None)

        who = "kde_temporal_filter_batch"
        refused(who, call(2, src=None), "null argument")
        for n in (5, 0, -1):
            refused(who, call(n), "outside 1..max_batch=4")
        for fmt in (2, -1):
            refused(who, call(2, dfmt=fmt), "unknown depth format")
            refused(who, call(2, ofmt=fmt), "unknown output format")
        refused(who, call(2, src=4098), "depth_dev is not 4-byte aligned")
        refused(who, call(2, src=4097, dfmt=DU), "depth_dev is not 2-byte aligned")
        refused(who, call(2, out_dev=65538), "out_dev is not 4-byte aligned")
        refused(who, call(2, ofmt=DU, out_dev=65537), "out_dev is not 2-byte aligned")
        frame = 20 * 13
        for out_dev in (4096 + 4 * frame, 4096 - 4 * (2 * frame - 1), 4096 + 4 * (2 * frame - 1), 4100):        # partial overlaps
            refused(who, call(2, out_dev=out_dev), "out_dev overlaps depth_dev (in place is supported only with out_dev == depth_dev and "
                    "out_format == depth_format)")
        refused(who, call(2, ofmt=DU, out_dev=4096), "in place")            # the same pointer in another format
        refused(who, call(2, dfmt=DU, ofmt=DF, out_dev=4096), "in place")
        big = 1 << 20
        for bgr in (big, big + 8 * frame - 1, big - 6 * frame + 1, big + 5):                                     # the written frames and the guide
            refused(who, call(2, bgr=bgr), "out_dev overlaps bgr_dev")
        refused(who, call(2, bgr=4096 + 3, out_dev=4096), "out_dev overlaps bgr_dev")                            # in place, but on the guide too
        # still no call went through
        refused("kde_temporal_depth_device", lib.kde_temporal_depth_device(h, ctypes.byref(p)))
        refused("kde_temporal_changed_host", lib.kde_temporal_changed_host(h, None, ctypes.byref(p)))
    finally:
        assert lib.kde_temporal_destroy(h) == native.KDE_OK


@pytest.mark.timeout(120)
def test_a_valid_call_on_a_host_without_a_device_is_a_hip_error(native):
    """the object is created without buffers there; everything validates as usual and the launch then answers KDE_ERR_HIP.  In
    place -- out_dev == depth_dev in depth's format -- is such a valid call, and so is a reset."""
    import torch
    if torch.cuda.is_available():
        pytest.skip("this host has a device: tests/test_gpu_temporal.py makes the same calls for real")
    lib = native.lib()
    h = native.TemporalHandle()
    assert lib.kde_temporal_create(ctypes.byref(h), 20, 13, 2, None) == native.KDE_OK
    px = 2 * 20 * 13
    assert lib.kde_temporal_filter_batch(h, 2, 4096, 0, None, 1, None, None) == native.KDE_ERR_HIP
    assert lib.kde_temporal_filter_batch(h, 2, 4096, 0, None, 0, 4096, None) == native.KDE_ERR_HIP            # in place, float
    assert lib.kde_temporal_filter_batch(h, 2, 4098, 1, 1 << 20, 1, 4098, None) == native.KDE_ERR_HIP         # in place, uint16, a guide
    assert lib.kde_temporal_filter_batch(h, 2, 4097 * 4, 0, 4097 * 4 + px * 8 + 1, 0, 4097 * 4 + px * 4, None) == native.KDE_ERR_HIP   # the frames just do not overlap
    assert b"kde_temporal_filter_batch" in lib.kde_last_error_string() and b"without a device" in lib.kde_last_error_string()
    assert lib.kde_temporal_reset(h, None) == native.KDE_ERR_HIP
    assert b"kde_temporal_reset" in lib.kde_last_error_string() and b"without a device" in lib.kde_last_error_string()
    p, q = ctypes.c_void_p(), ctypes.c_void_p(5)
    assert lib.kde_temporal_depth_device(h, ctypes.byref(p)) == native.KDE_ERR_INVALID
    assert lib.kde_temporal_state_device(h, ctypes.byref(p), ctypes.byref(q)) == native.KDE_OK and p.value is None and q.value is None
    assert lib.kde_temporal_destroy(h) == native.KDE_OK
    from kinectdepthmapenhancement_amd import filters
    T = filters.DepthTemporalFilter((20, 13), 2)
    with pytest.raises(native.KdeError, match="was not called"):
        T.smoothed_device()
    with pytest.raises(AttributeError):
        T.filled()
    with pytest.raises(TypeError):
        T.filter(torch.zeros((2, 13, 20)))                             # a host tensor
    assert T.shape(2)[1] <= 2
    T.close()


@pytest.mark.timeout(600)
def test_cpp_class_and_demo_compile(tmp_path):
    src = tmp_path / "temporal_user.cpp"
    src.write_text(r"""
#include "kde/kde.hpp"
#include <cstdint>
static_assert(sizeof(kde_temporal_params) == 28, "kde_temporal_params: seven four-byte fields");
int main()
{
    kde::DepthTemporalFilter one(1920, 1080);                         // one frame per call, the defaults
    kde_temporal_params p = kde::DepthTemporalFilter::defaultParams();
    p.alpha = 0.25f;
    p.persist_min = 2;
    p.color_thresh = 765;
    kde::DepthTemporalFilter temporal(640, 480, 8, p);                // RAII over kde_temporal_create / _destroy
    float* depth = nullptr;
    uint16_t* depth16 = nullptr;
    float* out = nullptr;
    uint16_t* out16 = nullptr;
    uint8_t* bgr = nullptr;
    temporal.filter(8, depth, bgr, out);
    temporal.filter(8, depth16, nullptr, out);
    temporal.filter(8, depth, bgr, out16);
    temporal.filter(8, depth16, bgr, depth16);                        // in place
    temporal.reset();
    temporal.setStream(nullptr);
    float* value = nullptr;
    uint32_t* hist = nullptr;
    temporal.state_Device(value, hist);
    const void* host = temporal.depth_Host();
    const uint32_t* smoothed = temporal.smoothed_Host();
    const uint32_t* jumped = temporal.jumped_Host();
    const uint32_t* held = temporal.held_Host();
    const uint32_t* changed = temporal.changed_Host();
    void* dev = temporal.depth_Device();
    uint32_t* sdev = temporal.smoothed_Device();
    uint32_t* jdev = temporal.jumped_Device();
    uint32_t* hdev = temporal.held_Device();
    uint32_t* cdev = temporal.changed_Device();
    kde_temporal* h = temporal.handle();
    kde::DepthSpeckleFilter speckle(640, 480, 8);                     // the chain of examples/temporal_demo.cpp
    speckle.filter(8, depth, depth);
    kde::DepthHoleFilling fill(640, 480, 8);
    fill.fill(8, static_cast<const float*>(dev), bgr, 8, out);
    return (host != nullptr) + (int)smoothed[0] + (int)jumped[0] + (int)held[0] + (int)changed[0] + (sdev != nullptr) + (jdev != nullptr) +
           (hdev != nullptr) + (cdev != nullptr) + (h != nullptr) + (value != nullptr) + (hist != nullptr);
}
""")
    inc = os.path.join(ROOT, "include")
    r = subprocess.run([_hipcc(), "-std=c++17", "-fsyntax-only", "-I", inc, str(src)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    hidden = tmp_path / "hidden.cpp"                                   # this stage fills nothing
    hidden.write_text('#include "kde/kde.hpp"\nint main() { kde::DepthTemporalFilter s(8, 8); return s.filled_Host() != nullptr; }\n')
    r = subprocess.run([_hipcc(), "-std=c++17", "-fsyntax-only", "-I", inc, str(hidden)], capture_output=True, text=True, timeout=300)
    assert r.returncode != 0 and "private" in r.stderr
    demo = os.path.join(ROOT, "examples", "temporal_demo.cpp")
    r = subprocess.run([_hipcc(), "-std=c++17", "-x", "hip", "--offload-arch=gfx950", "-fsyntax-only", demo], capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    text = open(demo).read()
    for stage in ("DepthSpeckleFilter", "DepthTemporalFilter", "DepthHoleFilling", "JointBilateralFilter"):
        assert "kde::" + stage in text or "kde::ref::" + stage in text, stage
    assert "temporal_demo" in open(os.path.join(ROOT, "examples", "Makefile")).read()
    size = tmp_path / "size.c"
    size.write_text('#include "kde_hip.h"\n#include <stdio.h>\nint main(void) { printf("%zu\\n", sizeof(kde_temporal_params)); return 0; }\n')
    exe = str(tmp_path / "size")
    subprocess.check_call(["cc", "-std=c11", "-I", inc, "-o", exe, str(size)], timeout=120)
    assert subprocess.run([exe], capture_output=True, text=True, check=True, timeout=60).stdout.split() == ["28"]


def test_the_kernel_file_is_what_the_issue_asks_for():
    csrc = os.path.join(ROOT, "kinectdepthmapenhancement_amd", "csrc")
    kernels = open(os.path.join(csrc, "temporal_kernels.hip")).read()
    assert "__builtin_nontemporal_load" in kernels and "__builtin_nontemporal_store" in kernels
    for banned in ("hipMemsetAsync", "hipMemset(", "hipMalloc", "hipStreamSynchronize", "hipDeviceSynchronize", "atomicAdd", "__syncthreads_or"):
        assert banned not in kernels, banned
    assert "temporal_kernels.o" in open(os.path.join(csrc, "objects.mk")).read()
    assert "kde_api_temporal.o" in open(os.path.join(csrc, "objects.mk")).read()
    assert "launch_temporal" in open(os.path.join(csrc, "kde_internal.h")).read()
