"""LensUndistortion (kde_undist_*) at the ABI level, without a GPU: declared, exported and bound; the typed handle; every
refusal that precedes a HIP call; the C++ class and the demo compile.

On a host without a device kde_undist_create makes the object without buffers, so the refusals that need a handle (a call
before the calibration, results before a call, ...) are checked here as well."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

HEADER = os.path.join(ROOT, "include", "kde_hip.h")
FUNCS = ("kde_undist_default_params", "kde_undist_create", "kde_undist_destroy", "kde_undist_set_calibration", "kde_undist_color_batch",
         "kde_undist_depth_batch", "kde_undist_depth_device", "kde_undist_depth_host", "kde_undist_filled_device",
         "kde_undist_filled_host", "kde_undist_map_device")
FLT_MAX = float(np.finfo(np.float32).max)


@pytest.fixture(scope="module")
def native():
    from kinectdepthmapenhancement_amd import _native
    if not os.path.exists(_native.LIB_PATH):
        _native.build()
    return _native


def _hipcc():
    return os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "bin", "hipcc")


@pytest.mark.timeout(120)
def test_declared_exported_and_bound(native):
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    for name in FUNCS:
        assert re.search(r"\bint\s+" + name + r"\s*\(", text), name
    assert "#define KDE_ABI_VERSION 1" in text                     # the new entry points only add to the ABI
    lib = ctypes.CDLL(native.LIB_PATH)
    assert all(hasattr(lib, n) for n in FUNCS)
    assert {n for n in native.SIGNATURES if n.startswith("kde_undist_")} == set(FUNCS)
    assert native.lib().kde_abi_version() == 1
    assert ctypes.sizeof(native.UndistParams) == 16
    # none of them is picked up by the enumeration of tools/abi_refusals.py, whose record is frozen
    frozen = (ctypes.c_void_p, ctypes.POINTER(ctypes.c_void_p))
    assert [n for n in FUNCS if native.SIGNATURES[n][1][0] in frozen] == []
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "abi_refusals.py")], capture_output=True, text=True, timeout=100)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "kde_undist" not in r.stdout
    # the header states the rule, and the registration's block points here
    raw = open(HEADER).read()
    for must in ("rad = num / den", "k1, k2, p1, p2, k3, k4, k5, k6", "no rectifying rotation", "ties to even", "max - min of the four <= max_gap",
                 "before the uint16 rounding", "kde_undist_*, below"):
        assert must in raw, must
    p = native.UndistParams(1.0, 2.0, 3, 4.0)
    assert native.lib().kde_undist_default_params(ctypes.byref(p)) == native.KDE_OK
    assert (p.z_min, p.z_max, p.depth_interp, p.max_gap) == (0.0, FLT_MAX, 0, 0.0)


@pytest.mark.timeout(120)
def test_the_typed_handle_refuses_a_plain_void_pointer(native):
    lib = native.lib()
    assert issubclass(native.UndistHandle, ctypes.c_void_p)
    assert lib.kde_undist_destroy(None) == native.KDE_OK
    assert lib.kde_undist_destroy(native.UndistHandle()) == native.KDE_OK
    out = ctypes.c_void_p()
    for plain in (ctypes.c_void_p(), ctypes.c_void_p(16)):
        with pytest.raises(ctypes.ArgumentError):
            lib.kde_undist_destroy(plain)
        with pytest.raises(ctypes.ArgumentError):
            lib.kde_undist_set_calibration(plain, None, None, None)
        with pytest.raises(ctypes.ArgumentError):
            lib.kde_undist_color_batch(plain, 1, None, 1, None, None)
        with pytest.raises(ctypes.ArgumentError):
            lib.kde_undist_depth_batch(plain, 1, None, 0, 0, None, None)
        for name in ("kde_undist_depth_device", "kde_undist_filled_device"):
            with pytest.raises(ctypes.ArgumentError):
                getattr(lib, name)(plain, ctypes.byref(out))
        for name in ("kde_undist_depth_host", "kde_undist_filled_host", "kde_undist_map_device"):
            with pytest.raises(ctypes.ArgumentError):
                getattr(lib, name)(plain, None, ctypes.byref(out))
        with pytest.raises(ctypes.ArgumentError):
            lib.kde_undist_create(ctypes.byref(plain), 8, 8, 8, 8, 1, None)
    for other in (native.CloudHandle(), native.RegHandle()):       # another typed handle is refused as well
        with pytest.raises(ctypes.ArgumentError):
            lib.kde_undist_destroy(other)
    from kinectdepthmapenhancement_amd import filters
    assert filters.LensUndistortion._handle_type is native.UndistHandle


@pytest.mark.timeout(120)
def test_refusals_name_their_function(native):
    lib = native.lib()
    INVALID = native.KDE_ERR_INVALID
    Params = native.UndistParams
    DF, DU = native.KDE_DEPTH_F32, native.KDE_DEPTH_U16
    nan, inf = float("nan"), float("inf")

    def refused(name, rc):
        assert rc == INVALID, (name, rc, lib.kde_last_error_string())
        assert name.encode() in lib.kde_last_error_string(), (name, lib.kde_last_error_string())

    out = native.UndistHandle()
    refused("kde_undist_default_params", lib.kde_undist_default_params(None))
    # create: null out, sizes below 1, bad batch, then every bad parameter block
    refused("kde_undist_create", lib.kde_undist_create(None, 8, 8, 8, 8, 1, None))
    for sizes in ((0, 8, 8, 8), (8, 0, 8, 8), (8, 8, 0, 8), (8, 8, 8, 0), (-1, 8, 8, 8), (8, 8, 8, -3), ((1 << 24) + 1, 1, 8, 8),
                  (8, 8, 1, (1 << 24) + 1)):
        refused("kde_undist_create", lib.kde_undist_create(ctypes.byref(out), *sizes, 1, None))
    refused("kde_undist_create", lib.kde_undist_create(ctypes.byref(out), 8, 8, 8, 8, 0, None))
    for zmin, zmax in ((nan, 100.0), (inf, inf), (-inf, 100.0), (-1.0, 100.0), (-1e-30, 100.0), (50.0, nan), (100.0, 100.0),
                       (200.0, 100.0), (FLT_MAX, FLT_MAX)):
        refused("kde_undist_create", lib.kde_undist_create(ctypes.byref(out), 8, 8, 8, 8, 1, ctypes.byref(Params(zmin, zmax, 0, 0.0))))
    for interp in (-1, 2, 1 << 20):
        refused("kde_undist_create", lib.kde_undist_create(ctypes.byref(out), 8, 8, 8, 8, 1, ctypes.byref(Params(0.0, FLT_MAX, interp, 50.0))))
    for gap in (0.0, -0.0, -50.0, nan, inf, -inf):                # depth_interp 1 needs a finite max_gap > 0 ...
        refused("kde_undist_create", lib.kde_undist_create(ctypes.byref(out), 8, 8, 8, 8, 1, ctypes.byref(Params(0.0, FLT_MAX, 1, gap))))
        assert b"max_gap" in lib.kde_last_error_string()
    assert out.value is None
    for gap in (0.0, -50.0, nan, inf):                            # ... which depth_interp 0 does not read
        assert lib.kde_undist_create(ctypes.byref(out), 8, 8, 8, 8, 1, ctypes.byref(Params(0.0, FLT_MAX, 0, gap))) == native.KDE_OK
        assert lib.kde_undist_destroy(out) == native.KDE_OK
        out = native.UndistHandle()
    # null handles
    K = (ctypes.c_double * 9)(500, 0, 3.5, 0, 500, 2.5, 0, 0, 1)
    Kn = (ctypes.c_double * 9)(480, 0, 4.5, 0, 480, 3.5, 0, 0, 1)
    D = (ctypes.c_double * 8)(-0.2, 0.05, 0.001, -0.001, 0.01, 0.02, 0.003, 0.0004)
    p = ctypes.c_void_p()
    refused("kde_undist_set_calibration", lib.kde_undist_set_calibration(None, K, D, Kn))
    refused("kde_undist_color_batch", lib.kde_undist_color_batch(None, 1, 8192, 1, 16384, None))
    refused("kde_undist_depth_batch", lib.kde_undist_depth_batch(None, 1, 4096, DF, DF, None, None))
    refused("kde_undist_depth_device", lib.kde_undist_depth_device(None, ctypes.byref(p)))
    refused("kde_undist_filled_device", lib.kde_undist_filled_device(None, ctypes.byref(p)))
    refused("kde_undist_depth_host", lib.kde_undist_depth_host(None, None, ctypes.byref(p)))
    refused("kde_undist_filled_host", lib.kde_undist_filled_host(None, None, ctypes.byref(p)))
    refused("kde_undist_map_device", lib.kde_undist_map_device(None, None, ctypes.byref(p)))
    assert lib.kde_undist_destroy(None) == native.KDE_OK

    # an object for 4 frames (with buffers on a GPU host, without on any other: the checks are the same), non-default parameters
    h = native.UndistHandle()
    assert lib.kde_undist_create(ctypes.byref(h), 8, 6, 10, 7, 4, ctypes.byref(Params(100.0, 2000.0, 1, 50.0))) == native.KDE_OK, \
        lib.kde_last_error_string()
    assert h.value
    try:
        for name in ("kde_undist_depth_device", "kde_undist_filled_device"):
            refused(name, getattr(lib, name)(h, None))
            refused(name, getattr(lib, name)(h, ctypes.byref(p)))                              # getters before the first call
        for name in ("kde_undist_depth_host", "kde_undist_filled_host"):
            refused(name, getattr(lib, name)(h, None, None))
            refused(name, getattr(lib, name)(h, None, ctypes.byref(p)))
        refused("kde_undist_map_device", lib.kde_undist_map_device(h, None, None))

        def color(n, bgr=8192, frames=1, out_dev=16384):
            return lib.kde_undist_color_batch(h, n, bgr, frames, out_dev, None)

        def depth(n, src=4096, dfmt=DF, ofmt=DF, out_dev=None):
            return lib.kde_undist_depth_batch(h, n, src, dfmt, ofmt, out_dev, None)

        # a call before the calibration
        for name, call in (("kde_undist_color_batch", lambda: color(2)), ("kde_undist_depth_batch", lambda: depth(2)),
                           ("kde_undist_map_device", lambda: lib.kde_undist_map_device(h, None, ctypes.byref(p)))):
            refused(name, call())
            assert b"kde_undist_set_calibration" in lib.kde_last_error_string()
        # the calibration: null pointers (K_new may be null), non-finite values, fx or fy not above 0
        refused("kde_undist_set_calibration", lib.kde_undist_set_calibration(h, None, D, Kn))
        refused("kde_undist_set_calibration", lib.kde_undist_set_calibration(h, K, None, Kn))
        for which, size in ((0, 9), (1, 8), (2, 9)):
            for i in range(size):
                for bad in (nan, inf, -inf, 1e300):                                            # 1e300 is finite, (float)1e300 is not
                    args = [(ctypes.c_double * 9)(*K), (ctypes.c_double * 8)(*D), (ctypes.c_double * 9)(*Kn)]
                    args[which][i] = bad
                    rc = lib.kde_undist_set_calibration(h, *args)
                    if bad == 1e300 and which != 1 and i not in (0, 2, 4, 5):
                        assert rc == native.KDE_OK                                             # an entry of K nothing reads as a float
                    else:
                        refused("kde_undist_set_calibration", rc)
        for which in (0, 2):
            for i in (0, 4):
                for bad in (0.0, -0.0, -500.0, 1e-60):                                         # (float)1e-60 is 0
                    args = [(ctypes.c_double * 9)(*K), D, (ctypes.c_double * 9)(*Kn)]
                    args[which][i] = bad
                    refused("kde_undist_set_calibration", lib.kde_undist_set_calibration(h, *args))
        bad_K = (ctypes.c_double * 9)(*K)
        bad_K[0] = -1.0
        refused("kde_undist_set_calibration", lib.kde_undist_set_calibration(h, bad_K, D, None))   # K_new NULL: K is both cameras
        # a refused calibration leaves an object that had none without one
        h2 = native.UndistHandle()
        assert lib.kde_undist_create(ctypes.byref(h2), 8, 6, 10, 7, 4, None) == native.KDE_OK
        refused("kde_undist_set_calibration", lib.kde_undist_set_calibration(h2, K, (ctypes.c_double * 8)(nan, 0, 0, 0, 0, 0, 0, 0), None))
        refused("kde_undist_depth_batch", lib.kde_undist_depth_batch(h2, 1, 4096, DF, DF, None, None))
        assert b"kde_undist_set_calibration" in lib.kde_last_error_string()
        assert lib.kde_undist_destroy(h2) == native.KDE_OK
        assert lib.kde_undist_set_calibration(h, K, D, Kn) == native.KDE_OK
        assert lib.kde_undist_set_calibration(h, K, D, None) == native.KDE_OK

        refused("kde_undist_depth_batch", depth(2, src=None))                                  # null depth
        refused("kde_undist_depth_batch", depth(5))                                            # n > max_batch
        refused("kde_undist_depth_batch", depth(0))
        refused("kde_undist_depth_batch", depth(-1))
        for fmt in (2, -1):
            refused("kde_undist_depth_batch", depth(2, dfmt=fmt))                              # unknown formats
            refused("kde_undist_depth_batch", depth(2, ofmt=fmt))
        refused("kde_undist_depth_batch", depth(2, src=4098))                                  # float depth not 4-byte aligned
        refused("kde_undist_depth_batch", depth(2, src=4097, dfmt=DU))                         # uint16 depth not 2-byte aligned
        refused("kde_undist_depth_batch", depth(2, out_dev=65538))                             # float output not 4-byte aligned
        refused("kde_undist_depth_batch", depth(2, ofmt=DU, out_dev=65537))                    # uint16 output not 2-byte aligned
        refused("kde_undist_color_batch", color(2, bgr=None))
        refused("kde_undist_color_batch", color(2, out_dev=None))
        refused("kde_undist_color_batch", color(5))
        refused("kde_undist_color_batch", color(0))
        refused("kde_undist_color_batch", color(3, frames=2))                                  # bgr_frames neither 1 nor n
        refused("kde_undist_color_batch", color(3, frames=0))
        # still no call went through
        refused("kde_undist_depth_device", lib.kde_undist_depth_device(h, ctypes.byref(p)))
        refused("kde_undist_filled_host", lib.kde_undist_filled_host(h, None, ctypes.byref(p)))
    finally:
        assert lib.kde_undist_destroy(h) == native.KDE_OK


@pytest.mark.timeout(120)
def test_a_valid_call_on_a_host_without_a_device_is_a_hip_error(native):
    """the object is created without buffers there; everything validates as usual and the launch then answers KDE_ERR_HIP"""
    import torch
    if torch.cuda.is_available():
        return                                                     # tests/test_gpu_undist.py runs the same calls for real
    lib = native.lib()
    h = native.UndistHandle()
    assert lib.kde_undist_create(ctypes.byref(h), 8, 6, 10, 7, 2, None) == native.KDE_OK
    K = (ctypes.c_double * 9)(500, 0, 3.5, 0, 500, 2.5, 0, 0, 1)
    D = (ctypes.c_double * 8)(-0.2, 0.05, 0.001, -0.001, 0.01, 0, 0, 0)
    assert lib.kde_undist_set_calibration(h, K, D, None) == native.KDE_OK
    assert lib.kde_undist_color_batch(h, 2, 8192, 1, 16384, None) == native.KDE_ERR_HIP
    assert lib.kde_undist_depth_batch(h, 2, 4096, 0, 1, None, None) == native.KDE_ERR_HIP
    p = ctypes.c_void_p()
    assert lib.kde_undist_map_device(h, None, ctypes.byref(p)) == native.KDE_ERR_HIP
    assert lib.kde_undist_depth_device(h, ctypes.byref(p)) == native.KDE_ERR_INVALID
    assert lib.kde_undist_destroy(h) == native.KDE_OK


@pytest.mark.timeout(600)
def test_cpp_class_and_demo_compile(tmp_path):
    src = tmp_path / "undist_user.cpp"
    src.write_text(r"""
#include "kde/kde.hpp"
#include <cstdint>
static_assert(sizeof(kde_undist_params) == 16, "kde_undist_params: two floats, an int and a float");
int main()
{
    kde::LensUndistortion one(512, 424, 512, 424);                // one frame, the defaults
    kde_undist_params p = kde::LensUndistortion::defaultParams();
    p.depth_interp = 1;
    p.max_gap = 50.0f;
    kde::LensUndistortion und(512, 424, 640, 480, 8, p);          // RAII over kde_undist_create / _destroy
    const kde::Mat33d K{{365.0, 0, 255.5, 0, 365.0, 211.5, 0, 0, 1}}, Kn{{400.0, 0, 319.5, 0, 400.0, 239.5, 0, 0, 1}};
    const double dist[8] = {-0.27, 0.09, 0.001, -0.0005, -0.02, 0, 0, 0};
    one.setCalibration(K, dist);
    und.setCalibration(K, dist, Kn);
    float* depth = nullptr;
    uint16_t* depth16 = nullptr;
    float* out = nullptr;
    uint16_t* out16 = nullptr;
    uint8_t* bgr = nullptr;
    und.undistortDepth(8, depth, out);
    und.undistortDepth(8, depth16, out);
    und.undistortDepth(8, depth, out16);
    und.undistortDepth(8, depth16, out16);
    und.undistortColor(8, bgr, 1, bgr);
    und.undistortColor(8, bgr, 8, bgr);
    und.setStream(nullptr);
    const void* host = und.depth_Host();
    const uint32_t* filled = und.filled_Host();
    void* dev = und.depth_Device();
    uint32_t* fdev = und.filled_Device();
    const float* map = und.map_Device();
    kde_undist* h = und.handle();
    kde::DepthRegistration reg(640, 480, 1920, 1080, 8);          // the chain of examples/undist_demo.cpp
    reg.registerDepth(8, static_cast<const float*>(dev), out);
    return (host != nullptr) + (int)filled[0] + (fdev != nullptr) + (h != nullptr) + (map != nullptr);
}
""")
    inc = os.path.join(ROOT, "include")
    r = subprocess.run([_hipcc(), "-std=c++17", "-fsyntax-only", "-I", inc, str(src)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    demo = os.path.join(ROOT, "examples", "undist_demo.cpp")
    r = subprocess.run([_hipcc(), "-std=c++17", "-x", "hip", "--offload-arch=gfx950", "-fsyntax-only", demo], capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    assert "undist_demo" in open(os.path.join(ROOT, "examples", "Makefile")).read()
    # the struct is what the compiler says, from C
    size = tmp_path / "size.c"
    size.write_text('#include "kde_hip.h"\n#include <stdio.h>\nint main(void) { printf("%zu\\n", sizeof(kde_undist_params)); return 0; }\n')
    exe = str(tmp_path / "size")
    subprocess.check_call(["cc", "-std=c11", "-I", inc, "-o", exe, str(size)], timeout=120)
    assert subprocess.run([exe], capture_output=True, text=True, check=True, timeout=60).stdout.split() == ["16"]
