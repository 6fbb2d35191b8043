"""DepthRegistration (kde_reg_*, Kinect.cpp:71-75) at the ABI level, without a GPU: declared, exported and bound; the typed
handle; every refusal that precedes a HIP call; the C++ class and the demo compile.

On a host without a device kde_reg_create makes the object without buffers, so the refusals that need a handle (a call before
the calibration, results before a call, ...) are checked here as well."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

HEADER = os.path.join(ROOT, "include", "kde_hip.h")
FUNCS = ("kde_reg_default_params", "kde_reg_create", "kde_reg_destroy", "kde_reg_set_calibration", "kde_reg_register_batch",
         "kde_reg_color_to_depth_batch", "kde_reg_depth_device", "kde_reg_depth_host", "kde_reg_filled_device", "kde_reg_filled_host")
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
    assert set(FUNCS) <= set(native.SIGNATURES)
    assert {n for n in native.SIGNATURES if n.startswith("kde_reg_")} == set(FUNCS)
    assert native.lib().kde_abi_version() == 1
    assert ctypes.sizeof(native.RegParams) == 12
    # none of them is picked up by the enumeration of tools/abi_refusals.py, whose record is frozen
    frozen = (ctypes.c_void_p, ctypes.POINTER(ctypes.c_void_p))
    assert [n for n in FUNCS if native.SIGNATURES[n][1][0] in frozen] == []
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "abi_refusals.py")], capture_output=True, text=True, timeout=100)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "kde_reg" not in r.stdout
    # every entry point cites the reference's lines in the header
    raw = open(HEADER).read()
    for name in FUNCS:
        at = raw.index("int " + name + "(")
        assert "Kinect.cpp:71-75" in raw[raw.rindex("/*", 0, at):at] or "Kinect.cpp:71-75" in raw[at:raw.index("\n", at)], name
    # the header states the rule and what it does not do
    for must in ("not truncated to int", "NO OCCLUSION TEST", "No lens distortion", "ties to even", "half-open"):
        assert must in raw, must
    p = native.RegParams(1.0, 2.0, 3)
    assert native.lib().kde_reg_default_params(ctypes.byref(p)) == native.KDE_OK
    assert (p.z_min, p.z_max, p.max_splat) == (0.0, FLT_MAX, 0)


@pytest.mark.timeout(120)
def test_the_typed_handle_refuses_a_plain_void_pointer(native):
    lib = native.lib()
    assert issubclass(native.RegHandle, ctypes.c_void_p)
    assert lib.kde_reg_destroy(None) == native.KDE_OK
    assert lib.kde_reg_destroy(native.RegHandle()) == native.KDE_OK
    out = ctypes.c_void_p()
    for plain in (ctypes.c_void_p(), ctypes.c_void_p(16)):
        with pytest.raises(ctypes.ArgumentError):
            lib.kde_reg_destroy(plain)
        with pytest.raises(ctypes.ArgumentError):
            lib.kde_reg_set_calibration(plain, None, None, None, None)
        with pytest.raises(ctypes.ArgumentError):
            lib.kde_reg_register_batch(plain, 1, None, 0, 0, None, None)
        with pytest.raises(ctypes.ArgumentError):
            lib.kde_reg_color_to_depth_batch(plain, 1, None, 0, None, 1, None, None)
        for name in ("kde_reg_depth_device", "kde_reg_filled_device"):
            with pytest.raises(ctypes.ArgumentError):
                getattr(lib, name)(plain, ctypes.byref(out))
        for name in ("kde_reg_depth_host", "kde_reg_filled_host"):
            with pytest.raises(ctypes.ArgumentError):
                getattr(lib, name)(plain, None, ctypes.byref(out))
        with pytest.raises(ctypes.ArgumentError):
            lib.kde_reg_create(ctypes.byref(plain), 8, 8, 8, 8, 1, None)
    with pytest.raises(ctypes.ArgumentError):
        lib.kde_reg_destroy(native.CloudHandle())                  # another typed handle is refused as well
    from kinectdepthmapenhancement_amd import filters
    assert filters.DepthRegistration._handle_type is native.RegHandle


@pytest.mark.timeout(120)
def test_refusals_name_their_function(native):
    lib = native.lib()
    INVALID = native.KDE_ERR_INVALID
    Params = native.RegParams
    DF, DU = native.KDE_DEPTH_F32, native.KDE_DEPTH_U16
    nan, inf = float("nan"), float("inf")

    def refused(name, rc):
        assert rc == INVALID, (name, rc, lib.kde_last_error_string())
        assert name.encode() in lib.kde_last_error_string(), (name, lib.kde_last_error_string())

    out = native.RegHandle()
    refused("kde_reg_default_params", lib.kde_reg_default_params(None))
    # create: null out, sizes below 1, bad batch, then every bad parameter block
    refused("kde_reg_create", lib.kde_reg_create(None, 8, 8, 8, 8, 1, None))
    for sizes in ((0, 8, 8, 8), (8, 0, 8, 8), (8, 8, 0, 8), (8, 8, 8, 0), (-1, 8, 8, 8), (8, 8, 8, -3)):
        refused("kde_reg_create", lib.kde_reg_create(ctypes.byref(out), *sizes, 1, None))
    refused("kde_reg_create", lib.kde_reg_create(ctypes.byref(out), 8, 8, 8, 8, 0, None))
    for zmin, zmax in ((nan, 100.0), (inf, inf), (-inf, 100.0), (-1.0, 100.0), (-1e-30, 100.0), (50.0, nan), (100.0, 100.0),
                       (200.0, 100.0), (FLT_MAX, FLT_MAX)):
        refused("kde_reg_create", lib.kde_reg_create(ctypes.byref(out), 8, 8, 8, 8, 1, ctypes.byref(Params(zmin, zmax, 0))))
    for splat in (-1, 17, 1 << 20):
        refused("kde_reg_create", lib.kde_reg_create(ctypes.byref(out), 8, 8, 8, 8, 1, ctypes.byref(Params(0.0, FLT_MAX, splat))))
    assert out.value is None
    # null handles
    Kd = (ctypes.c_double * 9)(500, 0, 3.5, 0, 500, 2.5, 0, 0, 1)
    Kc = (ctypes.c_double * 9)(510, 0, 4.5, 0, 510, 3.5, 0, 0, 1)
    R = (ctypes.c_double * 9)(1, 0, 0, 0, 1, 0, 0, 0, 1)
    t = (ctypes.c_double * 3)(25, 0, 0)
    p = ctypes.c_void_p()
    refused("kde_reg_set_calibration", lib.kde_reg_set_calibration(None, Kd, Kc, R, t))
    refused("kde_reg_register_batch", lib.kde_reg_register_batch(None, 1, 4096, DF, DF, None, None))
    refused("kde_reg_color_to_depth_batch", lib.kde_reg_color_to_depth_batch(None, 1, 4096, DF, 8192, 1, 16384, None))
    refused("kde_reg_depth_device", lib.kde_reg_depth_device(None, ctypes.byref(p)))
    refused("kde_reg_filled_device", lib.kde_reg_filled_device(None, ctypes.byref(p)))
    refused("kde_reg_depth_host", lib.kde_reg_depth_host(None, None, ctypes.byref(p)))
    refused("kde_reg_filled_host", lib.kde_reg_filled_host(None, None, ctypes.byref(p)))
    assert lib.kde_reg_destroy(None) == native.KDE_OK

    # an object for 4 frames (with buffers on a GPU host, without on any other: the checks are the same), non-default parameters
    h = native.RegHandle()
    assert lib.kde_reg_create(ctypes.byref(h), 8, 6, 10, 7, 4, ctypes.byref(Params(100.0, 2000.0, 16))) == native.KDE_OK, \
        lib.kde_last_error_string()
    assert h.value
    try:
        for name in ("kde_reg_depth_device", "kde_reg_filled_device"):
            refused(name, getattr(lib, name)(h, None))
            refused(name, getattr(lib, name)(h, ctypes.byref(p)))                              # getters before the first call
        for name in ("kde_reg_depth_host", "kde_reg_filled_host"):
            refused(name, getattr(lib, name)(h, None, None))
            refused(name, getattr(lib, name)(h, None, ctypes.byref(p)))

        def reg(n, depth=4096, dfmt=DF, ofmt=DF, out_dev=None):
            return lib.kde_reg_register_batch(h, n, depth, dfmt, ofmt, out_dev, None)

        def c2d(n, depth=4096, dfmt=DF, bgr=8192, frames=1, out_dev=16384):
            return lib.kde_reg_color_to_depth_batch(h, n, depth, dfmt, bgr, frames, out_dev, None)

        # a call before the calibration
        refused("kde_reg_register_batch", reg(2))
        assert b"kde_reg_set_calibration" in lib.kde_last_error_string()
        refused("kde_reg_color_to_depth_batch", c2d(2))
        assert b"kde_reg_set_calibration" in lib.kde_last_error_string()
        # the calibration: null pointers, non-finite values, fx or fy not above 0
        for args in ((None, Kc, R, t), (Kd, None, R, t), (Kd, Kc, None, t), (Kd, Kc, R, None)):
            refused("kde_reg_set_calibration", lib.kde_reg_set_calibration(h, *args))
        for which, size in ((0, 9), (1, 9), (2, 9), (3, 3)):
            for i in range(size):
                for bad in (nan, inf, -inf, 1e300):                                            # 1e300 is finite, (float)1e300 is not
                    args = [(ctypes.c_double * 9)(*Kd), (ctypes.c_double * 9)(*Kc), (ctypes.c_double * 9)(*R), (ctypes.c_double * 3)(*t)]
                    args[which][i] = bad
                    rc = lib.kde_reg_set_calibration(h, *args)
                    if bad == 1e300 and which < 2 and i not in (0, 2, 4, 5):
                        assert rc == native.KDE_OK                                             # an entry of K nothing reads as a float
                    else:
                        refused("kde_reg_set_calibration", rc)
        for which in (0, 1):
            for i in (0, 4):
                for bad in (0.0, -0.0, -500.0, 1e-60):                                         # (float)1e-60 is 0
                    args = [(ctypes.c_double * 9)(*Kd), (ctypes.c_double * 9)(*Kc), R, t]
                    args[which][i] = bad
                    refused("kde_reg_set_calibration", lib.kde_reg_set_calibration(h, *args))
        # the refused calibrations (and the accepted odd ones) left the object as it was before its first good one
        h2 = native.RegHandle()
        assert lib.kde_reg_create(ctypes.byref(h2), 8, 6, 10, 7, 4, None) == native.KDE_OK
        refused("kde_reg_set_calibration", lib.kde_reg_set_calibration(h2, Kd, Kc, R, (ctypes.c_double * 3)(nan, 0, 0)))
        refused("kde_reg_register_batch", lib.kde_reg_register_batch(h2, 1, 4096, DF, DF, None, None))
        assert b"kde_reg_set_calibration" in lib.kde_last_error_string()
        assert lib.kde_reg_destroy(h2) == native.KDE_OK
        assert lib.kde_reg_set_calibration(h, Kd, Kc, R, t) == native.KDE_OK

        refused("kde_reg_register_batch", reg(2, depth=None))                                  # null depth
        refused("kde_reg_register_batch", reg(5))                                              # n > max_batch
        refused("kde_reg_register_batch", reg(0))
        refused("kde_reg_register_batch", reg(-1))
        for fmt in (2, -1):
            refused("kde_reg_register_batch", reg(2, dfmt=fmt))                                # unknown formats
            refused("kde_reg_register_batch", reg(2, ofmt=fmt))
        refused("kde_reg_register_batch", reg(2, depth=4098))                                  # float depth not 4-byte aligned
        refused("kde_reg_register_batch", reg(2, depth=4097, dfmt=DU))                         # uint16 depth not 2-byte aligned
        refused("kde_reg_register_batch", reg(2, out_dev=65538))                               # float output not 4-byte aligned
        refused("kde_reg_register_batch", reg(2, ofmt=DU, out_dev=65537))                      # uint16 output not 2-byte aligned
        refused("kde_reg_color_to_depth_batch", c2d(2, depth=None))
        refused("kde_reg_color_to_depth_batch", c2d(2, bgr=None))
        refused("kde_reg_color_to_depth_batch", c2d(2, out_dev=None))
        refused("kde_reg_color_to_depth_batch", c2d(5))
        refused("kde_reg_color_to_depth_batch", c2d(0))
        refused("kde_reg_color_to_depth_batch", c2d(3, frames=2))                              # bgr_frames neither 1 nor n
        refused("kde_reg_color_to_depth_batch", c2d(3, frames=0))
        refused("kde_reg_color_to_depth_batch", c2d(2, dfmt=7))
        refused("kde_reg_color_to_depth_batch", c2d(2, depth=4098))
        refused("kde_reg_color_to_depth_batch", c2d(2, depth=4097, dfmt=DU))
        # still no call went through
        refused("kde_reg_depth_device", lib.kde_reg_depth_device(h, ctypes.byref(p)))
        refused("kde_reg_filled_host", lib.kde_reg_filled_host(h, None, ctypes.byref(p)))
    finally:
        assert lib.kde_reg_destroy(h) == native.KDE_OK


@pytest.mark.timeout(120)
def test_a_valid_call_on_a_host_without_a_device_is_a_hip_error(native):
    """the object is created without buffers there; everything validates as usual and the launch then answers KDE_ERR_HIP"""
    import torch
    if torch.cuda.is_available():
        return                                                     # tests/test_gpu_reg.py runs the same calls for real
    lib = native.lib()
    h = native.RegHandle()
    assert lib.kde_reg_create(ctypes.byref(h), 8, 6, 10, 7, 2, None) == native.KDE_OK
    Kd = (ctypes.c_double * 9)(500, 0, 3.5, 0, 500, 2.5, 0, 0, 1)
    R = (ctypes.c_double * 9)(1, 0, 0, 0, 1, 0, 0, 0, 1)
    assert lib.kde_reg_set_calibration(h, Kd, Kd, R, (ctypes.c_double * 3)(0, 0, 0)) == native.KDE_OK
    assert lib.kde_reg_register_batch(h, 2, 4096, 0, 1, None, None) == native.KDE_ERR_HIP
    assert lib.kde_reg_color_to_depth_batch(h, 2, 4096, 1, 8192, 1, 16384, None) == native.KDE_ERR_HIP
    p = ctypes.c_void_p()
    assert lib.kde_reg_depth_device(h, ctypes.byref(p)) == native.KDE_ERR_INVALID
    assert lib.kde_reg_destroy(h) == native.KDE_OK


@pytest.mark.timeout(600)
def test_cpp_class_and_demo_compile(tmp_path):
    src = tmp_path / "reg_user.cpp"
    src.write_text(r"""
#include "kde/kde.hpp"
#include <cstdint>
static_assert(sizeof(kde_reg_params) == 12, "kde_reg_params: two floats and an int");
int main()
{
    kde::DepthRegistration one(512, 424, 1920, 1080);             // one frame, the defaults
    kde_reg_params p = kde::DepthRegistration::defaultParams();
    p.max_splat = 4;
    kde::DepthRegistration reg(512, 424, 1920, 1080, 8, p);       // RAII over kde_reg_create / _destroy
    const kde::Mat33d Kd{{365.0, 0, 255.5, 0, 365.0, 211.5, 0, 0, 1}}, Kc{{1060.0, 0, 959.5, 0, 1060.0, 539.5, 0, 0, 1}};
    const double R[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1}, t[3] = {52.0, 0, 0};
    reg.setCalibration(Kd, Kc, R, t);
    float* depth = nullptr;
    uint16_t* depth16 = nullptr;
    float* out = nullptr;
    uint16_t* out16 = nullptr;
    uint8_t* bgr = nullptr;
    reg.registerDepth(8, depth, out);
    reg.registerDepth(8, depth16, out);
    reg.registerDepth(8, depth, out16);
    reg.registerDepth(8, depth16, out16);
    reg.colorToDepth(8, depth, bgr, 1, bgr);
    reg.colorToDepth(8, depth16, bgr, 8, bgr);
    reg.setStream(nullptr);
    const void* host = reg.depth_Host();
    const uint32_t* filled = reg.filled_Host();
    void* dev = reg.depth_Device();
    uint32_t* fdev = reg.filled_Device();
    kde_reg* h = reg.handle();
    KinectDepthEnhancement KDE(1920, 1080, 8);
    KDE.ProcessBatch(8, static_cast<const float*>(dev), bgr);     // the composition of examples/reg_demo.cpp
    return (host != nullptr) + (int)filled[0] + (fdev != nullptr) + (h != nullptr);
}
""")
    inc = os.path.join(ROOT, "include")
    r = subprocess.run([_hipcc(), "-std=c++17", "-fsyntax-only", "-I", inc, str(src)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    demo = os.path.join(ROOT, "examples", "reg_demo.cpp")
    r = subprocess.run([_hipcc(), "-std=c++17", "-x", "hip", "--offload-arch=gfx950", "-fsyntax-only", demo], capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    assert "reg_demo" in open(os.path.join(ROOT, "examples", "Makefile")).read()
    # the struct is what the compiler says, from C
    size = tmp_path / "size.c"
    size.write_text('#include "kde_hip.h"\n#include <stdio.h>\nint main(void) { printf("%zu\\n", sizeof(kde_reg_params)); return 0; }\n')
    exe = str(tmp_path / "size")
    subprocess.check_call(["cc", "-std=c11", "-I", inc, "-o", exe, str(size)], timeout=120)
    assert subprocess.run([exe], capture_output=True, text=True, check=True, timeout=60).stdout.split() == ["12"]
