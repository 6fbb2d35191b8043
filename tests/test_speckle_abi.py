"""DepthSpeckleFilter (kde_speckle_*) at the ABI level, without a GPU: declared, exported and bound; the typed handle; the
defaults; every refusal that precedes a HIP call and its message; the in-place rule; getters before the first call; a
device-less create; the Python class, the C++ class and the demo.

On a host without a device kde_speckle_create makes the object without buffers, so the refusals that need a handle are checked
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
COUNTS = ("removed", "components", "capped")
DEVICE_GETTERS = ("kde_speckle_depth_device",) + tuple(f"kde_speckle_{c}_device" for c in COUNTS)
HOST_GETTERS = ("kde_speckle_depth_host",) + tuple(f"kde_speckle_{c}_host" for c in COUNTS)
FUNCS = ("kde_speckle_default_params", "kde_speckle_create", "kde_speckle_destroy", "kde_speckle_filter_batch") + DEVICE_GETTERS + HOST_GETTERS
FLT_MAX = float(np.finfo(np.float32).max)
DEFAULTS = (64, 10.0, float(np.float32(0.02)), 4, 0.0, FLT_MAX)


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
    assert {n for n in native.SIGNATURES if n.startswith("kde_speckle_")} == set(FUNCS)
    assert native.lib().kde_abi_version() == 1
    assert ctypes.sizeof(native.SpeckleParams) == 24
    assert [n for n, _ in native.SpeckleParams._fields_] == ["min_size", "max_diff", "rel_diff", "connectivity", "z_min", "z_max"]
    # none of them is picked up by the enumeration of tools/abi_refusals.py, whose record is frozen
    frozen = (ctypes.c_void_p, ctypes.POINTER(ctypes.c_void_p))
    assert [n for n in FUNCS if native.SIGNATURES[n][1][0] in frozen] == []
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "abi_refusals.py")], capture_output=True, text=True, timeout=100)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "kde_speckle" not in r.stdout
    # the header states the rule, the order-freedom and the launches
    raw = re.sub(r"\s*\n \*\s*", " ", open(HEADER).read())                  # comment lines joined
    for must in ("z = (d > z_min && d < z_max) ? (float)d : 0", "fabsf(za - zb) <= max_diff + rel_diff * fminf(za, zb)",
                 "the product and the sum rounded separately", "the smallest raster index", "before the uint16 rounding",
                 "anything else is a defect of the library and the frame is not to be trusted", "min_size 1 removes nothing",
                 "the order in which atomics land", "In place is allowed exactly when out_dev == depth_dev", "No workgroup waits",
                 "capturable from the first call"):
        assert must in raw, must
    p = native.SpeckleParams(9, 1.0, 2.0, 3, 4.0, 5.0)
    assert native.lib().kde_speckle_default_params(ctypes.byref(p)) == native.KDE_OK
    assert _fields(p) == DEFAULTS


@pytest.mark.timeout(120)
def test_the_typed_handle_refuses_a_plain_void_pointer(native):
    lib = native.lib()
    assert issubclass(native.SpeckleHandle, ctypes.c_void_p)
    assert lib.kde_speckle_destroy(None) == native.KDE_OK
    assert lib.kde_speckle_destroy(native.SpeckleHandle()) == native.KDE_OK
    out = ctypes.c_void_p()
    for plain in (ctypes.c_void_p(), ctypes.c_void_p(16)):
        with pytest.raises(ctypes.ArgumentError):
            lib.kde_speckle_destroy(plain)
        with pytest.raises(ctypes.ArgumentError):
            lib.kde_speckle_filter_batch(plain, 1, None, 0, 0, None, None, None)
        for name in DEVICE_GETTERS:
            with pytest.raises(ctypes.ArgumentError):
                getattr(lib, name)(plain, ctypes.byref(out))
        for name in HOST_GETTERS:
            with pytest.raises(ctypes.ArgumentError):
                getattr(lib, name)(plain, None, ctypes.byref(out))
        with pytest.raises(ctypes.ArgumentError):
            lib.kde_speckle_create(ctypes.byref(plain), 8, 8, 1, None)
    for other in (native.CloudHandle(), native.RegHandle(), native.UndistHandle(), native.UpsampleHandle(), native.HolefillHandle()):
        with pytest.raises(ctypes.ArgumentError):
            lib.kde_speckle_destroy(other)
    from kinectdepthmapenhancement_amd import filters
    assert filters.DepthSpeckleFilter._handle_type is native.SpeckleHandle
    assert _fields(filters.DepthSpeckleFilter.default_params()) == DEFAULTS


@pytest.mark.timeout(120)
def test_refusals_name_their_function(native):
    lib = native.lib()
    INVALID = native.KDE_ERR_INVALID
    Params = native.SpeckleParams
    DF, DU = native.KDE_DEPTH_F32, native.KDE_DEPTH_U16
    nan, inf = float("nan"), float("inf")

    def refused(name, rc, *words):
        assert rc == INVALID, (name, rc, lib.kde_last_error_string())
        assert name.encode() in lib.kde_last_error_string(), (name, lib.kde_last_error_string())
        for word in words:
            assert word.encode() in lib.kde_last_error_string(), (word, lib.kde_last_error_string())

    def create(out, size=(8, 6), batch=1, params=None):
        return lib.kde_speckle_create(out if out is None else ctypes.byref(out), *size, batch, None if params is None else ctypes.byref(params))

    def with_(**kw):
        p = Params(*DEFAULTS)
        for k, v in kw.items():
            setattr(p, k, v)
        return p

    out = native.SpeckleHandle()
    refused("kde_speckle_default_params", lib.kde_speckle_default_params(None))
    refused("kde_speckle_create", create(None))
    for size in ((0, 6), (8, 0), (-1, 6), (8, -3), (1 << 16, 1 << 15), (1 << 30, 2)):
        refused("kde_speckle_create", create(out, size), "bad size")
    for size in (((1 << 24) + 1, 1), (1, (1 << 24) + 1)):
        refused("kde_speckle_create", create(out, size), "a side above")
    for batch in (0, -1, 65536):
        refused("kde_speckle_create", create(out, batch=batch), "max_batch")
    bad = dict(min_size=(0, -1, (1 << 24) + 1), max_diff=(-1.0, -1e-30, nan, inf, -inf), rel_diff=(-1.0, -1e-30, nan, inf, -inf),
               connectivity=(0, 6, -4, 5), z_min=(nan, inf, -inf, -1.0, -1e-30))
    for field, values in bad.items():
        for v in values:
            refused("kde_speckle_create", create(out, params=with_(**{field: v})), field)
    for zmin, zmax in ((100.0, 100.0), (200.0, 100.0), (FLT_MAX, FLT_MAX), (inf, inf), (0.0, nan), (0.0, 0.0), (0.0, -1.0)):
        refused("kde_speckle_create", create(out, params=with_(z_min=zmin, z_max=zmax)))
    assert out.value is None
    for params in (with_(min_size=1, max_diff=0.0, rel_diff=0.0, connectivity=8, z_max=inf),
                   with_(min_size=1 << 24, max_diff=1e30, rel_diff=1e30, z_min=5.0, z_max=6.0), with_(max_diff=-0.0, rel_diff=-0.0)):   # the limits are inside
        for size in ((8, 6), (1, 1), (1 << 24, 1)):
            assert create(out, size, params=params) == native.KDE_OK, lib.kde_last_error_string()
            assert lib.kde_speckle_destroy(out) == native.KDE_OK
            out = native.SpeckleHandle()
    # null handles
    p = ctypes.c_void_p()
    refused("kde_speckle_filter_batch", lib.kde_speckle_filter_batch(None, 1, 4096, DF, DF, None, None, None))
    for name in DEVICE_GETTERS:
        refused(name, getattr(lib, name)(None, ctypes.byref(p)))
    for name in HOST_GETTERS:
        refused(name, getattr(lib, name)(None, None, ctypes.byref(p)))
    assert lib.kde_speckle_destroy(None) == native.KDE_OK

    h = native.SpeckleHandle()
    assert create(h, (20, 13), 4, Params(5, 3.0, 0.5, 8, 100.0, 5000.0)) == native.KDE_OK, lib.kde_last_error_string()
    assert h.value
    try:
        for name in DEVICE_GETTERS:
            refused(name, getattr(lib, name)(h, None))
            refused(name, getattr(lib, name)(h, ctypes.byref(p)), "kde_speckle_filter_batch was not called")      # getters before the first call
        for name in HOST_GETTERS:
            refused(name, getattr(lib, name)(h, None, None))
            refused(name, getattr(lib, name)(h, None, ctypes.byref(p)), "kde_speckle_filter_batch was not called")

        def call(n, src=4096, dfmt=DF, ofmt=DF, out_dev=1 << 20, labels=None):
            return lib.kde_speckle_filter_batch(h, n, src, dfmt, ofmt, out_dev, labels, None)

        who = "kde_speckle_filter_batch"
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
        for labels in (8193, 8194, 8195):
            refused(who, call(2, labels=labels), "labels_dev is not 4-byte aligned")
        frame = 20 * 13
        for out_dev in (4096 + 4 * frame, 4096 - 4 * (2 * frame - 1), 4096 + 4 * (2 * frame - 1), 4100):        # partial overlaps
            refused(who, call(2, out_dev=out_dev), "out_dev overlaps depth_dev (in place is supported only with out_dev == depth_dev and "
                    "out_format == depth_format)")
        refused(who, call(2, ofmt=DU, out_dev=4096), "in place")            # the same pointer in another format
        refused(who, call(2, dfmt=DU, ofmt=DF, out_dev=4096), "in place")
        refused(who, call(2, labels=4096), "labels_dev overlaps depth_dev")
        refused(who, call(2, labels=4096 + 8 * frame - 4), "labels_dev overlaps depth_dev")
        refused(who, call(2, labels=(1 << 20) + 4 * frame), "labels_dev overlaps out_dev")
        refused(who, call(2, src=1 << 20, labels=1 << 20), "labels_dev overlaps")
        # still no call went through
        refused("kde_speckle_depth_device", lib.kde_speckle_depth_device(h, ctypes.byref(p)))
        refused("kde_speckle_capped_host", lib.kde_speckle_capped_host(h, None, ctypes.byref(p)))
    finally:
        assert lib.kde_speckle_destroy(h) == native.KDE_OK


@pytest.mark.timeout(120)
def test_a_valid_call_on_a_host_without_a_device_is_a_hip_error(native):
    """the object is created without buffers there; everything validates as usual and the launch then answers KDE_ERR_HIP.  In
    place -- out_dev == depth_dev in depth's format -- is such a valid call."""
    import torch
    if torch.cuda.is_available():
        pytest.skip("this host has a device: tests/test_gpu_speckle.py makes the same calls for real")
    lib = native.lib()
    h = native.SpeckleHandle()
    assert lib.kde_speckle_create(ctypes.byref(h), 20, 13, 2, None) == native.KDE_OK
    px = 2 * 20 * 13
    assert lib.kde_speckle_filter_batch(h, 2, 4096, 0, 1, None, None, None) == native.KDE_ERR_HIP
    assert lib.kde_speckle_filter_batch(h, 2, 4096, 0, 0, 4096, None, None) == native.KDE_ERR_HIP             # in place, float
    assert lib.kde_speckle_filter_batch(h, 2, 4098, 1, 1, 4098, 1 << 20, None) == native.KDE_ERR_HIP          # in place, uint16, labels
    assert lib.kde_speckle_filter_batch(h, 2, 4096, 0, 0, 4096 + px * 4, 4096 + 2 * px * 4, None) == native.KDE_ERR_HIP   # the frames just do not overlap
    assert b"kde_speckle_filter_batch" in lib.kde_last_error_string() and b"without a device" in lib.kde_last_error_string()
    p = ctypes.c_void_p()
    assert lib.kde_speckle_depth_device(h, ctypes.byref(p)) == native.KDE_ERR_INVALID
    assert lib.kde_speckle_destroy(h) == native.KDE_OK
    from kinectdepthmapenhancement_amd import filters
    S = filters.DepthSpeckleFilter((20, 13), 2)
    with pytest.raises(native.KdeError, match="was not called"):
        S.removed_device()
    with pytest.raises(AttributeError):
        S.filled()
    with pytest.raises(TypeError):
        S.filter(torch.zeros((2, 13, 20)))                             # a host tensor
    S.close()


@pytest.mark.timeout(600)
def test_cpp_class_and_demo_compile(tmp_path):
    src = tmp_path / "speckle_user.cpp"
    src.write_text(r"""
#include "kde/kde.hpp"
#include <cstdint>
static_assert(sizeof(kde_speckle_params) == 24, "kde_speckle_params: six four-byte fields");
int main()
{
    kde::DepthSpeckleFilter one(1920, 1080);                          // one frame, the defaults
    kde_speckle_params p = kde::DepthSpeckleFilter::defaultParams();
    p.min_size = 32;
    p.connectivity = 8;
    kde::DepthSpeckleFilter speckle(640, 480, 8, p);                  // RAII over kde_speckle_create / _destroy
    float* depth = nullptr;
    uint16_t* depth16 = nullptr;
    float* out = nullptr;
    uint16_t* out16 = nullptr;
    int32_t* labels = nullptr;
    speckle.filter(8, depth, out);
    speckle.filter(8, depth16, out, labels);
    speckle.filter(8, depth, out16);
    speckle.filter(8, depth16, depth16, labels);                      // in place
    speckle.setStream(nullptr);
    const void* host = speckle.depth_Host();
    const uint32_t* removed = speckle.removed_Host();
    const uint32_t* components = speckle.components_Host();
    const uint32_t* capped = speckle.capped_Host();
    void* dev = speckle.depth_Device();
    uint32_t* rdev = speckle.removed_Device();
    uint32_t* cdev = speckle.components_Device();
    uint32_t* kdev = speckle.capped_Device();
    kde_speckle* h = speckle.handle();
    uint8_t* bgr = nullptr;
    kde::DepthHoleFilling fill(640, 480, 8);                           // the chain of examples/speckle_demo.cpp
    fill.fill(8, static_cast<const float*>(dev), bgr, 8, out);
    return (host != nullptr) + (int)removed[0] + (int)components[0] + (int)capped[0] + (rdev != nullptr) + (cdev != nullptr) + (kdev != nullptr) +
           (h != nullptr);
}
""")
    inc = os.path.join(ROOT, "include")
    r = subprocess.run([_hipcc(), "-std=c++17", "-fsyntax-only", "-I", inc, str(src)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    hidden = tmp_path / "hidden.cpp"                                   # this stage fills nothing
    hidden.write_text('#include "kde/kde.hpp"\nint main() { kde::DepthSpeckleFilter s(8, 8); return s.filled_Host() != nullptr; }\n')
    r = subprocess.run([_hipcc(), "-std=c++17", "-fsyntax-only", "-I", inc, str(hidden)], capture_output=True, text=True, timeout=300)
    assert r.returncode != 0 and "private" in r.stderr
    demo = os.path.join(ROOT, "examples", "speckle_demo.cpp")
    r = subprocess.run([_hipcc(), "-std=c++17", "-x", "hip", "--offload-arch=gfx950", "-fsyntax-only", demo], capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    assert "speckle_demo" in open(os.path.join(ROOT, "examples", "Makefile")).read()
    size = tmp_path / "size.c"
    size.write_text('#include "kde_hip.h"\n#include <stdio.h>\nint main(void) { printf("%zu\\n", sizeof(kde_speckle_params)); return 0; }\n')
    exe = str(tmp_path / "size")
    subprocess.check_call(["cc", "-std=c11", "-I", inc, "-o", exe, str(size)], timeout=120)
    assert subprocess.run([exe], capture_output=True, text=True, check=True, timeout=60).stdout.split() == ["24"]


def test_the_union_header_is_what_the_kernels_include():
    csrc = os.path.join(ROOT, "kinectdepthmapenhancement_amd", "csrc")
    kernels = open(os.path.join(csrc, "speckle_kernels.hip")).read()
    assert '#include "kde_union.h"' in kernels and "uf_union(" in kernels and "uf_find(" in kernels
    for banned in ("cooperative", "hipLaunchCooperativeKernel", "grid.sync", "hipMemsetAsync"):
        assert banned not in kernels.replace("no cooperative launch", ""), banned
    assert "kUnionCap" in open(os.path.join(csrc, "kde_union.h")).read()
