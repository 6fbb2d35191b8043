"""DepthDecimation (kde_decimate_*) at the ABI level, without a GPU: declared, exported and bound; the typed handle; the defaults;
every refusal that precedes a HIP call and its message; the in-place rule; getters before the first call; a device-less create;
the output size and the intrinsics, which need no device; the Python class, the C++ class and the demo.

On a host without a device kde_decimate_create makes the object without buffers, so the refusals that need a handle are checked
here as well."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import decimate_cases as DC
from conftest import ROOT

HEADER = os.path.join(ROOT, "include", "kde_hip.h")
COUNTS = ("filled", "mixed")
DEVICE_GETTERS = ("kde_decimate_depth_device",) + tuple(f"kde_decimate_{c}_device" for c in COUNTS)
HOST_GETTERS = ("kde_decimate_depth_host",) + tuple(f"kde_decimate_{c}_host" for c in COUNTS)
FUNCS = ("kde_decimate_default_params", "kde_decimate_create", "kde_decimate_destroy", "kde_decimate_out_size", "kde_decimate_depth_batch",
         "kde_decimate_color_batch", "kde_decimate_intrinsics") + DEVICE_GETTERS + HOST_GETTERS
FLT_MAX = float(np.finfo(np.float32).max)
DEFAULTS = (2, 0, 1, 0.0, 0.0, FLT_MAX)
FIELDS = ["factor", "mode", "min_valid", "max_gap", "z_min", "z_max"]


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
    assert re.search(r"enum\s*\{\s*KDE_DECIMATE_MEDIAN\s*=\s*0\s*,\s*KDE_DECIMATE_MEAN\s*=\s*1\s*\}", text)
    lib = ctypes.CDLL(native.LIB_PATH)
    assert all(hasattr(lib, n) for n in FUNCS)
    assert {n for n in native.SIGNATURES if n.startswith("kde_decimate_")} == set(FUNCS)
    assert native.lib().kde_abi_version() == 1
    assert ctypes.sizeof(native.DecimateParams) == 24
    assert [n for n, _ in native.DecimateParams._fields_] == FIELDS
    assert (native.KDE_DECIMATE_MEDIAN, native.KDE_DECIMATE_MEAN) == (0, 1)
    # none of them is picked up by the enumeration of tools/abi_refusals.py, whose record is frozen
    frozen = (ctypes.c_void_p, ctypes.POINTER(ctypes.c_void_p))
    assert [n for n in FUNCS if native.SIGNATURES[n][1][0] in frozen] == []
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "abi_refusals.py")], capture_output=True, text=True, timeout=100)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "kde_decimate" not in r.stdout
    p = native.DecimateParams(9, 9, 9, 1.0, 5.0, 6.0)
    assert native.lib().kde_decimate_default_params(ctypes.byref(p)) == native.KDE_OK
    assert _fields(p) == DEFAULTS


def test_the_header_states_the_rule():
    raw = re.sub(r"\s*\n \*\s*", " ", open(HEADER).read())                  # comment lines joined
    for must in ("No reference counterpart",
                 "k = factor, an integer in 2..8",
                 "out_w = ceil(src_w / k) by out_h = ceil(src_h / k)",
                 "qy = j * k .. min(j * k + k, src_h) - 1 (outer loop), qx = i * k .. min(i * k + k, src_w) - 1 (inner loop)",
                 "this loop order is the tap order",
                 "they use only the samples that exist, and nothing is scaled for them",
                 "Every operation is one IEEE binary32 operation in the order written, the division correctly rounded",
                 "nothing transcendental is evaluated",
                 "A sample is valid iff z > z_min && z < z_max (NaN and +-inf fail)",
                 "If m < min_valid the pixel is 0",
                 "A partial block with fewer existing samples than min_valid is therefore a hole",
                 "sorted ascending to v[0 .. m - 1], v[(m - 1) / 2]",
                 "It is always one of the samples",
                 "It never lies between two surfaces; uint16 in to uint16 out is exact",
                 "for each valid sample in tap order with max_gap == 0 || fabsf(z - zmed) <= max_gap: num = num + z, cnt = cnt + 1",
                 "The pixel is num / (float)cnt; cnt >= 1 because zmed passes its own test",
                 "depth_to_u16 of it as kde_points_to_depth rounds",
                 "counted before the uint16 rounding",
                 "with m >= 1 whose largest valid sample minus smallest valid sample exceeds max_gap",
                 "It is 0 for every frame when max_gap == 0",
                 "(2 * s + c) / (2 * c) in integer division, the area mean rounded half up",
                 "It is exact; it does not claim to equal OpenCV's INTER_AREA, which rounds half to even",
                 "fx' = fx / k, fy' = fy / k, cx' = (cx + 0.5) / k - 0.5, cy' likewise",
                 "which holds exactly only when both sides are multiples of k",
                 "does not depend on n, a frame's position in the batch or pointer alignment",
                 "In place is refused",
                 "no memset node and nothing to reset; no allocation, no host synchronisation: capturable from the first call",
                 "works without a device"):
        assert must in raw, must


@pytest.mark.timeout(120)
def test_the_typed_handle_refuses_a_plain_void_pointer(native):
    lib = native.lib()
    assert issubclass(native.DecimateHandle, ctypes.c_void_p)
    assert lib.kde_decimate_destroy(None) == native.KDE_OK
    assert lib.kde_decimate_destroy(native.DecimateHandle()) == native.KDE_OK
    out = ctypes.c_void_p()
    a, b = ctypes.c_int(), ctypes.c_int()
    for plain in (ctypes.c_void_p(), ctypes.c_void_p(16)):
        with pytest.raises(ctypes.ArgumentError):
            lib.kde_decimate_destroy(plain)
        with pytest.raises(ctypes.ArgumentError):
            lib.kde_decimate_depth_batch(plain, 1, None, 0, 0, None, None)
        with pytest.raises(ctypes.ArgumentError):
            lib.kde_decimate_color_batch(plain, 1, None, None, None)
        with pytest.raises(ctypes.ArgumentError):
            lib.kde_decimate_out_size(plain, ctypes.byref(a), ctypes.byref(b))
        with pytest.raises(ctypes.ArgumentError):
            lib.kde_decimate_intrinsics(plain, None, None)
        for name in DEVICE_GETTERS:
            with pytest.raises(ctypes.ArgumentError):
                getattr(lib, name)(plain, ctypes.byref(out))
        for name in HOST_GETTERS:
            with pytest.raises(ctypes.ArgumentError):
                getattr(lib, name)(plain, None, ctypes.byref(out))
        with pytest.raises(ctypes.ArgumentError):
            lib.kde_decimate_create(ctypes.byref(plain), 8, 8, 1, None)
    for other in (native.CloudHandle(), native.RegHandle(), native.UndistHandle(), native.UpsampleHandle(), native.HolefillHandle(),
                  native.SpeckleHandle(), native.TemporalHandle()):
        with pytest.raises(ctypes.ArgumentError):
            lib.kde_decimate_destroy(other)
    from kinectdepthmapenhancement_amd import filters
    assert filters.DepthDecimation._handle_type is native.DecimateHandle
    assert _fields(filters.DepthDecimation.default_params()) == DEFAULTS


@pytest.mark.timeout(120)
def test_refusals_name_their_function(native):
    lib = native.lib()
    INVALID = native.KDE_ERR_INVALID
    Params = native.DecimateParams
    DF, DU = native.KDE_DEPTH_F32, native.KDE_DEPTH_U16
    nan, inf = float("nan"), float("inf")

    def refused(name, rc, *words):
        assert rc == INVALID, (name, rc, lib.kde_last_error_string())
        assert name.encode() in lib.kde_last_error_string(), (name, lib.kde_last_error_string())
        for word in words:
            assert word.encode() in lib.kde_last_error_string(), (word, lib.kde_last_error_string())

    def create(out, size=(8, 6), batch=1, params=None):
        return lib.kde_decimate_create(out if out is None else ctypes.byref(out), *size, batch, None if params is None else ctypes.byref(params))

    def with_(**kw):
        p = Params(*DEFAULTS)
        for k, v in kw.items():
            setattr(p, k, v)
        return p

    out = native.DecimateHandle()
    refused("kde_decimate_default_params", lib.kde_decimate_default_params(None))
    refused("kde_decimate_create", create(None))
    for size in ((0, 6), (8, 0), (-1, 6), (8, -3), (1 << 16, 1 << 15), (1 << 30, 2)):
        refused("kde_decimate_create", create(out, size), "bad size")
    refused("kde_decimate_create", create(out, ((1 << 24) + 1, 1)), "a side above 16777216")
    refused("kde_decimate_create", create(out, (1, (1 << 24) + 1)), "a side above 16777216")
    for batch in (0, -1, 65536):
        refused("kde_decimate_create", create(out, batch=batch), "max_batch")
    for factor in (1, 0, -2, 9, 64):
        refused("kde_decimate_create", create(out, params=with_(factor=factor)), f"factor={factor} outside 2..8")
    for mode in (2, -1, 100):
        refused("kde_decimate_create", create(out, params=with_(mode=mode)), f"mode={mode} is neither KDE_DECIMATE_MEDIAN (0) nor KDE_DECIMATE_MEAN (1)")
    for factor, mv in ((2, 0), (2, 5), (2, -1), (3, 10), (8, 65)):
        refused("kde_decimate_create", create(out, params=with_(factor=factor, min_valid=mv)), f"min_valid={mv} outside 1..factor^2={factor * factor}")
    for v in (-1.0, -1e-30, nan, inf, -inf):
        refused("kde_decimate_create", create(out, params=with_(max_gap=v)), "max_gap", "must be finite and >= 0 (0: no guard)")
    for v in (nan, inf, -inf, -1.0, -1e-30):
        refused("kde_decimate_create", create(out, params=with_(z_min=v)), "z_min", "must be finite and >= 0")
    for zmin, zmax in ((100.0, 100.0), (200.0, 100.0), (FLT_MAX, FLT_MAX), (0.0, nan), (0.0, 0.0), (0.0, -1.0)):
        refused("kde_decimate_create", create(out, params=with_(z_min=zmin, z_max=zmax)), "must be below z_max")
    assert out.value is None
    for params in (with_(factor=2, min_valid=4, z_max=inf), with_(factor=8, mode=1, min_valid=64, max_gap=1e30, z_min=5.0, z_max=6.0),
                   with_(factor=3, min_valid=9, max_gap=-0.0)):             # the limits are inside
        for size in ((8, 6), (1, 1), (1 << 24, 1)):
            assert create(out, size, params=params) == native.KDE_OK, lib.kde_last_error_string()
            assert lib.kde_decimate_destroy(out) == native.KDE_OK
            out = native.DecimateHandle()
    # null handles
    p = ctypes.c_void_p()
    a, b = ctypes.c_int(), ctypes.c_int()
    K = (ctypes.c_double * 9)()
    refused("kde_decimate_depth_batch", lib.kde_decimate_depth_batch(None, 1, 4096, DF, DF, None, None))
    refused("kde_decimate_color_batch", lib.kde_decimate_color_batch(None, 1, 4096, 1 << 20, None))
    refused("kde_decimate_out_size", lib.kde_decimate_out_size(None, ctypes.byref(a), ctypes.byref(b)))
    refused("kde_decimate_intrinsics", lib.kde_decimate_intrinsics(None, K, K))
    for name in DEVICE_GETTERS:
        refused(name, getattr(lib, name)(None, ctypes.byref(p)))
    for name in HOST_GETTERS:
        refused(name, getattr(lib, name)(None, None, ctypes.byref(p)))
    assert lib.kde_decimate_destroy(None) == native.KDE_OK

    h = native.DecimateHandle()
    assert create(h, (20, 13), 4, Params(3, 1, 2, 50.0, 100.0, 5000.0)) == native.KDE_OK, lib.kde_last_error_string()
    assert h.value
    try:
        for name in DEVICE_GETTERS:
            refused(name, getattr(lib, name)(h, None))
            refused(name, getattr(lib, name)(h, ctypes.byref(p)), "kde_decimate_depth_batch was not called")      # getters before the first call
        for name in HOST_GETTERS:
            refused(name, getattr(lib, name)(h, None, None))
            refused(name, getattr(lib, name)(h, None, ctypes.byref(p)), "kde_decimate_depth_batch was not called")
        refused("kde_decimate_out_size", lib.kde_decimate_out_size(h, None, ctypes.byref(b)))
        refused("kde_decimate_out_size", lib.kde_decimate_out_size(h, ctypes.byref(a), None))
        refused("kde_decimate_intrinsics", lib.kde_decimate_intrinsics(h, None, K))
        refused("kde_decimate_intrinsics", lib.kde_decimate_intrinsics(h, K, None))

        def call(n, src=4096, dfmt=DF, ofmt=DF, out_dev=1 << 20):
            return lib.kde_decimate_depth_batch(h, n, src, dfmt, ofmt, out_dev, None)

        who = "kde_decimate_depth_batch"
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
        frame, small = 20 * 13, 7 * 5                                       # the source and the output frame
        for out_dev in (4096, 4096 + 4 * frame, 4096 - 4 * (2 * small - 1), 4096 + 4 * (2 * frame - 1), 4100):     # every kind of overlap
            refused(who, call(2, out_dev=out_dev), "out_dev overlaps depth_dev (in place is not supported)")
        refused(who, call(2, ofmt=DU, out_dev=4096), "in place")
        refused(who, call(2, dfmt=DU, out_dev=4096 + 2 * (2 * frame) - 4), "in place")      # the last two uint16 samples
        # the colour call
        who = "kde_decimate_color_batch"
        refused(who, lib.kde_decimate_color_batch(h, 2, None, 1 << 20, None), "null argument")
        refused(who, lib.kde_decimate_color_batch(h, 2, 4096, None, None), "null argument")
        for n in (5, 0, -1):
            refused(who, lib.kde_decimate_color_batch(h, n, 4096, 1 << 20, None), "outside 1..max_batch=4")
        for out_dev in (4097, 4097 + 3 * 2 * frame - 1, 4097 - 3 * 2 * small + 1, 5000):
            refused(who, lib.kde_decimate_color_batch(h, 2, 4097, out_dev, None), "out_bgr_dev overlaps bgr_dev (in place is not supported)")
        # still no call went through
        refused("kde_decimate_depth_device", lib.kde_decimate_depth_device(h, ctypes.byref(p)))
        refused("kde_decimate_mixed_host", lib.kde_decimate_mixed_host(h, None, ctypes.byref(p)))
    finally:
        assert lib.kde_decimate_destroy(h) == native.KDE_OK


@pytest.mark.timeout(120)
def test_out_size_and_intrinsics_need_no_device(native):
    """host arithmetic only; the handle is created in a child process that sees no device, so that it is device-less on any host"""
    code = r"""
import ctypes as C, json, sys
sys.path.insert(0, %r)
from kinectdepthmapenhancement_amd import _native as N
lib = N.lib()
res = {"sizes": [], "K": [], "hip": []}
for (w, h), k in (((1, 1), 2), ((1, 1), 8), ((8, 8), 3), ((101, 37), 5), ((1920, 1080), 4), ((1920, 1080), 7), ((16, 9), 8)):
    p = N.DecimateParams(k, 0, 1, 0.0, 0.0, 1e30)
    H = N.DecimateHandle()
    assert lib.kde_decimate_create(C.byref(H), w, h, 2, C.byref(p)) == N.KDE_OK, lib.kde_last_error_string()
    a, b = C.c_int(), C.c_int()
    assert lib.kde_decimate_out_size(H, C.byref(a), C.byref(b)) == N.KDE_OK
    res["sizes"].append([a.value, b.value])
    Kin = (C.c_double * 9)(525.0, 0.25, 319.5, 0.125, 530.0, 239.5, 0.0, 0.0, 1.0)
    Kout = (C.c_double * 9)()
    assert lib.kde_decimate_intrinsics(H, Kin, Kout) == N.KDE_OK
    assert lib.kde_decimate_intrinsics(H, Kin, Kin) == N.KDE_OK          # in place
    assert list(Kin) == list(Kout)
    res["K"].append(list(Kout))
    # a valid call on a host without a device: everything validates and the launch answers KDE_ERR_HIP
    px = 2 * w * h
    res["hip"].append([lib.kde_decimate_depth_batch(H, 2, 4096, 0, 1, None, None), lib.kde_decimate_depth_batch(H, 2, 4096, 1, 0, 4096 + 2 * px, None),
                       lib.kde_decimate_depth_batch(H, 1, 4098, 1, 1, 1 << 40, None), lib.kde_decimate_color_batch(H, 2, 4097, 4097 + 3 * px, None),
                       lib.kde_last_error_string().decode()])
    q = C.c_void_p()
    assert lib.kde_decimate_depth_device(H, C.byref(q)) == N.KDE_ERR_INVALID
    assert lib.kde_decimate_destroy(H) == N.KDE_OK
print(json.dumps(res))
""" % ROOT
    env = dict(os.environ, HIP_VISIBLE_DEVICES="", ROCR_VISIBLE_DEVICES="")
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=100, env=env)
    assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
    import json
    res = json.loads(r.stdout.strip().splitlines()[-1])
    cases = (((1, 1), 2), ((1, 1), 8), ((8, 8), 3), ((101, 37), 5), ((1920, 1080), 4), ((1920, 1080), 7), ((16, 9), 8))
    assert [tuple(s) for s in res["sizes"]] == [DC.out_size(size, k) for size, k in cases]
    assert res["sizes"][4] == [480, 270] and res["sizes"][5] == [275, 155] and res["sizes"][0] == [1, 1]
    K = [525.0, 0.25, 319.5, 0.125, 530.0, 239.5, 0.0, 0.0, 1.0]
    for got, (_, k) in zip(res["K"], cases):
        assert got == DC.intrinsics(K, k).reshape(-1).tolist()
    for a, b, c, d, msg in res["hip"]:
        assert (a, b, c, d) == (native.KDE_ERR_HIP,) * 4, (a, b, c, d, msg)
        assert "kde_decimate_color_batch" in msg and "without a device" in msg
    from kinectdepthmapenhancement_amd import filters
    D = filters.DepthDecimation((101, 37), 2, native.DecimateParams(5, 1, 3, 50.0, 0.0, 1e30))
    assert D.out_size == (21, 8)
    assert np.array_equal(D.intrinsics(np.array(K).reshape(3, 3)), DC.intrinsics(K, 5))
    with pytest.raises(native.KdeError, match="was not called"):
        D.mixed_device()
    import torch
    with pytest.raises(TypeError):
        D.decimate(torch.zeros((2, 37, 101)))                          # a host tensor
    D.close()


@pytest.mark.timeout(600)
def test_cpp_class_and_demo_compile(tmp_path):
    src = tmp_path / "decimate_user.cpp"
    src.write_text(r"""
#include "kde/kde.hpp"
#include <cstdint>
static_assert(sizeof(kde_decimate_params) == 24, "kde_decimate_params: six four-byte fields");
static_assert(KDE_DECIMATE_MEDIAN == 0 && KDE_DECIMATE_MEAN == 1, "the modes");
int main()
{
    kde::DepthDecimation one(1920, 1080);                             // one frame per call, the defaults
    kde_decimate_params p = kde::DepthDecimation::defaultParams();
    p.factor = 4;
    p.mode = KDE_DECIMATE_MEAN;
    p.min_valid = 3;
    p.max_gap = 50.0f;
    kde::DepthDecimation decimate(1920, 1080, 8, p);                  // RAII over kde_decimate_create / _destroy
    const int w = decimate.outWidth(), h = decimate.outHeight();
    float* depth = nullptr;
    uint16_t* depth16 = nullptr;
    float* out = nullptr;
    uint16_t* out16 = nullptr;
    uint8_t* bgr = nullptr;
    uint8_t* small_bgr = nullptr;
    decimate.decimate(8, depth, out);
    decimate.decimate(8, depth16, out);
    decimate.decimate(8, depth, out16);
    decimate.decimate(8, depth16, out16);
    decimate.decimateColor(8, bgr, small_bgr);
    decimate.setStream(nullptr);
    const double K[9] = {1000, 0, 959.5, 0, 1000, 539.5, 0, 0, 1};
    double Ks[9];
    decimate.intrinsics(static_cast<const double*>(K), Ks);
    const void* host = decimate.depth_Host();
    const uint32_t* filled = decimate.filled_Host();
    const uint32_t* mixed = decimate.mixed_Host();
    void* dev = decimate.depth_Device();
    uint32_t* fdev = decimate.filled_Device();
    uint32_t* mdev = decimate.mixed_Device();
    kde_decimate* handle = decimate.handle();
    kde_jbf_params jp;
    kde_jbf_default_params(&jp);
    kde::ref::JointBilateralFilter jbf(w, h, jp, 8);                  // the chain of examples/decimate_demo.cpp
    jbf.ProcessBatch(8, static_cast<const float*>(dev), small_bgr);
    kde::GuidedDepthUpsampling up(w, h, 1920, 1080, 8);
    up.upsample(8, jbf.getFiltered_Device(), bgr, 8, out);
    return (host != nullptr) + (int)filled[0] + (int)mixed[0] + (fdev != nullptr) + (mdev != nullptr) + (handle != nullptr) + (int)Ks[0];
}
""")
    inc = os.path.join(ROOT, "include")
    r = subprocess.run([_hipcc(), "-std=c++17", "-fsyntax-only", "-I", inc, str(src)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    demo = os.path.join(ROOT, "examples", "decimate_demo.cpp")
    r = subprocess.run([_hipcc(), "-std=c++17", "-x", "hip", "--offload-arch=gfx950", "-fsyntax-only", demo], capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    text = open(demo).read()
    for stage in ("DepthDecimation", "JointBilateralFilter", "GuidedDepthUpsampling"):
        assert "kde::" + stage in text or "kde::ref::" + stage in text, stage
    assert "decimate_demo" in open(os.path.join(ROOT, "examples", "Makefile")).read()
    assert "examples/decimate_demo" in open(os.path.join(ROOT, ".gitignore")).read().split()
    size = tmp_path / "size.c"
    size.write_text('#include "kde_hip.h"\n#include <stdio.h>\nint main(void) { printf("%zu\\n", sizeof(kde_decimate_params)); return 0; }\n')
    exe = str(tmp_path / "size")
    subprocess.check_call(["cc", "-std=c11", "-I", inc, "-o", exe, str(size)], timeout=120)
    assert subprocess.run([exe], capture_output=True, text=True, check=True, timeout=60).stdout.split() == ["24"]


def test_the_kernel_file_is_what_the_issue_asks_for():
    csrc = os.path.join(ROOT, "kinectdepthmapenhancement_amd", "csrc")
    kernels = open(os.path.join(csrc, "decimate_kernels.hip")).read()
    for banned in ("hipMemsetAsync", "hipMemset(", "hipMalloc", "hipStreamSynchronize", "hipDeviceSynchronize", "atomicAdd", "asm("):
        assert banned not in kernels, banned
    assert kernels.count("hipLaunchKernelGGL") == 3                   # the decimation, the sum of the counts, the colour kernel
    objects = open(os.path.join(csrc, "objects.mk")).read()
    assert "decimate_kernels.o" in objects and "kde_api_decimate.o" in objects
    assert "launch_decimate" in open(os.path.join(csrc, "kde_internal.h")).read()
    api = open(os.path.join(csrc, "kde_api_decimate.cpp")).read()
    for shared in ("DepthStage stage", "KDE_STAGE_DEPTH_GETTERS", "KDE_STAGE_COUNT_GETTERS", "check_not_in_place", "check_z_range", "check_max_gap",
                   "check_batch_n", "check_depth_in", "check_depth_out", "check_has_device"):
        assert shared in api, shared
    assert "getenv" not in api and "getenv" not in kernels
