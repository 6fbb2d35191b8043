"""DepthHoleFilling (kde_holefill_*) at the ABI level, without a GPU: declared, exported and bound; the typed handle; every
refusal that precedes a HIP call; both tables; the C++ class and the demo compile.

On a host without a device kde_holefill_create makes the object without buffers, so the refusals that need a handle (results
before a call, a bad n, ...) and the tables are checked here as well."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import holefill_cases as HC
from conftest import ROOT

HEADER = os.path.join(ROOT, "include", "kde_hip.h")
FUNCS = ("kde_holefill_default_params", "kde_holefill_create", "kde_holefill_destroy", "kde_holefill_fill_batch",
         "kde_holefill_depth_device", "kde_holefill_depth_host", "kde_holefill_filled_device", "kde_holefill_filled_host",
         "kde_holefill_remaining_device", "kde_holefill_remaining_host", "kde_holefill_passes_per_launch", "kde_holefill_space_table",
         "kde_holefill_range_table")
DEVICE_GETTERS = ("kde_holefill_depth_device", "kde_holefill_filled_device", "kde_holefill_remaining_device")
HOST_GETTERS = ("kde_holefill_depth_host", "kde_holefill_filled_host", "kde_holefill_remaining_host")
FLT_MAX = float(np.finfo(np.float32).max)
DEFAULTS = (2, 8, 3, 2.0, 30.0, 0.0, 0, 0.0, FLT_MAX, 0)


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
    assert {n for n in native.SIGNATURES if n.startswith("kde_holefill_")} == set(FUNCS)
    assert native.lib().kde_abi_version() == 1
    assert ctypes.sizeof(native.HolefillParams) == 40
    assert [n for n, _ in native.HolefillParams._fields_] == ["radius", "iterations", "min_taps", "sigma_space", "sigma_color", "max_gap", "gap_rule",
                                                             "z_min", "z_max", "passes_per_launch"]
    # none of them is picked up by the enumeration of tools/abi_refusals.py, whose record is frozen
    frozen = (ctypes.c_void_p, ctypes.POINTER(ctypes.c_void_p))
    assert [n for n in FUNCS if native.SIGNATURES[n][1][0] in frozen] == []
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "abi_refusals.py")], capture_output=True, text=True, timeout=100)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "kde_holefill" not in r.stdout
    # the header states the rule and the launches
    raw = open(HEADER).read()
    for must in ("space[dy + r][dx + r] = (float)exp(-(double)(dx * dx + dy * dy) / (2.0 * (double)sigma_space * (double)sigma_space))",
                 "range[k] = (float)exp(-(double)(k * k) / (2.0 * (double)sigma_color * (double)sigma_color))",
                 "z = (d > z_min && d < z_max) ? (float)d : 0", "reads the state of pass p - 1 as a snapshot", "w = space[dy + r][dx + r] * range[k]",
                 "w > 0 is the test", "the first such tap in tap order winning a tie", "support is not recounted",
                 "num = num + w * z, den = den + w", "iff support >= min_taps and v > 0", "Pixels with z > 0 never change",
                 "before the uint16 rounding", "In place is refused", "ceil(N / k) launches", "capturable from the first call"):
        assert must in raw, must
    p = native.HolefillParams(9, 9, 9, 1.0, 2.0, 3.0, 4, 5.0, 6.0, 7)
    assert native.lib().kde_holefill_default_params(ctypes.byref(p)) == native.KDE_OK
    assert _fields(p) == DEFAULTS


@pytest.mark.timeout(120)
def test_the_typed_handle_refuses_a_plain_void_pointer(native):
    lib = native.lib()
    assert issubclass(native.HolefillHandle, ctypes.c_void_p)
    assert lib.kde_holefill_destroy(None) == native.KDE_OK
    assert lib.kde_holefill_destroy(native.HolefillHandle()) == native.KDE_OK
    out = ctypes.c_void_p()
    k = ctypes.c_int()
    for plain in (ctypes.c_void_p(), ctypes.c_void_p(16)):
        with pytest.raises(ctypes.ArgumentError):
            lib.kde_holefill_destroy(plain)
        with pytest.raises(ctypes.ArgumentError):
            lib.kde_holefill_fill_batch(plain, 1, None, 0, None, 1, 0, None, None, None)
        for name, size in (("kde_holefill_space_table", 49), ("kde_holefill_range_table", 766)):
            with pytest.raises(ctypes.ArgumentError):
                getattr(lib, name)(plain, None, size)
        with pytest.raises(ctypes.ArgumentError):
            lib.kde_holefill_passes_per_launch(plain, ctypes.byref(k))
        for name in DEVICE_GETTERS:
            with pytest.raises(ctypes.ArgumentError):
                getattr(lib, name)(plain, ctypes.byref(out))
        for name in HOST_GETTERS:
            with pytest.raises(ctypes.ArgumentError):
                getattr(lib, name)(plain, None, ctypes.byref(out))
        with pytest.raises(ctypes.ArgumentError):
            lib.kde_holefill_create(ctypes.byref(plain), 8, 8, 1, None)
    for other in (native.CloudHandle(), native.RegHandle(), native.UndistHandle(), native.UpsampleHandle()):   # another typed handle as well
        with pytest.raises(ctypes.ArgumentError):
            lib.kde_holefill_destroy(other)
    from kinectdepthmapenhancement_amd import filters
    assert filters.DepthHoleFilling._handle_type is native.HolefillHandle


@pytest.mark.timeout(120)
def test_refusals_name_their_function(native):
    lib = native.lib()
    INVALID = native.KDE_ERR_INVALID
    Params = native.HolefillParams
    DF, DU = native.KDE_DEPTH_F32, native.KDE_DEPTH_U16
    nan, inf = float("nan"), float("inf")

    def refused(name, rc):
        assert rc == INVALID, (name, rc, lib.kde_last_error_string())
        assert name.encode() in lib.kde_last_error_string(), (name, lib.kde_last_error_string())

    def create(out, size=(8, 6), batch=1, params=None):
        return lib.kde_holefill_create(out if out is None else ctypes.byref(out), *size, batch, None if params is None else ctypes.byref(params))

    def with_(**kw):
        p = Params(*DEFAULTS)
        for k, v in kw.items():
            setattr(p, k, v)
        return p

    out = native.HolefillHandle()
    refused("kde_holefill_default_params", lib.kde_holefill_default_params(None))
    refused("kde_holefill_create", create(None))
    for size in ((0, 6), (8, 0), (-1, 6), (8, -3), ((1 << 24) + 1, 1), (1, (1 << 24) + 1)):
        refused("kde_holefill_create", create(out, size))
    for batch in (0, -1, 65536):
        refused("kde_holefill_create", create(out, batch=batch))
    bad = dict(radius=(0, 4, -1, 1 << 20), iterations=(0, 65, -1), min_taps=(0, 25, -1, 1 << 20), sigma_space=(0.0, -0.0, -2.0, nan, inf, -inf),
               sigma_color=(0.0, -0.0, -30.0, nan, inf, -inf), max_gap=(-1.0, -1e-30, nan, inf, -inf), gap_rule=(2, -1), z_min=(nan, inf, -inf, -1.0, -1e-30),
               z_max=(nan, 0.0, -1.0), passes_per_launch=(-1, 5, 1 << 20))
    for field, values in bad.items():
        for v in values:
            refused("kde_holefill_create", create(out, params=with_(**{field: v})))
            if field not in ("z_max",):
                assert field.encode() in lib.kde_last_error_string(), (field, v, lib.kde_last_error_string())
    for r, taps in ((1, 9), (3, 49)):                               # min_taps is bounded by the radius's window without its centre
        refused("kde_holefill_create", create(out, params=with_(radius=r, min_taps=taps)))
    for zmin, zmax in ((100.0, 100.0), (200.0, 100.0), (FLT_MAX, FLT_MAX), (inf, inf)):
        refused("kde_holefill_create", create(out, params=with_(z_min=zmin, z_max=zmax)))
    assert out.value is None
    for params in (with_(radius=1, iterations=1, min_taps=8, sigma_space=1e-3, sigma_color=1e-3, z_max=inf, passes_per_launch=4),
                   with_(radius=3, iterations=64, min_taps=48, sigma_space=1e6, sigma_color=1e6, max_gap=1e30, gap_rule=1, z_min=5.0, z_max=6.0,
                         passes_per_launch=1), with_(max_gap=-0.0)):                                  # the limits are inside
        for size in ((8, 6), (1, 1), (1 << 24, 1)):
            assert create(out, size, params=params) == native.KDE_OK, lib.kde_last_error_string()
            assert lib.kde_holefill_destroy(out) == native.KDE_OK
            out = native.HolefillHandle()
    # null handles
    p = ctypes.c_void_p()
    k = ctypes.c_int()
    table = (ctypes.c_float * 766)()
    refused("kde_holefill_fill_batch", lib.kde_holefill_fill_batch(None, 1, 4096, DF, 8192, 1, DF, None, None, None))
    for name in DEVICE_GETTERS:
        refused(name, getattr(lib, name)(None, ctypes.byref(p)))
    for name in HOST_GETTERS:
        refused(name, getattr(lib, name)(None, None, ctypes.byref(p)))
    refused("kde_holefill_passes_per_launch", lib.kde_holefill_passes_per_launch(None, ctypes.byref(k)))
    refused("kde_holefill_space_table", lib.kde_holefill_space_table(None, table, 49))
    refused("kde_holefill_range_table", lib.kde_holefill_range_table(None, table, 766))
    assert lib.kde_holefill_destroy(None) == native.KDE_OK

    # an object for 4 frames (with buffers on a GPU host, without on any other: the checks are the same), non-default parameters
    h = native.HolefillHandle()
    assert create(h, (20, 13), 4, Params(3, 5, 2, 1.5, 12.0, 80.0, 1, 100.0, 5000.0, 2)) == native.KDE_OK, lib.kde_last_error_string()
    assert h.value
    try:
        for name in DEVICE_GETTERS:
            refused(name, getattr(lib, name)(h, None))
            refused(name, getattr(lib, name)(h, ctypes.byref(p)))                              # getters before the first call
        for name in HOST_GETTERS:
            refused(name, getattr(lib, name)(h, None, None))
            refused(name, getattr(lib, name)(h, None, ctypes.byref(p)))
        refused("kde_holefill_passes_per_launch", lib.kde_holefill_passes_per_launch(h, None))
        assert lib.kde_holefill_passes_per_launch(h, ctypes.byref(k)) == native.KDE_OK and k.value == 2
        refused("kde_holefill_range_table", lib.kde_holefill_range_table(h, None, 766))
        refused("kde_holefill_space_table", lib.kde_holefill_space_table(h, None, 49))
        for capacity in (765, 0, -1):
            refused("kde_holefill_range_table", lib.kde_holefill_range_table(h, table, capacity))
        for capacity in (48, 25, 0, -1):
            refused("kde_holefill_space_table", lib.kde_holefill_space_table(h, table, capacity))

        def call(n, src=4096, dfmt=DF, bgr=8192, frames=1, ofmt=DF, out_dev=None, pass_of=None):
            return lib.kde_holefill_fill_batch(h, n, src, dfmt, bgr, frames, ofmt, out_dev, pass_of, None)

        refused("kde_holefill_fill_batch", call(2, src=None))                                  # null depth
        refused("kde_holefill_fill_batch", call(2, bgr=None))                                  # null guide
        refused("kde_holefill_fill_batch", call(5))                                            # n > max_batch
        refused("kde_holefill_fill_batch", call(0))
        refused("kde_holefill_fill_batch", call(-1))
        for frames in (2, 0, 4, -1):
            refused("kde_holefill_fill_batch", call(3, frames=frames))                         # bgr_frames neither 1 nor n
            assert b"bgr_frames" in lib.kde_last_error_string()
        for fmt in (2, -1):
            refused("kde_holefill_fill_batch", call(2, dfmt=fmt))                              # unknown formats
            refused("kde_holefill_fill_batch", call(2, ofmt=fmt))
        refused("kde_holefill_fill_batch", call(2, src=4098))                                  # float depth not 4-byte aligned
        refused("kde_holefill_fill_batch", call(2, src=4097, dfmt=DU))                         # uint16 depth not 2-byte aligned
        refused("kde_holefill_fill_batch", call(2, out_dev=65538))                             # float output not 4-byte aligned
        refused("kde_holefill_fill_batch", call(2, ofmt=DU, out_dev=65537))                    # uint16 output not 2-byte aligned
        frame = 20 * 13
        for out_dev in (4096, 4096 + 4 * frame, 4096 - 4 * (2 * frame - 1), 4096 + 4 * (2 * frame - 1)):    # in place, and partial overlaps
            refused("kde_holefill_fill_batch", call(2, out_dev=out_dev))
            assert b"in place" in lib.kde_last_error_string()
        refused("kde_holefill_fill_batch", call(2, dfmt=DU, ofmt=DU, out_dev=4096))
        # still no call went through
        refused("kde_holefill_depth_device", lib.kde_holefill_depth_device(h, ctypes.byref(p)))
        refused("kde_holefill_remaining_host", lib.kde_holefill_remaining_host(h, None, ctypes.byref(p)))
    finally:
        assert lib.kde_holefill_destroy(h) == native.KDE_OK


@pytest.mark.timeout(120)
def test_a_valid_call_on_a_host_without_a_device_is_a_hip_error(native):
    """the object is created without buffers there; everything validates as usual and the launch then answers KDE_ERR_HIP"""
    import torch
    if torch.cuda.is_available():
        pytest.skip("this host has a device: tests/test_gpu_holefill.py makes the same calls for real")
    lib = native.lib()
    h = native.HolefillHandle()
    assert lib.kde_holefill_create(ctypes.byref(h), 20, 13, 2, None) == native.KDE_OK
    assert lib.kde_holefill_fill_batch(h, 2, 4096, 0, 8192, 1, 1, None, None, None) == native.KDE_ERR_HIP
    assert lib.kde_holefill_fill_batch(h, 2, 4096, 1, 8192, 2, 0, 16384, 32768, None) == native.KDE_ERR_HIP   # the frames just do not overlap
    assert lib.kde_holefill_fill_batch(h, 2, 4096, 0, 8192, 2, 0, 4096 + 2 * 20 * 13 * 4, None, None) == native.KDE_ERR_HIP
    assert b"kde_holefill_fill_batch" in lib.kde_last_error_string()
    p = ctypes.c_void_p()
    assert lib.kde_holefill_depth_device(h, ctypes.byref(p)) == native.KDE_ERR_INVALID
    assert lib.kde_holefill_destroy(h) == native.KDE_OK


def _ulp_distance(a, b):
    """in units of the last place of binary32, over the non-negative floats (their bit patterns are ordered like them)"""
    return np.abs(a.view(np.int32).astype(np.int64) - b.view(np.int32).astype(np.int64))


@pytest.mark.timeout(120)
def test_both_tables_agree_with_numpy(native):
    """needs no device: the tables are made on the host at create.  One ulp for a libm whose exp is not correctly rounded;
    exact at the centre and at k = 0"""
    from kinectdepthmapenhancement_amd import filters
    for radius, ss, sc in ((2, 2.0, 30.0), (1, 0.5, 10.0), (3, 1.0, 1.0), (3, 0.37, 0.37), (2, 255.0, 255.0), (1, 1e6, 1e6)):
        p = filters.DepthHoleFilling.default_params()
        p.radius, p.sigma_space, p.sigma_color = radius, ss, sc
        H = filters.DepthHoleFilling((8, 6), 1, p)
        space, rng = H.space_table(), H.range_table()
        assert H.passes_per_launch() in (1, 2, 3, 4)
        H.close()
        want_s, want_r = HC.space_table(radius, ss), HC.range_table(sc)
        side = 2 * radius + 1
        assert space.dtype == np.float32 and space.shape == (side, side) and rng.dtype == np.float32 and rng.shape == (766,)
        assert space[radius, radius] == 1.0 and rng[0] == 1.0
        assert int(_ulp_distance(space, want_s).max()) <= 1 and int(_ulp_distance(rng, want_r).max()) <= 1, (radius, ss, sc)
        assert (space == space.T).all() and (space == space[::-1, ::-1]).all()
        assert (np.diff(rng.astype(np.float64)) <= 0).all()
    assert (rng > 0.9999).all() and (space > 0.9999).all()         # sigma 1e6: every tap weighs the same


@pytest.mark.timeout(600)
def test_cpp_class_and_demo_compile(tmp_path):
    src = tmp_path / "holefill_user.cpp"
    src.write_text(r"""
#include "kde/kde.hpp"
#include <cstdint>
static_assert(sizeof(kde_holefill_params) == 40, "kde_holefill_params: ten four-byte fields");
int main()
{
    kde::DepthHoleFilling one(1920, 1080);                            // one frame, the defaults
    kde_holefill_params p = kde::DepthHoleFilling::defaultParams();
    p.radius = 3;
    p.max_gap = 100.0f;
    p.gap_rule = 1;
    p.passes_per_launch = 2;
    kde::DepthHoleFilling fill(640, 480, 8, p);                       // RAII over kde_holefill_create / _destroy
    float* depth = nullptr;
    uint16_t* depth16 = nullptr;
    float* out = nullptr;
    uint16_t* out16 = nullptr;
    uint8_t* bgr = nullptr;
    uint8_t* pass_of = nullptr;
    fill.fill(8, depth, bgr, 8, out);
    fill.fill(8, depth16, bgr, 1, out, pass_of);
    fill.fill(8, depth, bgr, 8, out16);
    fill.fill(8, depth16, bgr, 1, out16, pass_of);
    fill.setStream(nullptr);
    const void* host = fill.depth_Host();
    const uint32_t* filled = fill.filled_Host();
    const uint32_t* remaining = fill.remaining_Host();
    void* dev = fill.depth_Device();
    uint32_t* fdev = fill.filled_Device();
    uint32_t* rdev = fill.remaining_Device();
    float space[49], range[766];
    fill.spaceTable(space, 49);
    fill.rangeTable(range);
    kde_holefill* h = fill.handle();
    kde::ref::JointBilateralFilter jbf(640, 480);                      // the chain of examples/holefill_demo.cpp
    jbf.ProcessBatch(1, static_cast<const float*>(dev), bgr);
    return (host != nullptr) + (int)filled[0] + (int)remaining[0] + (fdev != nullptr) + (rdev != nullptr) + (h != nullptr) + (space[24] == 1.0f) +
           (range[0] == 1.0f) + fill.passesPerLaunch();
}
""")
    inc = os.path.join(ROOT, "include")
    r = subprocess.run([_hipcc(), "-std=c++17", "-fsyntax-only", "-I", inc, str(src)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    demo = os.path.join(ROOT, "examples", "holefill_demo.cpp")
    r = subprocess.run([_hipcc(), "-std=c++17", "-x", "hip", "--offload-arch=gfx950", "-fsyntax-only", demo], capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    assert "holefill_demo" in open(os.path.join(ROOT, "examples", "Makefile")).read()
    # the struct is what the compiler says, from C
    size = tmp_path / "size.c"
    size.write_text('#include "kde_hip.h"\n#include <stdio.h>\nint main(void) { printf("%zu\\n", sizeof(kde_holefill_params)); return 0; }\n')
    exe = str(tmp_path / "size")
    subprocess.check_call(["cc", "-std=c11", "-I", inc, "-o", exe, str(size)], timeout=120)
    assert subprocess.run([exe], capture_output=True, text=True, check=True, timeout=60).stdout.split() == ["40"]


@pytest.mark.timeout(120)
def test_the_library_choice_of_passes_per_launch(native):
    """DESIGN.md, "Depth hole filling": 4 / 2 / 2 for radius 1 / 2 / 3 by measurement, 1 for radius 3 with the guard, where fusing
    did not beat one pass per launch; a given value is taken as it is"""
    lib = native.lib()
    k = ctypes.c_int()
    for radius, gap, fuse, want in ((1, 0.0, 0, 4), (1, 100.0, 0, 4), (2, 0.0, 0, 2), (2, 100.0, 0, 2), (3, 0.0, 0, 2), (3, 100.0, 0, 1),
                                    (3, 100.0, 4, 4), (1, 0.0, 1, 1), (2, 0.0, 3, 3)):
        h = native.HolefillHandle()
        p = native.HolefillParams(radius, 8, 3, 2.0, 30.0, gap, 0, 0.0, FLT_MAX, fuse)
        assert lib.kde_holefill_create(ctypes.byref(h), 8, 6, 1, ctypes.byref(p)) == native.KDE_OK
        assert lib.kde_holefill_passes_per_launch(h, ctypes.byref(k)) == native.KDE_OK and k.value == want, (radius, gap, fuse, k.value)
        assert lib.kde_holefill_destroy(h) == native.KDE_OK
