"""kde_points_to_depth and the host-fed KinectDepthEnhancement entry points (kde_enh_feed_*) at the ABI level, without a GPU:
declared, exported and bound; the typed feed handle; every refusal that precedes a HIP call; the record of their refusals;
the C++ classes compile; and the host side of the uint16 depth rule against its numpy statement."""
import ctypes
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT
from depth_u16_cases import CRAFTED, to_u16, values

HEADER = os.path.join(ROOT, "include", "kde_hip.h")
NEW_FUNCS = ("kde_points_to_depth", "kde_enh_feed_create", "kde_enh_feed_destroy", "kde_enh_feed_process",
             "kde_enh_feed_last_stats")


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
    for name in NEW_FUNCS:
        assert re.search(r"\bint\s+" + name + r"\s*\(", text), name
    assert "KDE_OUT_POINTS_F32 = 0, KDE_OUT_DEPTH_F32 = 1, KDE_OUT_DEPTH_U16 = 2" in text
    assert "#define KDE_ABI_VERSION 1" in text                     # the new entry points only add to the ABI
    lib = ctypes.CDLL(native.LIB_PATH)
    assert all(hasattr(lib, n) for n in NEW_FUNCS)
    assert set(NEW_FUNCS) <= set(native.SIGNATURES)
    assert native.lib().kde_abi_version() == 1
    assert (native.KDE_OUT_POINTS_F32, native.KDE_OUT_DEPTH_F32, native.KDE_OUT_DEPTH_U16) == (0, 1, 2)
    # none of them is picked up by the enumeration of tools/abi_refusals.py, whose record is frozen
    frozen = (ctypes.c_void_p, ctypes.POINTER(ctypes.c_void_p))
    assert [n for n in NEW_FUNCS if native.SIGNATURES[n][1][0] in frozen] == []


@pytest.mark.timeout(120)
def test_the_typed_handle_refuses_a_plain_void_pointer(native):
    lib = native.lib()
    st = native.FeedStats()
    assert issubclass(native.EnhFeedHandle, ctypes.c_void_p)
    assert lib.kde_enh_feed_destroy(None) == native.KDE_OK
    assert lib.kde_enh_feed_destroy(native.EnhFeedHandle()) == native.KDE_OK
    for plain in (ctypes.c_void_p(), ctypes.c_void_p(16)):
        with pytest.raises(ctypes.ArgumentError):
            lib.kde_enh_feed_destroy(plain)
        with pytest.raises(ctypes.ArgumentError):
            lib.kde_enh_feed_last_stats(plain, ctypes.byref(st))
        with pytest.raises(ctypes.ArgumentError):
            lib.kde_enh_feed_process(plain, 1, None, 0, None, 0, None)
        with pytest.raises(ctypes.ArgumentError):
            lib.kde_enh_feed_create(ctypes.byref(plain), None, 1)
    from kinectdepthmapenhancement_amd import filters
    assert filters._Handle._handle_type is ctypes.c_void_p
    assert filters.KinectDepthEnhancementFeed._handle_type is native.EnhFeedHandle


@pytest.mark.timeout(120)
def test_refusals_name_their_function(native):
    lib = native.lib()
    out = native.EnhFeedHandle()
    st = native.FeedStats()
    F32, U16 = native.KDE_DEPTH_F32, native.KDE_DEPTH_U16
    cases = [("kde_points_to_depth", lambda: lib.kde_points_to_depth(1, None, F32, None, None)),
             ("kde_points_to_depth", lambda: lib.kde_points_to_depth(8, 4096, F32, None, None)),          # null output
             ("kde_points_to_depth", lambda: lib.kde_points_to_depth(8, None, U16, 4096, None)),          # null points
             ("kde_points_to_depth", lambda: lib.kde_points_to_depth(8, 4096, 2, 8192, None)),            # unknown format
             ("kde_points_to_depth", lambda: lib.kde_points_to_depth(8, 4096, -1, 8192, None)),
             ("kde_points_to_depth", lambda: lib.kde_points_to_depth(8, 4098, F32, 8192, None)),          # points not 4-aligned
             ("kde_points_to_depth", lambda: lib.kde_points_to_depth(8, 4097, U16, 8192, None)),
             ("kde_points_to_depth", lambda: lib.kde_points_to_depth(8, 4096, F32, 8194, None)),          # f32 out not 4-aligned
             ("kde_points_to_depth", lambda: lib.kde_points_to_depth(8, 4096, U16, 8193, None)),          # u16 out not 2-aligned
             ("kde_enh_feed_create", lambda: lib.kde_enh_feed_create(None, None, 2)),
             ("kde_enh_feed_create", lambda: lib.kde_enh_feed_create(ctypes.byref(out), None, 2)),
             ("kde_enh_feed_process", lambda: lib.kde_enh_feed_process(None, 1, None, 0, None, 0, None)),
             ("kde_enh_feed_process", lambda: lib.kde_enh_feed_process(None, 4, 1, U16, 1, native.KDE_OUT_DEPTH_U16, 1)),
             ("kde_enh_feed_last_stats", lambda: lib.kde_enh_feed_last_stats(None, ctypes.byref(st))),
             ("kde_enh_feed_last_stats", lambda: lib.kde_enh_feed_last_stats(None, None))]
    for name, call in cases:
        assert call() == native.KDE_ERR_INVALID, name
        assert name.encode() in lib.kde_last_error_string(), (name, lib.kde_last_error_string())
    assert out.value is None
    # n_points == 0 launches nothing and is not an error, whatever the pointers (no HIP call: safe without a GPU)
    assert lib.kde_points_to_depth(0, None, F32, None, None) == native.KDE_OK
    assert lib.kde_points_to_depth(0, 4097, U16, 8193, None) == native.KDE_OK
    assert lib.kde_enh_feed_destroy(None) == native.KDE_OK


@pytest.mark.timeout(300)
def test_refused_calls_answer_as_recorded():
    """tests/golden/abi_refusals_enh_feed.json, written by tools/abi_refusals_new.py: the all-zero call of each of the five
    functions (KDE_ERR_INVALID; KDE_OK for kde_enh_feed_destroy(NULL) and for kde_points_to_depth, whose all-zero call is
    its documented n_points == 0 no-op), kde_enh_feed_create with a valid out-pointer, and kde_points_to_depth for one point.
    The same calls in the same order, in a child process, must give the same codes and messages."""
    golden = json.load(open(os.path.join(ROOT, "tests", "golden", "abi_refusals_enh_feed.json")))
    zero = {r["name"]: r["rc"] for r in golden if r["mode"] == "zero"}
    assert sorted(zero) == sorted(NEW_FUNCS)
    ok = {"kde_enh_feed_destroy", "kde_points_to_depth"}
    assert all(rc == (0 if name in ok else 1) for name, rc in zero.items()), zero
    assert all(r["rc"] == 1 and r["name"] in r["message"] for r in golden if r["mode"] != "zero")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "abi_refusals_new.py")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
    assert json.loads(r.stdout) == golden


@pytest.mark.timeout(300)
def test_cpp_classes_compile(tmp_path):
    src = tmp_path / "enh_feed_user.cpp"
    src.write_text(r"""
#include "kde/kde.hpp"
#include <cstdint>
#include <vector>
int main()
{
    KinectDepthEnhancement one(640, 480);                         // the reference's constructor: max_batch 1
    KinectDepthEnhancement enh(640, 480, 4);                      // added: chunks of up to 4 frames
    const double K[9] = {575.8, 0, 320, 0, 575.8, 240, 0, 0, 1};
    enh.SetParametor(15, 20, K);
    kde::KinectDepthEnhancementFeed feed(enh, 4);                 // RAII over kde_enh_feed_create / _destroy
    kde::KinectDepthEnhancementFeed raw(one.handle(), 1);
    const size_t px = 640 * 480;
    std::vector<uint16_t> d16(px), o16(px);
    std::vector<float> d32(px), o32(px);
    std::vector<float3> cloud(px);
    std::vector<kde_float3> cloud_c(px);
    std::vector<uint8_t> bgr(px * 3);
    feed.process(1, d16.data(), bgr.data(), o16.data());          // sensor depth in, sensor depth out
    feed.process(1, d16.data(), bgr.data(), o32.data());
    feed.process(1, d32.data(), bgr.data(), cloud.data());
    raw.process(1, d32.data(), bgr.data(), cloud_c.data());
    kde::pointsToDepth(px, enh.getOptimizedPoints_Device(), static_cast<float*>(nullptr));
    kde::pointsToDepth(px, enh.getOptimizedPoints_Device(), static_cast<uint16_t*>(nullptr), nullptr);
    const kde_feed_stats st = feed.lastStats();
    kde_enh_feed* h = feed.handle();
    try {
        kde::KinectDepthEnhancementFeed bad(enh, 5);
    } catch (const kde::Error& e) {
        return e.code();
    }
    return st.frames + (h != nullptr);
}
""")
    r = subprocess.run([_hipcc(), "-std=c++17", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    # an output pointer of a type that is no output format must not compile
    bad = tmp_path / "enh_feed_bad.cpp"
    bad.write_text(src.read_text().replace("std::vector<uint16_t> d16(px), o16(px);", "std::vector<uint16_t> d16(px); std::vector<int> o16(px);"))
    r = subprocess.run([_hipcc(), "-std=c++17", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(bad)],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode != 0


@pytest.mark.timeout(300)
def test_host_side_of_the_u16_rule_matches_numpy(tmp_path):
    """depth_to_u16 of csrc/kde_device_math.h is one __host__ __device__ function; its host side, compiled from that header,
    must be r = np.rint(z); where((r >= 1) & (r <= 65535), r, 0) on the crafted values, on random z in +-70000 with ties, and
    must return every uint16 that the widening (float)u produced."""
    src = tmp_path / "host_rule.cpp"
    src.write_text(r"""
#include "kde_device_math.h"
#include <cstdio>
int main()
{
    float z;
    while (std::fread(&z, sizeof z, 1, stdin) == 1) {
        const uint16_t v = kde::depth_to_u16(z);
        std::fwrite(&v, sizeof v, 1, stdout);
    }
    return 0;
}
""")
    exe = str(tmp_path / "host_rule")
    from kinectdepthmapenhancement_amd import _native
    subprocess.check_call([_hipcc(), "-std=c++17", "-O3", "-ffp-contract=off", "-x", "hip", "--cuda-host-only", "-I", _native.CSRC, "-o", exe,
                           str(src)], timeout=280)
    z = np.concatenate([CRAFTED, values(4096, seed=3), np.arange(65536, dtype=np.float32),
                        np.arange(65536, dtype=np.float32) + np.float32(0.5)])
    got = np.frombuffer(subprocess.run([exe], input=z.tobytes(), capture_output=True, check=True, timeout=60).stdout, np.uint16)
    want = to_u16(z)
    assert got.shape == want.shape
    assert np.array_equal(got, want), [(float(a), int(b), int(c)) for a, b, c in zip(z, got, want) if b != c][:10]
    # the numpy statement itself on the values the issue names
    named = {0.0: 0, -0.0: 0, 0.49999997: 0, 0.5: 0, 1.5: 2, 2.5: 2, 65534.5: 65534, 65535.0: 65535, 65535.4: 65535, 65535.5: 0,
             65536.0: 0, 1e9: 0, -3.0: 0, np.inf: 0, -np.inf: 0, np.nan: 0, 1e-45: 0}
    for v, w in named.items():
        assert int(to_u16(np.float32(v))) == w, v
    assert np.array_equal(to_u16(np.arange(65536, dtype=np.float32)), np.arange(65536).astype(np.uint16))     # exact inverse of widening
