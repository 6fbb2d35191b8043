"""PointCloudXYZRGB (kde_cloud_*, main.cpp:211-300) at the ABI level, without a GPU: declared, exported and bound; the typed
handle; every refusal that precedes a HIP call; the C++ class and the PCD writer compile; the record is 16 bytes; the PCD
files of both writers; and the numpy statement of the rule (cloud_cases.py) on a case worked out by hand.

On a host without a device kde_cloud_create makes the object without buffers, so the refusals that need a handle (a depth
map before the camera, results before a call, ...) are checked here as well."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import cloud_cases as CC
from conftest import ROOT

HEADER = os.path.join(ROOT, "include", "kde_hip.h")
FUNCS = ("kde_cloud_default_params", "kde_cloud_create", "kde_cloud_destroy", "kde_cloud_set_camera", "kde_cloud_build_batch",
         "kde_cloud_points_device", "kde_cloud_counts_device", "kde_cloud_counts_host", "kde_cloud_points_host")
PCD_LINES = ["# .PCD v0.7 - Point Cloud Data file format", "VERSION 0.7", "FIELDS x y z rgb", "SIZE 4 4 4 4", "TYPE F F F U",
             "COUNT 1 1 1 1", "WIDTH {w}", "HEIGHT {h}", "VIEWPOINT 0 0 0 1 0 0 0", "POINTS {n}", "DATA {data}"]


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
    assert native.lib().kde_abi_version() == 1
    assert ctypes.sizeof(native.CloudPoint) == 16 and ctypes.sizeof(native.CloudParams) == 20
    # none of them is picked up by the enumeration of tools/abi_refusals.py, whose record is frozen
    frozen = (ctypes.c_void_p, ctypes.POINTER(ctypes.c_void_p))
    assert [n for n in FUNCS if native.SIGNATURES[n][1][0] in frozen] == []
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "abi_refusals.py")], capture_output=True, text=True, timeout=100)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "kde_cloud" not in r.stdout
    # every entry point cites the reference's loop in the header
    raw = open(HEADER).read()
    for name in FUNCS:
        at = raw.index("int " + name + "(")
        assert "main.cpp:211-300" in raw[raw.rindex("/*", 0, at):at] or "main.cpp:211-300" in raw[at:raw.index("\n", at)], name
    p = native.CloudParams()
    assert native.lib().kde_cloud_default_params(ctypes.byref(p)) == native.KDE_OK
    assert (p.z_min, p.z_max, p.divisor, p.negate_z, p.organized) == (50.0, 15000.0, 1000.0, 1, 0)


@pytest.mark.timeout(120)
def test_the_typed_handle_refuses_a_plain_void_pointer(native):
    lib = native.lib()
    assert issubclass(native.CloudHandle, ctypes.c_void_p)
    assert lib.kde_cloud_destroy(None) == native.KDE_OK
    assert lib.kde_cloud_destroy(native.CloudHandle()) == native.KDE_OK
    out = ctypes.c_void_p()
    for plain in (ctypes.c_void_p(), ctypes.c_void_p(16)):
        with pytest.raises(ctypes.ArgumentError):
            lib.kde_cloud_destroy(plain)
        with pytest.raises(ctypes.ArgumentError):
            lib.kde_cloud_set_camera(plain, None)
        with pytest.raises(ctypes.ArgumentError):
            lib.kde_cloud_build_batch(plain, 1, None, None, 1, None, None)
        with pytest.raises(ctypes.ArgumentError):
            lib.kde_cloud_points_device(plain, ctypes.byref(out))
        with pytest.raises(ctypes.ArgumentError):
            lib.kde_cloud_counts_device(plain, ctypes.byref(out))
        with pytest.raises(ctypes.ArgumentError):
            lib.kde_cloud_counts_host(plain, None, ctypes.byref(out))
        with pytest.raises(ctypes.ArgumentError):
            lib.kde_cloud_points_host(plain, None, ctypes.byref(out), ctypes.byref(out))
        with pytest.raises(ctypes.ArgumentError):
            lib.kde_cloud_create(ctypes.byref(plain), 8, 8, 1, None)
    with pytest.raises(ctypes.ArgumentError):
        lib.kde_cloud_destroy(native.Error3dHandle())              # another typed handle is refused as well
    from kinectdepthmapenhancement_amd import filters
    assert filters.PointCloudXYZRGB._handle_type is native.CloudHandle
    assert filters.PointCloudXYZRGB.POINT_DTYPE == CC.POINT


@pytest.mark.timeout(120)
def test_refusals_name_their_function(native):
    lib = native.lib()
    INVALID = native.KDE_ERR_INVALID
    Src, Params = native.Error3dSource, native.CloudParams
    P, DF, DU = native.KDE_SRC_POINTS_F32, native.KDE_SRC_DEPTH_F32, native.KDE_SRC_DEPTH_U16
    nan, inf = float("nan"), float("inf")

    def refused(name, rc):
        assert rc == INVALID, (name, rc, lib.kde_last_error_string())
        assert name.encode() in lib.kde_last_error_string(), (name, lib.kde_last_error_string())

    out = native.CloudHandle()
    refused("kde_cloud_default_params", lib.kde_cloud_default_params(None))
    # create: null out, bad frame, bad batch, then every bad parameter block
    refused("kde_cloud_create", lib.kde_cloud_create(None, 8, 8, 1, None))
    refused("kde_cloud_create", lib.kde_cloud_create(ctypes.byref(out), 0, 8, 1, None))
    refused("kde_cloud_create", lib.kde_cloud_create(ctypes.byref(out), 8, 8, 0, None))
    for zmin, zmax in ((nan, 100.0), (50.0, nan), (50.0, inf), (-inf, 100.0), (100.0, 100.0), (200.0, 100.0)):
        refused("kde_cloud_create", lib.kde_cloud_create(ctypes.byref(out), 8, 8, 1, ctypes.byref(Params(zmin, zmax, 1000.0, 1, 0))))
    for divisor in (nan, inf, -inf, 0.0, -0.0, -1000.0):
        refused("kde_cloud_create", lib.kde_cloud_create(ctypes.byref(out), 8, 8, 1, ctypes.byref(Params(50.0, 15000.0, divisor, 1, 0))))
    assert out.value is None
    # null handles and null arguments
    K = (ctypes.c_double * 9)(500, 0, 4, 0, 500, 4, 0, 0, 1)
    src = Src(4096, P)
    p, q = ctypes.c_void_p(), ctypes.c_void_p()
    refused("kde_cloud_set_camera", lib.kde_cloud_set_camera(None, K))
    refused("kde_cloud_build_batch", lib.kde_cloud_build_batch(None, 1, ctypes.byref(src), 8192, 1, None, None))
    refused("kde_cloud_points_device", lib.kde_cloud_points_device(None, ctypes.byref(p)))
    refused("kde_cloud_counts_device", lib.kde_cloud_counts_device(None, ctypes.byref(p)))
    refused("kde_cloud_counts_host", lib.kde_cloud_counts_host(None, None, ctypes.byref(p)))
    refused("kde_cloud_points_host", lib.kde_cloud_points_host(None, None, ctypes.byref(p), ctypes.byref(q)))
    assert lib.kde_cloud_destroy(None) == native.KDE_OK

    # an object for 4 frames (with buffers on a GPU host, without on any other: the checks are the same), non-default parameters
    h = native.CloudHandle()
    assert lib.kde_cloud_create(ctypes.byref(h), 8, 6, 4, ctypes.byref(Params(100.0, 2000.0, 1.0, 0, 1))) == native.KDE_OK, \
        lib.kde_last_error_string()
    assert h.value
    try:
        refused("kde_cloud_set_camera", lib.kde_cloud_set_camera(h, None))
        for name in ("kde_cloud_points_device", "kde_cloud_counts_device"):
            refused(name, getattr(lib, name)(h, None))
            refused(name, getattr(lib, name)(h, ctypes.byref(p)))                              # results before any call
        refused("kde_cloud_counts_host", lib.kde_cloud_counts_host(h, None, None))
        refused("kde_cloud_counts_host", lib.kde_cloud_counts_host(h, None, ctypes.byref(p)))
        refused("kde_cloud_points_host", lib.kde_cloud_points_host(h, None, None, ctypes.byref(q)))
        refused("kde_cloud_points_host", lib.kde_cloud_points_host(h, None, ctypes.byref(p), None))
        refused("kde_cloud_points_host", lib.kde_cloud_points_host(h, None, ctypes.byref(p), ctypes.byref(q)))

        def call(n, s, bgr, frames, out_dev=None):
            return lib.kde_cloud_build_batch(h, n, ctypes.byref(s) if s is not None else None, bgr, frames, out_dev, None)

        refused("kde_cloud_build_batch", call(2, None, 8192, 1))                               # null source
        refused("kde_cloud_build_batch", call(2, src, None, 1))                                # null colour image
        refused("kde_cloud_build_batch", call(5, src, 8192, 1))                                # n > max_batch
        refused("kde_cloud_build_batch", call(0, src, 8192, 1))
        refused("kde_cloud_build_batch", call(3, src, 8192, 2))                                # bgr_frames neither 1 nor n
        refused("kde_cloud_build_batch", call(3, src, 8192, 0))
        refused("kde_cloud_build_batch", call(3, src, 8192, 4))
        refused("kde_cloud_build_batch", call(2, Src(4096, 3), 8192, 1))                       # unknown format
        refused("kde_cloud_build_batch", call(2, Src(4096, -1), 8192, 1))
        refused("kde_cloud_build_batch", call(2, Src(None, P), 8192, 1))                       # null data
        refused("kde_cloud_build_batch", call(2, Src(4098, P), 8192, 1))                       # float3 not 4-byte aligned
        refused("kde_cloud_build_batch", call(2, src, 8192, 1, 65544))                         # records not 16-byte aligned
        # a depth source before a camera is set, float and uint16
        refused("kde_cloud_build_batch", call(2, Src(4096, DF), 8192, 2))
        refused("kde_cloud_build_batch", call(2, Src(4096, DU), 8192, 2))
        assert b"kde_cloud_set_camera" in lib.kde_last_error_string()
        assert lib.kde_cloud_set_camera(h, K) == native.KDE_OK
        refused("kde_cloud_build_batch", call(2, Src(4098, DF), 8192, 1))                      # float depth not 4-byte aligned
        refused("kde_cloud_build_batch", call(2, Src(4097, DU), 8192, 1))                      # uint16 depth not 2-byte aligned
        # still no call went through
        refused("kde_cloud_points_device", lib.kde_cloud_points_device(h, ctypes.byref(p)))
    finally:
        assert lib.kde_cloud_destroy(h) == native.KDE_OK


@pytest.mark.timeout(300)
def test_cpp_headers_compile_and_the_record_is_16_bytes(tmp_path):
    src = tmp_path / "cloud_user.cpp"
    src.write_text(r"""
#include "kde/kde.hpp"
#include "kde/pcd_io.hpp"
#include <cstdint>
static_assert(sizeof(kde_cloud_point) == 16, "kde_cloud_point must be 16 bytes");
static_assert(sizeof(kde_cloud_params) == 20, "kde_cloud_params: three floats and two ints");
int main()
{
    kde::PointCloudXYZRGB one(640, 480);                          // one frame, the reference's literals
    kde_cloud_params p = kde::PointCloudXYZRGB::defaultParams();
    p.organized = 1;
    kde::PointCloudXYZRGB cloud(640, 480, 64, p);                 // RAII over kde_cloud_create / _destroy
    const double K[9] = {575.8, 0, 320, 0, 575.8, 240, 0, 0, 1};
    const kde::Mat33d M{{575.8, 0, 320, 0, 575.8, 240, 0, 0, 1}};
    cloud.setCamera(K);
    cloud.setCamera(M);
    float3* pts = nullptr;
    float* depth = nullptr;
    uint16_t* depth16 = nullptr;
    uint8_t* bgr = nullptr;
    kde_cloud_point* out = nullptr;
    cloud.build(64, kde::MeanError3D::source(pts), bgr);
    cloud.build(64, kde::MeanError3D::source(depth), bgr, 64);
    cloud.build(64, kde::MeanError3D::source(depth16), bgr, 64, out);
    cloud.setStream(nullptr);
    const uint64_t* offsets = nullptr;
    const kde_cloud_point* host = cloud.points_Host(&offsets);
    const uint32_t* counts = cloud.counts_Host();
    kde_cloud_point* dev = cloud.points_Device();
    uint32_t* cdev = cloud.counts_Device();
    kde_cloud* h = cloud.handle();
    const bool ok = kde::writePcd("a.pcd", host, counts[0]) && kde::writePcd("b.pcd", host + offsets[1], 640 * 480, 640, 480, false);
    return (int)ok + (dev != nullptr) + (cdev != nullptr) + (h != nullptr) + (int)kde::pcdHeader(1, 1, true).size();
}
""")
    r = subprocess.run([_hipcc(), "-std=c++17", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    # the size is what the compiler says, not what the header's comment says
    size = tmp_path / "size.c"
    size.write_text('#include "kde_hip.h"\n#include <stdio.h>\nint main(void) { printf("%zu %zu %zu\\n", sizeof(kde_cloud_point), '
                    '_Alignof(kde_cloud_point), sizeof(kde_cloud_params)); return 0; }\n')
    exe = str(tmp_path / "size")
    subprocess.check_call(["cc", "-std=c11", "-I", os.path.join(ROOT, "include"), "-o", exe, str(size)], timeout=120)
    assert subprocess.run([exe], capture_output=True, text=True, check=True, timeout=60).stdout.split() == ["16", "4", "20"]


def _sample_records():
    """records with everything a file has to carry: -0, denormals, the extremes, an inf, nine-digit fractions, every colour byte"""
    pts = CC.clouds(77, 1, 5, 7)[0]
    pts.reshape(-1, 3)[3] = (np.float32(1e-42), np.float32(-3.4028235e38), np.float32(1234.5677))
    rec = CC.statement(pts, CC.bgr_images(77, 1, 5, 7)[0])
    assert rec.size >= 12 and np.isnan(rec["x"]).any() and np.isinf(rec["y"]).any()
    assert (rec["x"].view(np.uint32) == 0x80000000).any()                 # a -0
    return rec


@pytest.mark.timeout(120)
def test_pcd_round_trip_and_header(tmp_path):
    from kinectdepthmapenhancement_amd import pcdio
    assert pcdio.POINT_DTYPE == CC.POINT
    dense = _sample_records()
    pts = CC.clouds(78, 1, 5, 7)[0]
    org = CC.statement(pts, CC.bgr_images(78, 1, 5, 7)[0], organized=True)
    assert org.size == 35 and (org["z"].view(np.uint32) == CC.QNAN).any()
    for rec, w, h, kw in ((dense, dense.size, 1, {}), (org, 7, 5, {"width": 7, "height": 5}), (dense[:0], 0, 1, {})):
        for binary in (True, False):
            path = str(tmp_path / f"c_{w}_{h}_{int(binary)}.pcd")
            pcdio.write_pcd(path, rec, binary=binary, **kw)
            blob = open(path, "rb").read()
            lines = [ln.format(w=w, h=h, n=w * h, data="binary" if binary else "ascii") for ln in PCD_LINES]
            head = ("\n".join(lines) + "\n").encode()
            assert blob.startswith(head), blob[:300]
            if binary:
                assert blob[len(head):] == rec.tobytes()
            else:
                assert blob.count(b"\n") == len(lines) + rec.size
            got, gw, gh = pcdio.read_pcd(path)
            assert (gw, gh) == (w, h) and got.dtype == CC.POINT
            assert got.tobytes() == rec.tobytes(), (w, h, binary)
    # raw bytes [k, 16] (what points_device().cpu().numpy() is) are taken as records
    path = str(tmp_path / "raw.pcd")
    pcdio.write_pcd(path, dense.view(np.uint8).reshape(-1, 16))
    assert pcdio.read_pcd(path)[0].tobytes() == dense.tobytes()
    with pytest.raises(ValueError):
        pcdio.write_pcd(path, dense, width=dense.size - 1, height=1)
    with pytest.raises(ValueError):
        pcdio.write_pcd(path, np.zeros(5, np.float32))


@pytest.mark.timeout(300)
def test_cpp_writer_writes_the_bytes_of_the_python_writer(tmp_path):
    from kinectdepthmapenhancement_amd import pcdio
    dense = _sample_records()
    org = CC.statement(CC.clouds(78, 1, 5, 7)[0], CC.bgr_images(78, 1, 5, 7)[0], organized=True)
    (tmp_path / "dense.bin").write_bytes(dense.tobytes())
    (tmp_path / "org.bin").write_bytes(org.tobytes())
    src = tmp_path / "writer.cpp"
    src.write_text(r"""
#include "kde/pcd_io.hpp"
#include <cstdio>
#include <cstdlib>
#include <vector>
// writer <records.bin> <out.pcd> <binary> [W H]
int main(int argc, char** argv)
{
    if (argc < 4) return 2;
    std::FILE* f = std::fopen(argv[1], "rb");
    if (!f) return 2;
    std::vector<kde_cloud_point> rec;
    kde_cloud_point p;
    while (std::fread(&p, sizeof p, 1, f) == 1) rec.push_back(p);
    std::fclose(f);
    const bool binary = std::atoi(argv[3]) != 0;
    const bool ok = argc > 5 ? kde::writePcd(argv[2], rec.data(), rec.size(), (size_t)std::atoi(argv[4]), (size_t)std::atoi(argv[5]), binary)
                             : kde::writePcd(argv[2], rec.data(), rec.size(), binary);
    return ok ? 0 : 1;
}
""")
    exe = str(tmp_path / "writer")
    subprocess.check_call(["c++", "-std=c++17", "-O1", "-I", os.path.join(ROOT, "include"), "-o", exe, str(src)], timeout=200)
    for name, rec, dims, kw in (("dense", dense, [], {}), ("org", org, ["7", "5"], {"width": 7, "height": 5})):
        for binary in (1, 0):
            cpp, py = str(tmp_path / f"{name}_{binary}_cpp.pcd"), str(tmp_path / f"{name}_{binary}_py.pcd")
            subprocess.check_call([exe, str(tmp_path / f"{name}.bin"), cpp, str(binary)] + dims, timeout=60)
            pcdio.write_pcd(py, rec, binary=bool(binary), **kw)
            assert open(cpp, "rb").read() == open(py, "rb").read(), (name, binary)
    # a size that does not fill the grid is refused by both
    assert subprocess.run([exe, str(tmp_path / "org.bin"), str(tmp_path / "bad.pcd"), "1", "7", "4"], timeout=60).returncode == 1


def test_statement_on_a_case_worked_out_by_hand():
    pts, bgr, dense, org = CC.hand_case()
    got = CC.statement(pts, bgr)
    assert got.dtype == CC.POINT and got.tobytes() == dense.tobytes(), got
    assert CC.count(pts) == 2
    assert CC.statement(pts, bgr, organized=True).tobytes() == org.tobytes()
    # main.cpp:230: -z / 1000, and the colour as PCL packs it
    assert got["z"][0] == np.float32(-3.0) and got["rgb"][0] == (30 << 16) | (20 << 8) | 10
    # other parameters: z kept, another divisor, a range that admits other pixels
    alt = CC.statement(pts, bgr, z_min=49.0, z_max=3000.0, divisor=2.0, negate_z=False)
    assert alt["z"].tolist() == [25.0, 25.25] and alt["x"].tolist() == [2.5, -125.0] and alt["rgb"].tolist() == [0x030201, 0x8000FF]
    # the validity rule at its edges, in every generated case
    z = CC.special_z()
    p = np.zeros((z.size, 3), np.float32)
    p[:, 2] = z
    assert CC.valid_mask(p).tolist() == CC.SPECIAL_VALID.tolist()
    for seed, (h, w) in enumerate(((5, 7), (48, 64), (35, 67))):
        c = CC.clouds(seed, 2, h, w)
        for f in range(2):
            zs = c[f].reshape(-1, 3)[:, 2]
            for v in z:
                assert (np.isnan(zs).any() if np.isnan(v) else (zs.view(np.uint32) == v.view(np.uint32)).any()), (h, w, f, v)
            frac = CC.count(c[f]) / (h * w)
            assert 0.4 < frac < 0.9, frac
            x = c[f].reshape(-1, 3)[CC.valid_mask(c[f].reshape(-1, 3))]
            assert np.isnan(x[:, 0]).any() and np.isinf(x[:, 1]).any() and (x[:, 0].view(np.uint32) == 0x80000000).any()
