"""OrganizedMesh (kde_mesh_*) at the ABI level, without a GPU: declared, exported and bound; the typed handle; every refusal
that precedes a HIP call, with its message; the build call on a host without a device; the C++ class and the PLY writer
compile; the records' sizes; the PLY files of both writers and their round trip.

On a host without a device kde_mesh_create makes the object without buffers, so the refusals that need a handle are checked
here as well."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import cloud_cases as CC
import mesh_cases as MC
from conftest import ROOT

HEADER = os.path.join(ROOT, "include", "kde_hip.h")
FUNCS = ("kde_mesh_default_params", "kde_mesh_create", "kde_mesh_destroy", "kde_mesh_set_camera", "kde_mesh_build_batch",
         "kde_mesh_vertices_device", "kde_mesh_triangles_device", "kde_mesh_counts_device", "kde_mesh_tri_counts_device",
         "kde_mesh_counts_host", "kde_mesh_tri_counts_host", "kde_mesh_vertices_host", "kde_mesh_triangles_host")
PLY_LINES = ["ply", "format {fmt} 1.0", "element vertex {nv}", "property float x", "property float y", "property float z",
             "property uchar red", "property uchar green", "property uchar blue", "element face {nf}",
             "property list uchar int vertex_indices", "end_header"]


@pytest.fixture(scope="module")
def native():
    from kinectdepthmapenhancement_amd import _native
    if not os.path.exists(_native.LIB_PATH):
        _native.build()
    return _native


def _hipcc():
    return os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "bin", "hipcc")


def _params(native, **over):
    p = native.MeshParams()
    assert native.lib().kde_mesh_default_params(ctypes.byref(p)) == native.KDE_OK
    for k, v in over.items():
        setattr(p, k, v)
    return p


@pytest.mark.timeout(120)
def test_declared_exported_and_bound(native):
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    for name in FUNCS:
        assert re.search(r"\bint\s+" + name + r"\s*\(", text), name
    assert "#define KDE_ABI_VERSION 1" in text                     # the new entry points only add to the ABI
    lib = ctypes.CDLL(native.LIB_PATH)
    assert all(hasattr(lib, n) for n in FUNCS)
    assert set(FUNCS) == {n for n in native.SIGNATURES if n.startswith("kde_mesh_")}
    assert ctypes.sizeof(native.MeshTriangle) == 12 and ctypes.sizeof(native.MeshParams) == 32
    assert (native.KDE_MESH_DIAG_AD, native.KDE_MESH_DIAG_BC, native.KDE_MESH_DIAG_ADAPTIVE) == (0, 1, 2)
    assert re.search(r"KDE_MESH_DIAG_AD = 0, KDE_MESH_DIAG_BC = 1, KDE_MESH_DIAG_ADAPTIVE = 2", text)
    # none of them is picked up by the enumeration of tools/abi_refusals.py, whose record is frozen
    frozen = (ctypes.c_void_p, ctypes.POINTER(ctypes.c_void_p))
    assert [n for n in FUNCS if native.SIGNATURES[n][1][0] in frozen] == []
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "abi_refusals.py")], capture_output=True, text=True, timeout=100)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "kde_mesh" not in r.stdout
    # every entry point says in the header what it stands in for
    raw = open(HEADER).read()
    for name in FUNCS:
        at = raw.index("int " + name + "(")
        assert "main.cpp:211-300" in raw[raw.rindex("/*", 0, at):at] or "main.cpp:211-300" in raw[at:raw.index("\n", at)], name
    p = _params(native)
    assert (p.z_min, p.z_max, p.divisor, p.negate_z) == (50.0, 15000.0, 1000.0, 1)
    assert (p.max_diff, p.rel_diff, p.diagonal, p.flip_winding) == (10.0, np.float32(0.02), native.KDE_MESH_DIAG_ADAPTIVE, 0)
    s = native.SpeckleParams()                                     # the link is the speckle filter's
    assert native.lib().kde_speckle_default_params(ctypes.byref(s)) == native.KDE_OK
    assert (s.max_diff, s.rel_diff) == (p.max_diff, p.rel_diff)


@pytest.mark.timeout(120)
def test_the_typed_handle_refuses_a_plain_void_pointer(native):
    lib = native.lib()
    assert issubclass(native.MeshHandle, ctypes.c_void_p) and native.MeshHandle is not ctypes.c_void_p
    assert native.MeshHandle is not native.CloudHandle
    assert lib.kde_mesh_destroy(None) == native.KDE_OK
    assert lib.kde_mesh_destroy(native.MeshHandle()) == native.KDE_OK
    out = ctypes.c_void_p()
    for plain in (ctypes.c_void_p(), ctypes.c_void_p(16)):
        with pytest.raises(ctypes.ArgumentError):
            lib.kde_mesh_destroy(plain)
        with pytest.raises(ctypes.ArgumentError):
            lib.kde_mesh_set_camera(plain, None)
        with pytest.raises(ctypes.ArgumentError):
            lib.kde_mesh_build_batch(plain, 1, None, None, 1, None, None, None)
        for name in ("kde_mesh_vertices_device", "kde_mesh_triangles_device", "kde_mesh_counts_device", "kde_mesh_tri_counts_device"):
            with pytest.raises(ctypes.ArgumentError):
                getattr(lib, name)(plain, ctypes.byref(out))
        for name in ("kde_mesh_counts_host", "kde_mesh_tri_counts_host"):
            with pytest.raises(ctypes.ArgumentError):
                getattr(lib, name)(plain, None, ctypes.byref(out))
        for name in ("kde_mesh_vertices_host", "kde_mesh_triangles_host"):
            with pytest.raises(ctypes.ArgumentError):
                getattr(lib, name)(plain, None, ctypes.byref(out), ctypes.byref(out))
        with pytest.raises(ctypes.ArgumentError):
            lib.kde_mesh_create(ctypes.byref(plain), 8, 8, 1, None)
    with pytest.raises(ctypes.ArgumentError):
        lib.kde_mesh_destroy(native.CloudHandle())                 # another typed handle is refused as well
    from kinectdepthmapenhancement_amd import filters, plyio
    assert filters.OrganizedMesh._handle_type is native.MeshHandle
    assert filters.OrganizedMesh.POINT_DTYPE == CC.POINT and filters.OrganizedMesh.TRIANGLE_DTYPE == MC.TRIANGLE == plyio.TRIANGLE_DTYPE
    assert (filters.OrganizedMesh.DIAG_AD, filters.OrganizedMesh.DIAG_BC, filters.OrganizedMesh.DIAG_ADAPTIVE) == (0, 1, 2)


@pytest.mark.timeout(120)
def test_refusals_name_their_function_and_their_reason(native):
    lib = native.lib()
    INVALID = native.KDE_ERR_INVALID
    Src = native.Error3dSource
    P, DF, DU = native.KDE_SRC_POINTS_F32, native.KDE_SRC_DEPTH_F32, native.KDE_SRC_DEPTH_U16
    nan, inf = float("nan"), float("inf")

    def refused(name, rc, *words):
        msg = lib.kde_last_error_string()
        assert rc == INVALID, (name, rc, msg)
        assert name.encode() in msg, (name, msg)
        for w in words:
            assert w.encode() in msg, (name, w, msg)

    out = native.MeshHandle()
    create = lambda w, h, b, p: lib.kde_mesh_create(ctypes.byref(out), w, h, b, ctypes.byref(p) if p is not None else None)
    refused("kde_mesh_default_params", lib.kde_mesh_default_params(None), "null")
    refused("kde_mesh_create", lib.kde_mesh_create(None, 8, 8, 1, None), "null out")
    refused("kde_mesh_create", create(0, 8, 1, None), "bad size")
    refused("kde_mesh_create", create(8, -1, 1, None), "bad size")
    refused("kde_mesh_create", create(8, 8, 0, None), "max_batch")
    refused("kde_mesh_create", create(8, 8, 65536, None), "max_batch")
    for w, h in ((1, 8), (8, 1), (1, 1)):                                          # a quad has two rows and two columns
        refused("kde_mesh_create", create(w, h, 1, None), ">= 2", f"width={w}", f"height={h}")
    for zmin, zmax in ((nan, 100.0), (50.0, nan), (50.0, inf), (-inf, 100.0), (100.0, 100.0), (200.0, 100.0)):   # the cloud's
        refused("kde_mesh_create", create(8, 8, 1, _params(native, z_min=zmin, z_max=zmax)), "z_min", "z_max")
    for divisor in (nan, inf, -inf, 0.0, -0.0, -1000.0):
        refused("kde_mesh_create", create(8, 8, 1, _params(native, divisor=divisor)), "divisor")
    for bad in (nan, inf, -inf, -1.0, -1e-30):
        refused("kde_mesh_create", create(8, 8, 1, _params(native, max_diff=bad)), "max_diff", ">= 0")
        refused("kde_mesh_create", create(8, 8, 1, _params(native, rel_diff=bad)), "rel_diff", ">= 0")
    for bad in (-1, 3, 2 ** 31 - 1):
        refused("kde_mesh_create", create(8, 8, 1, _params(native, diagonal=bad)), "diagonal", "0..2")
    assert out.value is None
    # null handles and null arguments
    K = (ctypes.c_double * 9)(500, 0, 4, 0, 500, 4, 0, 0, 1)
    src = Src(4096, P)
    p, q = ctypes.c_void_p(), ctypes.c_void_p()
    refused("kde_mesh_set_camera", lib.kde_mesh_set_camera(None, K), "null")
    refused("kde_mesh_build_batch", lib.kde_mesh_build_batch(None, 1, ctypes.byref(src), 8192, 1, None, None, None), "null")
    for name in ("kde_mesh_vertices_device", "kde_mesh_triangles_device", "kde_mesh_counts_device", "kde_mesh_tri_counts_device"):
        refused(name, getattr(lib, name)(None, ctypes.byref(p)), "null")
    for name in ("kde_mesh_counts_host", "kde_mesh_tri_counts_host"):
        refused(name, getattr(lib, name)(None, None, ctypes.byref(p)), "null")
    for name in ("kde_mesh_vertices_host", "kde_mesh_triangles_host"):
        refused(name, getattr(lib, name)(None, None, ctypes.byref(p), ctypes.byref(q)), "null")
    assert lib.kde_mesh_destroy(None) == native.KDE_OK

    # an object for 4 frames, the smallest frame, the largest thresholds and every flag set, zero thresholds: all accepted
    for ok in (_params(native, max_diff=0.0, rel_diff=0.0), _params(native, max_diff=3e38, rel_diff=3e38, diagonal=0, flip_winding=7, negate_z=0)):
        h = native.MeshHandle()
        assert lib.kde_mesh_create(ctypes.byref(h), 2, 2, 1, ctypes.byref(ok)) == native.KDE_OK, lib.kde_last_error_string()
        assert lib.kde_mesh_destroy(h) == native.KDE_OK
    h = native.MeshHandle()
    assert create is not None and lib.kde_mesh_create(ctypes.byref(h), 8, 6, 4, ctypes.byref(_params(native, diagonal=1))) == native.KDE_OK, \
        lib.kde_last_error_string()
    assert h.value
    try:
        refused("kde_mesh_set_camera", lib.kde_mesh_set_camera(h, None), "null")
        for name in ("kde_mesh_vertices_device", "kde_mesh_triangles_device", "kde_mesh_counts_device", "kde_mesh_tri_counts_device"):
            refused(name, getattr(lib, name)(h, None), "null")
            refused(name, getattr(lib, name)(h, ctypes.byref(p)), "kde_mesh_build_batch was not called")    # results before any call
        for name in ("kde_mesh_counts_host", "kde_mesh_tri_counts_host"):
            refused(name, getattr(lib, name)(h, None, None), "null")
            refused(name, getattr(lib, name)(h, None, ctypes.byref(p)), "kde_mesh_build_batch was not called")
        for name in ("kde_mesh_vertices_host", "kde_mesh_triangles_host"):
            refused(name, getattr(lib, name)(h, None, None, ctypes.byref(q)), "null")
            refused(name, getattr(lib, name)(h, None, ctypes.byref(p), None), "null")
            refused(name, getattr(lib, name)(h, None, ctypes.byref(p), ctypes.byref(q)), "kde_mesh_build_batch was not called")

        def call(n, s, bgr, frames, vout=None, tout=None):
            return lib.kde_mesh_build_batch(h, n, ctypes.byref(s) if s is not None else None, bgr, frames, vout, tout, None)

        who = "kde_mesh_build_batch"
        refused(who, call(2, None, 8192, 1), "null")                                        # null source
        refused(who, call(2, src, None, 1), "null")                                         # null colour image
        refused(who, call(5, src, 8192, 1), "n=5", "max_batch=4")
        refused(who, call(0, src, 8192, 1), "n=0")
        refused(who, call(3, src, 8192, 2), "bgr_frames=2", "n=3")                          # bgr_frames neither 1 nor n
        refused(who, call(3, src, 8192, 0), "bgr_frames=0")
        refused(who, call(3, src, 8192, 4), "bgr_frames=4")
        refused(who, call(2, Src(4096, 3), 8192, 1), "unknown format 3")
        refused(who, call(2, Src(4096, -1), 8192, 1), "unknown format -1")
        refused(who, call(2, Src(None, P), 8192, 1), "null data_dev")
        refused(who, call(2, Src(4098, P), 8192, 1), "not 4-byte aligned")                  # float3 needs 4
        refused(who, call(2, src, 8192, 1, 65544), "vertices_out_dev", "16-byte")           # 8 past a 16-byte boundary
        refused(who, call(2, src, 8192, 1, 65536, 131074), "triangles_out_dev", "4-byte")
        refused(who, call(2, src, 8192, 1, None, 131073), "triangles_out_dev", "4-byte")
        # a depth source before a camera is set, float and uint16
        refused(who, call(2, Src(4096, DF), 8192, 2), "kde_mesh_set_camera")
        refused(who, call(2, Src(4096, DU), 8192, 2), "kde_mesh_set_camera")
        assert lib.kde_mesh_set_camera(h, K) == native.KDE_OK
        refused(who, call(2, Src(4098, DF), 8192, 1), "not 4-byte aligned")
        refused(who, call(2, Src(4097, DU), 8192, 1), "not 2-byte aligned")
        # still no call went through
        refused("kde_mesh_triangles_device", lib.kde_mesh_triangles_device(h, ctypes.byref(p)), "was not called")
    finally:
        assert lib.kde_mesh_destroy(h) == native.KDE_OK


@pytest.mark.timeout(300)
def test_a_host_without_a_device_creates_the_object_and_refuses_the_build():
    """in a child that sees no device: create succeeds without buffers, every validation still answers, and a build call
    that passes them answers KDE_ERR_HIP -- it is not a crash and not a silent success"""
    code = r"""
import ctypes as C, json, sys
sys.path.insert(0, %r)
from kinectdepthmapenhancement_amd import _native as N
lib = N.lib()
n = C.c_int(-1)
rc_count = lib.kde_device_count(C.byref(n))
h = N.MeshHandle()
out = {"devices": n.value, "rc_count": rc_count}
out["create"] = lib.kde_mesh_create(C.byref(h), 8, 6, 2, None)
out["handle"] = bool(h.value)
src = N.Error3dSource(4096, N.KDE_SRC_POINTS_F32)
out["refused"] = lib.kde_mesh_build_batch(h, 3, C.byref(src), 8192, 1, None, None, None)
if n.value <= 0:                    # with a device in sight these pointers must not reach a kernel: the parent fails on "devices"
    out["build"] = lib.kde_mesh_build_batch(h, 2, C.byref(src), 8192, 1, None, None, None)
    out["message"] = lib.kde_last_error_string().decode()
p = C.c_void_p()
out["after"] = lib.kde_mesh_counts_device(h, C.byref(p))
out["destroy"] = lib.kde_mesh_destroy(h)
print(json.dumps(out))
""" % ROOT
    env = dict(os.environ, HIP_VISIBLE_DEVICES="", ROCR_VISIBLE_DEVICES="")
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=280, env=env)
    assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
    import json
    from kinectdepthmapenhancement_amd import _native as N
    got = json.loads(r.stdout.strip().splitlines()[-1])
    assert got["devices"] <= 0, got
    assert got["create"] == N.KDE_OK and got["handle"] and got["destroy"] == N.KDE_OK, got
    assert got["refused"] == N.KDE_ERR_INVALID, got
    assert got["build"] == N.KDE_ERR_HIP and "kde_mesh_build_batch" in got["message"] and "without a device" in got["message"], got
    assert got["after"] == N.KDE_ERR_INVALID, got                  # the refused build is no build


@pytest.mark.timeout(300)
def test_cpp_headers_compile_and_the_records_have_their_sizes(tmp_path):
    src = tmp_path / "mesh_user.cpp"
    src.write_text(r"""
#include "kde/kde.hpp"
#include "kde/ply_io.hpp"
#include <cstdint>
static_assert(sizeof(kde_mesh_triangle) == 12, "kde_mesh_triangle must be 12 bytes");
static_assert(sizeof(kde_mesh_params) == 32, "kde_mesh_params: five floats and three ints");
static_assert(KDE_MESH_DIAG_AD == 0 && KDE_MESH_DIAG_BC == 1 && KDE_MESH_DIAG_ADAPTIVE == 2, "the cuts");
int main()
{
    kde::OrganizedMesh one(640, 480);                             // one frame, the defaults
    kde_mesh_params p = kde::OrganizedMesh::defaultParams();
    p.diagonal = KDE_MESH_DIAG_BC;
    p.flip_winding = 1;
    kde::OrganizedMesh mesh(640, 480, 64, p);                     // RAII over kde_mesh_create / _destroy
    const double K[9] = {575.8, 0, 320, 0, 575.8, 240, 0, 0, 1};
    const kde::Mat33d M{{575.8, 0, 320, 0, 575.8, 240, 0, 0, 1}};
    mesh.setCamera(K);
    mesh.setCamera(M);
    float3* pts = nullptr;
    float* depth = nullptr;
    uint16_t* depth16 = nullptr;
    uint8_t* bgr = nullptr;
    kde_cloud_point* vout = nullptr;
    kde_mesh_triangle* tout = nullptr;
    mesh.build(64, kde::MeanError3D::source(pts), bgr);
    mesh.build(64, kde::MeanError3D::source(depth), bgr, 64);
    mesh.build(64, kde::MeanError3D::source(depth16), bgr, 64, vout, tout);
    mesh.setStream(nullptr);
    const uint64_t *voff = nullptr, *toff = nullptr;
    const kde_cloud_point* v = mesh.vertices_Host(&voff);
    const kde_mesh_triangle* t = mesh.triangles_Host(&toff);
    const uint32_t* counts = mesh.counts_Host();
    const uint32_t* tris = mesh.triCounts_Host();
    kde_cloud_point* vdev = mesh.vertices_Device();
    kde_mesh_triangle* tdev = mesh.triangles_Device();
    uint32_t *cdev = mesh.counts_Device(), *tcdev = mesh.triCounts_Device();
    kde_mesh* h = mesh.handle();
    const bool ok = kde::writePly("a.ply", v, counts[0], t, tris[0]) && kde::writePly("b.ply", v + voff[1], counts[1], t + toff[1], tris[1], false);
    return (int)ok + (vdev != nullptr) + (tdev != nullptr) + (cdev != nullptr) + (tcdev != nullptr) + (h != nullptr) +
           (int)kde::plyHeader(1, 1, true).size();
}
""")
    r = subprocess.run([_hipcc(), "-std=c++17", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    size = tmp_path / "size.c"
    size.write_text('#include "kde_hip.h"\n#include <stdio.h>\nint main(void) { printf("%zu %zu %zu\\n", sizeof(kde_mesh_triangle), '
                    '_Alignof(kde_mesh_triangle), sizeof(kde_mesh_params)); return 0; }\n')
    exe = str(tmp_path / "size")
    subprocess.check_call(["cc", "-std=c11", "-I", os.path.join(ROOT, "include"), "-o", exe, str(size)], timeout=120)
    assert subprocess.run([exe], capture_output=True, text=True, check=True, timeout=60).stdout.split() == ["12", "4", "32"]


def _sample_mesh():
    """a mesh with everything a file has to carry: -0, a denormal, the extremes, an inf and a NaN among the coordinates,
    nine-digit fractions, every colour byte, the first and the last vertex in a face"""
    w, h = 7, 5
    z = MC.salt(w, h)
    pts = MC.as_points(z, CC.camera(w, h))
    ok = np.flatnonzero(MC.valid_mask(z).reshape(-1))
    flat = pts.reshape(-1, 3)
    flat[ok[1], 0], flat[ok[2], 1], flat[ok[3], 0] = -0.0, np.inf, np.nan
    flat[ok[4], :2] = (np.float32(1e-42), np.float32(-3.4028235e38))
    rec = MC.vertices(pts, CC.bgr_images(77, 1, h, w)[0])
    tri = MC.triangles(z)
    assert rec.size == ok.size and tri.shape[0] >= 6 and tri.min() == 0 and tri.max() == rec.size - 1
    assert np.isnan(rec["x"]).any() and np.isinf(rec["y"]).any() and (rec["x"].view(np.uint32) == 0x80000000).any()
    return rec, tri


@pytest.mark.timeout(120)
def test_ply_round_trip_and_header(tmp_path):
    from kinectdepthmapenhancement_amd import plyio
    rec, tri = _sample_mesh()
    for v, t in ((rec, tri), (rec, tri[:0]), (rec[:0], tri[:0])):
        for binary in (True, False):
            path = str(tmp_path / f"m_{v.size}_{t.shape[0]}_{int(binary)}.ply")
            plyio.write_ply(path, v, t, binary=binary)
            blob = open(path, "rb").read()
            lines = [ln.format(fmt="binary_little_endian" if binary else "ascii", nv=v.size, nf=t.shape[0]) for ln in PLY_LINES]
            head = ("\n".join(lines) + "\n").encode()
            assert blob.startswith(head), blob[:400]
            if binary:
                assert len(blob) == len(head) + 15 * v.size + 13 * t.shape[0]
                if v.size:
                    assert blob[len(head):len(head) + 12] == v[:1].tobytes()[:12]
                    c = int(v["rgb"][0])
                    assert blob[len(head) + 12:len(head) + 15] == bytes([(c >> 16) & 255, (c >> 8) & 255, c & 255])
                if t.shape[0]:
                    assert blob[len(head) + 15 * v.size:][:13] == b"\x03" + t[:1].astype("<i4").tobytes()
            else:
                assert blob.count(b"\n") == len(lines) + v.size + t.shape[0]
            gv, gt = plyio.read_ply(path)
            assert gv.dtype == CC.POINT and gt.dtype == np.uint32 and gt.shape == (t.shape[0], 3)
            assert gv.tobytes() == v.tobytes() and gt.tobytes() == t.tobytes(), (v.size, t.shape, binary)
    # the records as the device getters hand them out: raw bytes [k, 16] and [m, 12], and TRIANGLE_DTYPE records
    path = str(tmp_path / "raw.ply")
    plyio.write_ply(path, rec.view(np.uint8).reshape(-1, 16), MC.records(tri).view(np.uint8).reshape(-1, 12))
    gv, gt = plyio.read_ply(path)
    assert gv.tobytes() == rec.tobytes() and gt.tobytes() == tri.tobytes()
    plyio.write_ply(path, rec, MC.records(tri))
    assert plyio.read_ply(path)[1].tobytes() == tri.tobytes()
    with pytest.raises(ValueError):
        plyio.write_ply(path, rec[:-1], tri)                       # an index without its vertex
    with pytest.raises(ValueError):
        plyio.write_ply(path, rec, np.zeros((2, 4), np.uint32))
    with pytest.raises(ValueError):
        plyio.write_ply(path, np.zeros(5, np.float32), tri)


@pytest.mark.timeout(300)
def test_cpp_writer_writes_the_bytes_of_the_python_writer(tmp_path):
    from kinectdepthmapenhancement_amd import plyio
    rec, tri = _sample_mesh()
    (tmp_path / "v.bin").write_bytes(rec.tobytes())
    (tmp_path / "t.bin").write_bytes(MC.records(tri).tobytes())
    (tmp_path / "none.bin").write_bytes(b"")
    src = tmp_path / "writer.cpp"
    src.write_text(r"""
#include "kde/ply_io.hpp"
#include <cstdio>
#include <cstdlib>
#include <vector>
template <class T>
static std::vector<T> slurp(const char* path)
{
    std::vector<T> out;
    std::FILE* f = std::fopen(path, "rb");
    if (!f) std::exit(2);
    T r;
    while (std::fread(&r, sizeof r, 1, f) == 1) out.push_back(r);
    std::fclose(f);
    return out;
}
// writer <vertices.bin> <triangles.bin> <out.ply> <binary>
int main(int argc, char** argv)
{
    if (argc < 5) return 2;
    const std::vector<kde_cloud_point> v = slurp<kde_cloud_point>(argv[1]);
    const std::vector<kde_mesh_triangle> t = slurp<kde_mesh_triangle>(argv[2]);
    return kde::writePly(argv[3], v.data(), v.size(), t.data(), t.size(), std::atoi(argv[4]) != 0) ? 0 : 1;
}
""")
    exe = str(tmp_path / "writer")
    subprocess.check_call(["c++", "-std=c++17", "-O1", "-I", os.path.join(ROOT, "include"), "-o", exe, str(src)], timeout=200)
    for name, vfile, tfile, v, t in (("mesh", "v.bin", "t.bin", rec, tri), ("points", "v.bin", "none.bin", rec, tri[:0]),
                                     ("empty", "none.bin", "none.bin", rec[:0], tri[:0])):
        for binary in (1, 0):
            cpp, py = str(tmp_path / f"{name}_{binary}_cpp.ply"), str(tmp_path / f"{name}_{binary}_py.ply")
            subprocess.check_call([exe, str(tmp_path / vfile), str(tmp_path / tfile), cpp, str(binary)], timeout=60)
            plyio.write_ply(py, v, t, binary=bool(binary))
            assert open(cpp, "rb").read() == open(py, "rb").read(), (name, binary)
    # an index without its vertex is refused by both
    assert subprocess.run([exe, str(tmp_path / "none.bin"), str(tmp_path / "t.bin"), str(tmp_path / "bad.ply"), "1"], timeout=60).returncode == 1
