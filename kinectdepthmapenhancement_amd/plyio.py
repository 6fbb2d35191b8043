"""PLY 1.0 files of the meshes of filters.OrganizedMesh: the vertex records (pcdio.POINT_DTYPE: x, y, z float32 and the packed
rgb) and the triangles (three uint32 per face).  Pure numpy; include/kde/ply_io.hpp is the same writer in C++ and produces
the same bytes.

    ply
    format binary_little_endian 1.0 | format ascii 1.0
    element vertex <N>
    property float x
    property float y
    property float z
    property uchar red
    property uchar green
    property uchar blue
    element face <M>
    property list uchar int vertex_indices
    end_header

binary_little_endian: N records of 15 bytes (three float32, then r, g, b), then M records of 13 bytes (the count 3, three
int32).  ascii: one line `x y z r g b` per vertex, the floats with nine significant digits (which identify a float32) and a
NaN as `nan` (read back as the quiet NaN 0x7fc00000), then one line `3 i j k` per face.
"""
from __future__ import annotations

import numpy as np

from .pcdio import POINT_DTYPE, _float_text, _records

TRIANGLE_DTYPE = np.dtype([("v0", "<u4"), ("v1", "<u4"), ("v2", "<u4")])
_VERTEX = np.dtype([("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("red", "u1"), ("green", "u1"), ("blue", "u1")])
_FACE = np.dtype([("n", "u1"), ("v", "<i4", (3,))])
assert _VERTEX.itemsize == 15 and _FACE.itemsize == 13


def header(vertices: int, faces: int, binary: bool) -> str:
    return ("ply\n"
            f"format {'binary_little_endian' if binary else 'ascii'} 1.0\n"
            f"element vertex {vertices}\n"
            "property float x\nproperty float y\nproperty float z\n"
            "property uchar red\nproperty uchar green\nproperty uchar blue\n"
            f"element face {faces}\n"
            "property list uchar int vertex_indices\n"
            "end_header\n")


def _faces(triangles) -> np.ndarray:
    a = np.ascontiguousarray(triangles)
    if a.dtype == TRIANGLE_DTYPE:
        return a.reshape(-1).view(np.uint32).reshape(-1, 3)
    if a.dtype == np.uint8 and a.ndim >= 1 and a.shape[-1] == 12:
        return a.reshape(-1).view(np.uint32).reshape(-1, 3)
    if a.dtype.kind in "iu" and a.dtype.itemsize == 4 and (a.size == 0 or (a.ndim >= 1 and a.shape[-1] == 3)):
        return a.reshape(-1, 3).view(np.uint32)
    raise ValueError(f"triangles: expected 12-byte records {TRIANGLE_DTYPE} or 32-bit integers [M, 3], got {a.dtype} {a.shape}")


def write_ply(path, vertices, triangles, binary: bool = True) -> None:
    """vertices: records of POINT_DTYPE (or raw bytes [..., 16]); triangles: records of TRIANGLE_DTYPE, raw bytes [..., 12] or
    32-bit integers [M, 3], every index < the number of vertices"""
    rec, tri = _records(vertices), _faces(triangles)
    if tri.size and int(tri.max()) >= rec.size:
        raise ValueError(f"triangles: index {int(tri.max())} with {rec.size} vertices")
    rgb = rec["rgb"]
    with open(path, "wb") as f:
        f.write(header(rec.size, tri.shape[0], binary).encode("ascii"))
        if binary:
            v = np.empty(rec.size, _VERTEX)
            v["x"], v["y"], v["z"] = rec["x"], rec["y"], rec["z"]
            v["red"], v["green"], v["blue"] = (rgb >> 16) & 0xFF, (rgb >> 8) & 0xFF, rgb & 0xFF
            t = np.empty(tri.shape[0], _FACE)
            t["n"] = 3
            t["v"] = tri.view(np.int32)
            f.write(v.tobytes())
            f.write(t.tobytes())
        else:
            x, y, z, c = rec["x"].tolist(), rec["y"].tolist(), rec["z"].tolist(), rgb.tolist()
            f.write("".join(f"{_float_text(x[i])} {_float_text(y[i])} {_float_text(z[i])} "
                            f"{(c[i] >> 16) & 255} {(c[i] >> 8) & 255} {c[i] & 255}\n" for i in range(rec.size)).encode("ascii"))
            f.write("".join(f"3 {a} {b} {c}\n" for a, b, c in tri.tolist()).encode("ascii"))


def read_ply(path):
    """(vertices, triangles) of a file write_ply (or the C++ writer) made: POINT_DTYPE records and uint32 [M, 3]"""
    with open(path, "rb") as f:
        blob = f.read()
    end = blob.find(b"end_header\n")
    if not blob.startswith(b"ply\n") or end < 0:
        raise ValueError(f"{path}: not a PLY file")
    at = end + len(b"end_header\n")
    lines = blob[:at].decode("ascii").split("\n")
    try:
        fmt = lines[1]
        nv, nf = int(lines[2].rsplit(" ", 1)[1]), int(lines[9].rsplit(" ", 1)[1])
    except (IndexError, ValueError):
        raise ValueError(f"{path}: not the header write_ply writes") from None
    binary = fmt == "format binary_little_endian 1.0"
    if blob[:at].decode("ascii") != header(nv, nf, binary):
        raise ValueError(f"{path}: not the header write_ply writes")
    rec = np.empty(nv, POINT_DTYPE)
    if binary:
        if len(blob) - at != 15 * nv + 13 * nf:
            raise ValueError(f"{path}: {len(blob) - at} payload bytes for {nv} vertices and {nf} faces")
        v = np.frombuffer(blob, _VERTEX, nv, at)
        t = np.frombuffer(blob, _FACE, nf, at + 15 * nv)
        if nf and not np.all(t["n"] == 3):
            raise ValueError(f"{path}: a face that is no triangle")
        rec["x"], rec["y"], rec["z"] = v["x"], v["y"], v["z"]
        rec["rgb"] = (v["red"].astype(np.uint32) << 16) | (v["green"].astype(np.uint32) << 8) | v["blue"]
        return rec, t["v"].view(np.uint32).reshape(-1, 3).copy()
    rows = blob[at:].decode("ascii").split("\n")
    if len(rows) != nv + nf + 1 or rows[-1] != "":
        raise ValueError(f"{path}: {len(rows) - 1} lines for {nv} vertices and {nf} faces")
    for i in range(nv):
        x, y, z, r, g, b = rows[i].split(" ")
        rec[i] = (np.float32(x), np.float32(y), np.float32(z), (int(r) << 16) | (int(g) << 8) | int(b))
    tri = np.empty((nf, 3), np.uint32)
    for i in range(nf):
        n, a, b, c = rows[nv + i].split(" ")
        if n != "3":
            raise ValueError(f"{path}: a face that is no triangle")
        tri[i] = (int(a), int(b), int(c))
    return rec, tri
