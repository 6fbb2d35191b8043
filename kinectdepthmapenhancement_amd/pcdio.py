"""PCD v0.7 files of XYZRGB clouds: what pcl::io::savePCDFile writes for a pcl::PointCloud<pcl::PointXYZRGB> holding the
records of filters.PointCloudXYZRGB (main.cpp:211-300 builds such clouds).  Pure numpy; include/kde/pcd_io.hpp is the same
writer in C++ and produces the same bytes.

The record is 16 bytes, (x, y, z: float32, rgb: uint32 = (r << 16) | (g << 8) | b), and the header

    # .PCD v0.7 - Point Cloud Data file format
    VERSION 0.7
    FIELDS x y z rgb
    SIZE 4 4 4 4
    TYPE F F F U
    COUNT 1 1 1 1
    WIDTH <w>
    HEIGHT <h>
    VIEWPOINT 0 0 0 1 0 0 0
    POINTS <w * h>
    DATA binary | ascii

with (w, h) = (count, 1) for a dense cloud and (W, H) for an organised one.  DATA binary is followed by the record array as
it is in memory (little endian); DATA ascii by one line per point, `x y z rgb`, the floats with nine significant digits
(which identify a float32) and a NaN as `nan` (read back as the quiet NaN 0x7fc00000, the one organised mode writes).
"""
from __future__ import annotations

import numpy as np

POINT_DTYPE = np.dtype([("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("rgb", "<u4")])


def header(width: int, height: int, binary: bool) -> str:
    return ("# .PCD v0.7 - Point Cloud Data file format\n"
            "VERSION 0.7\n"
            "FIELDS x y z rgb\n"
            "SIZE 4 4 4 4\n"
            "TYPE F F F U\n"
            "COUNT 1 1 1 1\n"
            f"WIDTH {width}\n"
            f"HEIGHT {height}\n"
            "VIEWPOINT 0 0 0 1 0 0 0\n"
            f"POINTS {width * height}\n"
            f"DATA {'binary' if binary else 'ascii'}\n")


def _records(points) -> np.ndarray:
    a = np.ascontiguousarray(points)
    if a.dtype != POINT_DTYPE:
        raw = a.reshape(-1).view(np.uint8)
        if a.dtype.itemsize != 16 and (a.ndim == 0 or a.shape[-1] * a.dtype.itemsize != 16):
            raise ValueError(f"points: expected 16-byte records {POINT_DTYPE}, got {a.dtype} {a.shape}")
        a = raw.view(POINT_DTYPE)
    return a.reshape(-1)


def _float_text(v: float) -> str:
    return "nan" if v != v else "%.9g" % v


def write_pcd(path, points, width=None, height: int = 1, binary: bool = True) -> None:
    """points: records of POINT_DTYPE (or raw bytes [..., 16]).  width None: a dense cloud, WIDTH = the number of points and
    HEIGHT = 1; width = W, height = H: an organised cloud of W * H points."""
    rec = _records(points)
    if width is None:
        if height != 1:
            raise ValueError("height without width")
        width = rec.size
    if width < 0 or height < 1 or width * height != rec.size:
        raise ValueError(f"{rec.size} points do not fill WIDTH {width} x HEIGHT {height}")
    with open(path, "wb") as f:
        f.write(header(int(width), int(height), binary).encode("ascii"))
        if binary:
            f.write(rec.tobytes())
        else:
            x, y, z, rgb = rec["x"].tolist(), rec["y"].tolist(), rec["z"].tolist(), rec["rgb"].tolist()
            f.write("".join(f"{_float_text(x[i])} {_float_text(y[i])} {_float_text(z[i])} {rgb[i]}\n" for i in range(rec.size)).encode("ascii"))


def read_pcd(path):
    """(points, width, height) of a file write_pcd (or the C++ writer) made: POINT_DTYPE records, WIDTH and HEIGHT"""
    with open(path, "rb") as f:
        blob = f.read()
    fields = {}
    at = 0
    while True:
        end = blob.index(b"\n", at)
        line = blob[at:end].decode("ascii")
        at = end + 1
        if line.startswith("#"):
            continue
        key, _, value = line.partition(" ")
        fields[key] = value
        if key == "DATA":
            break
    want = {"VERSION": "0.7", "FIELDS": "x y z rgb", "SIZE": "4 4 4 4", "TYPE": "F F F U", "COUNT": "1 1 1 1"}
    for key, value in want.items():
        if fields.get(key) != value:
            raise ValueError(f"{path}: {key} {fields.get(key)!r}, expected {value!r}")
    width, height, n = int(fields["WIDTH"]), int(fields["HEIGHT"]), int(fields["POINTS"])
    if width * height != n:
        raise ValueError(f"{path}: POINTS {n} != WIDTH {width} x HEIGHT {height}")
    if fields["DATA"] == "binary":
        if len(blob) - at != 16 * n:
            raise ValueError(f"{path}: {len(blob) - at} payload bytes for {n} points")
        return np.frombuffer(blob, POINT_DTYPE, n, at).copy(), width, height
    if fields["DATA"] != "ascii":
        raise ValueError(f"{path}: DATA {fields['DATA']!r}")
    rec = np.empty(n, POINT_DTYPE)
    rows = blob[at:].decode("ascii").split("\n")
    if len(rows) != n + 1 or rows[-1] != "":
        raise ValueError(f"{path}: {len(rows) - 1} lines for {n} points")
    for i in range(n):
        x, y, z, rgb = rows[i].split(" ")
        rec[i] = (np.float32(x), np.float32(y), np.float32(z), int(rgb))
    return rec, width, height
