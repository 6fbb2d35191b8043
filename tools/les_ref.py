"""ctypes front-end of tools/les_ref.c, the CPU restatement of LabelEquivalenceSeg::labelImage.

TEST INFRASTRUCTURE ONLY: imported by tests/ and tools/bench_les.py, never by the product package.
Arrays are numpy: normals / centers float32 [n_clusters, 3], labels int32 [H, W].
"""
from __future__ import annotations

import ctypes as C
import os
import subprocess

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_SRC = os.path.join(_HERE, "les_ref.c")
LIB_PATH = os.path.join(_HERE, "libles_ref.so")

ITERATIONS = 10                                                  # LabelEquivalenceSeg.cu:235
MAX_ANGLE = np.float32(3.141592653) / np.float32(8.0)            # :40
MAX_PLANE_DISTANCE = np.float32(150.0)                           # :42


class Float4(C.Structure):
    _fields_ = [("x", C.c_float), ("y", C.c_float), ("z", C.c_float), ("w", C.c_float)]


_lib = None


def build() -> str:
    if not os.path.exists(LIB_PATH) or os.path.getmtime(LIB_PATH) < os.path.getmtime(_SRC):
        subprocess.check_call(["make", "-C", _HERE, "-s", "libles_ref.so"])
    return LIB_PATH


def lib() -> C.CDLL:
    global _lib
    if _lib is None:
        build()
        l = C.CDLL(LIB_PATH)
        vp, i, f = C.c_void_p, C.c_int, C.c_float
        l.les_acos_threshold.restype = f
        l.les_acos_threshold.argtypes = [f]
        l.les_comp_normal.argtypes = [Float4, Float4, f, f]
        l.les_init_label.argtypes = [i, i, i, vp, vp, vp, vp, vp, vp]
        l.les_scan.argtypes = [i, i, vp, vp, vp, f, f, vp]
        l.les_analysis.argtypes = [i, i, vp, vp, vp, vp]
        l.les_count_and_nd.argtypes = [i, i, i, vp, vp, vp, vp, vp, vp, vp]
        l.les_label_image.argtypes = [i, i, i, vp, vp, vp, vp, i, f, f, vp, vp, vp, vp, vp, vp]
        _lib = l
    return _lib


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def _g(v) -> float:
    return float(np.float32(v))


def acos_threshold(max_angle=MAX_ANGLE) -> np.float32:
    return np.float32(lib().les_acos_threshold(_g(max_angle)))


def comp_normal(a, b, thr, max_dist=MAX_PLANE_DISTANCE) -> bool:
    return bool(lib().les_comp_normal(Float4(*[_g(t) for t in a]), Float4(*[_g(t) for t in b]), _g(thr), _g(max_dist)))


def prep(normals, labels, centers):
    normals = np.ascontiguousarray(normals, np.float32)
    centers = np.ascontiguousarray(centers, np.float32)
    labels = np.ascontiguousarray(labels, np.int32)
    assert normals.ndim == 2 and normals.shape[1] == 3 and centers.shape == normals.shape and labels.ndim == 2
    return normals, labels, centers


def label_image(normals, labels, centers, iterations=ITERATIONS, max_angle=MAX_ANGLE, max_plane_distance=MAX_PLANE_DISTANCE):
    """labelImage on a fresh object: dict of input_nd [H, W, 4], merged_label [H, W] int32, merged_nd [H, W, 4],
    size [n_clusters] int32, variance [n_clusters] (both indexed by merged label) and changed [iterations] (pixels whose
    merged label each round changed)"""
    normals, labels, centers = prep(normals, labels, centers)
    H, W = labels.shape
    nc = normals.shape[0]
    out = {"input_nd": np.zeros((H, W, 4), np.float32), "merged_label": np.zeros((H, W), np.int32),
           "merged_nd": np.zeros((H, W, 4), np.float32), "size": np.zeros(nc, np.int32), "variance": np.zeros(nc, np.float32),
           "changed": np.zeros(max(iterations, 1), np.int32)}
    rc = lib().les_label_image(W, H, nc, _p(normals), _p(labels), _p(centers), None, int(iterations), _g(max_angle),
                               _g(max_plane_distance), _p(out["input_nd"]), _p(out["merged_label"]), _p(out["merged_nd"]),
                               _p(out["size"]), _p(out["variance"]), _p(out["changed"]))
    assert rc == 0, f"les_label_image returned {rc}"
    out["changed"] = out["changed"][:max(iterations, 0)]
    return out
