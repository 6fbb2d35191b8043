"""ctypes front-end of tools/nasp_ref.c, the CPU restatement of NormalAdaptiveSuperpixel::Segmentation.

TEST INFRASTRUCTURE ONLY: imported by tests/ and tools/bench_nasp.py, never by the product package.
Arrays are numpy: bgr uint8 [H, W, 3], points / normals float32 [H, W, 3] (points in millimetres).
"""
from __future__ import annotations

import ctypes as C
import os
import subprocess

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_SRC = os.path.join(_HERE, "nasp_ref.c")
LIB_PATH = os.path.join(_HERE, "libnasp_ref.so")

SUPERPIXEL = np.dtype([("r", "u1"), ("g", "u1"), ("b", "u1"), ("pad_", "u1"), ("x", "<i4"), ("y", "<i4"), ("size", "<i4")])
LABEL_DISTANCE = np.dtype([("d", "<f4"), ("l", "<i4")])


class Superpixel(C.Structure):
    _fields_ = [("r", C.c_uint8), ("g", C.c_uint8), ("b", C.c_uint8), ("pad_", C.c_uint8), ("x", C.c_int32), ("y", C.c_int32),
                ("size", C.c_int32)]


class Float3(C.Structure):
    _fields_ = [("x", C.c_float), ("y", C.c_float), ("z", C.c_float)]


_lib = None


def build() -> str:
    if not os.path.exists(LIB_PATH) or os.path.getmtime(LIB_PATH) < os.path.getmtime(_SRC):
        subprocess.check_call(["make", "-C", _HERE, "-s", "libnasp_ref.so"])
    return LIB_PATH


def lib() -> C.CDLL:
    global _lib
    if _lib is None:
        build()
        l = C.CDLL(LIB_PATH)
        vp, i, f = C.c_void_p, C.c_int, C.c_float
        l.nasp_acos_threshold.restype = f
        l.nasp_acos_threshold.argtypes = []
        l.nasp_weight.restype = f
        l.nasp_weight.argtypes = [f, f]
        l.nasp_check_geometry.argtypes = [i, i, i, i]
        l.nasp_init_ld.argtypes = [i, i, i, i, vp]
        l.nasp_sample_clusters.argtypes = [i, i, i, i, vp, vp, vp, vp, vp, vp]
        l.nasp_candidate_distance.restype = f
        l.nasp_candidate_distance.argtypes = [i, i, vp, Float3, Float3, Superpixel, Float3, Float3, f, f, f, f, f]
        l.nasp_tree64.argtypes = [vp, vp]
        l.nasp_calculate_ld.argtypes = [i, i, i, i, vp, vp, vp, vp, vp, vp, vp, vp, f, f, f, f]
        l.nasp_analyze_clusters.argtypes = [i, i, i, i, vp, vp, vp, vp, vp, vp, vp, vp]
        l.nasp_weighted_average.argtypes = [i, i, i, i, vp, vp, vp, vp, vp, vp, vp, vp, f, f, vp]
        l.nasp_segmentation.argtypes = [i, i, i, i, vp, vp, vp, vp, f, f, f, f, i, vp, vp, vp, vp, vp, vp]
        l.nasp_segmentation.restype = i
        _lib = l
    return _lib


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def _f32(a):
    return np.ascontiguousarray(a, dtype=np.float32)


def acos_threshold() -> np.float32:
    return np.float32(lib().nasp_acos_threshold())


def weight(num, sigma) -> np.float32:
    return np.float32(lib().nasp_weight(float(np.float32(num)), float(np.float32(sigma))))


def check_geometry(width, height, rows, cols) -> bool:
    """True when SetParametor accepts the geometry"""
    return lib().nasp_check_geometry(width, height, rows, cols) == 0


def tree64(dist, lab):
    """the 64-way strict-'>' tree on copies of (dist, lab): returns (distance, label) of element 0"""
    d = _f32(dist).copy()
    l = np.ascontiguousarray(lab, np.int32).copy()
    assert d.shape == (64,) and l.shape == (64,)
    lib().nasp_tree64(_p(d), _p(l))
    return d[0], int(l[0])


def candidate_distance(x, y, color, point, normal, mean, center, sp_normal, win2, kc, ks, kd, kn) -> np.float32:
    """mean = (r, g, b, x, y)"""
    c = np.ascontiguousarray(color, np.uint8)
    m = Superpixel(int(mean[0]), int(mean[1]), int(mean[2]), 0, int(mean[3]), int(mean[4]), 0)
    f3 = lambda v: Float3(*[float(np.float32(t)) for t in v])
    g = lambda v: float(np.float32(v))
    return np.float32(lib().nasp_candidate_distance(int(x), int(y), _p(c), f3(point), f3(normal), m, f3(center), f3(sp_normal),
                                                    g(win2), g(kc), g(ks), g(kd), g(kn)))


class State:
    """the buffers of one NormalAdaptiveSuperpixel object after SetParametor (NA5: zero-filled)"""

    def __init__(self, width, height, rows, cols, K):
        if not check_geometry(width, height, rows, cols):
            raise ValueError(f"nasp_ref: geometry {width}x{height} rows {rows} cols {cols} rejected")
        self.width, self.height, self.rows, self.cols = width, height, rows, cols
        self.intr = np.asarray(K, np.float64).reshape(9).astype(np.float32)
        k = rows * cols
        self.labels = np.zeros((height, width), np.int32)
        self.ld = np.zeros((height, width), LABEL_DISTANCE)
        self.mean = np.zeros(k, SUPERPIXEL)
        self.centers = np.zeros((k, 3), np.float32)
        self.normals = np.zeros((k, 3), np.float32)
        self.variance = np.zeros(k, np.float32)

    def _geom(self):
        return self.width, self.height, self.rows, self.cols

    def outputs(self):
        return {"labels": self.labels.copy(), "ld": self.ld.copy(), "mean": self.mean.copy(), "centers": self.centers.copy(),
                "normals": self.normals.copy(), "variance": self.variance.copy()}

    # --- the kernels one by one (for the micro-cases) ---
    def init_ld(self):
        lib().nasp_init_ld(*self._geom(), _p(self.ld))

    def sample(self, bgr, points, normals):
        lib().nasp_sample_clusters(*self._geom(), _p(bgr), _p(points), _p(normals), _p(self.mean), _p(self.centers), _p(self.normals))

    def calculate_ld(self, bgr, points, normals, cs, ss, ds, ns):
        lib().nasp_calculate_ld(*self._geom(), _p(bgr), _p(points), _p(normals), _p(self.ld), _p(self.mean), _p(self.centers),
                                _p(self.normals), _p(self.labels), cs, ss, ds, ns)

    def analyze(self, bgr, points, normals):
        lib().nasp_analyze_clusters(*self._geom(), _p(bgr), _p(points), _p(normals), _p(self.ld), _p(self.mean), _p(self.centers),
                                    _p(self.normals), _p(self.intr))

    def weighted(self, bgr, points, normals, cs, ss):
        lib().nasp_weighted_average(*self._geom(), _p(bgr), _p(points), _p(normals), _p(self.ld), _p(self.mean), _p(self.centers),
                                    _p(self.normals), _p(self.variance), cs, ss, _p(self.intr))

    def segmentation(self, bgr, points, normals, color_sigma, spatial_sigma, depth_sigma, normal_sigma, iteration):
        bgr, points, normals = prep(bgr, points, normals, self.width, self.height)
        rc = lib().nasp_segmentation(*self._geom(), _p(self.intr), _p(bgr), _p(points), _p(normals), color_sigma, spatial_sigma,
                                     depth_sigma, normal_sigma, iteration, _p(self.labels), _p(self.ld), _p(self.mean),
                                     _p(self.centers), _p(self.normals), _p(self.variance))
        assert rc == 0
        return self.outputs()


def prep(bgr, points, normals, width, height):
    bgr = np.ascontiguousarray(bgr, np.uint8)
    points, normals = _f32(points), _f32(normals)
    assert bgr.shape == (height, width, 3) and points.shape == (height, width, 3) and normals.shape == (height, width, 3)
    return bgr, points, normals


def segmentation(bgr, points, normals, rows, cols, K, color_sigma, spatial_sigma, depth_sigma, normal_sigma, iteration):
    """Segmentation on a fresh object: dict of labels [H, W] int32, ld [H, W] (d, l), mean [rows*cols] records,
    centers / normals [rows*cols, 3], variance [rows*cols]"""
    H, W = np.asarray(bgr).shape[:2]
    return State(W, H, rows, cols, K).segmentation(bgr, points, normals, color_sigma, spatial_sigma, depth_sigma, normal_sigma,
                                                   iteration)
