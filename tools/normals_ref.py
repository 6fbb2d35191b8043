"""ctypes front-end of tools/normals_ref.c, the CPU restatement of NormalMapGenerator::generateNormalMap.

TEST INFRASTRUCTURE ONLY: imported by tests/ and tools/bench_normals.py, never by the product package.
Arrays are numpy: points / normals float32 [H, W, 3], maps [H, W].
"""
from __future__ import annotations

import ctypes as C
import os
import subprocess

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_SRC = os.path.join(_HERE, "normals_ref.c")
LIB_PATH = os.path.join(_HERE, "libnormals_ref.so")

SDC, CM, BILATERAL = 0, 1, 2
# decision codes of nref_eigen
SMALL_C0, ROOTS_FALLBACK, Z_NEGATIVE = 1, 2, 16

_lib = None


def build() -> str:
    if not os.path.exists(LIB_PATH) or os.path.getmtime(LIB_PATH) < os.path.getmtime(_SRC):
        subprocess.check_call(["make", "-C", _HERE, "-s", "libnormals_ref.so"])
    return LIB_PATH


def lib() -> C.CDLL:
    global _lib
    if _lib is None:
        build()
        l = C.CDLL(LIB_PATH)
        vp, i, f = C.c_void_p, C.c_int, C.c_float
        l.nref_scale.argtypes = [vp, vp, C.c_longlong]
        l.nref_dci.argtypes = [i, i, vp, f, vp]
        l.nref_dt.argtypes = [i, i, vp, vp]
        l.nref_fs.argtypes = [i, i, vp, vp, f, vp]
        l.nref_eigen.argtypes = [vp, vp, vp]
        l.nref_eigen.restype = i
        l.nref_bilateral.argtypes = [i, i, vp, vp]
        l.nref_normals.argtypes = [i, i, vp, i, f, f, vp, vp, vp]
        l.nref_normals.restype = i
        _lib = l
    return _lib


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def _f32(a):
    return np.ascontiguousarray(a, dtype=np.float32)


def scale(points_mm):
    p = _f32(points_mm)
    v = np.empty_like(p)
    lib().nref_scale(_p(p), _p(v), p.size)
    return v


def dci_map(v, factor=0.05):
    """the depth-change map of metre points v (definition N1): 0 or 255"""
    v = _f32(v)
    H, W = v.shape[:2]
    out = np.empty((H, W), np.uint8)
    lib().nref_dci(W, H, _p(v), factor, _p(out))
    return out


def distance_transform(d):
    """the reference's two-pass host distance transform of a DCI map (uint8 [H, W])"""
    d = np.ascontiguousarray(d, np.uint8)
    H, W = d.shape
    out = np.empty((H, W), np.float32)
    lib().nref_dt(W, H, _p(d), _p(out))
    return out


def eigen(m):
    """computeEigenValueAndVector on a 3x3 double matrix -> (eigen value, eigen vector, decision code)"""
    m = np.ascontiguousarray(np.asarray(m, np.float64).reshape(9))
    ev = np.zeros(1, np.float64)
    vec = np.zeros(3, np.float64)
    code = lib().nref_eigen(_p(m), _p(ev), _p(vec))
    return float(ev[0]), vec, code


def normals(points_mm, method=CM, factor=0.05, smoothing=20.0, want_band=True, return_rest=False):
    """generateNormalMap on one frame of millimetre points [H, W, 3].
    Returns (normals [H, W, 3], smoothing map [H, W] or None, band [H, W] bool or None).  With return_rest=True (CM) a
    fourth item: the pixels CM left bad, which the rest-normal pass serves."""
    p = _f32(points_mm)
    H, W = p.shape[:2]
    n = np.empty((H, W, 3), np.float32)
    cm = method == CM
    fs = np.empty((H, W), np.float32) if cm else None
    band = np.empty((H, W), np.uint8) if (cm and (want_band or return_rest)) else None
    rc = lib().nref_normals(W, H, _p(p), method, factor, smoothing, _p(n), None if fs is None else _p(fs),
                            None if band is None else _p(band))
    if rc != 0:
        raise MemoryError("nref_normals: out of memory")
    if return_rest:
        return n, fs, (band & 1).astype(bool), (band & 2).astype(bool)
    return n, fs, (None if band is None else (band & 1).astype(bool))
