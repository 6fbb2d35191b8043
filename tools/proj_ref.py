"""ctypes front-end of tools/proj_ref.c, the CPU restatement of the five-argument Projection_GPU::PlaneProjection.

TEST INFRASTRUCTURE ONLY: imported by tests/ and tools/bench_proj.py, never by the product package.
Arrays are numpy: nd float32 [H, W, 4], labels int32 [H, W], variance float32 [n_clusters], points float32 [H, W, 3],
size int32 [n_clusters]; K is the 3x3 intrinsic matrix.
"""
from __future__ import annotations

import ctypes as C
import os
import subprocess

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_SRC = os.path.join(_HERE, "proj_ref.c")
LIB_PATH = os.path.join(_HERE, "libproj_ref.so")

WINDOW_SIZE = 7                                                  # Projection_GPU.cpp:4
SPATIAL_SIGMA = np.float32(20.0)                                 # :3
DEPTH_SIGMA = np.float32(100.0)                                  # :5
MAX_ANGLE = np.float32(3.141592653) / np.float32(8.0)            # Projection_GPU.cu:38, :203
MIN_SIZE = 1300                                                  # :203
BAND_DEN = 2.0 ** -120                                           # below this binary64 denominator a hole pixel is BAND
# What the float32 quotient of a BAND pixel may lie outside [min, max] of its window's valid z by.  Below 2^-126 a weight w is
# a whole number of units u = 2^-149 and every z * w, and every partial sum, is rounded to that grid: an error of at most u / 2
# for each of the m taps whose weight is not 0, over a denominator of at least m u, is half a millimetre whatever the weights
# are.  Above the grid each of the at most 15 * 15 products, the sums of both accumulators and the division round by 2^-24
# relative: fewer than 2^9 roundings, 2^-15 of the depth.  (Found by the sweep: one tap of 2155.418 mm under a weight of one
# unit gives 2155 u / 1 u = 2155.)
BAND_SLACK_MM = 0.5
BAND_SLACK_REL = 2.0 ** -15

_lib = None


def build() -> str:
    if not os.path.exists(LIB_PATH) or os.path.getmtime(LIB_PATH) < os.path.getmtime(_SRC):
        subprocess.check_call(["make", "-C", _HERE, "-s", "libproj_ref.so"])
    return LIB_PATH


def lib() -> C.CDLL:
    global _lib
    if _lib is None:
        build()
        l = C.CDLL(LIB_PATH)
        vp, i, f = C.c_void_p, C.c_int, C.c_float
        l.proj_acos_threshold.restype = f
        l.proj_acos_threshold.argtypes = [f]
        l.proj_spatial_filter.restype = None
        l.proj_spatial_filter.argtypes = [i, f, vp]
        l.proj_init_normalized.restype = None
        l.proj_init_normalized.argtypes = [i, i, i, i, f, f, vp]
        l.proj_set_pseudo_depth.restype = None
        l.proj_set_pseudo_depth.argtypes = [i, i, i, vp, vp, vp, vp, vp, vp, f]
        l.proj_variance_optimization.restype = None
        l.proj_variance_optimization.argtypes = [i, i, i, vp, vp, vp, vp, vp, f, i]
        l.proj_bilateral_filter.restype = None
        l.proj_bilateral_filter.argtypes = [i, i, vp, vp, vp, vp, i, f, vp]
        l.proj_plane_projection.argtypes = [i, i, i, f, f, i, i, vp, vp, vp, vp, vp, i, f, f, f, i, vp, vp, vp, vp]
        _lib = l
    return _lib


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def _g(v) -> float:
    return float(np.float32(v))


def camera(K):
    """Fx, Fy as float32 and the truncated Cx, Cy (Projection_GPU.cpp:11-15)"""
    K = np.asarray(K, np.float64).reshape(3, 3)
    return _g(K[0, 0]), _g(K[1, 1]), int(K[0, 2]), int(K[1, 2])


def acos_threshold(max_angle=MAX_ANGLE) -> np.float32:
    return np.float32(lib().proj_acos_threshold(_g(max_angle)))


def spatial_filter(window=WINDOW_SIZE, sigma=SPATIAL_SIGMA) -> np.ndarray:
    t = np.zeros((window, window), np.float32)
    lib().proj_spatial_filter(window, _g(sigma), _p(t))
    return t


def init_normalized(width, height, K) -> np.ndarray:
    fx, fy, cx, cy = camera(K)
    t = np.zeros((height, width, 3), np.float32)
    lib().proj_init_normalized(width, height, cx, cy, fx, fy, _p(t))
    return t


def prep(nd, labels, variance, points, size):
    nd = np.ascontiguousarray(nd, np.float32)
    labels = np.ascontiguousarray(labels, np.int32)
    variance = np.ascontiguousarray(variance, np.float32)
    points = np.ascontiguousarray(points, np.float32)
    size = np.ascontiguousarray(size, np.int32)
    H, W = labels.shape
    assert nd.shape == (H, W, 4) and points.shape == (H, W, 3) and variance.ndim == 1 and size.shape == variance.shape
    return nd, labels, variance, points, size


def plane_projection(nd, labels, variance, points, size, K, window_size=WINDOW_SIZE, spatial_sigma=SPATIAL_SIGMA,
                     depth_sigma=DEPTH_SIGMA, max_angle=MAX_ANGLE, min_size=MIN_SIZE):
    """PlaneProjection on a fresh object: dict of plane_fitted [H, W, 3], prefilter [H, W, 3] (Optimized3D before the
    bilateral filter), optimized [H, W, 3], den64 [H, W] (the filter's denominator in binary64) and rays [H, W, 3]"""
    nd, labels, variance, points, size = prep(nd, labels, variance, points, size)
    H, W = labels.shape
    fx, fy, cx, cy = camera(K)
    out = {"plane_fitted": np.zeros((H, W, 3), np.float32), "prefilter": np.zeros((H, W, 3), np.float32),
           "optimized": np.zeros((H, W, 3), np.float32), "den64": np.zeros((H, W), np.float64)}
    rc = lib().proj_plane_projection(W, H, len(variance), fx, fy, cx, cy, _p(nd), _p(labels), _p(variance), _p(points), _p(size),
                                     int(window_size), _g(spatial_sigma), _g(depth_sigma), _g(max_angle), int(min_size),
                                     _p(out["plane_fitted"]), _p(out["prefilter"]), _p(out["optimized"]), _p(out["den64"]))
    assert rc == 0, f"proj_plane_projection returned {rc}"
    out["rays"] = init_normalized(W, H, K)
    return out


def differing(a, b) -> np.ndarray:
    """elementwise: the float32 bit patterns differ and the two are not both NaN (a NaN's sign and payload are not part of
    the result)"""
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return (a.view(np.uint32) != b.view(np.uint32)) & ~(np.isnan(a) & np.isnan(b))


def window_range(z, window_size):
    """per pixel the min and max of the valid (> 50) z of its window, +inf / -inf where there is none: the interval a BAND
    pixel's result must lie in"""
    z = np.asarray(z, np.float32)
    H, W = z.shape
    r = window_size // 2
    lo = np.full((H + 2 * r, W + 2 * r), np.inf, np.float32)
    hi = np.full((H + 2 * r, W + 2 * r), -np.inf, np.float32)
    ok = z > 50
    lo[r:r + H, r:r + W] = np.where(ok, z, np.inf)
    hi[r:r + H, r:r + W] = np.where(ok, z, -np.inf)
    mn, mx = np.full((H, W), np.inf, np.float32), np.full((H, W), -np.inf, np.float32)
    for i in range(window_size):
        for j in range(window_size):
            mn = np.minimum(mn, lo[i:i + H, j:j + W])
            mx = np.maximum(mx, hi[i:i + H, j:j + W])
    return mn, mx


def compare(got_plane_fitted, got_optimized, exp, window_size=WINDOW_SIZE):
    """The parity bar of DESIGN.md ("Plane projection (five-argument)") as counts of failing pixels, every pixel checked:
      plane_fitted  bit-identical (equal NaN / inf positions)
      strict        own pre-filter z > 50: <= 1e-4 relative, identical zero mask
      hole          own pre-filter z <= 50 (or NaN) and den64 >= 2^-120: <= 1e-4 relative
      band          the rest: 0, or within [min, max] of the window's valid z widened by BAND_SLACK_MM + BAND_SLACK_REL * |z|
    plus the population of each class and the largest relative error seen"""
    zc, ze, zg = exp["prefilter"][..., 2], exp["optimized"][..., 2], np.asarray(got_optimized, np.float32)[..., 2]
    with np.errstate(all="ignore"):
        rel = np.abs(zg.astype(np.float64) - ze) / np.abs(ze.astype(np.float64))
        close = (rel <= 1e-4) | ~differing(zg, ze)
        strict = zc > 50
        band = ~strict & (exp["den64"] < BAND_DEN)
        hole = ~strict & ~band
        mn, mx = window_range(zc, window_size)
        lo = mn.astype(np.float64) - (BAND_SLACK_MM + BAND_SLACK_REL * np.abs(mn.astype(np.float64)))
        hi = mx.astype(np.float64) + (BAND_SLACK_MM + BAND_SLACK_REL * np.abs(mx.astype(np.float64)))
        in_band = (zg == 0) | ((zg >= lo) & (zg <= hi))
        # x, y = ray * z with the GPU's own z: one float32 multiplication
        rays = exp["rays"]
        xy_bad = differing(rays[..., :2] * zg[..., None], np.asarray(got_optimized, np.float32)[..., :2]).any(-1)
    relmax = lambda m: float(np.nanmax(np.where(m & np.isfinite(rel), rel, 0.0))) if m.any() else 0.0
    return {"plane_fitted": int(differing(got_plane_fitted, exp["plane_fitted"]).any(-1).sum()),
            "strict": int((strict & ~(close & ((zg == 0) == (ze == 0)))).sum()),
            "hole": int((hole & ~close).sum()), "band": int((band & ~in_band).sum()), "xy": int(xy_bad.sum()),
            "n_strict": int(strict.sum()), "n_hole": int(hole.sum()), "n_band": int(band.sum()),
            "max_rel_strict": relmax(strict), "max_rel_hole": relmax(hole)}
