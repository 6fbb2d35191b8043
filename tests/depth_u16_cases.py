"""The uint16 depth rule of kde_points_to_depth (csrc/kde_device_math.h, depth_to_u16) stated in numpy, and the crafted
values on which test_enh_feed_abi.py (host side) and test_gpu_points_to_depth.py (kernels) check it."""
import numpy as np

CRAFTED = np.array([0.0, -0.0, 0.49999997, 0.5, 0.50000006, 1.0, 1.5, 2.5, 3.5, 65534.5, 65535.0, 65535.4, 65535.5, 65536.0, 1e9,
                    -3.0, -0.5, np.inf, -np.inf, np.nan, -np.nan, 1e-45, -1e-45, 1.1754942e-38, 1234.0, 1234.5, 1235.5, 4095.49],
                   dtype=np.float32)


def to_u16(z):
    """r = rint(z) (round half to even); r where 1 <= r <= 65535, else 0 (NaN and +-inf fail both comparisons)"""
    z = np.asarray(z, np.float32)
    with np.errstate(invalid="ignore"):
        r = np.rint(z)
        ok = (r >= 1) & (r <= 65535)
        return np.where(ok, r, 0).astype(np.uint16)


def values(n, seed=0):
    """n float32 z values: uniform in +-70000 with a quarter of them snapped to exact halves (the ties of the rounding), the
    crafted ones over the first elements (as many as fit) and, where there is room, over the last ones too (the tail that
    the vector kernel leaves to the scalar one)"""
    rng = np.random.default_rng(seed)
    z = rng.uniform(-70000.0, 70000.0, n).astype(np.float32)
    half = rng.random(n) < 0.25
    z[half] = np.floor(z[half]) + np.float32(0.5)
    k = min(n, CRAFTED.size)
    z[:k] = CRAFTED[:k]
    if n >= 2 * CRAFTED.size:
        z[-CRAFTED.size:] = CRAFTED
    return z
