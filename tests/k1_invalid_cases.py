"""Inputs of tests/test_gpu_k1_invalid_taps.py (and of tools/record_k1_invalid_pin.py, which recorded
tests/golden/k1_invalid_taps_pin.npz): small frames whose invalid taps (depth <= 50 mm, outside the image) and guide contrast
put every kind of wavefront of K1's packed kernels (csrc/jbf_fast.hip, jbf_pk_kernel) in front of invalid taps.

Frames: a batch of 2 x 100x40 (more than one 64x16 tile in x and y, ragged right and bottom wavefronts, width % 4 == 0: the
16-byte loads of the vector loader) and 1 x 37x21 (narrower than a tile, odd width: per-pixel loads).

Depth patterns (valid depths 1500..1512 mm; a few +1500 mm outliers in the lowest quarter of the frame, far above the 288.4 mm
depth-rule threshold of sigma_d = 20, make the wavefronts there run a depth-rule body and the rule trip; their 5x5 neighbourhood
stays valid, so that in no window the average lands 250..300 mm from a tap: no tap is near a depth decision, see make_depth):
  valid    every sample valid
  random   30 % invalid, drawn from {0, 50.0, 49.999, -1, other negatives}
  block    a 32x8-pixel wavefront footprint and its halo for the widest tested window (11 pixels) invalid
  one      one valid pixel in the frame
  centre   isolated invalid pixels (an invalid centre whose taps are valid)
Guide patterns (sigma_c = 7.65: the colour rule trips from a squared distance of 12170):
  flat      one colour +-1 per channel: no wavefront needs the colour rule
  contrast  two colours far apart, at random: every wavefront needs it
  split     left half flat, right half contrast: the wavefronts of one workgroup run both kinds of body over one staged tile"""
import numpy as np

SIGMA_S, SIGMA_C, SIGMA_D = 3.0, 7.65, 20.0
SIZES = ((100, 40, 2), (37, 21, 1))          # (width, height, frames)
DEPTHS = ("valid", "random", "block", "one", "centre")
GUIDES = ("flat", "contrast", "split")
HALO = 11                                     # radius of window 23, the widest one tested
# (key, window, variant name; None = the window's built-in kernel)
VARIANTS = (
    ("w3", 3, None),
    ("w11", 11, None),
    ("w11rows", 11, "w11-pk2-16x16-false-v4-rows"),
    ("w11t8x32", 11, "w11-pk2-8x32-false-v4"),
    ("w11v1", 11, "w11-pk2-16x16-false-v1"),
    ("w11noelide", 11, "w11-pk2-16x16-false-v4-noelide"),
    ("w19", 19, None),
    ("w19noelide", 19, "w19-pk1-16x16-false-v4-noelide"),
    ("w23", 23, None),
)
# twin without the per-wavefront rule elision (the full-rule body everywhere) of a built-in kernel
NOELIDE_TWIN = {"w11": "w11noelide", "w19": "w19noelide"}
# launches held to the binary64 oracle as well (the others run the same kernel template under another thread mapping)
ORACLE_KEYS = ("w3", "w11", "w11v1", "w19", "w23")
GENERIC = "generic-32x8-1px"                  # the reference-shaped kernel (variant 0)
FULL_OUTPUTS = ("s1_w11_random_split", "s1_w19_block_contrast")      # stored whole in the pin, the others as sha256

# colour-sigma guard of the tuned kernels: they serve log2(e) / (2 sigma_c^2) > 1e-34 (csrc/jbf_fast.hip, jbf_fast_supported),
# beyond that the generic kernel runs.  (name, color_sigma, a tuned kernel runs)
_EDGE = float(np.sqrt(1.4426950408889634 / 2.0e-34))
GUARD_SIGMAS = (("inside", 0.999 * _EDGE, True), ("outside", 1.001 * _EDGE, False), ("1e6", 1.0e6, True))


def outliers(w, h):
    return ((h - 2, w // 5), (h - 4, w - 3), (h - 3, w // 2))


def make_depth(kind, w, h, n, rng):
    d = (1500.0 + 12.0 * rng.random((n, h, w))).astype(np.float32)
    # the 5x5 neighbourhood of an outlier stays valid: with a handful of valid taps in a 3x3 window the outlier would carry a
    # sixth or a fifth of the weight, the average would lie 250..300 mm from the other taps, and single taps would sit on the
    # depth decision (288.4 mm) or at the underflow point of their weight -- the oracle holds such pixels to an interval only.
    # With all 9 taps valid the outlier carries 0.11..0.12 of the weight (160..190 mm), in the wider windows a few percent
    near = np.zeros((h, w), bool)
    for (y, x) in outliers(w, h):
        near[max(0, y - 2):y + 3, max(0, x - 2):x + 3] = True
    if kind == "valid":
        pass
    elif kind == "random":
        bad = (rng.random((n, h, w)) < 0.30) & ~near
        pool = np.array([0.0, 50.0, 49.999, -1.0, -3.5, -1500.0, -1.0e30], np.float32)
        d[bad] = pool[rng.integers(0, len(pool), int(bad.sum()))]
    elif kind == "block":
        bx, by = (32, 8) if w > 64 else (0, 0)
        d[:, max(0, by - HALO):by + 8 + HALO, max(0, bx - HALO):bx + 32 + HALO] = 0.0
    elif kind == "one":
        keep = d[:, h // 2, w // 3].copy()
        d[:] = 0.0
        d[:, h // 2, w // 3] = keep
    elif kind == "centre":
        hole = np.zeros((h, w), np.float32)
        hole[2::5, 3::7] = np.float32(50.0)
        hole[4::10, 6::14] = np.float32(-2.0)
        hole[near] = 0.0
        d[:, hole != 0] = hole[hole != 0]
    else:
        raise ValueError(kind)
    # the outliers, where their neighbourhood is valid (none under "one", none next to the block of the small frame)
    for (y, x) in outliers(w, h):
        ok = (d[:, max(0, y - 2):y + 3, max(0, x - 2):x + 3] > 50.0).all(axis=(1, 2))
        d[ok, y, x] += 1500.0
    return np.ascontiguousarray(d)


def make_guide(kind, w, h, n, rng):
    flat = (np.array([90, 140, 60]) + rng.integers(-1, 2, (n, h, w, 3))).astype(np.uint8)
    # two colours 36300 apart (squared), each +-1 per channel, at random: a squared distance is below 50 or above 35000, never
    # near the threshold -- a window with a single valid tap must not hang on how that tap's colour factor rounds
    far = np.where(rng.random((n, h, w, 1)) < 0.5, np.array([90, 140, 60]), np.array([200, 30, 170]))
    wild = (far + rng.integers(-1, 2, (n, h, w, 3))).astype(np.uint8)
    if kind == "flat":
        g = flat
    elif kind == "contrast":
        g = wild
    elif kind == "split":
        g = flat
        g[:, :, w // 2:] = wild[:, :, w // 2:]
    else:
        raise ValueError(kind)
    return np.ascontiguousarray(g)


def make_case(si, depth_kind, guide_kind):
    """(bgr [n,H,W,3] uint8, depth [n,H,W] float32) -- a function of its arguments alone"""
    w, h, n = SIZES[si]
    seed = 7000 + 100 * si + 10 * DEPTHS.index(depth_kind) + GUIDES.index(guide_kind)
    rng = np.random.default_rng(seed)
    depth = make_depth(depth_kind, w, h, n, rng)
    return make_guide(guide_kind, w, h, n, rng), depth


def case_keys():
    """(si, depth kind, guide kind) of every input"""
    return [(si, dk, gk) for si in range(len(SIZES)) for dk in DEPTHS for gk in GUIDES]


def pin_key(si, vkey, dk, gk):
    return f"s{si}_{vkey}_{dk}_{gk}"


def params(F, win, color_sigma=SIGMA_C):
    p = F.JointBilateralFilter.default_params()
    p.window_size, p.spatial_sigma, p.color_sigma, p.depth_sigma, p.presmooth = win, SIGMA_S, float(color_sigma), SIGMA_D, 0
    return p


def variant_index(F, vname):
    return -1 if vname is None else F.JointBilateralFilter.variants().index(vname)


def launch(torch, F, bgr, depth, win, vname, color_sigma=SIGMA_C):
    """K1 alone (no presmoothing) on the batch -> (params, name of the kernel that ran, output [n,H,W] numpy)"""
    n, h, w = depth.shape
    p = params(F, win, color_sigma)
    jbf = F.JointBilateralFilter(w, h, p, max_batch=n)
    try:
        jbf.set_variant(variant_index(F, vname))
        out = torch.empty((n, h, w), dtype=torch.float32, device="cuda")
        jbf.filter_batch(torch.from_numpy(depth).cuda(), torch.from_numpy(bgr).cuda(), out)
        name = jbf.active_variant()
        got = out.cpu().numpy()
    finally:
        jbf.close()
    return p, name, got
