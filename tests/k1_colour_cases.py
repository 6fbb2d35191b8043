"""Inputs of tests/test_gpu_k1_colour_code.py (and of the script that recorded tests/golden/k1_bits_pin.npz): two small
frames whose colours sit on every edge of K1's packed colour code and whose depths make tiles take different rule bodies.

Rows 0..3 ("wild"): the left half holds the 0 / 255 corner colours, their +-1 neighbours, and colour pairs (a, b), horizontally
adjacent, whose squared distance is cd_skip - 1, cd_skip and cd_skip + 1 (the colour-rule threshold of sigma_c) over calm
depths; the right half holds calm colours and two depth outliers of +1500 mm (far above the 288.4 mm depth-rule threshold of
sigma_d = 20: the outlier tap is skipped, and it moves no window average by more than 1500 / 8.3 = 180 mm -- the sum of
the spatial weights is 8.3 at window 3 and larger beyond -- so no tap comes near the threshold and the stage-wise check has no
open decision to excuse).  Rows 4.. ("calm"): one colour +-1 per channel and depths within 12 mm.  Every tuned window stages
a 16-row tile plus its halo: the tiles of rows 0..15 see the wild rows (colour range and depth range above both thresholds)
and run the full-rule body, the tiles below (their halo starts at row 5 or later for every window <= 23) see calm data only
and run the body without rules; window 3 has no rule elision."""
import numpy as np

SIGMA_S, SIGMA_C, SIGMA_D = 3.0, 7.65, 20.0
SIZES = ((32, 24), (37, 19))          # (width, height): vector loader / odd width: per-pixel loads, ragged tiles
WINDOWS = (3, 11, 19, 23)
WILD_ROWS = 4


def cd_skip(sigma_c=SIGMA_C):
    """smallest integer colour distance whose factor exp(-cd / (2 sigma_c^2)) is 0 in float32 (csrc/kde_host_math.h)"""
    den = np.float32(2) * (np.float32(sigma_c) * np.float32(sigma_c))
    t = 150.0 * 0.693147180559945309417232121458
    thr = np.float32(t)
    if float(thr) <= t:
        thr = np.nextafter(thr, np.float32(np.inf))
    lo, hi = 0, 195076
    while lo < hi:
        mid = (lo + hi) // 2
        if np.float32(mid) / den >= thr:
            hi = mid
        else:
            lo = mid + 1
    return lo


def pair_with_distance(target, rng):
    """brute force: two colours (uint8 BGR) with squared distance == target"""
    sols = [(x, y, z) for x in range(256) for y in range(x + 1) for z in range(y + 1) if x * x + y * y + z * z == target]
    assert sols, f"no colour difference has squared length {target}"
    d = np.array(sols[rng.integers(len(sols))])[rng.permutation(3)]
    a = np.array([rng.integers(0, 256 - v) for v in d])
    b = a + d
    assert ((a - b) ** 2).sum() == target and b.max() <= 255
    return a.astype(np.uint8), b.astype(np.uint8)


def make_case(w, h, seed=11):
    rng = np.random.default_rng(seed + 1000 * w + h)
    base = np.array([90, 140, 60])
    bgr = (base + rng.integers(-1, 2, (h, w, 3))).astype(np.uint8)
    depth = (1500.0 + 12.0 * rng.random((h, w))).astype(np.float32)
    # wild rows
    seq = []
    t = cd_skip()
    for k in range(3):                                            # each threshold pair three times, adjacent in a row
        for tgt in (t - 1, t, t + 1):
            seq.extend(pair_with_distance(tgt, rng))
    corners = [np.array([(i >> 0 & 1) * 255, (i >> 1 & 1) * 255, (i >> 2 & 1) * 255]) for i in range(8)]
    for c in corners:
        seq.append(c.astype(np.uint8))
        seq.append(np.clip(c + np.where(c == 0, 1, -1) * rng.integers(0, 2, 3), 0, 255).astype(np.uint8))   # a +-1 neighbour
    half = w // 2
    n = WILD_ROWS * half
    order = [seq[i % len(seq)] for i in range(n)]
    # pairs stay adjacent: permute the sequence in units of two pixels
    units = [order[i:i + 2] for i in range(0, n - 1, 2)]
    perm = rng.permutation(len(units))
    flat = [p for u in perm for p in units[u]]
    flat += [order[-1]] * (n - len(flat))
    bgr[:WILD_ROWS, :half] = np.array(flat, np.uint8).reshape(WILD_ROWS, half, 3)
    for (y, x) in ((1, w - 5), (3, w - 2)):          # >= 12 columns from the wild colours: no window (<= 23) holds both
        depth[y, x] += 1500.0
    depth[2, 5] = 0.0                                             # invalid taps: a hole and a value at the 50 mm limit
    depth[h - 3, w - 2] = 50.0
    return np.ascontiguousarray(bgr), np.ascontiguousarray(depth)


def runs(variant_names):
    """(key, size index, window, variant index) of every pinned launch: the built-in kernel of each window on both frames, plus
    the window-11 kernel with the plain (one pixel per iteration) loader on the odd-width frame"""
    out = []
    for si in range(len(SIZES)):
        for win in WINDOWS:
            out.append((f"s{si}_w{win}_auto", si, win, -1))
    out.append(("s1_w11_v1", 1, 11, variant_names.index("w11-pk2-16x16-false-v1")))
    return out
