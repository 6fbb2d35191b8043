"""K1's rule elision is decided per WAVEFRONT (csrc/jbf_fast.hip, jbf_pk_kernel; EXPERIMENTS.md Part I item 13): each
wavefront reduces the colour and depth ranges of its own region (its pixels plus the window radius) from LDS and picks its
body; the stage build counts one body per wavefront that owns at least one pixel.

A  a decision finer than a tile: one 4x4 patch of corner colours and a depth outlier in a calm 64x32 image
B  ragged tiles and wavefronts without work (37x19, 70x9)
C  awkward regions: no valid depth, a single valid depth, depths near 1e4 mm at sigma_d = 1 mm
D  windows 19 ({none, both} only) and 9
Every case: output bits equal to the stage build with the full-rule body forced, and the stage-wise oracle bar.
All at presmooth = 0; tools/elision_census.py predicts the counters (printed next to them)."""
import re

import numpy as np
import pytest

from conftest import assert_k1_stagewise
from gpu_util import dev, host

pytestmark = pytest.mark.gpu

SIGMA_S, SIGMA_C = 3.0, 7.65


@pytest.fixture(scope="module")
def F(torch_cuda):
    from kinectdepthmapenhancement_amd import filters
    return filters


# kernels whose wavefronts are 8x8-thread quarters of the tile instead of its rows (csrc/jbf_fast.hip, KQ entries of the table)
QUARTER_WAVEFRONTS = {"w11-pk2-16x16-false-v4"}


def footprint(name):
    """pixels (width, height) one wavefront of the packed kernel `name` owns"""
    m = re.match(r"w\d+-pk(\d+)-(\d+)x(\d+)-(?:true|false)-v[14](-rows)?(-noelide)?$", name)
    assert m, name
    np_, bx = int(m.group(1)), int(m.group(2))
    wtx = 8 if name in QUARTER_WAVEFRONTS else bx
    return wtx * 2 * np_, 64 // wtx


def wavefronts_with_work(name, w, h):
    fw, fh = footprint(name)          # tiles are whole multiples of the footprint and start at (0, 0)
    return -(-w // fw) * -(-h // fh)


def scene(w, h, seed=3, patch=True, base_depth=1500.0, spread=12.0):
    """calm colours (+-1) and depths (within `spread` mm); the patch at rows 0..3, columns 0..3 holds the eight corner colours
    and one depth 1500 mm above the rest (five times the depth limit of sigma_d = 20: its tap is skipped, and it moves no
    window average by more than 1500 / 8.3 = 180 mm, so no tap comes near the limit)"""
    rng = np.random.default_rng(seed + 1000 * w + h)
    bgr = (np.array([90, 140, 60]) + rng.integers(-1, 2, (h, w, 3))).astype(np.uint8)
    depth = (base_depth + spread * rng.random((h, w))).astype(np.float32)
    if patch:
        for k in range(16):
            bgr[k // 4, k % 4] = [(k & 1) * 255, (k >> 1 & 1) * 255, (k >> 2 & 1) * 255]
        depth[1, 2] += 1500.0
    return bgr, depth


def params(F, win, sigma_d=20.0):
    p = F.JointBilateralFilter.default_params()
    p.window_size, p.spatial_sigma, p.color_sigma, p.depth_sigma, p.presmooth = win, SIGMA_S, SIGMA_C, sigma_d, 0
    return p


def product(torch, F, p, bgr, depth, v=-1):
    h, w = depth.shape
    jbf = F.JointBilateralFilter(w, h, p)
    jbf.set_variant(v)
    out = torch.empty((1, h, w), dtype=torch.float32, device="cuda")
    jbf.filter_batch(dev(torch, depth[None]), dev(torch, bgr[None]), out)
    return jbf.active_variant(), host(out)[0].copy()


def check(torch, F, bgr, depth, win, sigma_d=20.0, what="", band_max=0.02):
    """the common part: forced-body bits, counters against the wavefront count, the oracle bar.  Returns (name, out, counters)"""
    from tools import elision_census as E
    from tools.hooks import stage
    p = params(F, win, sigma_d)
    name, got = product(torch, F, p, bgr, depth)
    assert name.startswith(f"w{win}-pk"), name
    h, w = depth.shape
    out, _, bodies = stage.jbf_stage_run(p, depth[None], bgr[None], -1)
    forced, _, bodies_forced = stage.jbf_stage_run(p, depth[None], bgr[None], -1, force_full_rules=True)
    fw, fh = footprint(name)
    nc, nd = E.census(bgr, depth, fw, fh, win, E.thresholds(SIGMA_C, sigma_d))
    print(f"{what} ({name}, {w}x{h}): bodies {bodies[:4].tolist()}, forced {bodies_forced[:4].tolist()}, census predicts "
          f"{E.body_mix(nc, nd, win)} for {wavefronts_with_work(name, w, h)} wavefronts of {fw}x{fh} pixels")
    assert stage.bits_equal(out[0], got), f"{what}: the stage build's output differs from the product library's"
    assert stage.bits_equal(forced[0], got), f"{what}: forcing the full-rule body changed the output"
    n = wavefronts_with_work(name, w, h)
    assert bodies[:4].sum() == n, f"{what}: {bodies[:4].tolist()} does not sum to the {n} wavefronts that own a pixel"
    assert bodies_forced[3] == n and bodies_forced[:3].sum() == 0, bodies_forced[:4]
    assert_k1_stagewise(p, depth, bgr, got, what=what, band_max=band_max)
    return name, got, bodies[:4]


def test_a_decision_finer_than_a_tile(torch_cuda, F):
    bgr, depth = scene(64, 32)
    name, got, bodies = check(torch_cuda, F, bgr, depth, 11, what="A")
    names = F.JointBilateralFilter.variants()
    nname, plain = product(torch_cuda, F, params(F, 11), bgr, depth, names.index("w11-pk2-16x16-false-v4-noelide"))
    assert nname.endswith("-noelide")
    from tools.hooks import stage
    assert stage.bits_equal(plain, got), "A: the kernel without rule elision computes other bits"
    # one decision per tile would count at most 2 here
    assert bodies[3] >= 1 and bodies[0] >= 4, bodies


@pytest.mark.parametrize("size", [(37, 19), (70, 9)])
def test_b_ragged_and_empty_wavefronts(torch_cuda, F, size):
    w, h = size
    bgr, depth = scene(w, h)
    depth[h - 2, w - 3] = 0.0                   # a hole and a 50 mm sample: invalid taps
    depth[h // 2, w // 2] = 50.0
    name, got, bodies = check(torch_cuda, F, bgr, depth, 11, what=f"B {w}x{h}")
    gname, ref0 = product(torch_cuda, F, params(F, 11), bgr, depth, 0)
    assert gname == "generic-32x8-1px"
    assert np.array_equal(got == 0, ref0 == 0), f"B {w}x{h}: zero mask differs from the reference-shaped kernel's"


def test_c_awkward_regions(torch_cuda, F):
    # 128 columns: the 80 invalid ones on the left hold a whole region of every footprint in use (up to 64 + 2 * 5 columns wide)
    bgr, depth = scene(128, 32, patch=False)
    depth[:, :80] = 0.0
    _, got, bodies = check(torch_cuda, F, bgr, depth, 11, what="C no valid depth")
    assert (got[:, :70] == 0).all() and bodies[2] == 0 and bodies[3] == 0, bodies       # and no depth step anywhere else
    depth[10, 20] = 1234.0
    _, got, bodies = check(torch_cuda, F, bgr, depth, 11, what="C one valid depth")
    assert abs(got[10, 20] - 1234.0) < 0.01 and bodies[2] == 0 and bodies[3] == 0, bodies
    # depths near 1e4 mm at sigma_d = 1 mm (limit 14.4 mm): the left half spreads over 14.39 mm -- within the float32 rounding
    # of a window average of the limit, so the rule has to stay --, the right half over 3 mm.  Many taps sit near the decision at this sigma, so the
    # share of interval-checked pixels is not bounded here; every pixel still has to pass its check.
    bgr, depth = scene(128, 32, patch=False, base_depth=1.0e4, spread=3.0)
    rng = np.random.default_rng(9)
    depth[:, :64] = (1.0e4 + 14.39 * rng.random((32, 64))).astype(np.float32)
    depth[5, 7], depth[6, 9] = 1.0e4, np.float32(1.0e4 + 14.39)
    _, got, bodies = check(torch_cuda, F, bgr, depth, 11, sigma_d=1.0, what="C 1e4 mm at sigma_d 1", band_max=1.0)
    assert bodies[2] + bodies[3] >= 1 and bodies[0] + bodies[1] >= 1, bodies


@pytest.mark.parametrize("win", [19, 9])
def test_d_other_windows(torch_cuda, F, win):
    bgr, depth = scene(64, 32)
    name, got, bodies = check(torch_cuda, F, bgr, depth, win, what=f"D window {win}")
    names = F.JointBilateralFilter.variants()
    from tools.hooks import stage
    _, plain = product(torch_cuda, F, params(F, win), bgr, depth, names.index(name + "-noelide"))
    assert stage.bits_equal(plain, got), f"D window {win}: the kernel without rule elision computes other bits"
    assert bodies[3] >= 1 and bodies[0] >= 4, bodies
    if win >= 15:
        assert bodies[1] == 0 and bodies[2] == 0, bodies
