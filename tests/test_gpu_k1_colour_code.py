"""K1's packed colour code on the GPU (csrc/jbf_fast.hip, jbf_pk_kernel; tests/test_k1_colour_code.py has the arithmetic).

(a) Pin of the bits: tests/golden/k1_bits_pin.npz holds the kernel's outputs from before the colour distance was formed
    with one packed fma per pair of taps (tests/golden/make_k1_bits_pin.py recorded it).  The new form computes the same
    integer -cd exactly, every later instruction is unchanged, so the outputs must stay equal to the bit.
(b) The project's stage-wise K1 bar against the binary64 oracle, and the zero mask of the reference-shaped kernel.
Inputs: tests/k1_colour_cases.py -- corner colours, +-1 neighbours, colour pairs on / next to the colour-rule threshold, tiles
on both sides of the rule elision, a hole and a 50 mm sample; 32x24 (vector loader) and 37x19 (odd width: per-pixel loads,
ragged tiles; window 11 also through the kernel variant with the plain loader).  Windows 3 (pass-1 arguments kept),
11 (two pixel pairs per thread, shifted LDS rows), 19 (one pair, two rule bodies), 23 (table from the device copy)."""
import os

import numpy as np
import pytest

import k1_colour_cases as K
from conftest import GOLDEN, assert_k1_stagewise
from gpu_util import dev, host

pytestmark = pytest.mark.gpu

RUN_KEYS = [f"s{si}_w{win}_auto" for si in range(len(K.SIZES)) for win in K.WINDOWS] + ["s1_w11_v1"]


@pytest.fixture(scope="module")
def F(torch_cuda):
    from kinectdepthmapenhancement_amd import filters
    return filters


@pytest.fixture(scope="module")
def pin():
    return np.load(os.path.join(GOLDEN, "k1_bits_pin.npz"))


@pytest.fixture(scope="module")
def cases(pin):
    out = [K.make_case(w, h) for (w, h) in K.SIZES]
    for si, (bgr, depth) in enumerate(out):      # the pin was recorded on exactly these inputs
        assert np.array_equal(bgr, pin[f"bgr_s{si}"]) and np.array_equal(depth.view(np.uint32), pin[f"depth_s{si}"].view(np.uint32))
    return out


def test_cases_hold_what_they_claim(cases):
    t = K.cd_skip()
    assert t == 12170
    for bgr, depth in cases:
        c = bgr[:K.WILD_ROWS].astype(np.int64)
        cd = ((c[:, 1:] - c[:, :-1]) ** 2).sum(axis=2)
        for want in (t - 1, t, t + 1, 0):
            assert (cd == want).any() or want == 0
        flat = c.reshape(-1, 3)
        corners = {tuple(v) for v in flat if set(v.tolist()) <= {0, 255}}
        assert len(corners) == 8
        assert (depth[:K.WILD_ROWS] > 2900).sum() == 2 and np.ptp(depth[K.WILD_ROWS + 1:][depth[K.WILD_ROWS + 1:] > 50]) < 12.5


def _run(torch_cuda, F, bgr, depth, win, v):
    h, w = depth.shape
    p = F.JointBilateralFilter.default_params()
    p.window_size, p.spatial_sigma, p.color_sigma, p.depth_sigma, p.presmooth = win, K.SIGMA_S, K.SIGMA_C, K.SIGMA_D, 0
    jbf = F.JointBilateralFilter(w, h, p)
    jbf.set_variant(v)
    out = torch_cuda.empty((1, h, w), dtype=torch_cuda.float32, device="cuda")
    jbf.filter_batch(dev(torch_cuda, depth[None]), dev(torch_cuda, bgr[None]), out)
    return p, jbf.active_variant(), host(out)[0].copy()


@pytest.mark.parametrize("key", RUN_KEYS)
def test_bits_pinned_and_oracle_bar(torch_cuda, F, pin, cases, key):
    from tools.hooks import stage
    run = {r[0]: r for r in K.runs(F.JointBilateralFilter.variants())}
    assert sorted(run) == sorted(RUN_KEYS)
    _, si, win, v = run[key]
    bgr, depth = cases[si]
    p, name, got = _run(torch_cuda, F, bgr, depth, win, v)
    assert name.startswith(f"w{win}-pk"), name
    # (a) the bits
    want = pin[key]
    diff = got.view(np.uint32) != want.view(np.uint32)
    print(f"{key} ({name}): {int(diff.sum())} of {diff.size} outputs differ from the pin; nonzero outputs {int(np.count_nonzero(got))}")
    assert not diff.any(), f"{key} ({name}): {int(diff.sum())} outputs differ from the pinned bits, first at {np.argwhere(diff)[:5].tolist()}"
    # more than one rule body ran (windows >= 9 pick a body per tile; counters of the stage build)
    if win >= 9:
        _, _, bodies = stage.jbf_stage_run(p, depth[None], bgr[None], v)
        assert bodies[3] > 0 and bodies[0] > 0, bodies[:4]
    # (b) the stage-wise bar; no tap of these inputs is near a depth decision (k1_colour_cases), so no pixel may be excused
    r = assert_k1_stagewise(p, depth, bgr, got, variant=v, what=f"colour code {key}", band_max=0.0)
    print(f"{key}: strict max rel {r['max_rel_strict']:.2e}, band {r['band']}")
    _, gname, ref0 = _run(torch_cuda, F, bgr, depth, win, 0)
    assert gname == "generic-32x8-1px"
    assert np.array_equal(got == 0, ref0 == 0), f"{key}: zero mask differs from the reference-shaped kernel's"
