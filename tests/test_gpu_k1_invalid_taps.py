"""Invalid taps in K1's packed kernels (csrc/jbf_fast.hip, jbf_pk_kernel; tests/test_k1_invalid_marker.py has the arithmetic).

A pixel with depth <= 50 mm or outside the image is staged with depth 0 and the colour-code term h_q = -2^126.  In the bodies
without the colour rule its weight is then exactly 0 by itself (no validity factor, plain packed adds into the sums of
weights); the bodies with the colour rule keep the validity factor.  Every output bit had to stay:

(a) tests/golden/k1_invalid_taps_pin.npz holds the sha256 of the kernel's output for every launch below, and two outputs
    whole, recorded from the commit before the change (tools/record_k1_invalid_pin.py);
(b) the built-in kernels of windows 11 and 19 against their "-noelide" twins (the full-rule body, validity factor kept, for
    every wavefront), and every launch against the stage build of the library;
(c) the project's stage-wise K1 bar against the binary64 oracle (conftest.assert_k1_stagewise) with band_max = 0, as
    tests/test_gpu_k1_colour_code.py holds it: no tap of these inputs is near a depth decision or a weight's underflow point
    (tests/k1_invalid_cases.py keeps every tap 24 mm or more away; tests/test_k1_invalid_cases.py checks it on the CPU), so no
    pixel may be excused to an interval; and the zero mask of the reference-shaped generic kernel.
Inputs: tests/k1_invalid_cases.py -- 2 x 100x40 and 1 x 37x21; five depth patterns x three guide patterns; windows 3 (pass-1
arguments kept), 11 (built-in, "-rows", 8x32 tile, plain loader), 19 (two rule bodies), 23 (table from the device copy)."""
import hashlib
import os

import numpy as np
import pytest

import k1_invalid_cases as K
from conftest import GOLDEN, assert_k1_stagewise

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def F(torch_cuda):
    from kinectdepthmapenhancement_amd import filters
    return filters


@pytest.fixture(scope="module")
def pin():
    z = np.load(os.path.join(GOLDEN, "k1_invalid_taps_pin.npz"))
    keys = str(z["keys"]).split("\n")
    assert len(keys) == len(z["digests"]) == len(set(keys))
    return {"sha": {k: bytes(d) for k, d in zip(keys, z["digests"])}, "full": {k: z["full_" + k] for k in K.FULL_OUTPUTS}}


@pytest.fixture(scope="module")
def inputs():
    return {ck: K.make_case(*ck) for ck in K.case_keys()}


_outputs = {}


def _product(torch, F, inputs, si, vkey, dk, gk):
    """the product library's output of one pinned launch (run once per module)"""
    key = K.pin_key(si, vkey, dk, gk)
    if key not in _outputs:
        _, win, vname = next(v for v in K.VARIANTS if v[0] == vkey)
        bgr, depth = inputs[(si, dk, gk)]
        p, name, got = K.launch(torch, F, bgr, depth, win, vname)
        assert name.startswith(f"w{win}-pk") and (vname is None or name == vname), (key, name)
        _outputs[key] = (p, got)
    return _outputs[key]


_generic_outputs = {}


def _generic(torch, F, inputs, si, win, dk, gk):
    """the reference-shaped generic kernel's output on the same launch (run once per module)"""
    key = (si, win, dk, gk)
    if key not in _generic_outputs:
        bgr, depth = inputs[(si, dk, gk)]
        _, name, out = K.launch(torch, F, bgr, depth, win, K.GENERIC)
        assert name == K.GENERIC, name
        _generic_outputs[key] = out
    return _generic_outputs[key]


def _sha(a):
    return hashlib.sha256(np.ascontiguousarray(a, np.float32).tobytes()).digest()


def test_cases_hold_what_they_claim(torch_cuda, F, inputs):
    from tools.hooks import stage
    for (si, dk, gk), (bgr, depth) in inputs.items():
        w, h, n = K.SIZES[si]
        assert depth.shape == (n, h, w) and bgr.shape == (n, h, w, 3)
        frac = float((depth <= 50.0).mean())
        want = {"valid": (0.0, 0.0), "random": (0.25, 0.35), "block": (0.3, 0.95), "one": (0.99, 1.0), "centre": (0.01, 0.06)}[dk]
        assert want[0] <= frac <= want[1], (si, dk, frac)
        assert np.isfinite(depth).all()
    d = inputs[(0, "random", "flat")][1]
    assert {0.0, 50.0, -1.0} <= set(np.unique(d[d <= 50.0]).tolist()) and (d == np.float32(49.999)).any()
    assert int((inputs[(0, "one", "flat")][1] > 50.0).sum()) == K.SIZES[0][2]
    d = inputs[(0, "centre", "flat")][1][0]
    assert d[2, 3] == 50.0 and (d[1:4, 2:5] > 50.0).sum() == 8          # an invalid centre, every neighbour valid
    # the wavefronts of the window-11 built-in kernel run all four rule bodies on the split guide, the body without rules and
    # the depth-only one on the flat guide (counters of the stage build: bit 0 = colour rule, bit 1 = depth rule)
    bgr, depth = inputs[(0, "random", "split")]
    bodies = stage.jbf_stage_run(K.params(F, 11), depth, bgr, -1)[2]
    print("window 11, random depths, split guide: bodies", bodies[:4].tolist())
    assert (bodies[:4] > 0).all(), bodies[:4]
    bgr, depth = inputs[(0, "random", "flat")]
    bodies = stage.jbf_stage_run(K.params(F, 11), depth, bgr, -1)[2]
    assert bodies[0] > 0 and bodies[2] > 0 and bodies[1] == 0 and bodies[3] == 0, bodies[:4]


@pytest.mark.parametrize("vkey", [v[0] for v in K.VARIANTS])
@pytest.mark.parametrize("si", range(len(K.SIZES)))
def test_bits_pinned_stage_build_and_oracle_bar(torch_cuda, F, pin, inputs, si, vkey):
    from tools.hooks import stage
    _, win, vname = next(v for v in K.VARIANTS if v[0] == vkey)
    bad = []
    for dk in K.DEPTHS:
        for gk in K.GUIDES:
            key = K.pin_key(si, vkey, dk, gk)
            bgr, depth = inputs[(si, dk, gk)]
            p, got = _product(torch_cuda, F, inputs, si, vkey, dk, gk)
            # (a) the bits
            if _sha(got) != pin["sha"][key]:
                bad.append(key)
            if key in K.FULL_OUTPUTS:
                diff = got.view(np.uint32) != pin["full"][key].view(np.uint32)
                print(f"{key}: {int(diff.sum())} of {diff.size} outputs differ from the pinned output")
                assert not diff.any(), f"{key}: outputs differ from the pin, first at {np.argwhere(diff)[:5].tolist()}"
            # every output of a window that holds no valid tap is 0, the others are not (flat guide: no weight underflows)
            if dk == "one" and gk == "flat":
                (_, h, w), r = depth.shape, win // 2
                cy, cx = h // 2, w // 3
                reach = (min(cy + r, h - 1) - max(cy - r, 0) + 1) * (min(cx + r, w - 1) - max(cx - r, 0) + 1)
                assert np.count_nonzero(got) == depth.shape[0] * reach, key
            # (b) the stage build, the whole batch
            sout = stage.jbf_stage_run(p, depth, bgr, K.variant_index(F, vname))[0]
            assert stage.bits_equal(sout, got), f"{key}: the stage build's output differs from the product library's"
            # (c) the stage-wise bar (first frame of the batch); no pixel may be excused to an interval
            if vkey in K.ORACLE_KEYS:
                r = assert_k1_stagewise(p, depth[0], bgr[0], got[0], variant=K.variant_index(F, vname), what=f"invalid taps {key}",
                                        band_max=0.0)
                print(f"{key}: strict max rel {r['max_rel_strict']:.2e}, band {r['band']}")
                ref0 = _generic(torch_cuda, F, inputs, si, win, dk, gk)
                assert np.array_equal(got == 0, ref0 == 0), f"{key}: zero mask differs from the reference-shaped kernel's"
    assert not bad, f"{len(bad)} launches differ from the pinned sha256: {bad[:6]}"


@pytest.mark.parametrize("vkey", sorted(K.NOELIDE_TWIN))
def test_equal_to_the_noelide_twin(torch_cuda, F, inputs, vkey):
    for si, dk, gk in K.case_keys():
        got = _product(torch_cuda, F, inputs, si, vkey, dk, gk)[1]
        twin = _product(torch_cuda, F, inputs, si, K.NOELIDE_TWIN[vkey], dk, gk)[1]
        diff = got.view(np.uint32) != twin.view(np.uint32)
        assert not diff.any(), f"{K.pin_key(si, vkey, dk, gk)}: {int(diff.sum())} outputs differ from the -noelide twin's"


@pytest.mark.parametrize("guard", K.GUARD_SIGMAS, ids=[g[0] for g in K.GUARD_SIGMAS])
def test_colour_sigma_guard(torch_cuda, F, pin, inputs, guard):
    """the tuned kernels serve kc = log2(e) / (2 sigma_c^2) > 1e-34, where kc * 2^126 drives exp2 to 0; beyond it the generic
    kernel runs, as before"""
    gname, sigma, tuned = guard
    for si in range(len(K.SIZES)):
        bgr, depth = inputs[(si, "random", "split")]
        _, name, got = K.launch(torch_cuda, F, bgr, depth, 11, None, color_sigma=sigma)
        assert name.startswith("w11-pk") == tuned and (tuned or name.startswith("generic")), (gname, name)
        assert _sha(got) == pin["sha"][f"guard_s{si}_{gname}"], f"sigma_c {sigma:g} ({name}), frame set {si}: output differs from the pin"
