"""The invalid-tap marker of K1's packed kernels (csrc/jbf_fast.hip: kInvalidHBits, kMinKc), restated in float32 numpy.

An invalid pixel (depth <= 50 mm or outside the image) is staged with the colour-code term h_q = -2^126 instead of
-(2^24 - 2^18 + |b|^2).  The value chain of unit_arg then gives, per tap,
    w   = fma(2^23 + a.b, 2, h_q)          ncd = w + negC,  negC = -(2^18 + |a|^2)
    without the colour rule:  a1 = fma(ncd, kc, ls)                     -> exp2(a1) must be exactly 0
    with the colour rule:     a1 = fma(ncd, kc * clamp(ncd + Tc), ls)   -> must be exactly ls (the validity factor removes the tap)
fma is evaluated in binary64 and rounded once (every product here is exact in binary64)."""
import os
import re

import numpy as np
import pytest

from conftest import ROOT

SRC = os.path.join(ROOT, "kinectdepthmapenhancement_amd", "csrc", "jbf_fast.hip")
LOG2E = 1.4426950408889634
LS_MAX = 24.0            # log2 of a spatial weight <= 1 at the 2^24 scale of the sums (kScaleLog2)
FLUSH = -150.0           # v_exp_f32 returns 0 below 2^-126; the kernel's header comment puts the sums' zero point at 2^-150


def fma32(a, b, c):
    with np.errstate(over="ignore", invalid="ignore"):
        return (np.asarray(a, np.float32).astype(np.float64) * np.asarray(b, np.float32).astype(np.float64)
                + np.asarray(c, np.float32).astype(np.float64)).astype(np.float32)


@pytest.fixture(scope="module")
def consts():
    src = open(SRC).read()
    bits = int(re.search(r"kInvalidHBits\s*=\s*0x([0-9A-Fa-f]+)u", src).group(1), 16)
    min_kc = float(re.search(r"kMinKc\s*=\s*([0-9.eE+-]+);", src).group(1))
    assert re.search(r"kc > kMinKc", src), "jbf_fast_supported no longer states the bound"
    return np.array([bits], np.uint32).view(np.float32)[0], min_kc


def test_marker_is_huge_negative_and_finite(consts):
    marker, _ = consts
    assert np.isfinite(marker) and marker == np.float32(-2.0 ** 126) and marker <= -np.finfo(np.float32).max / 4


def test_colour_terms_leave_it_finite(consts):
    marker, _ = consts
    ab = np.array([0, 1, 255, 65025, 130050, 195075], np.float64)              # a.b over BGR bytes: 0 .. 3 * 255^2
    na = np.array([0, 1, 65025, 195075], np.float64)                            # |a|^2
    two_ab = (2.0 ** 23 + ab).astype(np.float32)                                # the dot product's float result
    w = fma32(two_ab, np.float32(2.0), marker)
    neg_c = (-(2.0 ** 18 + na)).astype(np.float32)
    ncd = (w[:, None] + neg_c[None, :]).astype(np.float32)
    assert np.isfinite(w).all() and np.isfinite(ncd).all()
    assert (w == marker).all() and (ncd == marker).all()                        # the marker swallows every colour term


def test_weight_is_zero_for_every_kc_the_guard_admits(consts):
    marker, min_kc = consts
    # kc as the launcher forms it, (float)(log2(e) / (2 sigma_c^2)): from just above the bound to the upper bound 1e30
    kc = np.concatenate([[np.nextafter(np.float32(min_kc), np.float32(1))], np.float32(min_kc) * np.float32(1.001) ** np.arange(1, 50),
                         np.logspace(-33.9, 30, 400)]).astype(np.float32)
    kc = kc[(kc.astype(np.float64) > min_kc) & (kc < 1e30)]
    assert len(kc) > 400
    a1 = fma32(marker, kc, np.float32(LS_MAX))
    assert not np.isnan(a1).any() and (a1 < FLUSH).all(), float(a1.max())
    # pass 2 subtracts t^2 >= 0 (or nothing, when the depth rule skips the factor): the argument only falls
    t = np.float32(37.5)
    assert (fma32(-t, t, a1) <= a1).all()
    # practical sigmas are far inside: sigma_c = 1e6
    assert LOG2E / (2.0 * 1e6 ** 2) > 1e20 * min_kc
    # the other side of the bound is refused.  The bound is conservative (174 / 2^126 = 2.0e-36 is where the argument reaches
    # the flush point); from a hundredth of it downward the marker's argument stays above the flush point: a weight would survive
    for kc_out in (np.float32(1e-38), np.float32(1e-36), np.nextafter(np.float32(min_kc), np.float32(0)) * np.float32(0.01)):
        assert kc_out.astype(np.float64) <= min_kc
        a1_out = fma32(marker, kc_out, np.float32(LS_MAX))
        assert a1_out > FLUSH, (float(kc_out), float(a1_out))


def test_rule_body_chain_gives_exactly_ls(consts):
    marker, _ = consts
    ncd = marker
    for cd_skip in (1, 12170, 195075):
        m = np.clip(np.float32(ncd + np.float32(cd_skip)), np.float32(0), np.float32(1))      # v_pk_add_f32 ... clamp
        assert m == 0
        for kc in (np.float32(1.1e-34), np.float32(0.0123), np.float32(9e29)):
            kcm = np.float32(kc * m)
            for ls in (np.float32(0.0), np.float32(24.0), np.float32(-3.4028235e38), np.float32(17.123456), np.float32(-126.5)):
                a1 = fma32(ncd, kcm, ls)
                assert a1.view(np.uint32) == np.float32(ls).view(np.uint32), (cd_skip, kc, ls, a1)
    # why the marker is not -inf: the same chain gives NaN
    assert np.isnan(fma32(np.float32(-np.inf), np.float32(0.0), np.float32(24.0)))
