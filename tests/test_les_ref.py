"""The CPU checker of LabelEquivalenceSeg::labelImage (tools/les_ref.c, per pixel and per round) against an independent
numpy transcription (tests/les_cases.py), micro-cases with answers worked by hand, the L4 bound against the binary64
per-pixel sums, and the goldens.  Definition and L1-L7: DESIGN.md, "Superpixel merging"."""
import math
import os

import numpy as np
import pytest

import les_cases as LC
from les_cases import F

GOLDEN_ITS = (1, 3)


@pytest.fixture(scope="module")
def R():
    from tools import les_ref
    les_ref.build()
    return les_ref


def both(R, case, **kw):
    """checker and transcription on one case, compared bit for bit on every output"""
    ref = R.label_image(*case, **kw)
    tr = LC.np_label_image(*case, **kw)
    counts = LC.diff_counts(ref, tr, LC.OUTPUTS + ("input_nd", "changed"))
    assert not any(counts.values()), counts
    return ref, tr


def regions(out):
    return sorted(set(np.unique(out["merged_label"]).tolist()) - {-1})


def test_threshold_is_derived_the_same_way_twice(R):
    for c in (LC.MAX_ANGLE, F(3.141592653) / F(3.0), F(0.01), F(1.5), F(3.0), F(3.1415927), F(4.0), F(0.0), F(-1.0), F(np.nan)):
        a, b = R.acos_threshold(c), LC.acos_threshold(c)
        assert a.view(np.uint32) == b.view(np.uint32), (c, a, b)
    t = R.acos_threshold()
    assert abs(float(t) - math.cos(math.pi / 8)) < 1e-6
    assert R.acos_threshold(F(3.141592653) / F(3.0)).view(np.uint32) == 0x3F000000          # NA3's value
    assert R.acos_threshold(F(4.0)) < -1 and np.isinf(R.acos_threshold(F(0.0)))


def test_comp_normal_quirks(R):
    """L6: identical normals (d == 1.0f) and d > 1 by rounding do not pass; NaN fails; the distance test is strict"""
    t = R.acos_threshold()
    z = (0.0, 0.0, 1.0)
    assert R.comp_normal(LC.tilted(10).tolist() + [1000.0], z + (1000.0,), t)
    assert not R.comp_normal(z + (1000.0,), z + (1000.0,), t)
    assert not R.comp_normal((0.0, 0.0, 1.0000001, 1000.0), z + (1000.0,), t)
    assert not R.comp_normal(LC.tilted(30).tolist() + [1000.0], z + (1000.0,), t)
    assert not R.comp_normal((np.nan, 0.0, 1.0, 1000.0), z + (1000.0,), t)
    assert not R.comp_normal(LC.tilted(10).tolist() + [np.nan], z + (1000.0,), t)
    assert R.comp_normal(LC.tilted(10).tolist() + [1149.99], z + (1000.0,), t)
    assert not R.comp_normal(LC.tilted(10).tolist() + [1150.0], z + (1000.0,), t)


def test_two_adjacent_superpixels(R):
    ref, _ = both(R, LC.two_halves(10))
    assert regions(ref) == [0] and ref["size"].tolist() == [96, 0]
    # region 0: the average of 48 x (0,0,1) and 48 x tilted(10), binary32
    n1 = LC.tilted(10)
    sx = (F(48) * F(0) + F(48) * n1[0]) / F(96)
    sz = (F(48) * F(1) + F(48) * n1[2]) / F(96)
    assert ref["merged_nd"][0, 0, 0] == sx and ref["merged_nd"][0, 0, 2] == sz and (ref["merged_nd"] == ref["merged_nd"][0, 0]).all()
    assert ref["changed"].tolist() == [48] + [0] * 9
    ref, _ = both(R, LC.two_halves(30))
    assert regions(ref) == [0, 1] and ref["size"].tolist() == [48, 48] and not ref["changed"].any()
    ref, _ = both(R, LC.two_halves(10, extra_distance=200.0))
    assert regions(ref) == [0, 1]
    ref, _ = both(R, LC.two_halves(0))                       # identical normals: the L6 quirk
    assert regions(ref) == [0, 1]
    # variance of an unmerged region: dot(n, n) / size summed over its pixels
    n0 = np.array([0, 0, 1], F)
    assert ref["variance"][0] == F(48) * (((n0[0] * n0[0] + n0[1] * n0[1]) + n0[2] * n0[2]) / F(48))


def test_wrap_is_a_directed_edge(R):
    ref, _ = both(R, LC.wrap_case(swapped=False))
    m = ref["merged_label"]
    assert m[2, 15] == 1 and m[3, 0] == 1 and (np.delete(m.reshape(-1), [2 * 16 + 15, 3 * 16]) == 0).all()
    assert ref["size"].tolist() == [94, 2, 0]
    ref, _ = both(R, LC.wrap_case(swapped=True))
    m = ref["merged_label"]
    assert m[2, 15] == 1 and m[3, 0] == 2 and ref["size"].tolist() == [94, 1, 1]


def test_last_row_and_last_column(R):
    """L2 bound: the right neighbour of the last pixel and the down neighbours of the last row are past W*H"""
    normals = np.stack([LC.tilted(0), LC.tilted(10)])
    centers = (F(1000) * normals).astype(F)
    labels = np.ones((4, 8), np.int32)
    labels[3, 7] = 0                                          # superpixel 0 is the last pixel alone
    ref, _ = both(R, (normals, labels, centers))
    assert (ref["merged_label"] == 0).all()                   # (6,3) sees it to its right, (7,2) below
    labels = np.zeros((4, 8), np.int32)
    labels[3, 7] = 1
    ref, _ = both(R, (normals, labels, centers))
    assert (ref["merged_label"] == 0).all()
    labels = np.zeros((4, 8), np.int32)
    labels[3, :] = 1                                          # a whole last row
    ref, _ = both(R, (normals, labels, centers))
    assert (ref["merged_label"] == 0).all() and ref["size"].tolist() == [32, 0]
    for W, H in ((1, 9), (9, 1)):
        labels = (np.arange(W * H).reshape(H, W) >= 4).astype(np.int32)
        ref, _ = both(R, (normals, labels, centers))
        assert (ref["merged_label"] == 0).all()


def test_pixels_without_superpixel_and_bad_normals(R):
    """L1, L5, L7"""
    normals = np.stack([LC.tilted(0), np.full(3, -1, F), LC.tilted(10), np.array([-1, -1, 0.5], F)])
    centers = (F(1000) * normals).astype(F)
    labels = np.zeros((6, 16), np.int32)
    labels[:, 4:8] = 1            # bad normal
    labels[:, 8:12] = 2
    labels[:, 12:] = 3            # (-1, -1, z): valid for initLabel, dropped by countKernel's test (L7)
    labels[0, 0], labels[5, 9], labels[2, 2] = -1, 4, 1 << 20
    ref, _ = both(R, (normals, labels, centers))
    m = ref["merged_label"]
    assert (m[:, 4:8] == -1).all() and (m[:, 12:] == -1).all() and m[0, 0] == -1 and m[5, 9] == -1 and m[2, 2] == -1
    assert (ref["merged_nd"][m == -1] == 0).all() and (ref["input_nd"][labels == 1] == 5).all()
    assert (ref["input_nd"][labels == 3][:, :2] == -1).all()
    assert regions(ref) == [0, 2] and ref["size"].tolist() == [22, 0, 23, 0]


def test_unconverged_chain(R):
    """row 0 makes the first 17 pixels ineligible for L3 phase 1, so labels travel one hop per round"""
    ref, _ = both(R, LC.chain_case(row0_valid=False))
    assert [int(ref["merged_label"][1, 4 * k]) for k in range(16)] == [max(k - 10, 0) for k in range(16)]
    assert (ref["merged_label"][0] == -1).all() and (ref["changed"] > 0).all()
    for it in (15, 16, 20):
        ref, _ = both(R, LC.chain_case(row0_valid=False), iterations=it)
        assert (ref["merged_label"][1:] == 0).all()
    ref, _ = both(R, LC.chain_case(row0_valid=False), iterations=14)
    assert ref["merged_label"][1, 63] == 1
    ref, _ = both(R, LC.chain_case(row0_valid=True))
    assert (ref["merged_label"][1:] == 0).all() and (ref["merged_label"][0] == 16).all()


@pytest.mark.parametrize("seed,W,H,nc", LC.RANDOM_SHAPES)
def test_random_cases_against_the_transcription(R, seed, W, H, nc):
    case = LC.random_case(seed, W, H, nc)
    ref, tr = both(R, case)
    check_l4_bound(ref, tr)
    for kw in ({"iterations": 0}, {"iterations": 1}, {"max_angle": F(1.2), "max_plane_distance": F(30.0)}, {"max_angle": F(4.0), "max_plane_distance": F(1e9)}):
        both(R, case, **kw)


def test_random_cases_are_not_trivial(R):
    case = LC.random_case(5, 64, 48, 40)
    ref = R.label_image(*case)
    assert (case[1] == -1).any() and (case[1] >= 40).any() and np.isnan(case[0]).any() and (case[0] == -1).all(1).any()
    valid = len(set(np.unique(case[1][ref["merged_label"] > -1]).tolist()))
    assert 1 < len(regions(ref)) < valid and ref["changed"][0] > 0


def check_l4_bound(ref, tr):
    """every L4 sum within gamma_m * sum |c_A v_A| of the per-pixel sum in binary64, m = members + 1"""
    u = 2.0 ** -24
    checked = 0
    for m, s in tr["sums"].items():
        mem = tr["members"][m]
        k = len(mem) + 1
        gamma = k * u / (1 - k * u)
        for j in range(7):
            terms = [float(e[1]) * float(e[2 + j]) for e in mem]
            if not all(math.isfinite(t) for t in terms):
                continue
            exact = math.fsum(terms)                       # = the per-pixel binary64 sum (c_A equal terms each)
            assert abs(float(s[j]) - exact) <= gamma * math.fsum(abs(t) for t in terms), (m, j, float(s[j]), exact)
            checked += 1
        assert ref["variance"][m].view(np.uint32) == F(s[6]).view(np.uint32) or (np.isnan(ref["variance"][m]) and np.isnan(s[6]))
    return checked


@pytest.mark.parametrize("it", GOLDEN_ITS)
def test_goldens(R, it):
    case = LC.golden_inputs(it)
    ref, tr = both(R, case)
    assert check_l4_bound(ref, tr) > 300
    g = np.load(os.path.join(LC.GOLDEN, f"les_it{it}.npz"))
    assert np.array_equal(ref["merged_label"], g["merged_label"].astype(np.int32))
    assert np.array_equal(LC.ubits(ref["merged_nd"]), g["merged_nd"]) and np.array_equal(LC.ubits(ref["input_nd"]), g["input_nd"])
    assert np.array_equal(ref["size"], g["size"]) and np.array_equal(LC.ubits(ref["variance"]), g["variance"])
    assert np.array_equal(ref["changed"], g["changed"])
    # not vacuous
    valid = len(set(np.unique(case[1][ref["merged_label"] > -1]).tolist()))
    assert 1 < len(regions(ref)) < valid, (len(regions(ref)), valid)
    assert (ref["changed"] > 0).sum() >= 2, ref["changed"]
    lab = case[1]
    wrap = (lab[:-1, -1] != lab[1:, 0]) & (ref["merged_label"][:-1, -1] > -1) & (ref["merged_label"][1:, 0] > -1)
    assert wrap.sum() > 100                                    # L2's wrap pairs with distinct valid labels
    print(f"it{it}: {valid} superpixels -> {len(regions(ref))} regions, changed per round {ref['changed'].tolist()}, wrap pairs {int(wrap.sum())}")
