"""tests/spdsr_tail_cases.py without a GPU: the crafted cases hold what they claim, and its two binary64 references agree
with the float32 restatement of oracle/ (okde_spdsr_cluster_planes, okde_projection_plane) within the bars the GPU test
(tests/test_gpu_spdsr_tail.py) holds the kernels to -- two independent restatements checking each other."""
import numpy as np
import pytest

import spdsr_tail_cases as SC

# the float32 restatement against binary64: 25 taps of (difference, square, sum, division, product, two accumulations) and the
# final division, each rounded to 2^-24 relative; the sums are of same-signed terms, so the errors add at most linearly
E32_BOUND = (25 * 7 + 1) * 2.0 ** -24


def pts_as_f32(p):
    """oracle float3 record array -> float32 [...,3]"""
    return p.view(np.float32).reshape(p.shape + (3,))


def f3(oracle, pts):
    return np.ascontiguousarray(pts, np.float32).view(oracle.FLOAT3).reshape(pts.shape[:-1])


@pytest.mark.parametrize("name", list(SC.FIT_CASES))
def test_fit_case_holds_its_features(name):
    c = SC.fit_case(name)
    w, h, k = c["w"], c["h"], c["k"]
    lab = c["labels"].reshape(-1)
    valid = (lab >= 0) & (lab < k)
    change = valid[1:] & valid[:-1] & (lab[1:] != lab[:-1])
    pos = (np.arange(1, lab.size) % 8)[change]
    assert set(pos.tolist()) == set(range(8)), "a label change at each of the 8 positions of a register run"
    if w % 8:
        ends = np.arange(1, h) * w                                  # first pixel of rows 1..h-1
        inside = ends[(ends % 8 != 0)]
        assert any(valid[e - 1] and valid[e] and lab[e - 1] != lab[e] for e in inside), "a run with a label change across a row end"
    assert (lab.size % 8 != 0) or (lab.size % 2048 != 0) or name == "lds-1024"
    assert name != "odd-8" or (lab.size == 1407 and lab.size < 2048)
    assert name != "global-1056" or k > 1024
    assert name != "lds-1024" or k == 1024
    counts = np.bincount(lab[valid], minlength=k)
    for l, left in c["starved"].items():
        assert counts[l] == left
    assert set(c["starved"].values()) == {0, 1, 2, 3}
    assert (lab == k + 5).mean() > 0.01 and (lab == -1).any() and (lab == -7).any()
    assert counts[c["nan_cluster"]] >= 3 and np.isnan(c["points"][c["labels"] == c["nan_cluster"]]).sum() == 1
    assert np.isfinite(c["points"][c["labels"] != c["nan_cluster"]]).all()
    A, B, row = c["band"]
    assert counts[A] >= 3 and counts[B] >= 3 and set(np.unique(c["labels"][row:row + 2])) <= {A, B, k + 5, -1, -7}
    assert (np.bincount(c["full_labels"].reshape(-1), minlength=k) >= 3).all()


@pytest.mark.parametrize("name", list(SC.FIT_CASES) + ["micro"])
def test_fit_case_is_well_conditioned_and_planes64_agrees_with_the_oracle(oracle, name):
    c = SC.fit_micro_case() if name == "micro" else SC.fit_case(name)
    ref = SC.planes64(c["labels"], c["points"], c["k"])
    live = (ref["nd"][:, 0] != 5.0) & ~np.isnan(ref["nd"][:, 0])
    skip = [5] if name == "micro" else []                           # the collinear cluster: invariants only
    live[skip] = False
    assert ref["gap"][live].min() >= 1e-6
    z, proj, den = SC.plane_fitted64(ref["nd"], c["labels"], c["points"], c["tx"], c["ty"])
    ok = proj & ~np.isin(c["labels"], skip)
    assert ok.mean() > 0.3 and den[ok].min() >= 0.5
    nd = oracle.spdsr_cluster_planes(c["labels"], f3(oracle, c["points"]), c["k"])
    SC.planes_compare(nd, ref, name, skip)
    pf, _ = oracle.projection_plane(nd, c["labels"], f3(oracle, c["points"]), c["K"], 0)
    z, proj, den = SC.plane_fitted64(nd, c["labels"], c["points"], c["tx"], c["ty"])
    ok = proj & ~np.isin(c["labels"], skip)
    assert SC.ulps32(pf["z"][ok], z[ok]).max() <= 8.0
    assert np.array_equal(pts_as_f32(pf)[~proj].view(np.uint32), c["points"][~proj].view(np.uint32))


def test_micro_clusters_are_what_they_claim(oracle):
    c = SC.fit_micro_case()
    ref = SC.planes64(c["labels"], c["points"], c["k"])
    nd, cnt = ref["nd"], ref["count"]
    assert cnt[0] == 3 and nd[0, 0] != 5.0
    assert np.linalg.norm(ref["mean"][1]) > 14000 and abs(ref["mean"][1][0]) > 2900
    assert np.array_equal(nd[2], np.float32([0, 0, 1, 1250]))
    assert np.array_equal(nd[3], np.float32([1, 0, 0, 750])) and np.array_equal(nd[4], np.float32([-1, 0, 0, 750]))
    for nd_side in (nd, oracle.spdsr_cluster_planes(c["labels"], f3(oracle, c["points"]), c["k"])):
        n = nd_side[5, :3].astype(np.float64)
        assert abs(np.linalg.norm(n) - 1.0) <= 1e-6 and abs(n @ c["direction"]) <= 1e-6
        assert SC.ulps32(nd_side[5, 3], abs(n @ ref["mean"][5])) <= 2.0
    # x = const: |nx| < 1 fails and the pixels come back unprojected
    _, proj, _ = SC.plane_fitted64(nd, c["labels"], c["points"], c["tx"], c["ty"])
    assert not proj[np.isin(c["labels"], (3, 4))].any() and proj[c["labels"] == 2].all()


def test_marker_keeps_w_in_both_restatements(oracle):
    c = SC.fit_case("odd-8")
    first = SC.planes64(c["full_labels"], c["full_points"], c["k"])["nd"]
    assert (first[:, 0] != 5.0).all()
    ref = SC.planes64(c["labels"], c["points"], c["k"], nd_prev=first)["nd"]
    got = oracle.spdsr_cluster_planes(c["labels"], f3(oracle, c["points"]), c["k"], nd_prev=first)
    marker = [l for l, left in c["starved"].items() if left < 3]
    assert len(marker) == 3
    for side in (ref, got):
        assert np.array_equal(side[marker, :3], np.full((3, 3), 5, np.float32))
        assert np.array_equal(side[marker, 3].view(np.uint32), first[marker, 3].view(np.uint32))


@pytest.mark.parametrize("name", list(SC.SWEEP_CASES))
def test_sweep_case_and_sweeps64_against_the_oracle(oracle, name):
    c = SC.sweep_case(name)
    pts, lab = c["points"], c["labels"]
    assert 0.03 < (pts[..., 2] <= 50).mean() < 0.08 and (lab[pts[..., 2] <= 50] == -1).all()
    assert ((lab == -1) & (pts[..., 2] > 50)).mean() > 0.01
    assert len(np.unique(c["nd"][np.unique(lab[lab >= 0])], axis=0)) >= 2
    res = {}
    for sweeps in SC.SWEEP_COUNTS:
        pf, opt = oracle.projection_plane(c["nd"], lab, f3(oracle, pts), c["K"], sweeps)
        pf, opt = pts_as_f32(pf), pts_as_f32(opt)
        z, proj, den = SC.plane_fitted64(c["nd"], lab, pts, c["tx"], c["ty"])
        assert den[proj].min() >= 0.5 and SC.ulps32(pf[..., 2][proj], z[proj]).max() <= 8.0
        ref = SC.sweeps64(pf[..., 2], pts[..., 2], sweeps)
        e32 = SC.sweep_compare(opt, ref, pts, c["tx"], c["ty"], f"{name} x{sweeps} (oracle)")
        assert e32 <= E32_BOUND, e32
        flagged = ref["flagged"].mean()
        assert flagged <= (SC.MAX_FLAGGED if sweeps > 1 else 0.0)
        res[sweeps] = (ref, opt, e32)
        print(f"{name} x{sweeps}: rewritten {ref['rewritten'].mean():.3f}, flagged {flagged:.4f}, smallest margin "
              f"{ref['margin'].min():.2e}, e32 {e32:.2e}")
    assert np.array_equal(res[0][1].view(np.uint32), pts.view(np.uint32)) and not res[0][0]["rewritten"].any()
    assert res[20][0]["rewritten"].mean() >= 0.5
    assert (res[20][1][..., 2] != res[1][1][..., 2]).mean() >= 0.05


def test_sweep_micro_taps(oracle):
    """a tap at exactly 50.0f is none, one at nextafter(50.0f) is: the pixels that see only the former stay at exactly 50.25"""
    c = SC.sweep_micro()
    h, w = c["h"], c["w"]
    pf, opt = oracle.projection_plane(c["nd"], c["labels"], f3(oracle, c["points"]), c["K"], 1)
    pf, opt = pts_as_f32(pf), pts_as_f32(opt)
    ref = SC.sweeps64(pf[..., 2], c["points"][..., 2], 1)
    assert ref["rewritten"].all() and not ref["flagged"].any()
    for side in (ref["z"], opt[..., 2]):
        assert (side[SC.window_of(SC.TAP_INVALID, h, w)] == 50.25).all()
        assert (side[SC.window_of(SC.TAP_VALID, h, w)] < 50.245).all()      # a full tap moves them by 5e-3 and more
        assert (side[:, :6] == 1000.0).all()
    SC.sweep_compare(opt, ref, c["points"], c["tx"], c["ty"], "micro taps (oracle)")


@pytest.mark.parametrize("item", SC.MICRO_ITEMS)
def test_sweep_micro_non_finite(oracle, item):
    c = SC.sweep_micro(item)
    h, w = c["h"], c["w"]
    y, x = SC.MICRO_AT
    for sweeps in (1, 2, 20):
        pf, opt = oracle.projection_plane(c["nd"], c["labels"], f3(oracle, c["points"]), c["K"], sweeps)
        pf, opt = pts_as_f32(pf), pts_as_f32(opt)
        ref = SC.sweeps64(pf[..., 2], c["points"][..., 2], sweeps)
        assert not ref["flagged"].any()
        SC.sweep_compare(opt, ref, c["points"], c["tx"], c["ty"], f"micro {item} x{sweeps} (oracle)")
        assert np.array_equal(opt[y, x].view(np.uint32), c["points"][y, x].view(np.uint32))       # the item itself is never rewritten
        nan = np.isnan(opt[..., 2])
        nan[y, x] = False
        if item == "plus_inf":      # its 24 neighbours: inf * 0 in the numerator
            assert np.array_equal(nan, SC.window_of(SC.MICRO_AT, h, w)) and nan.sum() == 24
            assert np.isnan(opt[nan]).all()
        else:
            assert not nan.any()
        if item == "pf_inf":
            assert np.isinf(pf[y, x, 2])
