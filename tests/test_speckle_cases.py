"""The statement of DepthSpeckleFilter (tests/speckle_cases.py) on cases whose answer is known in closed form, without a GPU.
Where scipy imports, the labelling is cross-checked against scipy.sparse.csgraph.connected_components over the same links."""
import numpy as np
import pytest

import speckle_cases as SC

F = np.float32


def _run(name, f=0, **over):
    return SC.filter_parts(SC.depth_frames(name)[f], **SC.params(name, **over))


def test_one_pixel():
    for f, valid in ((0, True), (1, False), (2, False)):
        p = _run("one_pixel", f, min_size=1)
        assert p["z"][0, 0] == (1000.0 if valid else 0.0) and p["labels"][0, 0] == (0 if valid else -1)
        assert (p["removed"], p["components"]) == (0, int(valid))
        p = _run("one_pixel", f, min_size=2)
        assert p["z"][0, 0] == 0.0 and p["labels"][0, 0] == -1 and (p["removed"], p["components"]) == (int(valid), 0)


@pytest.mark.parametrize("conn", (4, 8))
def test_identity_stairs_and_all_invalid(conn):
    for name in ("identity", "stairs"):
        for f in range(3):
            d = SC.depth_frames(name)[f]
            p = _run(name, f, connectivity=conn)
            assert (p["z"] == d).all() and (p["labels"] == 0).all() and (p["removed"], p["components"]) == (0, 1)
    for f in range(3):
        p = _run("all_invalid", f, connectivity=conn, min_size=1)
        assert (p["z"] == 0).all() and (p["labels"] == -1).all() and (p["removed"], p["components"]) == (0, 0)


def test_checker():
    w, h = SC.CASES["checker"].size
    for f in range(3):
        p = _run("checker", f, connectivity=4, min_size=1)
        assert (p["labels"] == np.arange(w * h).reshape(h, w)).all() and p["components"] == w * h
        p = _run("checker", f, connectivity=4)
        assert (p["z"] == 0).all() and p["removed"] == w * h and p["components"] == 0
        p = _run("checker", f, connectivity=8)
        y, x = np.mgrid[0:h, 0:w]
        assert (p["labels"] == (x + y) % 2).all() and (p["removed"], p["components"]) == (0, 2)


@pytest.mark.parametrize("conn", (4, 8))
def test_snake(conn):
    w, h = SC.CASES["snake"].size
    for f in range(3):
        n = SC.snake_length(f)
        d = SC.depth_frames("snake")[f]
        assert int((d > 0).sum()) == n > 2000
        p = _run("snake", f, connectivity=conn, min_size=n)
        first = int(np.flatnonzero(d.reshape(-1) > 0)[0])
        assert (p["z"] == d).all() and (p["labels"][d > 0] == first).all() and (p["removed"], p["components"]) == (0, 1)
        p = _run("snake", f, connectivity=conn, min_size=n + 1)
        assert (p["z"] == 0).all() and (p["removed"], p["components"]) == (n, 0)
    # it crosses the seams of a 32 x 16 tiling many times
    (a, _), _ = SC.seam_pairs(SC.depth_frames("snake")[0], 10.0, 0.02, 4)
    assert a.size == 25 * 3 + 3                                 # 25 runs over the seams at 32, 64 and 96; 3 of the 24 joints over a row seam


def test_comb_and_corner():
    for f, comps in ((0, 1), (1, 1), (2, 2)):
        p = _run("comb", f)
        assert p["components"] == comps and p["removed"] == 0
        assert set(np.unique(p["labels"])) == ({-1, 2 * 96 + 4} if comps == 1 else {-1, 2 * 96 + 4, 5 * 96 + 4})
    for f in range(3):
        for conn in (4, 8):
            p = _run("corner", f, connectivity=conn)
            assert (p["removed"], p["components"]) == (7 + 4, 1) and int((p["z"] > 0).sum()) == 8
            q = _run("corner", f, connectivity=conn, min_size=1)
            assert q["labels"][31, 31] == 31 * 96 + 31 and q["labels"][31, 64] == 31 * 96 + 64
            assert q["labels"][32, 32] == (32 * 96 + 32 if conn == 4 else 31 * 96 + 31)
            assert q["labels"][32, 63] == (32 * 96 + 63 if conn == 4 else 31 * 96 + 64)
            assert q["components"] == (6 if conn == 4 else 4)


def test_exact_and_rounding():
    w, h = SC.CASES["exact"].size
    for f in range(3):
        p = _run("exact", f, min_size=1)
        assert p["components"] == 2
        sizes = sorted(int(s) for s in p["sizes"] if s)
        assert sizes == ([20 * h, 40 * h] if f < 2 else [6 * w, 14 * w])
    pairs = SC._rounding_pairs(**SC.CASES["rounding"].params)
    assert sorted(k for _, _, k in pairs) == [False] * 4 + [True] * 4
    for a, b, kept in pairs:
        z = np.array([[a, b]], np.float32)
        sep = bool(SC.linked(z[:, :1], z[:, 1:], 0.7, 0.3)[0, 0])
        fused = bool(np.float64(b) - np.float64(a) <= np.float64(F(np.float64(F(0.7)) + np.float64(F(0.3)) * np.float64(a))))
        assert sep == kept and fused != kept
    for f in range(3):
        p = _run("rounding", f)
        assert (p["components"], p["removed"]) == (4, 8)


def test_exact_only_and_noise():
    for f in range(3):
        d = SC.depth_frames("exact_only", integer=True)[f].astype(np.uint16)
        p = SC.filter_parts(d, **SC.params("exact_only", min_size=1))
        a, b = SC.links(SC.sanitise(d), 0.0, 0.0, 4)
        assert (d.reshape(-1)[a] == d.reshape(-1)[b]).all() and a.size > 100
        lab = p["all_labels"]
        assert (d.reshape(-1)[lab.reshape(-1)] == d.reshape(-1)).all()
        p = _run("noise", f, min_size=1)
        assert p["components"] > 0.8 * 100 * 50


@pytest.mark.parametrize("name", SC.IDS)
@pytest.mark.parametrize("conn", (4, 8))
def test_against_scipy(name, conn):
    csgraph = pytest.importorskip("scipy.sparse.csgraph")
    sparse = pytest.importorskip("scipy.sparse")
    for f in range(3):
        d = SC.depth_frames(name)[f]
        kw = SC.params(name, connectivity=conn, min_size=SC.min_size_of(name, f))
        p = SC.filter_parts(d, **kw)
        z = SC.sanitise(d, kw["z_min"], kw["z_max"])
        a, b = SC.links(z, kw["max_diff"], kw["rel_diff"], conn)
        n = z.size
        _, comp = csgraph.connected_components(sparse.coo_matrix((np.ones(a.size), (a, b)), shape=(n, n)), directed=False)
        first = np.full(comp.max() + 1, n)
        np.minimum.at(first, comp, np.arange(n))
        want = np.where(z.reshape(-1) > 0, first[comp], -1)
        assert (p["all_labels"].reshape(-1) == want).all()
        sizes = np.bincount(want[want >= 0], minlength=n)
        keep = (want >= 0) & (sizes[np.maximum(want, 0)] >= kw["min_size"])
        assert ((p["z"].reshape(-1) > 0) == keep).all() and p["removed"] == int(((want >= 0) & ~keep).sum())


def test_the_frame_case_has_what_it_is_there_for():
    z, base, injected = SC.injected_frame(0, 96, 64)
    assert injected.sum() > 50 and np.isnan(z).any() and np.isinf(z).any() and (z == 7000.0).any()
    p = SC.filter_parts(z, **SC.params("frame"))
    assert p["removed"] > 0 and p["components"] >= 1
