"""The numpy statement of OrganizedMesh (mesh_cases.py) against itself: the vectorised form equals the loop over the quads on
every named case and on seeded frames, the named cases give the counts their sentences promise, and every mesh has the
properties a mesh of a depth grid must have.  No GPU."""
import numpy as np
import pytest

import cloud_cases as CC
import mesh_cases as MC

MODES = (MC.DIAG_AD, MC.DIAG_BC, MC.DIAG_ADAPTIVE)
SIZES = ((2, 2), (3, 3), (7, 5), (13, 9), (2, 11), (12, 2))


def _all_frames():
    for w, h in SIZES:
        for name, z, link in MC.frames(w, h):
            yield f"{name}-{w}x{h}", z, link


FRAMES = list(_all_frames())


def test_every_case_has_a_sentence_and_every_size_its_frames():
    assert set(MC.CASES) == {"plane", "one_hole", "corners", "step", "exact", "diagonal", "checker", "rim", "nan_inf", "salt"}
    assert all(len(what) > 30 for what, _ in MC.CASES.values())
    names = {n.split("-")[0].rstrip("0123456789") for n, _, _ in FRAMES}
    assert names == set(MC.CASES) | {"noisy", "exactfused"}
    assert sum(n.startswith("corners") for n, _, _ in FRAMES) == 4


@pytest.mark.parametrize("name,z,link", FRAMES, ids=[n for n, _, _ in FRAMES])
def test_vectorised_equals_scalar(name, z, link):
    for mode in MODES:
        for flip in (False, True):
            a = MC.triangles(z, diagonal=mode, flip_winding=flip, **link)
            b = MC.triangles_scalar(z, diagonal=mode, flip_winding=flip, **link)
            assert a.dtype == np.uint32 and a.shape == b.shape and np.array_equal(a, b), (name, mode, flip)


def test_vectorised_equals_scalar_on_seeded_frames_and_other_parameters():
    rng = np.random.default_rng(5)
    for i in range(12):
        w, h = int(rng.integers(2, 24)), int(rng.integers(2, 24))
        z = MC.noisy(w, h, 10 + i) + rng.uniform(-0.5, 0.5, (h, w)).astype(np.float32)
        kw = dict(z_min=float(rng.uniform(-10, 1400)), z_max=float(rng.uniform(1510, 1600)), max_diff=float(rng.uniform(0, 30)),
                  rel_diff=float(rng.uniform(0, 0.03)), diagonal=int(rng.integers(0, 3)), flip_winding=bool(rng.integers(0, 2)))
        a, b = MC.triangles(z, **kw), MC.triangles_scalar(z, **kw)
        assert np.array_equal(a, b), (i, kw)
    # the extremes of the link: nothing but equal depths, and everything
    z = MC.noisy(9, 7, 3)
    assert np.array_equal(MC.triangles(z, max_diff=0.0, rel_diff=0.0), MC.triangles_scalar(z, max_diff=0.0, rel_diff=0.0))
    assert MC.triangles(MC.plane(9, 7) * 0 + 700, max_diff=0.0, rel_diff=0.0).shape[0] == 2 * 8 * 6


def test_named_cases_give_what_their_sentences_say():
    for w, h in ((2, 2), (7, 5), (13, 9)):
        full = 2 * (w - 1) * (h - 1)
        for mode in MODES:
            assert MC.triangles(MC.plane(w, h), diagonal=mode).shape[0] == full
            if w >= 3:
                assert MC.triangles(MC.one_hole(w, h), diagonal=mode).shape[0] == full - 4
            assert MC.triangles(MC.checker(w, h), diagonal=mode).shape[0] == 0
            assert MC.triangles(MC.checker(w, h, 1), diagonal=mode).shape[0] == 0
            assert MC.triangles(MC.rim(w, h), diagonal=mode).shape[0] == 1
            assert MC.triangles(MC.diagonal(w, h), diagonal=mode).shape[0] == MC.diagonal_count(w, h, mode)
            assert MC.triangles(MC.exact(w, h), diagonal=mode).shape[0] == MC.exact_count(w, h, 0, mode)
    # the owner of rim's triangle is the invalid pixel (W-2, H-2): b, c, d in that order
    w, h = 7, 5
    v = MC.valid_mask(MC.rim(w, h))
    r = MC.ranks(v)
    assert MC.triangles(MC.rim(w, h)).tolist() == [[int(r[h - 2, w - 1]), int(r[h - 1, w - 2]), int(r[h - 1, w - 1])]]
    # one_hole: each missing-corner form once, around the hole
    z = MC.one_hole(7, 5)
    r = MC.ranks(MC.valid_mask(z))
    y, x = 5 // 2, 7 // 2
    R = lambda dx, dy: int(r[y + dy, x + dx])
    tri = [tuple(t) for t in MC.triangles(z, diagonal=MC.DIAG_AD).tolist()]
    assert (R(-1, -1), R(-1, 0), R(0, -1)) in tri           # d missing: (a, c, b)
    assert (R(0, -1), R(1, 0), R(1, -1)) in tri             # c missing: (a, d, b)
    assert (R(-1, 0), R(-1, 1), R(0, 1)) in tri             # b missing: (a, c, d)
    assert (R(1, 0), R(0, 1), R(1, 1)) in tri               # a missing: (b, c, d)
    # corners: the four forms in a 2 x 2 frame, by hand (ranks 0, 1, 2 of the three valid pixels)
    assert [MC.triangles(MC.corners(variant=k)).tolist() for k in range(4)] == [[[0, 1, 2]], [[0, 1, 2]], [[0, 2, 1]], [[0, 2, 1]]]
    # diagonal: the three modes differ as sets, the tie goes to a-d
    d = MC.diagonal(14, 2)
    sets = [set(map(tuple, MC.triangles(d, diagonal=m).tolist())) for m in MODES]
    assert sets[0] != sets[1] and sets[1] != sets[2] and sets[0] != sets[2]
    tie = MC.DIAGONAL_BLOCKS[0].reshape(2, 2)
    assert np.array_equal(MC.triangles(tie), MC.triangles(tie, diagonal=MC.DIAG_AD))
    assert not np.array_equal(MC.triangles(tie), MC.triangles(tie, diagonal=MC.DIAG_BC))
    # exact: linked at the threshold, not one ulp beyond; under FUSED_LINK a fused threshold would decide six more pairs
    # the other way
    assert [k for _, _, k in MC.rounding_pairs()] == [True] * 3 + [False] * 3
    pairs = MC.rounding_pairs(**MC.FUSED_LINK)
    assert [k for _, _, k in pairs] == [True] * 3 + [False] * 3 + [True] * 3 + [False] * 3
    r, m = np.float64(np.float32(0.3)), np.float64(np.float32(0.7))
    for a, b, kept in pairs[6:]:
        assert (np.float64(b) - np.float64(a) <= np.float64(np.float32(m + r * np.float64(a)))) != kept
    for w, h in ((2, 2), (13, 9)):
        for k in range(12):
            z = MC.exact(w, h, k, **MC.FUSED_LINK)
            assert MC.triangles(z, **MC.FUSED_LINK).shape[0] == MC.exact_count(w, h, k, **MC.FUSED_LINK)
    # step: no triangle has vertices on two surfaces
    for w, h in ((7, 5), (13, 9), (2, 2)):
        z = MC.step(w, h)
        side = MC.side_of_step(w, h)                        # every pixel is valid: rank == raster index
        t = MC.triangles(z)
        assert t.shape[0] > 0 or (w, h) == (2, 2)
        assert np.all(side[t[:, 0]] == side[t[:, 1]]) and np.all(side[t[:, 0]] == side[t[:, 2]])
    # nan_inf: no special value is a vertex
    z = MC.nan_inf(13, 9)
    assert MC.valid_mask(z).sum() == np.isfinite(z).sum() - (z == 0).sum() - (z == MC.Z_MIN).sum() - (z == MC.Z_MAX).sum()
    assert np.isnan(z).any() and np.isinf(z).any() and (z == MC.Z_MIN).any() and (z == MC.Z_MAX).any()
    assert 0.6 < MC.valid_mask(MC.salt(64, 48)).mean() < 0.8


@pytest.mark.parametrize("name,z,link", FRAMES, ids=[n for n, _, _ in FRAMES])
def test_properties(name, z, link):
    h, w = z.shape
    v = MC.valid_mask(z).reshape(-1)
    count = int(v.sum())
    pixel_of = np.flatnonzero(v)                            # vertex index -> raster index
    zf = z.reshape(-1)
    for mode in MODES:
        t = MC.triangles(z, diagonal=mode, **link)
        assert t.shape[0] <= 2 * (w - 1) * (h - 1)
        if t.shape[0] == 0:
            continue
        assert t.max() < count                                                              # every index < count
        assert np.all(t[:, 0] != t[:, 1]) and np.all(t[:, 1] != t[:, 2]) and np.all(t[:, 0] != t[:, 2])   # no repeated vertex
        p = pixel_of[t]                                                                     # [M, 3] raster indices
        for i, j in ((0, 1), (1, 2), (2, 0)):                                               # every edge linked
            assert np.all(MC.linked(zf[p[:, i]], zf[p[:, j]], True, True, **link)), (name, mode, i, j)
        x, y = (p % w).astype(np.int64), (p // w).astype(np.int64)
        cross = (x[:, 1] - x[:, 0]) * (y[:, 2] - y[:, 0]) - (y[:, 1] - y[:, 0]) * (x[:, 2] - x[:, 0])
        assert np.all(cross == -1), (name, mode)            # every triangle is half a pixel quad and turns the same way
        # the corners of a triangle lie in one quad, and triangles come in the raster order of their quads
        owner = y.min(axis=1) * w + x.min(axis=1)
        assert np.all(x.max(axis=1) - x.min(axis=1) == 1) and np.all(y.max(axis=1) - y.min(axis=1) == 1)
        assert np.all(np.diff(owner) >= 0) and np.all(np.bincount(owner) <= 2)
        f = MC.triangles(z, diagonal=mode, flip_winding=True, **link)                               # flip_winding swaps v1 and v2
        assert np.array_equal(f, t[:, [0, 2, 1]])
        assert MC.records(t).dtype.itemsize == 12 and MC.records(t).size == t.shape[0]


def test_vertices_are_the_dense_cloud():
    for w, h in ((7, 5), (13, 9)):
        K = CC.camera(w, h)
        bgr = CC.bgr_images(3, 1, h, w)[0]
        for name, z, _ in MC.frames(w, h):
            for pts in (MC.as_points(z), MC.as_points(z, K)):
                rec = MC.vertices(pts, bgr)
                assert rec.dtype == CC.POINT and rec.tobytes() == CC.statement(pts, bgr).tobytes()
                assert rec.size == int(MC.valid_mask(z).sum()) == CC.count(pts), name
                t = MC.triangles(z)
                assert t.size == 0 or t.max() < rec.size
        # a vertex's record is the record of its pixel
        z = MC.salt(w, h)
        pts = MC.as_points(z, K)
        org = CC.statement(pts, bgr, organized=True)
        assert MC.vertices(pts, bgr).tobytes() == org.reshape(-1)[MC.valid_mask(z).reshape(-1)].tobytes()
