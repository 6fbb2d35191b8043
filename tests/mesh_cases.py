"""The rule of OrganizedMesh (kde_mesh_*) stated in numpy, twice, and the frames its tests share.

A frame is a depth map z [H, W] float32 in millimetres (the z of a float3 source), W, H >= 2.
    vertex    pixel i is a vertex iff z > z_min and z < z_max; its index is its rank among the valid pixels in raster order;
              its record is the dense record of cloud_cases.statement
    linked    two valid pixels with |za - zb| <= max_diff + rel_diff * min(za, zb): one float32 subtraction, one product, one sum
    quad      pixel (x, y), x < W - 1, y < H - 1, owns a = (x, y), b = (x + 1, y), c = (x, y + 1), d = (x + 1, y + 1)
    triangle  emitted iff its three corners are valid and its three edges linked.  Four valid corners: DIAG_AD gives (a, c, d)
              then (a, d, b); DIAG_BC (a, c, b) then (b, c, d); DIAG_ADAPTIVE cuts b-c iff |zb - zc| < |za - zd|, else a-d.
              Three valid corners: a missing (b, c, d), b missing (a, c, d), c missing (a, d, b), d missing (a, c, b).
              flip_winding swaps v1 and v2.  Order: owning pixel in raster order, within a quad the first before the second.
`triangles` is the vectorised statement, `triangles_scalar` a loop over the quads that shares nothing with it but the link.
"""
import numpy as np

import cloud_cases as CC

F32 = np.float32
Z_MIN, Z_MAX = CC.Z_MIN, CC.Z_MAX
MAX_DIFF, REL_DIFF = F32(10.0), F32(0.02)
DIAG_AD, DIAG_BC, DIAG_ADAPTIVE = 0, 1, 2
TRIANGLE = np.dtype([("v0", "<u4"), ("v1", "<u4"), ("v2", "<u4")])
# the four triangles of a quad by corner (0 = a, 1 = b, 2 = c, 3 = d), in the order they are emitted in
FORMS = np.array([[0, 2, 3], [0, 3, 1], [0, 2, 1], [1, 2, 3]])


def valid_mask(z, z_min=Z_MIN, z_max=Z_MAX):
    z = np.asarray(z, F32)
    with np.errstate(invalid="ignore"):
        return (z > F32(z_min)) & (z < F32(z_max))


def ranks(valid):
    """the vertex index of every pixel (meaningful where it is valid)"""
    v = np.asarray(valid, bool)
    return (np.cumsum(v.reshape(-1)) - v.reshape(-1)).astype(np.uint32).reshape(v.shape)


def linked(za, zb, va, vb, max_diff=MAX_DIFF, rel_diff=REL_DIFF):
    """elementwise on float32 arrays (or scalars): every operation is one binary32 operation"""
    za, zb = np.asarray(za, F32), np.asarray(zb, F32)
    with np.errstate(invalid="ignore", over="ignore"):
        m = F32(rel_diff) * np.minimum(za, zb)
        t = F32(max_diff) + m
        d = np.abs(za - zb)
        assert m.dtype == F32 and t.dtype == F32 and d.dtype == F32
        return np.asarray(va, bool) & np.asarray(vb, bool) & (d <= t)


def triangles(z, z_min=Z_MIN, z_max=Z_MAX, max_diff=MAX_DIFF, rel_diff=REL_DIFF, diagonal=DIAG_ADAPTIVE, flip_winding=False):
    """the triangles of one frame, uint32 [M, 3], vectorised"""
    z = np.asarray(z, F32)
    h, w = z.shape
    assert h >= 2 and w >= 2
    v = valid_mask(z, z_min, z_max)
    r = ranks(v)
    corner = lambda a: (a[:-1, :-1], a[:-1, 1:], a[1:, :-1], a[1:, 1:])         # a, b, c, d of every quad
    zc, vc, rc = corner(z), corner(v), np.stack(corner(r), axis=-1)
    link = lambda i, j: linked(zc[i], zc[j], vc[i], vc[j], max_diff, rel_diff)
    lab, lac, lbd, lcd, lad, lbc = link(0, 1), link(0, 2), link(1, 3), link(2, 3), link(0, 3), link(1, 2)
    ok = np.stack([lac & lcd & lad, lad & lbd & lab, lac & lbc & lab, lbc & lcd & lbd], axis=-1)
    four = vc[0] & vc[1] & vc[2] & vc[3]
    with np.errstate(invalid="ignore", over="ignore"):
        shorter_bc = np.abs(zc[1] - zc[2]) < np.abs(zc[0] - zc[3])
    bc = {DIAG_AD: np.zeros_like(four), DIAG_BC: np.ones_like(four), DIAG_ADAPTIVE: shorter_bc}[diagonal]
    # four corners: only the two triangles of the cut; three: a triangle with the missing corner has no linked edge there
    cut = np.stack([~bc, ~bc, bc, bc], axis=-1)
    emit = ok & (cut | ~four[..., None])
    tri = rc[:, :, FORMS]                                                       # [h-1, w-1, 4, 3]
    out = tri[emit].astype(np.uint32).reshape(-1, 3)
    return out[:, [0, 2, 1]] if flip_winding else out


def triangles_scalar(z, z_min=Z_MIN, z_max=Z_MAX, max_diff=MAX_DIFF, rel_diff=REL_DIFF, diagonal=DIAG_ADAPTIVE, flip_winding=False):
    """the same, one quad at a time in the words of the rule"""
    z = np.asarray(z, F32)
    h, w = z.shape
    lo, hi = F32(z_min), F32(z_max)
    valid = [[bool(z[y, x] > lo and z[y, x] < hi) for x in range(w)] for y in range(h)]
    rank, nvert = {}, 0
    for y in range(h):
        for x in range(w):
            if valid[y][x]:
                rank[(x, y)] = nvert
                nvert += 1

    def link(p, q):
        if not (valid[p[1]][p[0]] and valid[q[1]][q[0]]):
            return False
        za, zb = z[p[1], p[0]], z[q[1], q[0]]
        m = F32(rel_diff) * min(za, zb)
        t = F32(max_diff) + m
        return bool(abs(F32(za - zb)) <= t)

    out = []

    def emit(p0, p1, p2):
        if link(p0, p1) and link(p1, p2) and link(p2, p0):
            out.append((rank[p0], rank[p2], rank[p1]) if flip_winding else (rank[p0], rank[p1], rank[p2]))

    for y in range(h - 1):
        for x in range(w - 1):
            a, b, c, d = (x, y), (x + 1, y), (x, y + 1), (x + 1, y + 1)
            missing = [p for p in (a, b, c, d) if not valid[p[1]][p[0]]]
            if len(missing) == 0:
                if diagonal == DIAG_ADAPTIVE:
                    with np.errstate(invalid="ignore", over="ignore"):
                        use_bc = bool(abs(F32(z[b[1], b[0]] - z[c[1], c[0]])) < abs(F32(z[a[1], a[0]] - z[d[1], d[0]])))
                else:
                    use_bc = diagonal == DIAG_BC
                if use_bc:
                    emit(a, c, b)
                    emit(b, c, d)
                else:
                    emit(a, c, d)
                    emit(a, d, b)
            elif len(missing) == 1:
                if missing[0] == a:
                    emit(b, c, d)
                elif missing[0] == b:
                    emit(a, c, d)
                elif missing[0] == c:
                    emit(a, d, b)
                else:
                    emit(a, c, b)
    return np.array(out, np.uint32).reshape(-1, 3)


def records(tri):
    """uint32 [M, 3] as kde_mesh_triangle records"""
    return np.ascontiguousarray(tri, np.uint32).reshape(-1).view(TRIANGLE)


def vertices(points, bgr, z_min=Z_MIN, z_max=Z_MAX, divisor=CC.DIVISOR, negate_z=True):
    """the vertex records of one frame: the dense cloud"""
    return CC.statement(points, bgr, z_min, z_max, divisor, negate_z)


def as_points(z, K=None):
    """a float3 source [H, W, 3] with this z: the projection with K, or x = y = pixel coordinates in millimetres"""
    z = np.asarray(z, F32)
    if K is not None:
        return CC.project(z, K)
    y, x = np.mgrid[0:z.shape[0], 0:z.shape[1]].astype(F32)
    return np.stack([x, -y, z], axis=-1).astype(F32)


# ---- the named cases: name -> (what it catches, generator(w, h, variant) -> z [h, w]) ---------------------------------

def _plane(w, h, slope_x=0.5, slope_y=0.25, z0=1000.0):
    y, x = np.mgrid[0:h, 0:w]
    return (z0 + slope_x * x + slope_y * y).astype(F32)


def plane(w, h, variant=0):
    return _plane(w, h)


def one_hole(w, h, variant=0):
    assert w >= 3 and h >= 3
    z = _plane(w, h)
    z[h // 2, w // 2] = 0.0
    return z


def corners(w=2, h=2, variant=0):
    """the 2 x 2 frame with corner `variant` (a, b, c, d) missing"""
    z = _plane(2, 2)
    z.reshape(-1)[variant % 4] = np.nan
    return z


def step(w, h, variant=0):
    z = _plane(w, h)
    z[:, w // 2:] += F32(500.0)
    z[h // 2:, :] += F32(900.0)
    return z


def side_of_step(w, h):
    """which of the four surfaces of `step` a pixel lies on"""
    y, x = np.mgrid[0:h, 0:w]
    return (2 * (y >= h // 2) + (x >= w // 2)).reshape(-1)


def rounding_pairs(max_diff=MAX_DIFF, rel_diff=REL_DIFF, want=3):
    """(za, zb, linked) for zb > za, found by search among thresholds max_diff + rel_diff * za that are not exact (the
    product or the sum rounds): `want` pairs with zb - za exactly the threshold (linked: the test is <=), the same pairs with
    zb one ulp further (not linked), and, where they exist (they do for 0.7 and 0.3, the speckle filter's rounding case, not
    for the defaults), `want` pairs at a threshold that a fused multiply-add would make smaller (linked; a contracted kernel
    would not link them) and `want` at the larger threshold a fused multiply-add would give (not linked)"""
    rng = np.random.default_rng(11)
    za = rng.uniform(600.0, 4000.0, 1 << 16).astype(F32)
    sep = F32(max_diff) + F32(rel_diff) * za
    real = np.float64(F32(max_diff)) + np.float64(F32(rel_diff)) * za.astype(np.float64)
    fused = real.astype(F32)
    exact = lambda t: (za + t).astype(np.float64) - za.astype(np.float64) == t.astype(np.float64)       # za + t is exact
    at = np.flatnonzero(exact(sep) & (fused == sep) & (real != sep.astype(np.float64)))[:want]
    smaller = np.flatnonzero(exact(sep) & (fused < sep))[:want]
    larger = np.flatnonzero(exact(fused) & (fused > sep))[:want]
    assert at.size == want
    out = [(za[i], za[i] + sep[i], True) for i in at]
    out += [(za[i], np.nextafter(za[i] + sep[i], F32(np.inf)), False) for i in at]
    out += [(za[i], za[i] + sep[i], True) for i in smaller]
    out += [(za[i], za[i] + fused[i], False) for i in larger]
    for a, b, want_link in out:
        assert bool(linked(a, b, True, True, max_diff, rel_diff)) == want_link and bool(linked(b, a, True, True, max_diff, rel_diff)) == want_link
    return out


def _cells(w, h):
    """the top left pixels of 2 x 2 blocks separated by a row and a column (the frame's last block may touch its border)"""
    return [(x, y) for y in range(0, h - 1, 3) for x in range(0, w - 1, 3)]


FUSED_LINK = {"max_diff": 0.7, "rel_diff": 0.3}     # a link whose threshold a fused multiply-add changes at exact distances


def exact(w, h, variant=0, **link):
    """2 x 2 blocks a = c = d = za, b = zb: linked, two triangles; not linked, only (a, c, d)"""
    pairs = rounding_pairs(**link)
    z = np.zeros((h, w), F32)
    for i, (x, y) in enumerate(_cells(w, h)):
        za, zb, _ = pairs[(i + variant) % len(pairs)]
        z[y:y + 2, x:x + 2] = za
        z[y, x + 1] = zb
    return z


def exact_count(w, h, variant=0, mode=DIAG_ADAPTIVE, **link):
    """a block that is not linked keeps (a, c, d) under the a-d cut (the adaptive one too: |za - zd| is 0), nothing under b-c"""
    pairs = rounding_pairs(**link)
    return sum(2 if pairs[(i + variant) % len(pairs)][2] else int(mode != DIAG_BC) for i in range(len(_cells(w, h))))


# (a, b, c, d) of blocks whose triangles depend on the cut (thresholds near 30 at these depths):
DIAGONAL_BLOCKS = np.array([
    [1000, 1005, 1010, 1005],       # |zb - zc| == |za - zd|: the tie goes to a-d
    [1000, 1004, 1004, 1012],       # b-c shorter: adaptive cuts b-c; every edge linked
    [1000, 1025, 1025, 1050],       # a-d not linked: AD gives nothing, BC two
    [1025, 1000, 1050, 1025],       # b-c not linked: BC gives nothing, AD two
    [1000, 1020, 1045, 1028],       # adaptive cuts b-c, a-c is not linked: only (b, c, d); AD gives only (a, d, b)
], F32)
DIAGONAL_COUNTS = {DIAG_AD: [2, 2, 0, 2, 1], DIAG_BC: [2, 2, 2, 0, 1], DIAG_ADAPTIVE: [2, 2, 2, 2, 1]}


def diagonal(w, h, variant=0):
    z = np.zeros((h, w), F32)
    for i, (x, y) in enumerate(_cells(w, h)):
        z[y:y + 2, x:x + 2] = DIAGONAL_BLOCKS[(i + variant) % 5].reshape(2, 2)
    return z


def diagonal_count(w, h, mode, variant=0):
    return sum(DIAGONAL_COUNTS[mode][(i + variant) % 5] for i in range(len(_cells(w, h))))


def checker(w, h, variant=0):
    z = _plane(w, h)
    y, x = np.mgrid[0:h, 0:w]
    z[(x + y + variant) % 2 == 1] = 0.0
    return z


def rim(w, h, variant=0):
    z = np.zeros((h, w), F32)
    p = _plane(w, h)
    z[-1, :], z[:, -1] = p[-1, :], p[:, -1]
    return z


def nan_inf(w, h, variant=0):
    z = _plane(w, h)
    flat = z.reshape(-1)
    special = np.array([np.nan, np.inf, -np.inf, 0.0, -0.0, Z_MIN, Z_MAX, np.nextafter(Z_MIN, F32(np.inf)),
                        np.nextafter(Z_MAX, F32(0.0))], F32)
    at = np.random.default_rng(17 + variant).permutation(flat.size)[:max(1, flat.size // 7)]
    flat[at] = special[(np.arange(at.size) + variant) % special.size]
    return z


def salt(w, h, variant=0):
    z = _plane(w, h, 1.5, -0.75, 2000.0)
    z[np.random.default_rng(23 + variant).random((h, w)) < 0.3] = 0.0
    return z


def noisy(w, h, variant=0):
    """not a named case: a surface rough enough that about half of the edges are linked, 15 % of the pixels invalid, whole
    millimetres (so that a uint16 map holds it)"""
    rng = np.random.default_rng(101 + variant)
    z = np.rint(1500.0 + rng.normal(0.0, 18.0, (h, w))).astype(F32)
    z[rng.random((h, w)) < 0.15] = 0.0
    return z


CASES = {
    "plane": ("every pixel valid and linked: 2 (W-1) (H-1) triangles in all three modes -- ranks, order and the last row and column", plane),
    "one_hole": ("one interior invalid pixel: exactly 4 triangles fewer, each missing-corner form once", one_hole),
    "corners": ("each of a, b, c, d missing in turn in a 2 x 2 frame: the vertex order of the four three-corner forms", corners),
    "step": ("a depth step beyond the threshold along a column and along a row: no triangle crosses it", step),
    "exact": ("a step of exactly the threshold is linked (<=), one ulp beyond is not; thresholds that round: no fused multiply-add", exact),
    "diagonal": ("quads where AD, BC and ADAPTIVE differ, the tie |zb - zc| == |za - zd| (a-d), a cut whose triangles fail singly", diagonal),
    "checker": ("alternate pixels invalid: no quad has three corners, 0 triangles, yet half the pixels are vertices", checker),
    "rim": ("only the last row and the last column valid: those pixels own no quad; the one triangle belongs to an invalid pixel", rim),
    "nan_inf": ("NaN, +-inf, 0, -0, z_min and z_max themselves: none is a vertex, none reaches a subtraction that decides", nan_inf),
    "salt": ("a seeded 30 % of the pixels invalid on a slanted plane: every mix of forms, ranks across rows and segments", salt),
}


def frames(w, h):
    """[(name, z, link)]: every named case that fits a w x h frame (corners only 2 x 2, one_hole from 3 x 3), `exact` once
    more under FUSED_LINK, the 2 x 2 frame with every variant of the block cases, and two noisy frames; link is {} (the
    default link) or FUSED_LINK"""
    tiny = (w, h) == (2, 2)
    out = []
    for name, (_, gen) in CASES.items():
        if name == "corners":
            if tiny:
                out += [(f"corners{k}", corners(variant=k), {}) for k in range(4)]
            continue
        if name == "one_hole" and (w < 3 or h < 3):
            continue
        variants = range({"exact": len(rounding_pairs()), "diagonal": 5}.get(name, 1)) if tiny else (0,)
        out += [(name if k == 0 else f"{name}{k}", gen(w, h, k), {}) for k in variants]
    out += [(f"exactfused{k}", exact(w, h, k, **FUSED_LINK), FUSED_LINK) for k in (range(len(rounding_pairs(**FUSED_LINK))) if tiny else (0,))]
    out += [("noisy0", noisy(w, h, 0), {}), ("noisy1", noisy(w, h, 1), {})]
    return out
