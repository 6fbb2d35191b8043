"""Shared by tests/test_les_ref.py and tests/test_gpu_les.py (not a test module): an independent numpy transcription of
LabelEquivalenceSeg::labelImage under L1-L7 ("Superpixel merging"), vectorised per pixel, and the inputs of the
micro-cases whose answers are worked by hand in tests/test_les_ref.py."""
import math
import os

import numpy as np

F = np.float32
MAX_ANGLE = F(3.141592653) / F(8.0)
MAX_DIST = F(150.0)
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def acos_threshold(c):
    """L6 in numpy: the largest float32 t in [-1, 1] with float32(arccos(float64(t))) >= c, by bisection on the floats in
    value order"""
    c = F(c)
    reaches = lambda t: F(np.arccos(np.float64(t))) >= c
    if np.isnan(c):
        return F(np.inf)
    if not reaches(F(-1)):
        return np.nextafter(F(-1), F(-np.inf))
    if reaches(F(1)):
        return F(np.inf)

    def key(f):
        u = int(np.array([f], F).view(np.uint32)[0])
        return (~u & 0xFFFFFFFF) if u & 0x80000000 else (u | 0x80000000)

    def unkey(k):
        u = (k & 0x7FFFFFFF) if k & 0x80000000 else (~k & 0xFFFFFFFF)
        return np.array([u], np.uint32).view(F)[0]

    lo, hi = key(F(-1)), key(F(1))
    while hi - lo > 1:
        mid = (lo + hi) // 2
        if reaches(unkey(mid)):
            lo = mid
        else:
            hi = mid
    return unkey(lo)


def np_label_image(normals, labels, centers, iterations=10, max_angle=MAX_ANGLE, max_plane_distance=MAX_DIST):
    """dict like tools/les_ref.label_image, plus 'sums': per merged label the seven float32 L4 sums with their members
    (label, count, the seven float32 values) for the L4 bound"""
    normals, centers = np.ascontiguousarray(normals, F), np.ascontiguousarray(centers, F)
    H, W = labels.shape
    npix, nc = H * W, len(normals)
    lab = labels.reshape(-1).astype(np.int64)
    inr = (lab >= 0) & (lab < nc)                                                  # L1
    ls = np.where(inr, lab, 0)
    n, c = normals[ls], centers[ls]
    valid = inr & ((n[:, 0] != -1) | (n[:, 1] != -1) | (n[:, 2] != -1))
    with np.errstate(all="ignore"):
        w = np.abs((n[:, 0] * c[:, 0] + n[:, 1] * c[:, 1]) + n[:, 2] * c[:, 2])
    nd = np.where(valid[:, None], np.concatenate([n, w[:, None]], 1), F(5)).astype(F)
    merged = np.where(valid, lab, -1)
    ref = np.arange(npix)
    thr, max_dist = acos_threshold(max_angle), F(max_plane_distance)
    p = np.arange(npix)
    x, y = p % W, p // W
    nbrs = [x + np.maximum(y - 1, 0) * W, np.maximum(x - 1, 0) + y * W, np.where(x + 1 < W, x + 1, W) + y * W,
            x + np.where(y + 1 < H, y + 1, H) * W]                                  # L2
    changed = []
    for _ in range(iterations):
        before = merged.copy()
        cur = merged.copy()
        for q in nbrs:
            okq = q < npix
            qs = np.where(okq, q, 0)
            with np.errstate(all="ignore"):
                d = (nd[qs, 0] * nd[:, 0] + nd[qs, 1] * nd[:, 1]) + nd[qs, 2] * nd[:, 2]
                comp = (d < F(1)) & (d > thr) & (np.abs(nd[qs, 3] - nd[:, 3]) < max_dist)        # L6
            take = okq & (merged[qs] > -1) & ((lab[qs] == lab) | comp) & (merged[qs] < cur)
            cur = np.where(take, merged[qs], cur)
        act = (merged > -1) & (cur < merged)
        np.minimum.at(ref, merged[act], cur[act])
        root = ref.copy()                                                           # L3 phase 1 on the table as it stood
        while True:
            nxt = ref[root]
            if np.array_equal(nxt, root):
                break
            root = nxt
        elig = merged == lab
        ref = np.where(elig, root, ref)
        merged = np.where(merged > -1, ref[np.maximum(merged, 0)], -1)              # phase 2
        changed.append(int((before != merged).sum()))
    passing = (merged > -1) & ((nd[:, 0] != -1) | (nd[:, 1] != -1) | (nd[:, 1] != -1))
    merged = np.where(passing, merged, -1)
    size = np.bincount(merged[passing], minlength=nc).astype(np.int32)
    cnt = np.bincount(lab[passing], minlength=nc)
    firstpix = {}
    u, idx = np.unique(lab[passing], return_index=True)
    pp = p[passing]
    for a, i in zip(u, idx):
        firstpix[int(a)] = int(pp[i])
        assert (merged[passing][lab[passing] == a] == merged[pp[i]]).all()           # the invariant
    sums, members = {}, {}
    with np.errstate(all="ignore"):
        for a in sorted(firstpix):                                                  # L4: ascending label
            q = firstpix[a]
            m, ca = int(merged[q]), F(cnt[a])
            vals = [ca * nd[q, 0], ca * nd[q, 1], ca * nd[q, 2], ca * centers[a, 0], ca * centers[a, 1], ca * centers[a, 2]]
            sums[m] = vals if m not in sums else [s + v for s, v in zip(sums[m], vals)]
            members.setdefault(m, []).append([a, int(cnt[a]), nd[q, 0], nd[q, 1], nd[q, 2], centers[a, 0], centers[a, 1], centers[a, 2]])
        mnd = np.zeros((nc, 4), F)
        variance = np.zeros(nc, F)
        for m, s in sums.items():
            sz = F(size[m])
            mx, my, mz = s[0] / sz, s[1] / sz, s[2] / sz
            ox, oy, oz = s[3] / sz, s[4] / sz, s[5] / sz
            mnd[m] = [mx, my, mz, np.abs((mx * ox + my * oy) + mz * oz)]
            var = None
            for mem in members[m]:
                v = (mem[2] * mx + mem[3] * my) + mem[4] * mz
                v = v / sz
                pv = F(mem[1]) * v
                var = pv if var is None else var + pv
                mem.append(v)
            variance[m] = var
            s.append(var)
    merged_nd = np.where((merged > -1)[:, None], mnd[np.maximum(merged, 0)], F(0)).astype(F)
    return {"input_nd": nd.reshape(H, W, 4), "merged_label": merged.reshape(H, W).astype(np.int32),
            "merged_nd": merged_nd.reshape(H, W, 4), "size": size, "variance": variance, "changed": np.array(changed, np.int32),
            "sums": sums, "members": members}


def ubits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def differing(got, exp):
    """number of float elements that differ in their bits, NaNs compared by position"""
    got, exp = np.asarray(got, F), np.asarray(exp, F)
    assert got.shape == exp.shape, (got.shape, exp.shape)
    return int(((ubits(got) != ubits(exp)) & ~(np.isnan(got) & np.isnan(exp))).sum())


OUTPUTS = ("merged_label", "merged_nd", "size", "variance")


def diff_counts(got, exp, keys=OUTPUTS):
    out = {}
    for k in keys:
        if np.asarray(exp[k]).dtype.kind == "f":
            out[k] = differing(got[k], exp[k])
        else:
            out[k] = int((np.asarray(got[k]) != np.asarray(exp[k])).sum())
    return out


# ---- inputs ------------------------------------------------------------------------------------------------------------
def tilted(deg):
    """unit normal `deg` degrees off z in the xz plane, float32"""
    return np.array([math.sin(math.radians(deg)), 0.0, math.cos(math.radians(deg))], F)


def two_halves(deg, extra_distance=0.0, W=16, H=6):
    """left half superpixel 0 with normal z, right half superpixel 1 `deg` degrees off; centres 1000 n (+ extra along n)"""
    labels = np.zeros((H, W), np.int32)
    labels[:, W // 2:] = 1
    normals = np.stack([tilted(0), tilted(deg)])
    centers = np.stack([F(1000) * normals[0], F(1000 + extra_distance) * normals[1]]).astype(F)
    return normals, labels, centers


def wrap_case(swapped):
    """16 x 6, superpixel 0 everywhere with normal (0,1,0); pixel (15,2) and pixel (0,3) are superpixels 2 and 1 (1 and 2 if
    swapped), the first 10 degrees off z, the second z: (15,2) sees (0,3) through the L2 wrap, not the reverse"""
    labels = np.zeros((6, 16), np.int32)
    a, b = (1, 2) if swapped else (2, 1)
    labels[2, 15], labels[3, 0] = a, b
    normals = np.zeros((3, 3), F)
    normals[0] = [0, 1, 0]
    normals[a], normals[b] = tilted(10), tilted(0)
    return normals, labels, (F(1000) * normals).astype(F)


def chain_case(row0_valid):
    """64 x 8, 17 superpixels: row 0 is superpixel 16 (bad normal unless row0_valid), rows 1-7 are 16 strips of 4 columns
    labelled 0..15 with normals 10 k degrees off z"""
    labels = np.empty((8, 64), np.int32)
    labels[0] = 16
    labels[1:] = (np.arange(64) // 4)[None, :]
    normals = np.stack([tilted(10 * k) for k in range(16)] + [np.array([0, 1, 0], F) if row0_valid else np.full(3, -1, F)])
    return normals, labels, (F(1000) * normals).astype(F)


def random_case(seed, W, H, nc):
    """random label map with -1 and out-of-range labels, blocks of equal labels, bad, NaN and (-1,-1,z) normals"""
    rng = np.random.default_rng(seed)
    bw, bh = max(1, W // 6), max(1, H // 5)
    coarse = rng.integers(0, nc, ((H + bh - 1) // bh, (W + bw - 1) // bw))
    labels = np.kron(coarse, np.ones((bh, bw), np.int64))[:H, :W].astype(np.int32)
    r = rng.random((H, W))
    labels[r < 0.10] = rng.integers(0, nc, int((r < 0.10).sum()))
    labels[(r >= 0.10) & (r < 0.13)] = -1
    labels[(r >= 0.13) & (r < 0.15)] = nc + rng.integers(0, 3)
    labels[(r >= 0.15) & (r < 0.16)] = -7
    base = rng.normal(size=3)
    normals = base[None, :] + 0.25 * rng.normal(size=(nc, 3))
    normals = (normals / np.linalg.norm(normals, axis=1, keepdims=True)).astype(F)
    centers = (normals * (1000 + 120 * rng.normal(size=(nc, 1)))).astype(F)
    kind = rng.random(nc)
    normals[kind < 0.10] = -1
    normals[(kind >= 0.10) & (kind < 0.15), rng.integers(0, 3)] = np.nan
    normals[(kind >= 0.15) & (kind < 0.20), :2] = -1                                # L7
    dup = rng.integers(0, nc, 2)
    normals[dup[0]], centers[dup[0]] = normals[dup[1]], centers[dup[1]]             # identical normals (L6 quirk)
    return normals, labels, centers


RANDOM_SHAPES = [(1, 23, 16, 5), (2, 40, 30, 12), (3, 1, 37, 6), (4, 29, 1, 6), (5, 64, 48, 40), (6, 7, 5, 35), (7, 33, 21, 3),
                 (8, 1, 1, 1)]


def golden_inputs(it):
    """labels, centres and normals of tests/golden/nasp_it{it}.npz (320 x 240, 10 x 10 superpixels)"""
    g = np.load(os.path.join(GOLDEN, f"nasp_it{it}.npz"))
    return g["normals"].view(F).reshape(-1, 3), g["labels"].astype(np.int32), g["centers"].view(F).reshape(-1, 3)
