"""Crafted inputs for the tail of SPDepthSuperResolution::Process (csrc/spdsr_kernels.hip: per-cluster plane fit, plane
projection, mrf sweeps) and two plain binary64 references in numpy, written from the reference's formulas
(SPDepthSuperResolution.cpp:65-142 as oracle/kde_oracle.c restates it; Projection_GPU.cu:55-81, 148-187 with deviation D5),
not from the kernels.  tests/test_spdsr_tail_cases.py proves on the CPU that the cases hold what they claim and that these
references agree with the float32 restatement of oracle/; tests/test_gpu_spdsr_tail.py holds the kernels to them through
kde_stage_spdsr_tail (include/kde_test_hooks.h).

Layout: labels [H,W] int32, points [H,W,3] float32, nd [k,4] float32 (unit normal, plane distance)."""
import functools

import numpy as np

MARGIN = 1e-5          # a decision closer than this (relative) to its threshold is not held to a value bar
MAX_FLAGGED = 0.01     # share of pixels such decisions may reach after 20 sweeps (0 after one sweep)


# ---- camera -------------------------------------------------------------------------------------------------------------
def intrinsics(w, h):
    f = float(np.float32(0.9 * w))
    return np.array([[f, 0, w // 2], [0, f, h // 2], [0, 0, 1]], np.float64)


def rays(w, h, K):
    """Normalized3D (initTemp, Projection_GPU.cu:3-19) in float32: x = (x - cx) / fx, y = (cy - y) / fy"""
    K = np.asarray(K, np.float64).reshape(3, 3)
    fx, fy, cx, cy = np.float32(K[0, 0]), np.float32(K[1, 1]), np.float32(int(K[0, 2])), np.float32(int(K[1, 2]))
    x = np.arange(w, dtype=np.float32)[None, :].repeat(h, 0)
    y = np.arange(h, dtype=np.float32)[:, None].repeat(w, 1)
    return ((x - cx) / fx).astype(np.float32), ((cy - y) / fy).astype(np.float32)


# ---- reference 1: the plane of every cluster ---------------------------------------------------------------------------------
def planes64(labels, points, nclusters, nd_prev=None):
    """-> dict(nd [k,4] float32, gap [k], mean [k,3] float64, count [k]).  Per cluster of >= 3 points: two-pass mean and
    covariance / n in binary64, np.linalg.eigh, normal = eigenvector of the smallest eigenvalue cast to float32 and flipped so
    that n . mean >= 0, d = |n . mean|.  Fewer points: (5, 5, 5) and w as nd_prev has it (0 without one).  gap is the relative
    eigen-gap (l2 - l3) / l1 that conditions the normal (NaN for markers); a cluster with a non-finite point gets a NaN row."""
    nd = np.zeros((nclusters, 4), np.float32) if nd_prev is None else np.array(nd_prev, np.float32).reshape(nclusters, 4).copy()
    gap = np.full(nclusters, np.nan)
    mean = np.full((nclusters, 3), np.nan)
    L = np.asarray(labels).reshape(-1)
    P = np.asarray(points, np.float32).reshape(-1, 3).astype(np.float64)
    ok = (L >= 0) & (L < nclusters)
    idx = np.flatnonzero(ok)
    idx = idx[np.argsort(L[idx], kind="stable")]
    count = np.bincount(L[idx], minlength=nclusters)
    start = np.concatenate([[0], np.cumsum(count)])
    for l in range(nclusters):
        p = P[idx[start[l]:start[l + 1]]]
        if len(p) < 3:
            nd[l, :3] = 5.0
            continue
        m = p.mean(0)
        mean[l] = m
        if not np.isfinite(p).all():
            nd[l] = np.nan
            continue
        c = (p - m).T @ (p - m) / len(p)
        ev, V = np.linalg.eigh(c)
        n = V[:, 0].astype(np.float32)
        d = float(n.astype(np.float64) @ m)
        if d < 0:
            n = -n
        nd[l] = [n[0], n[1], n[2], abs(d)]
        gap[l] = (ev[1] - ev[0]) / ev[2] if ev[2] > 0 else 0.0
    return {"nd": nd, "gap": gap, "mean": mean, "count": count}


def plane_fitted64(nd, labels, points, tx, ty):
    """setPsuedoDepth (Projection_GPU.cu:55-81) in binary64 from float32 planes and rays -> (z [H,W] float64, projected mask,
    |a rx + b ry + c|).  Unprojected pixels (label outside the table, |nx| >= 1 or NaN) keep the input point."""
    nd = np.asarray(nd, np.float32)
    k = nd.shape[0]
    lab = np.asarray(labels)
    inside = (lab > -1) & (lab < k)
    n = nd[np.where(inside, lab, 0)].astype(np.float64)
    with np.errstate(all="ignore"):
        proj = inside & (np.abs(n[..., 0]) < 1.0)
        den = n[..., 0] * tx.astype(np.float64) + n[..., 1] * ty.astype(np.float64) + n[..., 2]
        z = np.abs(n[..., 3] / den)
    return np.where(proj, z, np.asarray(points, np.float32)[..., 2].astype(np.float64)), proj, np.abs(den)


# ---- reference 2: the sweeps -------------------------------------------------------------------------------------------------
def _dilate5(m):
    h, w = m.shape
    p = np.pad(m, 2)
    out = np.zeros_like(m)
    for i in range(5):
        for j in range(5):
            out |= p[i:i + h, j:j + w]
    return out


def sweeps64(pfz, z_in, sweeps):
    """mrf_optimization (Projection_GPU.cu:148-187; window 5, K 0.5, smooth_sigma 1) on z alone in binary64, every sweep
    reading a snapshot of the previous one (D5).  pfz: the plane-fitted z (float32), z_in: the input cloud's z.
    -> dict(z: the final z (the input's where never rewritten), rewritten: mask, margin: per pixel the smallest decision
    margin met in any sweep -- | |o - pf| - 0.01 o | / o for the centre test, |z - 50| / 50 for a COMPUTED value used as
    a tap (input values compare exactly on both sides) --, flagged: pixels whose margin is below MARGIN plus everything such a
    pixel can reach through the 5x5 window in the remaining sweeps)."""
    z = np.asarray(z_in, np.float32).astype(np.float64)
    pf = np.asarray(pfz, np.float32).astype(np.float64)
    h, w = z.shape
    rw = np.zeros((h, w), bool)
    margin = np.full((h, w), np.inf)
    flagged = np.zeros((h, w), bool)
    with np.errstate(all="ignore"):
        for _ in range(sweeps):
            flagged = _dilate5(flagged)
            c = (pf > 50.0) & (np.abs(z - pf) < z * 0.01)
            mc = np.abs(np.abs(z - pf) - z * 0.01) / z
            mc = np.where((pf > 50.0) & np.isfinite(pf) & np.isfinite(z) & (z > 0), mc, np.inf)
            mt = np.where(rw & np.isfinite(z), np.abs(z - 50.0) / 50.0, np.inf)
            m = np.minimum(mc, mt)
            margin = np.minimum(margin, m)
            flagged |= m < MARGIN
            zp = np.pad(z, 2, constant_values=0.0)
            num, den = pf.copy(), np.ones_like(pf)
            for i in range(5):
                for j in range(5):
                    oq = zp[i:i + h, j:j + w]
                    v = oq > 50.0
                    f = np.where(v, 0.5 / (1.0 + (z - oq) ** 2), 0.0)
                    num = num + np.where(v, oq * f, 0.0)
                    den = den + f
            z = np.where(c, num / den, z)
            rw |= c
    return {"z": z, "rewritten": rw, "margin": margin, "flagged": flagged}


# ---- case builders -----------------------------------------------------------------------------------------------------------
def block_labels(w, h, rows, cols, perm=None):
    wx, wy = w // cols, h // rows
    lab = np.minimum(np.arange(h)[:, None] // wy, rows - 1) * cols + np.minimum(np.arange(w)[None, :] // wx, cols - 1)
    lab = lab.astype(np.int32)
    return lab if perm is None else perm[lab]


def _plane_points(rng, lab, k, tx, ty, noise, d_range, tilt):
    """every labelled pixel on its cluster's plane through its camera ray; -> points, true planes [k,4] float32"""
    h, w = lab.shape
    nd = np.zeros((k, 4), np.float64)
    nd[:, 0], nd[:, 1], nd[:, 2] = rng.uniform(-tilt, tilt, k), rng.uniform(-tilt, tilt, k), 1.0
    nd[:, :3] /= np.linalg.norm(nd[:, :3], axis=1)[:, None]
    nd[:, 3] = rng.uniform(*d_range, k)
    inside = (lab >= 0) & (lab < k)
    n = nd[np.where(inside, lab, 0)]
    z = n[..., 3] / (n[..., 0] * tx + n[..., 1] * ty + n[..., 2])
    z = np.where(inside, z, 2000.0) * (1.0 + rng.uniform(-noise, noise, (h, w)))
    return z, nd.astype(np.float32)


OFF_RAY = np.float32(0.5)      # the sweep cases' x and y lie this far off the ray: a rewritten pixel (x = ray * z) shows


def _points_from_z(z, tx, ty, off=np.float32(0.0)):
    z = np.asarray(z, np.float32)
    return np.stack([tx * z + off, ty * z + off, z], -1).astype(np.float32)


FIT_CASES = {   # name: (width, height, rows, cols, starved clusters, seed)
    "odd-8": (67, 21, 2, 4, 4, 11),              # runs straddle row ends; 1407 px is one partly filled block
    "lds-1024": (128, 128, 32, 32, 60, 12),      # the last table that fits in LDS (48 KB in the covariance pass)
    "global-1056": (132, 128, 32, 33, 60, 13),   # use_lds == 0
}


@functools.lru_cache(maxsize=None)
def fit_case(name, frame=0):
    """-> dict(w, h, rows, cols, k, K, tx, ty, labels, points, starved {cluster: points left}, nan_cluster, band (A, B, row),
    full_labels / full_points: the same frame before any cluster was starved or poisoned).  frame > 0: another label
    permutation and other planes on the same geometry (the frames of a batch)."""
    w, h, rows, cols, nstarve, seed = FIT_CASES[name]
    rng = np.random.default_rng(seed + 100 * frame)
    k = rows * cols
    K = intrinsics(w, h)
    tx, ty = rays(w, h, K)
    perm = rng.permutation(k).astype(np.int32)
    lab = block_labels(w, h, rows, cols, perm)
    # one row band where the labels alternate A,B,A,B at every pixel: a label change at each of the 8 run positions
    A, B = int(perm[0]), int(perm[k - 1])
    row = h // 2
    lab[row, 0::2], lab[row, 1::2] = A, B
    lab[row + 1, 0::2], lab[row + 1, 1::2] = B, A
    z, nd_true = _plane_points(rng, lab, k, tx, ty, 0.001, (600.0, 6000.0), 0.4)
    full_labels, full_points = lab.copy(), _points_from_z(z, tx, ty)
    # starved clusters: 0, 1, 2 or 3 points left (the first four counts in turn, then at random); the survivors are three
    # corners of the cluster's block, so that three of them span a well-conditioned triangle
    pool = [int(l) for l in rng.permutation(k) if l not in (A, B)]
    starved = {}
    for i, l in enumerate(pool[:nstarve]):
        keep = i % 4 if i < 8 else int(rng.integers(0, 4))
        idx = np.flatnonzero(lab.reshape(-1) == l)
        ys, xs = idx // w, idx % w
        top, bottom = idx[ys == ys.min()], idx[ys == ys.max()]
        corners = [top[0], top[-1], bottom[0]]
        lab.reshape(-1)[np.setdiff1d(idx, corners[:keep])] = -1
        starved[l] = keep
    nan_cluster = pool[nstarve]
    # labels outside the table: 2 % beyond its end, some negative ones
    r = rng.random((h, w))
    keepers = np.isin(lab, [l for l, c in starved.items() if c > 0])          # the survivors of the starved clusters stay
    lab[(r < 0.02) & ~keepers] = k + 5
    lab[(r > 0.02) & (r < 0.025) & ~keepers] = -1
    lab[(r > 0.025) & (r < 0.03) & ~keepers] = -7
    pts = _points_from_z(z, tx, ty)
    iy, ix = np.argwhere(lab == nan_cluster)[1]
    pts[iy, ix, 0] = np.nan
    return dict(w=w, h=h, rows=rows, cols=cols, k=k, K=K, tx=tx, ty=ty, labels=lab, points=pts, starved=starved,
                nan_cluster=nan_cluster, band=(A, B, row), full_labels=full_labels, full_points=full_points, nd_true=nd_true)


MICRO_CLUSTERS = ("three", "far", "zconst", "xplus", "xminus", "collinear")


@functools.lru_cache(maxsize=None)
def fit_micro_case():
    """odd-8's geometry (67x21, 2x4) with six micro clusters (0..5 in MICRO_CLUSTERS' order) and two ordinary ones (6, 7).
    The points of the micro clusters are free 3-D points (the fit does not ask them to lie on the pixel's ray)."""
    w, h, rows, cols = FIT_CASES["odd-8"][:4]
    rng = np.random.default_rng(21)
    k = rows * cols
    K = intrinsics(w, h)
    tx, ty = rays(w, h, K)
    lab = block_labels(w, h, rows, cols)
    z, _ = _plane_points(rng, lab, k, tx, ty, 0.001, (600.0, 6000.0), 0.4)
    pts = _points_from_z(z, tx, ty)
    yy, xx = np.mgrid[0:h, 0:w]
    # 0: exactly three non-collinear points
    m = lab == 0
    lab[m] = -1
    for (y, x), p in zip(((1, 2), (7, 3), (4, 12)), ((-300.0, 200.0, 1500.0), (-280.0, 90.0, 1530.0), (-120.0, 150.0, 1490.0))):
        lab[y, x], pts[y, x] = 0, p
    # 1: a plane 14 m away and 3 m off axis, 0.5 mm noise (the centroid is 50 times the cluster's extent)
    m = lab == 1
    u, v = (xx[m] - xx[m].mean()) * 25.0, (yy[m] - yy[m].mean()) * 25.0
    pts[m] = np.stack([3000.0 + u, -400.0 + v, 14000.0 + 0.3 * u - 0.2 * v + rng.uniform(-0.5, 0.5, u.size)], -1)
    # 2: an exact z = const patch
    m = lab == 2
    pts[m] = np.stack([(xx[m] - 40) * 8.0, (yy[m] - 5) * 8.0, np.full(m.sum(), 1250.0)], -1)
    # 3, 4: exact x = const patches of either sign: the normal is exactly (+-1, 0, 0), |nx| < 1 fails (Projection_GPU.cu:70)
    # and the pixels come back unprojected -- the reference's quirk, pinned
    for l, x0 in ((3, 750.0), (4, -750.0)):
        m = lab == l
        pts[m] = np.stack([np.full(m.sum(), x0), (yy[m] - 15) * 8.0, 1400.0 + (xx[m] - 30) * 8.0 + (yy[m] % 3) * 16.0], -1)
    # 5: collinear points (invariants only: the normal is any unit vector across the line)
    m = lab == 5
    t = (xx[m] + 7.0 * yy[m]).astype(np.float64)
    pts[m] = np.stack([100.0 + 2.0 * t, -50.0 + 1.0 * t, 900.0 + 4.0 * t], -1)
    direction = np.array([2.0, 1.0, 4.0]) / np.sqrt(21.0)
    return dict(w=w, h=h, rows=rows, cols=cols, k=k, K=K, tx=tx, ty=ty, labels=lab, points=pts.astype(np.float32),
                direction=direction)


SWEEP_CASES = {   # name: (width, height, rows, cols, seed)
    "sweep-67x21": (67, 21, 2, 4, 1),
    "sweep-130x9": (130, 9, 2, 4, 2),       # height >= 6 and wy = 4 hold; one tile row and a bit, three tile columns
    "sweep-33x50": (33, 50, 2, 4, 3),       # narrower than a tile, seven tile rows
}
SWEEP_COUNTS = (0, 1, 2, 20)


@functools.lru_cache(maxsize=None)
def sweep_case(name, frame=0):
    """-> dict(w, h, rows, cols, k, K, tx, ty, labels, points, nd).  One plane per block of the grid; +-0.3 % noise (inside the
    1 % centre test), 6 % outliers at +-3..5 % (outside it), 5 % invalid z out of {0, 30, -500} labelled -1, 3 % more
    unlabelled pixels.  nd holds the true planes: passed to the hook, the projection is deterministic to the bit.  x and y
    lie OFF_RAY off the pixel's ray (the sweeps read z alone), so the output shows which pixels were rewritten."""
    w, h, rows, cols, seed = SWEEP_CASES[name]
    rng = np.random.default_rng(seed + 100 * frame)
    k = rows * cols
    K = intrinsics(w, h)
    tx, ty = rays(w, h, K)
    lab = block_labels(w, h, rows, cols, rng.permutation(k).astype(np.int32) if frame else None)
    z, nd = _plane_points(rng, lab, k, tx, ty, 0.003, (800.0, 3000.0), 0.3)
    out = rng.random((h, w)) < 0.06
    nd64 = nd.astype(np.float64)[lab]
    clean = nd64[..., 3] / (nd64[..., 0] * tx + nd64[..., 1] * ty + nd64[..., 2])
    z[out] = (clean * (1.0 + rng.choice([-1.0, 1.0], (h, w)) * rng.uniform(0.03, 0.05, (h, w))))[out]
    inv = rng.random((h, w)) < 0.05
    z[inv] = rng.choice([0.0, 30.0, -500.0], int(inv.sum()))
    lab[inv] = -1
    lab[rng.random((h, w)) < 0.03] = -1
    return dict(w=w, h=h, rows=rows, cols=cols, k=k, K=K, tx=tx, ty=ty, labels=lab, points=_points_from_z(z, tx, ty, OFF_RAY), nd=nd)


MICRO_ITEMS = ("plus_inf", "minus_inf", "nan", "huge", "negative", "pf_inf")
MICRO_AT = (4, 3)                # (y, x) of the non-finite item
TAP_INVALID, TAP_VALID = (1, 12), (6, 12)      # z = 50.0f exactly / nextafter(50.0f): 5x5 windows that do not meet


@functools.lru_cache(maxsize=None)
def sweep_micro(item=None):
    """16x8, grid 2x2.  Columns 0..7: cluster 0, the plane z = 1000 with z = 1000 everywhere -- plus, at MICRO_AT, one item of
    the non-finite class (pf_inf: that pixel belongs to cluster 2, whose plane (0, 0, 0, 1000) makes the denominator 0).
    Columns 8..15: cluster 1, the plane z = 50.25 with z = 50.25, one pixel at exactly 50.0f (not a tap: z > 50 fails) and one
    at nextafter(50.0f) (a tap); every 5x5 window that holds one of them lies inside the cluster and misses the other."""
    w, h, rows, cols = 16, 8, 2, 2
    K = intrinsics(w, h)
    tx, ty = rays(w, h, K)
    lab = np.zeros((h, w), np.int32)
    lab[:, 8:] = 1
    z = np.where(lab == 0, np.float32(1000.0), np.float32(50.25)).astype(np.float32)
    z[TAP_INVALID] = np.float32(50.0)
    z[TAP_VALID] = np.nextafter(np.float32(50.0), np.float32(100.0))
    nd = np.array([[0, 0, 1, 1000.0], [0, 0, 1, 50.25], [0, 0, 0, 1000.0], [5, 5, 5, 0]], np.float32)
    pts = _points_from_z(z, tx, ty, OFF_RAY)
    if item is not None:
        y, x = MICRO_AT
        if item == "pf_inf":
            lab[y, x] = 2
        else:
            v = {"plus_inf": np.inf, "minus_inf": -np.inf, "nan": np.nan, "huge": 3e38, "negative": -1000.0}[item]
            pts[y, x] = (0.0, 0.0, v)
    return dict(w=w, h=h, rows=rows, cols=cols, k=4, K=K, tx=tx, ty=ty, labels=lab, points=pts, nd=nd)


def window_of(yx, h, w):
    """the pixels whose 5x5 window holds yx (yx itself excluded)"""
    m = np.zeros((h, w), bool)
    m[max(yx[0] - 2, 0):yx[0] + 3, max(yx[1] - 2, 0):yx[1] + 3] = True
    m[yx] = False
    return m


def ulps32(got, ref64):
    """|got - ref| in units of the float32 spacing at ref"""
    ref64 = np.asarray(ref64, np.float64)
    with np.errstate(all="ignore"):
        return np.abs(np.asarray(got, np.float64) - ref64) / np.spacing(np.abs(ref64).astype(np.float32)).astype(np.float64)


# ---- what an output is held to -------------------------------------------------------------------------------------------------
def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def planes_compare(nd, ref, what, skip=()):
    """nd [k,4] (either side's planes) against ref = planes64(...).  Marker rows bit-equal, NaN rows NaN; every other row but
    those of `skip`: each component of the normal within 2 * 2^-23 of the binary64 fit's (the moments differ from the serial sums
    by ~1e-15, which turns the normal by at most 1e-15 / gap <= 1e-9 at gap >= 1e-6: what is left is the cast to float32, with
    one ulp of slack), and d within 2 float32 ulps of |n . mean| with the side's OWN normal and the binary64 centroid, which
    keeps the normal's rounding out of d.  -> (largest normal deviation in units of 2^-23, largest deviation of d in ulps)"""
    r = ref["nd"]
    marker = r[:, 0] == 5.0
    nan = np.isnan(r[:, 0])
    assert np.array_equal(nd[marker].view(np.uint32), r[marker].view(np.uint32)), f"{what}: marker rows differ"
    # (a marker row is held to the bit above: its w is the slot's previous one, which is NaN after a NaN row)
    assert np.isnan(nd[nan]).all() and not np.isnan(nd[~nan & ~marker]).any(), f"{what}: NaN rows differ"
    ok = ~marker & ~nan
    ok[list(skip)] = False
    if not ok.any():                          # nothing but markers, NaN rows and skipped rows: a table of one poisoned cluster
        return 0.0, 0.0
    dn = np.abs(nd[ok, :3].astype(np.float64) - r[ok, :3].astype(np.float64)).max() / 2.0 ** -23
    assert dn <= 2.0, f"{what}: a normal is {dn:.2f} x 2^-23 from the binary64 fit"
    d_ref = np.abs((nd[ok, :3].astype(np.float64) * ref["mean"][ok]).sum(1))        # the side's own normal, binary64 centroid
    dd = ulps32(nd[ok, 3], d_ref).max()
    assert dd <= 2.0, f"{what}: a plane distance is {dd:.2f} float32 ulps from |n . mean|"
    return dn, dd


def sweep_compare(opt, ref, points, tx, ty, what):
    """opt [H,W,3] float32 (either side's optimized cloud) against ref = sweeps64(...) of the same plane-fitted z.
    Asserts what holds to the bit -- on unflagged pixels the rewritten mask is the reference's (a pixel that was never
    rewritten is the input point, a rewritten one is not: the cases' x, y lie off the ray), z is NaN exactly where the
    reference's is, and everywhere x, y = ray * z in float32 where the point was rewritten -- and returns the largest relative
    error of z over the unflagged, rewritten, finite pixels (0.0 without any)."""
    opt, points = np.asarray(opt, np.float32), np.asarray(points, np.float32)
    rewritten = (_bits(opt) != _bits(points)).any(-1)
    u = ~ref["flagged"]
    bad = (rewritten != ref["rewritten"]) & u
    assert not bad.any(), f"{what}: rewritten mask differs from the binary64 reference at {np.argwhere(bad)[:8].tolist()} ({int(bad.sum())} px)"
    z = opt[..., 2]
    with np.errstate(all="ignore"):
        assert np.array_equal(opt[..., 0][rewritten], (tx * z)[rewritten], equal_nan=True), f"{what}: x != ray * z"
        assert np.array_equal(opt[..., 1][rewritten], (ty * z)[rewritten], equal_nan=True), f"{what}: y != ray * z"
    m = rewritten & u
    bad = m & (np.isfinite(z) != np.isfinite(ref["z"]))
    assert not bad.any(), f"{what}: non-finite z at other pixels than the reference's: {np.argwhere(bad)[:8].tolist()} ({int(bad.sum())} px)"
    m &= np.isfinite(ref["z"])
    return float((np.abs(z[m].astype(np.float64) - ref["z"][m]) / np.abs(ref["z"][m])).max()) if m.any() else 0.0
