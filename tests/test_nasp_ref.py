"""tools/nasp_ref.c, the CPU restatement of NormalAdaptiveSuperpixel::Segmentation, pinned without a CUDA binary:
an independent numpy-float32 port of the two kernels that carry the new arithmetic, hand-checkable micro-cases of every
quirk DESIGN.md lists, the NA3 / NA4 definitions probed directly, and committed golden outputs."""
import math
import os

import numpy as np
import pytest

from conftest import GOLDEN, ROOT

F = np.float32


@pytest.fixture(scope="module")
def R():
    from tools import nasp_ref
    nasp_ref.build()
    return nasp_ref


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def same_floats(a, b):
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    return a.shape == b.shape and bool(((bits(a) == bits(b)) | (np.isnan(a) & np.isnan(b))).all())


def small_frame(seed, W, H, nan_normals=True):
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float32)
    base = rng.integers(0, 256, (H // 8 + 1, W // 8 + 1, 3))
    bgr = np.clip(base[(yy // 8).astype(int), (xx // 8).astype(int)] + rng.integers(-6, 7, (H, W, 3)), 0, 255).astype(np.uint8)
    z = (900.0 + 4.0 * xx + 2.5 * yy + 300.0 * (xx > W * 0.55)).astype(np.float32)
    z[rng.random((H, W)) < 0.04] = 0.0                              # holes
    z[rng.random((H, W)) < 0.01] = 50.0                             # exactly on the '> 50' / '< 50' tests
    f = F(575.8)
    pts = np.stack([(xx - W / 2) / f * z, (H / 2 - yy) / f * z, z], -1).astype(np.float32)
    n = rng.normal(0, 1, (H, W, 3)).astype(np.float32) * F(0.15) + np.array([0.1, -0.2, -0.95], np.float32)
    n /= np.sqrt((n * n).sum(-1, keepdims=True)).astype(np.float32)
    n[rng.random((H, W)) < 0.05] = -1.0                             # bad normals
    n[rng.random((H, W)) < 0.02, 1] = -1.0                          # one component -1: bad for '&&', good for '||'
    if nan_normals:
        n[rng.random((H, W)) < 0.01] = np.nan
    return np.ascontiguousarray(bgr), np.ascontiguousarray(pts), np.ascontiguousarray(n.astype(np.float32))


K = np.array([[575.8, 0, 48.0], [0, 575.8, 32.0], [0, 0, 1]], np.float64)


# ---------------------------------------------------------------------------------------------------------------------
# an independent port: numpy float32 arrays over all pixels / all (cluster, thread) pairs, one IEEE operation per numpy
# operation, in the CUDA text's order
# ---------------------------------------------------------------------------------------------------------------------
def port_calculate_ld(W, H, rows, cols, bgr, pts, nrm, ld_l, ld_d, mean, centers, spn, cs, ss, ds, ns):
    wx, wy = W // cols, H // rows
    half = F(wx + wy) / F(2.0)
    win2 = half * half
    sum_sigma = F(F(F(ss) + F(cs)) + F(ns)) + F(ds)
    kc, ks, kd, kn = [(F(s) / sum_sigma) * (F(s) / sum_sigma) for s in (cs, ss, ds, ns)]
    y, x = np.mgrid[0:H, 0:W]
    x, y = x.ravel(), y.ravel()
    c = bgr.reshape(-1, 3).astype(np.float32)
    p, n = pts.reshape(-1, 3), nrm.reshape(-1, 3)
    l0, d0 = ld_l.ravel().copy(), ld_d.ravel().copy()
    ccx = np.fmod(l0, cols).astype(np.int64)                 # C's truncating % and /
    ccy = np.trunc(l0 / cols).astype(np.int64)
    dist = np.empty((64, W * H), np.float32)
    lab = np.empty((64, W * H), np.int32)
    n_ok = (n[:, 0] != -1) | (n[:, 1] != -1) | (n[:, 2] != -1)
    with np.errstate(all="ignore"):
        for t in range(64):
            rx, ry = ccx - 4 + (t & 7), ccy - 4 + (t >> 3)
            inside = (rx >= 0) & (rx < cols) & (ry >= 0) & (ry < rows)
            cid = np.where(inside, ry * cols + rx, 0)
            m = mean[cid]
            e0, e1, e2 = c[:, 0] - m["r"].astype(np.float32), c[:, 1] - m["g"].astype(np.float32), c[:, 2] - m["b"].astype(np.float32)
            color = e0 * e0 + e1 * e1 + e2 * e2
            px = (x - m["x"].astype(np.int64)).astype(np.int32).astype(np.float32)
            py = (y - m["y"].astype(np.int64)).astype(np.int32).astype(np.float32)
            spatial = np.sqrt(px * px + py * py) * win2
            cz = centers[cid, 2]
            valid = (p[:, 2] > 50) & (cz > 50)
            depth = np.where(valid, np.abs(p[:, 2] - cz), F(0))
            s = spn[cid]
            s_ok = (s[:, 0] != -1) | (s[:, 1] != -1) | (s[:, 2] != -1)
            nd = (n[:, 0] * s[:, 0] + n[:, 1] * s[:, 1]) + n[:, 2] * s[:, 2]
            nd = np.where(nd < 0, F(0), nd)
            ndist = (np.float64(65025.0) * (1.0 - nd.astype(np.float64))).astype(np.float32)
            ndist = np.where(valid & n_ok & s_ok, ndist, F(0))                      # NA2
            d = ((color * kc + spatial * ks) + depth * kd) + ndist * kn
            dist[t] = np.where(inside, d, d0)
            lab[t] = np.where(inside, cid, l0)
        step = 32
        while step >= 1:
            a, b = dist[:step], dist[step:2 * step]
            take = a > b
            dist[:step] = np.where(take, b, a)
            lab[:step] = np.where(take, lab[step:2 * step], lab[:step])
            step //= 2
    out_l, out_d = lab[0].copy(), dist[0].copy()
    reset = (p[:, 2] < 50) & ((ds != 0) or (ns != 0))
    out_l[reset], out_d[reset] = -1, 0
    return out_l.reshape(H, W), out_d.reshape(H, W)


def f2i(v):
    v = np.float32(v)
    if np.isnan(v):
        return 0
    if v >= 2147483648.0:
        return 2147483647
    if v <= -2147483648.0:
        return -2147483648
    return int(v)


def port_weighted(W, H, rows, cols, bgr, pts, nrm, labels, mean, centers, spn, var, cs, ss, intr, thr):
    """returns new (mean, centers, spn, var) copies"""
    mean, centers, spn, var = mean.copy(), centers.copy(), spn.copy(), var.copy()
    wx, wy = W // cols, H // rows
    rpx, rpy = wx * 2 // 16 + 1, wy * 2 // 16 + 1
    wcache = {}

    def weight(num, sigma):          # NA4, per distinct numerator, with the C library's exp
        key = (float(num), sigma)
        if key not in wcache:
            with np.errstate(all="ignore"):
                arg = -F(num) / (F(2.0) * (F(sigma) * F(sigma)))
            wcache[key] = F(math.exp(float(arg))) if np.isfinite(arg) else (F(0) if arg < 0 else F(np.nan))
        return wcache[key]

    def clamp(v):
        v = F(255) if v > 255 else v
        return F(0) if v < 0 else v

    for cid in range(rows * cols):
        m = mean[cid]
        sums = np.zeros((14, 256), np.float32)
        npts = np.zeros(256, np.int64)
        for tid in range(256):
            tx, ty = tid & 15, tid >> 4
            acc = [F(0)] * 13
            for yy in range(rpy):
                for xx in range(rpx):
                    ax, ay = int(m["x"]) + (tx - 8) * rpx + xx, int(m["y"]) + (ty - 8) * rpy + yy
                    if not (0 <= ax < W and 0 <= ay < H) or labels[ay, ax] != cid:
                        continue
                    c = bgr[ay, ax].astype(np.float32)
                    e = c - np.array([m["r"], m["g"], m["b"]], np.float32)
                    cf = weight((e[0] * e[0] + e[1] * e[1]) + e[2] * e[2], cs)
                    dx, dy = F(ax - int(m["x"])), F(ay - int(m["y"]))
                    sf = weight(dx * dx + dy * dy, ss)
                    with np.errstate(all="ignore"):
                        for k in range(3):
                            acc[k] = acc[k] + clamp(c[k] * cf * sf)
                        acc[3] = acc[3] + F(ax) * cf * sf
                        acc[4] = acc[4] + F(ay) * cf * sf
                        acc[5] = acc[5] + cf * sf
                        n, p = nrm[ay, ax], pts[ay, ax]
                        if p[2] > 50 and (n[0] != -1 or n[1] != -1 or n[2] != -1):
                            nd = (n[0] * spn[cid, 0] + n[1] * spn[cid, 1]) + n[2] * spn[cid, 2]
                            nd = F(0) if nd < 0 else nd
                            if nd > thr:
                                for k in range(3):
                                    acc[6 + k] = acc[6 + k] + p[k]
                                    acc[9 + k] = acc[9 + k] + n[k]
                                acc[12] = acc[12] + nd
                                npts[tid] += 1
            sums[:13, tid] = acc
        with np.errstate(all="ignore"):
            step = 128
            while step >= 1:
                sums[:, :step] = sums[:, :step] + sums[:, step:2 * step]
                npts[:step] += npts[step:2 * step]
                step //= 2
            s, np_ = sums[:, 0], int(npts[0])
            size = s[5]
            if not (size != 0):
                continue
            rgb = [max(0, min(255, f2i(s[k] / size))) for k in range(3)]
            px, py = f2i(s[3] / size), f2i(s[4] / size)
            if np_ != 0:
                if 0 <= px < W and 0 <= py < H and pts[py, px, 2] > 50:
                    centers[cid] = pts[py, px]
                else:
                    centers[cid] = s[6:9] / F(np_)
                    nx, ny = centers[cid, 0] / centers[cid, 2], centers[cid, 1] / centers[cid, 2]
                    qx, qy = f2i(nx * intr[0] + intr[2]), f2i(intr[5] - ny * intr[4])
                    if not (qx < 0 or qx >= W or qy < 0 or qy <= H):
                        px, py = qx, qy
                v = s[9:12] / F(np_)
                ln = np.sqrt((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2])
                spn[cid] = v / ln
                var[cid] = s[12] / F(np_)
            else:
                spn[cid], centers[cid], var[cid] = -1, 0, 0
            mean[cid] = (rgb[0], rgb[1], rgb[2], 0, px, py, f2i(size))
    return mean, centers, spn, var


def test_python_port_of_the_two_new_kernels_is_bit_equal(R):
    W, H, rows, cols = 96, 64, 4, 6
    bgr, pts, nrm = small_frame(5, W, H)
    assert np.isnan(nrm).any() and (nrm == -1).all(-1).any() and (pts[..., 2] == 0).any()
    st = R.State(W, H, rows, cols, K)
    st.init_ld()
    st.sample(bgr, pts, nrm)
    sig = (10.0, 50.0, 50.0, 150.0)
    thr = R.acos_threshold()
    for it in range(2):
        exp_l, exp_d = port_calculate_ld(W, H, rows, cols, bgr, pts, nrm, st.ld["l"], st.ld["d"], st.mean, st.centers, st.normals, *sig)
        st.calculate_ld(bgr, pts, nrm, *sig)
        assert np.array_equal(st.ld["l"], exp_l) and np.array_equal(st.labels, exp_l), f"labels, iteration {it}"
        assert same_floats(st.ld["d"], exp_d), f"distances, iteration {it}"
        st.analyze(bgr, pts, nrm)
        exp = port_weighted(W, H, rows, cols, bgr, pts, nrm, st.labels, st.mean, st.centers, st.normals, st.variance,
                            sig[0], sig[1], st.intr, thr)
        st.weighted(bgr, pts, nrm, sig[0], sig[1])
        assert np.array_equal(st.mean, exp[0]), f"mean, iteration {it}"
        assert same_floats(st.centers, exp[1]) and same_floats(st.normals, exp[2]) and same_floats(st.variance, exp[3]), it
    assert (st.labels == -1).any() and len(np.unique(st.labels)) > rows * cols // 2
    # the kernel-by-kernel walk is what nasp_segmentation does
    full = R.segmentation(bgr, pts, nrm, rows, cols, K, *sig, 2)
    assert np.array_equal(full["labels"], st.labels) and np.array_equal(full["mean"], st.mean)
    assert same_floats(full["ld"]["d"], st.ld["d"]) and same_floats(full["variance"], st.variance)


# ---------------------------------------------------------------------------------------------------------------------
# micro-cases
# ---------------------------------------------------------------------------------------------------------------------
def dist(R, normal=(0, 0, -1), sp_normal=(0, 0, -1), z=1000.0, cz=1000.0, color=(10, 20, 30), mean=(10, 20, 30, 5, 5), xy=(5, 5),
         k=(1.0, 1.0, 1.0, 1.0)):
    return R.candidate_distance(xy[0], xy[1], color, (0, 0, z), normal, mean, (0, 0, cz), sp_normal, 1.0, *k)


def test_na2_normal_term_is_zero_without_valid_depth_or_normal(R):
    assert dist(R) == 0.0                                                # parallel normals, same colour, place and depth
    assert dist(R, sp_normal=(0, 1, 0)) == F(65025.0)                    # orthogonal: 255^2 * (1 - 0)
    assert dist(R, sp_normal=(0, 0, 1)) == F(65025.0)                    # opposite: clamped to 0 from below
    # invalid depth on either side: no depth term and NO normal term (uninitialised in the reference)
    assert dist(R, sp_normal=(0, 1, 0), z=50.0) == 0.0
    assert dist(R, sp_normal=(0, 1, 0), cz=0.0) == 0.0
    # a bad normal on either side: depth term only
    assert dist(R, normal=(-1, -1, -1), sp_normal=(0, 1, 0), cz=1007.0) == 7.0
    assert dist(R, normal=(0, 0, -1), sp_normal=(-1, -1, -1), cz=1007.0) == 7.0
    # the term is formed in double and rounded once: 65025 * (1 - 0.123f) != 65025.0f * (1.0f - 0.123f)
    nd = F(0.123)
    got = dist(R, normal=(0, 0, float(nd)), sp_normal=(0, 0, 1))
    assert got == F(65025.0 * (1.0 - float(nd))) and got != F(65025.0) * (F(1.0) - nd)
    # unnormalised cluster normals: normal_diff above 1 gives a negative term
    assert dist(R, normal=(0, 0, 2), sp_normal=(0, 0, 1)) == F(-65025.0)


def test_bad_normal_tests_and_in_sampling_or_elsewhere(R):
    # one component equal to -1: a GOOD normal for calculateLD ('||', .cu:240-245) ...
    assert dist(R, normal=(-1, 0, 0), sp_normal=(-1, 0, 0)) == 0.0      # normal_diff = 1
    assert dist(R, normal=(-1, 0, 0), sp_normal=(0, 1, 0)) == F(65025.0)
    # ... and a BAD one for the sampling kernel ('&&', .cu:57-62): its gradient terms are not scaled.
    # Rows 0..5 (all 61 taps inside the buffer, the taps being absolute) are white, the 60 taps with a negative index read
    # colour 0 and normal 0 (NA1), the candidates' colour grows with x: unscaled, 61 bright taps against 60 dark ones make the
    # BRIGHTEST candidate (x = centre + 3) the flattest; with normals (1, 0, 0) -- good for '&&', normal_diff = 1 -- the
    # in-buffer terms are g * (1 - 1) = 0, only the dark taps count and the DARKEST candidate (x = centre - 4) wins
    W, H, rows, cols = 32, 40, 2, 2
    bgr = np.repeat((100 + 4 * np.arange(W, dtype=np.int64))[None, :, None], H, 0).repeat(3, 2).astype(np.uint8)
    bgr[:6] = 255
    pts = np.zeros((H, W, 3), np.float32)
    pts[..., 2] = 1000
    base = np.zeros((H, W, 3), np.float32)
    base[..., 2] = -1.0                                                   # unit normals (0, 0, -1): bad for '&&'
    tilted = np.zeros((H, W, 3), np.float32)
    tilted[..., 0] = 1.0
    a, b = R.State(W, H, rows, cols, K), R.State(W, H, rows, cols, K)
    a.sample(bgr, pts, base)
    b.sample(bgr, pts, tilted)
    assert a.mean["x"].tolist() == [11, 27, 11, 27]
    assert b.mean["x"].tolist() == [4, 20, 4, 20]
    # sic: b = first channel + 2 (.cu:173), wrapping in a byte
    assert a.mean["b"].tolist() == [(int(v) + 2) & 255 for v in a.mean["r"]]
    assert same_floats(a.normals, base[a.mean["y"], a.mean["x"]]) and same_floats(a.centers, pts[a.mean["y"], a.mean["x"]])


def test_label_reset_with_depth_sigma_zero_and_normal_sigma_nonzero(R):
    W, H, rows, cols = 32, 32, 2, 2
    bgr, pts, nrm = small_frame(3, W, H, nan_normals=False)
    pts[3, 3, 2], pts[4, 4, 2], pts[5, 5, 2] = 49.0, 50.0, 0.0
    outs = {}
    for ds, ns in ((0.0, 150.0), (50.0, 0.0), (0.0, 0.0)):
        outs[ds, ns] = R.segmentation(bgr, pts, nrm, rows, cols, K, 10.0, 50.0, ds, ns, 1)
    for key in ((0.0, 150.0), (50.0, 0.0)):
        o = outs[key]
        assert o["labels"][3, 3] == -1 and o["labels"][5, 5] == -1 and o["ld"]["d"][3, 3] == 0 and o["ld"]["l"][5, 5] == -1
        assert o["labels"][4, 4] >= 0                                     # z == 50 is not '< 50'
        assert ((o["labels"] == -1) == (pts[..., 2] < 50)).all()
    assert (outs[0.0, 0.0]["labels"] >= 0).all()                          # both sigmas 0: no reset


def flat_frame(W, H, z=1000.0):
    bgr = np.full((H, W, 3), 100, np.uint8)
    pts = np.zeros((H, W, 3), np.float32)
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float32)
    pts[..., 0], pts[..., 1], pts[..., 2] = (xx - W / 2) * z / F(575.8), (H / 2 - yy) * z / F(575.8), z
    nrm = np.zeros((H, W, 3), np.float32)
    nrm[..., 2] = -1.0
    return bgr, pts, nrm


def test_in_image_projection_is_discarded_by_the_height_test(R):
    """.cu:652 / :1031 read pixel.y <= height: a projected centre inside the image is replaced by the mean position; one
    BELOW the image (row > height) is kept"""
    W, H, rows, cols = 32, 32, 2, 2
    bgr, pts, nrm = flat_frame(W, H)
    pts[2:30, 2:30, 2] = 0.0                      # the points under the cluster means are invalid -> the else branch runs
    st = R.State(W, H, rows, cols, np.array([[575.8, 0, 16.0], [0, 575.8, 16.0], [0, 0, 1]]))
    st.init_ld()
    st.sample(bgr, pts, nrm)
    st.calculate_ld(bgr, pts, nrm, 10.0, 50.0, 50.0, 150.0)
    st.analyze(bgr, pts, nrm)
    # the centres are averages (no valid point has these coordinates), i.e. the else branch ran; its projection falls
    # inside the image and is thrown away: the mean position of the members stays
    assert (st.centers[:, 2] == 1000.0).all() and not (st.centers[:, None, :2] == pts[None, pts[..., 2] > 50][..., :2]).all(-1).any()
    ys = np.mgrid[0:H, 0:W][0]
    members_y = [int(ys[st.labels == k].sum()) // int((st.labels == k).sum()) for k in range(4)]
    assert (st.mean["size"] > 0).all() and st.mean["y"].tolist() == members_y and max(members_y) < H
    # intrinsics that project every centre to a row below the image: kept, although it is outside
    st2 = R.State(W, H, rows, cols, np.array([[575.8, 0, 16.0], [0, 575.8, 40.0 + H], [0, 0, 1]]))
    st2.init_ld()
    st2.sample(bgr, pts, nrm)
    st2.calculate_ld(bgr, pts, nrm, 10.0, 50.0, 50.0, 150.0)
    st2.analyze(bgr, pts, nrm)
    assert (st2.mean["y"] > H).all() and st2.mean["x"].tolist() == st.mean["x"].tolist()


def test_tree_tie_break_and_nan(R):
    d = np.full(64, 5.0, np.float32)
    lab = np.arange(64)
    assert R.tree64(d, lab) == (5.0, 0)                                   # all equal: element 0 stays
    d[:] = 9.0
    d[[3, 32, 17]] = 1.0
    # equal minima: the first in BIT-REVERSED order wins (32 = reversed 1 comes before 17 and 3)
    assert R.tree64(d, lab) == (1.0, 32)
    d[:] = 9.0
    d[[48, 16]] = 1.0
    assert R.tree64(d, lab)[1] == 16                                      # 16 = reversed 2, 48 = reversed 3
    # a NaN neither replaces nor is replaced: as the LEFT operand it shadows its right sibling ...
    d[:] = 9.0
    d[0] = np.nan
    d[32] = 1.0
    v, l = R.tree64(d, lab)
    assert np.isnan(v) and l == 0                                         # element 0 is NaN and is never replaced
    # ... as a RIGHT operand it is ignored
    d[:] = 9.0
    d[32] = np.nan
    d[5] = 2.0
    assert R.tree64(d, lab) == (2.0, 5)
    # a left NaN deeper in the tree hides the minimum behind it and then loses higher up
    d[:] = 9.0
    d[1] = np.nan            # level one: N(1, 33) keeps the NaN, 33 (the true minimum) is gone
    d[33] = 0.5
    d[2] = 3.0
    assert R.tree64(d, lab) == (3.0, 2)


def test_nan_normal_through_calculate_ld(R):
    W, H, rows, cols = 32, 32, 2, 2
    bgr, pts, nrm = flat_frame(W, H)
    nrm[10, 10] = np.nan
    o = R.segmentation(bgr, pts, nrm, rows, cols, K, 10.0, 50.0, 50.0, 150.0, 1)
    # candidates 0..63 of pixel (10, 10): cluster grid 2 x 2 around cell (0, 0) -> leaves t = 36, 37, 44, 45 are clusters,
    # all with a NaN distance; leaf 0 (outside the grid) carries the previous assignment (999999.9, label 0) and is the
    # left-most operand all the way up: a NaN never replaces it
    assert o["labels"][10, 10] == 0 and o["ld"]["d"][10, 10] == F(999999.9)
    assert o["ld"]["d"][10, 11] < 999999.0


def test_cluster_with_weight_sum_zero_keeps_its_record(R):
    W, H, rows, cols = 32, 32, 2, 2
    bgr, pts, nrm = flat_frame(W, H)
    rng = np.random.default_rng(0)
    bgr[:16, :16] = rng.integers(0, 2, (16, 16, 1)) * 255        # cluster 0: black / white, mean colour grey
    st = R.State(W, H, rows, cols, K)
    st.init_ld()
    st.sample(bgr, pts, nrm)
    st.ld["l"][:] = (np.mgrid[0:H, 0:W][0] // 16) * 2 + np.mgrid[0:H, 0:W][1] // 16
    st.analyze(bgr, pts, nrm)
    after_analyze = st.outputs()
    st.weighted(bgr, pts, nrm, 0.5, 50.0)                        # colour sigma 0.5: exp(-d / 0.5) = 0 for every d >= 52
    m = st.mean
    # every pixel of cluster 0 is > 100 levels from the mean colour: weight sum 0 -> nothing stored (NA5: as analyzed)
    assert m[0] == after_analyze["mean"][0] and m[0]["size"] == 256
    assert st.variance[0] == 0.0 and same_floats(st.normals[0], after_analyze["normals"][0])
    # the uniform clusters store a float weight sum truncated to int (.cu:1064)
    assert 0 < m[3]["size"] < 256 and after_analyze["mean"][3]["size"] == 256
    assert st.variance[3] == 1.0
    # NA5: a fresh Segmentation starts every cluster at size 0 / variance 0 whatever the buffers held
    st.mean["size"][:] = 77
    st.variance[:] = 0.25
    o = st.segmentation(bgr, pts, nrm, 10.0, 50.0, 50.0, 150.0, 0)
    assert (o["mean"]["size"] == 0).all() and (o["variance"] == 0).all()


def test_geometry_rejection(R):
    assert R.check_geometry(640, 480, 15, 20) and R.check_geometry(320, 240, 7, 9) and R.check_geometry(70, 50, 3, 5)
    assert not R.check_geometry(640, 480, 15, 81)        # 7-pixel windows
    assert not R.check_geometry(640, 56, 8, 20)          # window height 7
    assert not R.check_geometry(80, 480, 15, 9)          # window 80 / 9 = 8, but 80 / 8 = 10 != 9: the mean index would overrun
    assert not R.check_geometry(120, 480, 15, 11) and R.check_geometry(120, 480, 15, 12)
    assert R.check_geometry(64, 64, 8, 8) and not R.check_geometry(64, 5, 1, 8) and not R.check_geometry(0, 64, 8, 8)


# ---------------------------------------------------------------------------------------------------------------------
# NA3 / NA4
# ---------------------------------------------------------------------------------------------------------------------
def test_na3_threshold_is_the_acos_decision(R):
    t = R.acos_threshold()
    assert t == F(0.5) and bits(np.array([t]))[0] == 0x3F000000
    c = F(3.141592653) / F(3.0)
    x = t
    for _ in range(2000):
        x = np.nextafter(x, F(0), dtype=np.float32)
    for _ in range(4001):
        acos_says = F(math.acos(float(x))) < c
        assert bool(x > t) == bool(acos_says), float(x)
        x = np.nextafter(x, F(1), dtype=np.float32)
    assert not (F(np.nan) > t)                                   # a NaN normal_diff fails the test, as acos(NaN) < c does


# share of numerators whose weight is one ulp off the correctly rounded exp (it is never more than one ulp off).
# Measured with the C library's exp on the three sigmas below: 0 of 390 553 weights (every numerator 0 .. 3*255^2 for sigma 10 and 50, 0 .. 400 for sigma 0.7).  The bound allows for a libm whose
# exp is only faithfully rounded: the float rounding then differs only when the double falls within one double-ulp of a
# float rounding boundary, 2 / 2^29 of all arguments.
NA4_OFF_BY_ONE_BOUND = 1e-6
NA4_OFF_BY_ONE_MEASURED = 0.0


def test_na4_weight_against_extended_precision_exp(R):
    from decimal import Decimal, getcontext
    getcontext().prec = 50
    total = off = 0
    for sigma, top in ((10.0, 3 * 255 * 255), (50.0, 3 * 255 * 255), (0.7, 400)):
        den = F(2.0) * (F(sigma) * F(sigma))
        for num in range(top + 1):                    # every integer numerator the kernel can form
            got = R.weight(num, sigma)
            arg = -F(num) / den
            exact = Decimal(float(arg)).exp()
            # correctly rounded float of the exact value: round the 50-digit value through float64 is not enough in
            # general, so compare against both float neighbours
            near = F(float(exact))
            if got != near:
                lo, hi = np.nextafter(near, F(-1)), np.nextafter(near, F(2))
                assert got in (lo, hi), (num, sigma, got, near)
                # 'near' itself may be a double-rounded value: accept only if got is at least as close
                if abs(Decimal(float(got)) - exact) > abs(Decimal(float(near)) - exact):
                    off += 1
            total += 1
    print(f"NA4: {off} of {total} weights one ulp off the correctly rounded value")
    assert off <= NA4_OFF_BY_ONE_BOUND * total, (off, total)
    # monotone, ending in exact zeros: what lets the library truncate its table
    w = np.array([R.weight(n, 10.0) for n in range(0, 30000, 50)])
    assert (np.diff(w) <= 0).all() and w[0] == 1.0 and w[-1] == 0.0
    assert R.weight(0, 0.0) != R.weight(0, 0.0) and R.weight(1, 0.0) == 0.0      # sigma 0: -0/0 = NaN, -1/0 = -inf


# ---------------------------------------------------------------------------------------------------------------------
# goldens
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("iteration", [1, 3])
def test_goldens(R, iteration):
    import types
    path = os.path.join(GOLDEN, "make_golden_nasp.py")          # the generator's own inputs and parameters
    gen = types.ModuleType("make_golden_nasp")
    gen.__file__ = path
    exec(compile(open(path).read(), path, "exec"), gen.__dict__)
    bgr, pts, nrm = gen.inputs()
    g = np.load(os.path.join(GOLDEN, f"nasp_it{iteration}.npz"))
    assert os.path.getsize(os.path.join(GOLDEN, f"nasp_it{iteration}.npz")) < os.path.getsize(os.path.join(GOLDEN, "golden_crops.npz"))
    o = R.segmentation(bgr, pts, nrm, gen.ROWS, gen.COLS, gen.intrinsics(), *gen.SIGMAS, iteration)
    assert np.array_equal(o["labels"].astype(np.int16), g["labels"])
    assert np.array_equal(o["mean"].view(np.uint8), g["mean"])
    for key in ("centers", "normals", "variance"):
        assert np.array_equal(bits(o[key]), g[key]), key
    assert gen.crc(bits(o["ld"]["d"])) == int(g["ld_d_crc32"])
