"""A seeded draw of cases for the output side of the library -- the tail of SPDepthSuperResolution::Process (plane fit, plane
projection and mrf sweeps, csrc/spdsr_kernels.hip, through kde_stage_spdsr_tail), Buffer2D (K4) and DimensionConvertor (K2/K3,
csrc/stream_kernels.hip), PointCloudXYZRGB (csrc/cloud_kernels.hip) and MeanError3D (csrc/error3d_kernels.hip) -- and the
comparison of the library with the binary64 references of tests/spdsr_tail_cases.py, the CPU oracle (oracle/kde_oracle.c
through oracle/oracle.py) and the numpy statements of tests/cloud_cases.py and tests/error3d_cases.py.

    draw(kind, seed, index)   one self-contained case: sizes, parameters, pointer offsets and every input
    run_case(torch, F_, c)    builds the object, runs the calls on the device and returns the violations (strings); none: equal

A case is drawn from np.random.default_rng([seed, kind number, index]) alone, so any case can be made again without the ones
before it.  Every parameter is drawn from the whole domain create, SetParametor and the calls admit, so a refusal is a
violation.  The kind numbers are positions in ALL_KINDS.  A `process` case is the `spdsr` case of superpixel_sweep of the same
seed and index, drawn by that module's generator: that sweep holds the head, this one the tail as Process runs it.

The bars, none new:
  tail      tests/test_gpu_spdsr_tail.py: SC.planes_compare for fitted planes (normals within 2 x 2^-23, d within 2 ulps, markers
            to the bit with the w the frame slot held, NaN rows NaN), handed-in planes back to the bit; check_fit's bars for the
            projection (8 ulps where |den| >= 0.5, unprojected pixels to the bit, x, y = ray * z to the bit, the NaN / inf
            classes of okde_projection_plane for every denominator); SC.sweep_compare against sweeps64 from the device's own
            plane-fitted z, the NaN / inf masks of okde_projection_plane, 8 x TAIL_E32[sweeps] on the value, at most MAX_FLAGGED
            of the pixels within MARGIN of a decision (none at 0 or 1 sweeps).  A second call is compared against the reference
            with the planes the first call left in the frame slot, never against the first call
  process   after Process, in the product build and in the stage build: ClusterND against planes64 of the build's OWN refined labels
            and EdgeEnhanced3DPoints under SC.planes_compare, PlaneFitted3D under check_fit's bars; then kde_stage_spdsr_tail on
            those labels and points with that ClusterND and 20 sweeps gives Process's PlaneFitted3D and OptimizedPoints bit for bit
  buffer2d  test_buffer2d_bit_exact: after every operation the raw buffer and both maps have NaN where oracle.Buffer2D has it
            and the same bits everywhere else (the bits of a NaN are not compared: x86 and the GPU give other signs and payloads)
  convert   test_dimension_convertor_bit_exact: the same rule against oracle.p2r_depth / p2r_points / p2r_interp / r2p, and
            depth_u16_cases.to_u16 for points_to_depth
  cloud     test_gpu_cloud.py: the bytes of cloud_cases.statement, exact counts, nothing written behind count[f]
  error3d   test_gpu_error3d.py: exact counts, the sum within count * 2^-53 * sum of the exact sum of the float32 terms, the
            mean as the float conversion of sum / count
tests/test_output_sweep.py holds the conditions on the draw.  The non-temporal forms of K2/K3, the cloud and the metric start
at calls that move more than 256 MiB, far beyond the frames drawn here: tests/test_gpu_output_sweep.py reaches the vector and
the scalar forms only, tests/test_gpu_streaming_forms.py runs the same cases again on the stage build with the threshold at 0
(convert_streaming_sites says which `convert` cases then stream).

This module needs no GPU: torch and the filters module are handed to run_case().
"""
from types import SimpleNamespace

import numpy as np

import cloud_cases as CC
import depth_u16_cases as DU
import error3d_cases as EC
import spdsr_tail_cases as SC
import superpixel_sweep as SS
from plane_sweep import camera_matrix
from superpixel_sweep import ERS_STYLES, PIPE_PINNED, admitted, same_floats

F = np.float32
ALL_KINDS = ("tail", "process", "buffer2d", "convert", "cloud", "error3d")      # the kind number is the position here
KINDS = ALL_KINDS

MAX_W, MAX_H = 264, 136
SEGMENT, OCTET, SCAN_PASS = 2048, 8, 256            # csrc/cloud_kernels.hip, csrc/error3d_kernels.hip
MULTI_PASS = (1024, 520)                            # 260 segments: the cloud scan's second pass, once per seed

INF = F(np.inf)
# depth, and through insertData(float2) / insertWeighted the state: NaN, +-inf, 3e38, +-2^31 and their neighbours, -0, denormals,
# negative values (-1.5 converts to -1: against a depth >= 2^31 the integer difference is INT_MIN, whose abs is INT_MIN)
HOSTILE = np.array([np.nan, np.inf, -np.inf, 3.0e38, 2.0 ** 31, -2.0 ** 31, -0.0, 1.0e-40, -1.0e-40, np.nextafter(F(2.0 ** 31), F(0)),
                    -1.5, -1000.0, 4.0e9, -3.0e38], F)
HOSTILE_W = np.array([-1.0, -0.5, 0.0, 1.0e38, np.nan], F)
UNIT_Z = np.array([np.nextafter(F(1), F(0)), 1.0, 0.999, -np.nextafter(F(1), F(0)), -1.0, -0.999, np.nextafter(F(1), F(2))], F)
BUF_CLASSES = ("scene", "limit", "fifty", "hostile")
BUF_OPS = ("update", "update_seq", "insert_depth", "insert_float2", "insert_weighted", "get")
FORMATS = ("points", "depth", "u16")

# the budget of tests/test_gpu_output_sweep.py; tests/test_output_sweep.py holds the conditions on the draw over exactly this
SEEDS = (1, 2)
CASES_PER_KIND = dict(tail=14, process=SS.CASES_PER_KIND["spdsr"], buffer2d=48, convert=32, cloud=32, error3d=24)


def kinds():
    return KINDS


def budget(kind):
    return [(seed, index) for seed in SEEDS for index in range(CASES_PER_KIND[kind])]


def oracle():
    from oracle import oracle as O
    return O


def _factor(px):
    """every (W, H) with W * H = px inside MAX_W x MAX_H"""
    return [(w, px // w) for w in range(1, min(px, MAX_W) + 1) if px % w == 0 and px // w <= MAX_H]


# pixel counts around the octet of 8, the wave's 512 and the segment of 2048 (2049 = 3 x 683 has no frame inside 264 x 136: 2050)
PIXELS = tuple(p for p in (1, 7, 8, 9, 15, 16, 17, 63, 64, 65, 511, 512, 513, 2040, 2047, 2048, 2050, 2056, 4095, 4096, 4097, 6144,
                           6150) if _factor(p))


def _size(rng, slot):
    """(W, H) of a case: slot < len(PIXELS) deals that pixel count, any other slot is free"""
    if 0 <= slot < len(PIXELS):
        f = _factor(PIXELS[slot])
        return f[int(rng.integers(0, len(f)))]
    return int(rng.integers(1, MAX_W + 1)), int(rng.integers(1, MAX_H + 1))


def _camera(rng, W, H):
    """an intrinsic matrix with a fractional principal point (the library truncates it), in a quarter of the draws outside the frame"""
    f = float(rng.uniform(0.5, 2.0)) * max(W, H, 8)
    cx, cy = W / 2.0 + float(rng.uniform(-0.9, 0.9)), H / 2.0 + float(rng.uniform(-0.9, 0.9))
    if rng.random() < 0.25:
        cx, cy = [(-3.7, cy), (cx, H + 10.4), (W + 0.5, -0.6)][int(rng.integers(0, 3))]
    return np.array([[f, 0.0, cx], [0.0, f * float(rng.uniform(0.9, 1.1)), cy], [0.0, 0.0, 1.0]], np.float64)


# ---- buffer2d -----------------------------------------------------------------------------------------------------------
def limit_pair(k):
    """(d_lo, d_hi): neighbouring float32 around 100 k with (float)k < d_hi * 0.01f and not (float)k < d_lo * 0.01f"""
    d = F(100 * k)
    while F(d * F(0.01)) > F(k):
        d = np.nextafter(d, F(0))
    while F(np.nextafter(d, INF) * F(0.01)) <= F(k):
        d = np.nextafter(d, INF)
    return d, np.nextafter(d, INF)


def _buf_frame(rng, c, exact=False):
    """one depth frame of the case's scene: 0.2 % noise (inside the 1 % rule), 5 % outliers outside it, 5 % holes; at the
    case's marked pixels what its class deals"""
    W, H = c.size
    z = c.base.astype(np.float64)
    if not exact:
        z = z * (1.0 + rng.uniform(-0.002, 0.002, (H, W)))
        out = rng.random((H, W)) < 0.05
        z[out] *= 1.0 + rng.choice([-1.0, 1.0], int(out.sum())) * rng.uniform(0.03, 0.05, int(out.sum()))
        z[rng.random((H, W)) < 0.05] = 0.0
    z = z.astype(F)
    m = c.marked
    k = int(m.sum())
    if c.cls == "limit" and not exact:
        z[m] = np.where(rng.random(k) < 0.5, c.pairs[0], c.pairs[1])
    elif c.cls == "fifty" and not exact:
        z[m] = rng.choice(np.array([50.0, np.nextafter(F(50), F(100)), 50.3], F), k)
    elif c.cls == "hostile":
        z[m] = rng.choice(HOSTILE, k)
    return z


def _buf_op(rng, c, op):
    W, H = c.size
    o = SimpleNamespace(op=op, off=int(rng.integers(0, 4)), get_off=tuple(int(v) for v in rng.integers(0, 4, 2)), data=None)
    if op == "update" or op == "insert_depth":
        o.data = _buf_frame(rng, c)
    elif op == "update_seq":
        o.data = np.stack([_buf_frame(rng, c) for _ in range(int(rng.integers(2, 7)))])
    elif op == "insert_float2":
        o.data = np.stack([_buf_frame(rng, c), rng.uniform(-10.0, 10.0, (H, W)).astype(F)], -1)
    elif op == "insert_weighted":
        w = rng.choice(np.array([1.0, 2.0, 3.0, 7.0], F), (H, W))
        d = _buf_frame(rng, c)
        if c.cls == "hostile":                                # a state neither update nor insertData(float*) can leave
            k = int(c.marked.sum())
            w[c.marked] = np.where(rng.random(k) < 0.7, rng.choice(HOSTILE_W, k), w[c.marked])
            d[c.marked] = np.where(rng.random(k) < 0.5, c.base[c.marked], d[c.marked])
        o.data = np.stack([d, w], -1)
    return o


def _draw_buffer2d(rng, c):
    c.cls = BUF_CLASSES[c.index % 4]
    rest = (c.index // 4) % 4                                 # W * H % 4: whole quads, and the three scalar tails
    if rng.random() < 0.15:
        c.size = [(4, 1), (1, 1), (2, 1), (1, 3)][rest] if rng.random() < 0.5 else [(2, 2), (5, 1), (3, 2), (7, 1)][rest]
    else:
        while True:
            W, H = int(rng.integers(1, 81)), int(rng.integers(1, 41))
            if W * H % 4 == rest:
                c.size = (W, H)
                break
    W, H = c.size
    y, x = np.mgrid[0:H, 0:W]
    c.base = (float(rng.uniform(600.0, 4000.0)) + rng.uniform(-2.0, 2.0) * x + rng.uniform(-2.0, 2.0) * y).astype(F)
    c.marked = rng.random((H, W)) < float(rng.uniform(0.05, 0.25))
    c.marked.reshape(-1)[int(rng.integers(0, W * H))] = True
    k = int(c.marked.sum())
    if c.cls == "limit":                                      # the record at 101 k (or 99 k), the sample on either side of 100 k
        ks = rng.integers(6, 41, k)
        pairs = np.array([limit_pair(int(v)) for v in ks], F)
        below = (rng.random(k) < 0.5) & (pairs[:, 0] >= 100 * ks)       # int(d_lo) is 100 k: the difference is k from below too
        c.base[c.marked] = (np.where(below, 99 * ks, 101 * ks) + rng.uniform(0.0, 0.99, k)).astype(F)
        c.pairs = (pairs[:, 0], pairs[:, 1])
    elif c.cls == "fifty":
        c.base[c.marked] = np.where(rng.random(k) < 0.5, F(50.3), F(0.0))
    count = int(rng.integers(3, 9))
    p = np.array([0.34, 0.26, 0.1, 0.1, 0.1, 0.1])
    names = [str(v) for v in rng.choice(BUF_OPS, count, p=p)]
    if c.cls == "limit":                                      # the scene itself, then the samples on the limit
        names[:2] = ["insert_depth", "update"]
    if c.cls == "hostile":                                    # a hostile state, then an update of it
        names[:2] = [str(rng.choice(["insert_float2", "insert_weighted"])), str(rng.choice(["update", "update_seq"]))]
    c.ops = [_buf_op(rng, c, name) for name in names]
    if c.cls == "limit":
        c.ops[0].data = _buf_frame(rng, c, exact=True)


def buffer2d_mirror(c):
    """the history of the case on oracle.Buffer2D -> per operation (raw [H,W,2], depth map, weight map), and the largest weight
    an update raised a record to"""
    O = oracle()
    W, H = c.size
    ob = O.Buffer2D(W, H)
    out, raised = [], 0.0
    for o in c.ops:
        before = ob.weight_map()
        if o.op == "update":
            ob.update(o.data)
        elif o.op == "update_seq":
            for frame in o.data:
                ob.update(frame)
        elif o.op == "insert_depth":
            ob.insert_depth(o.data)
        elif o.op == "insert_float2":
            ob.insert_float2(o.data)
        elif o.op == "insert_weighted":
            ob.insert_weighted(np.ascontiguousarray(o.data))
        after = ob.weight_map()
        if o.op.startswith("update"):
            with np.errstate(invalid="ignore"):
                up = (after != before) & np.isfinite(after)
            if up.any():
                raised = max(raised, float(after[up].max()))
        out.append((ob.buf.copy().view(F).reshape(H, W, 2), ob.depth_map(), after))
    return out, raised


def _want_buffer2d(c):
    c.want, c.raised = buffer2d_mirror(c)


def int_min_difference_case(n):
    """found by reading the scalar form's code object: a record whose integer difference from the sample is INT_MIN.  n x 1
    records, n = 4 (one quad: the packed form) or n = 3 (the scalar form), with the same state and samples: the state (-1.5, 1),
    (-1, 2), (-2^31, 1), (3e38, 2), installed by insertWeighted; the samples 2^31, +inf, 100, 60.  (int)-1.5 - (int)2^31 = -1 -
    INT_MAX = INT_MIN, abs keeps it (Buffer2D.cu:19), and (float)INT_MIN < d * 0.01f holds: records 0 and 1 are averaged to
    (715827904, 2) = ((-1.5 * 2 + 2^31) / 3, 2) and (+inf, 3).  Records 2 and 3: the differences wrap to 2^31 - 100 and are INT_MAX - 60, nothing changes"""
    state = np.array([[-1.5, 1.0], [-1.0, 2.0], [-2.0 ** 31, 1.0], [3.0e38, 2.0]], F)
    d = np.array([2.0 ** 31, np.inf, 100.0, 60.0], F)
    c = SimpleNamespace(kind="buffer2d", seed=0, index=-n, cls="named", size=(n, 1), want=None)
    c.ops = [SimpleNamespace(op="insert_weighted", off=0, get_off=(0, 0), data=state[:n].reshape(1, n, 2).copy()),
             SimpleNamespace(op="update", off=0, get_off=(0, 0), data=d[:n].reshape(1, n).copy())]
    return c


# ---- convert ------------------------------------------------------------------------------------------------------------
def _hostile_depth(rng, shape, base=1500.0):
    """sensor-like depth with holes, a tenth of the samples out of HOSTILE and UNIT_Z"""
    z = (base + rng.uniform(-900.0, 2500.0, shape)).astype(F)
    z[rng.random(shape) < 0.05] = 0.0
    hit = rng.random(shape) < 0.1
    z[hit] = rng.choice(np.concatenate([HOSTILE, UNIT_Z]), int(hit.sum()))
    z.reshape(-1)[int(rng.integers(0, z.size))] = UNIT_Z[int(rng.integers(0, UNIT_Z.size))]
    return z


def _draw_convert(rng, c):
    c.n = 1 + c.index % 3
    rest = (c.index // 3) % 4
    while True:
        W, H = (int(rng.integers(1, 12)), int(rng.integers(1, 6))) if rng.random() < 0.2 else (int(rng.integers(1, 121)), int(rng.integers(1, 61)))
        if W * H % 4 == rest:
            break
    c.size, c.K = (W, H), _camera(rng, W, H)
    c.off = {k: int(rng.integers(0, 4)) if rng.random() < 0.6 else 0 for k in ("depth", "points", "out", "zf", "zu")}
    c.depth = _hostile_depth(rng, (c.n, H, W))
    pts = np.stack([rng.uniform(-3000.0, 3000.0, (c.n, H, W)), rng.uniform(-3000.0, 3000.0, (c.n, H, W)), np.zeros((c.n, H, W))], -1).astype(F)
    pts[..., 2] = _hostile_depth(rng, (c.n, H, W))
    hit = rng.random((c.n, H, W)) < 0.05                      # hostile x and y as well
    pts[..., 0][hit] = rng.choice(HOSTILE, int(hit.sum()))
    pts[..., 1][rng.random((c.n, H, W)) < 0.03] = F(-0.0)
    half = rng.random((c.n, H, W)) < 0.1                      # the ties of points_to_depth's rounding
    pts[..., 2][half] = np.floor(rng.uniform(-3.0, 66000.0, int(half.sum()))).astype(F) + F(0.5)
    c.points = pts


def depth_stack_case():
    """found by the draw, ('convert', seed 1, index 29): three depth frames of 3 x 3 have the shape [3, 3, 3] of one 3 x 3 cloud,
    and filters.DimensionConvertor.projectiveToReal took them for the cloud.  Depth 1000 + 10 * (pixel index), a camera with
    f = 5 and the principal point (1.5, 1.5), truncated to (1, 1): pixel (0, 0) of frame 0 is (-200, 200, 1000)"""
    c = SimpleNamespace(kind="convert", seed=0, index=-1, n=3, size=(3, 3), want=None, off=dict(depth=0, points=0, out=0, zf=0, zu=0))
    c.K = np.array([[5.0, 0.0, 1.5], [0.0, 5.0, 1.5], [0.0, 0.0, 1.0]])
    c.depth = (1000.0 + 10.0 * np.arange(27)).astype(F).reshape(3, 3, 3)
    c.points = np.stack([c.depth * F(0.5), c.depth * F(-0.25), c.depth], -1).astype(F)
    return c


def convert_streaming_sites(c):
    """the launch sites of csrc/stream_kernels.hip whose streaming form a `convert` case reaches once the cache threshold is 0
    (tools/hooks/stage.py: set_cache_bytes), as _run_convert places its tensors: the streaming forms are vector forms.
    launch_p2r_any wants depth and out on 16-byte boundaries and, with more than one frame, W * H % 4 == 0; launch_points_any
    wants its two clouds there (r2p_chain goes from `out` to `out`); points_to_depth wants the cloud and its map there and
    at least one group of 8 points"""
    (W, H), o = c.size, c.off
    sites = set()
    if o["depth"] == 0 and o["out"] == 0 and (c.n == 1 or W * H % 4 == 0):
        sites.add("p2r_depth")
    if o["out"] == 0:
        sites.add("points_map")
    for key, site in (("zf", "points_to_depth_f32"), ("zu", "points_to_depth_u16")):
        if o["points"] == 0 and o[key] == 0 and c.n * W * H >= 8:
            sites.add(site)
    return sites


def _f3(p):
    return np.ascontiguousarray(p).view(F).reshape(p.shape + (3,))


def _want_convert(c):
    O = oracle()
    fr = range(c.n)
    w = c.want = {}
    w["p2r_depth"] = np.stack([_f3(O.p2r_depth(c.depth[f], c.K)) for f in fr])
    w["r2p_chain"] = np.stack([_f3(O.r2p(w["p2r_depth"][f], c.K)) for f in fr])
    w["p2r_chain"] = np.stack([_f3(O.p2r_points(w["r2p_chain"][f], c.K)) for f in fr])
    w["interp"] = np.stack([_f3(O.p2r_interp(c.depth[f], c.K)) for f in fr])
    w["r2p"] = np.stack([_f3(O.r2p(c.points[f], c.K)) for f in fr])
    w["p2r_points"] = np.stack([_f3(O.p2r_points(c.points[f], c.K)) for f in fr])
    w["z_f32"] = c.points[..., 2].copy()
    w["z_u16"] = DU.to_u16(c.points[..., 2])


# ---- cloud, error3d -------------------------------------------------------------------------------------------------------
def _range(rng):
    if rng.random() < 0.4:
        return 50.0, 15000.0
    lo = float(rng.choice([0.0, 0.5, 100.25, -10.0, 400.0]))
    return lo, float(rng.choice([2000.0, 15000.0, 60000.5, 1.0e9]))


def _frame_shares(rng, n):
    """the valid share of every frame: whole empty and whole full frames among them"""
    u = rng.random(n)
    return np.where(u < 0.07, 0.0, np.where(u < 0.14, 1.0, rng.uniform(0.02, 0.98, n)))


def _depth_values(rng, shape, shares, lo, hi, integer):
    """z [n, ...]: a share of every frame inside (lo, hi), their two inner neighbours among them, the others out of the
    invalid values: 0, both ends and their outer neighbours, negative, NaN, +-inf, -0"""
    lo32, hi32 = F(lo), F(hi)
    n = shape[0]
    span = min(float(hi32) - float(lo32), 8000.0)
    z = (float(lo32) + span * rng.uniform(0.01, 0.99, shape)).astype(F)
    edge = rng.random(shape) < 0.02
    z[edge] = rng.choice(np.array([np.nextafter(lo32, INF), np.nextafter(hi32, -INF)], F), int(edge.sum()))
    bad = np.array([0.0, lo32, hi32, np.nextafter(lo32, -INF), np.nextafter(hi32, INF), -1000.0, np.nan, np.inf, -np.inf, -0.0,
                    float(lo32) - 1.0, float(hi32) + 1.0], F)
    if integer:                                               # what a uint16 holds
        z = np.clip(np.rint(z), 0, 65535).astype(F)
        bad = np.unique(np.clip(np.array([0.0, np.floor(lo32), np.ceil(hi32), np.ceil(hi32) + 1.0, 65535.0 if hi32 < 65535 else 0.0]), 0, 65535)).astype(F)
        with np.errstate(invalid="ignore"):
            bad = bad[~((bad > lo32) & (bad < hi32))]
        if bad.size == 0:                                     # a range that holds every uint16
            return z
    valid = rng.random(shape) < np.asarray(shares).reshape((n,) + (1,) * (len(shape) - 1))
    return np.where(valid, z, bad[rng.integers(0, bad.size, shape)]).astype(F)


def _source(rng, c, shares, fmt, hostile_xy):
    """one source of n frames in a format -> SimpleNamespace(fmt, data as the device gets it, points [n, H, W, 3] it stands for, off)"""
    (W, H), n = c.size, c.n
    z = _depth_values(rng, (n, H, W), shares, c.z_min, c.z_max, fmt == "u16")
    if fmt == "points":
        pts = np.stack([rng.uniform(-4000.0, 4000.0, (n, H, W)).astype(F), rng.uniform(-3000.0, 3000.0, (n, H, W)).astype(F), z], -1)
        if hostile_xy:
            hit = rng.random((n, H, W)) < 0.01
            pts[..., 0][hit] = rng.choice(np.array([np.nan, np.inf, -0.0, -np.inf], F), int(hit.sum()))
            pts[..., 1][rng.random((n, H, W)) < 0.01] = F(-0.0)
        data = pts
    else:
        pts = np.stack([CC.project(z[f], c.K) for f in range(n)])
        data = z if fmt == "depth" else z.astype(np.uint16).view(np.int16)
    return SimpleNamespace(fmt=fmt, data=np.ascontiguousarray(data), points=np.ascontiguousarray(pts, F), off=int(rng.integers(0, 4)) if rng.random() < 0.5 else 0)


def _draw_frames(rng, c, slot):
    c.size = _size(rng, slot)
    c.n = int(rng.integers(1, 5))
    c.max_batch = c.n + int(rng.integers(1, 3))
    c.K = _camera(rng, *c.size)
    c.z_min, c.z_max = _range(rng)
    c.shares = _frame_shares(rng, c.n)


def _draw_cloud(rng, c):
    _draw_frames(rng, c, c.index - 1)
    if c.index == 0:                                          # more segments than one pass of the scan takes
        c.size, c.n, c.max_batch = MULTI_PASS, 1, 2
        c.shares = np.array([float(rng.uniform(0.3, 0.7))])
    W, H = c.size
    c.divisor = float(rng.choice([1000.0, 1.0, 3.0, 0.1, 1024.0]))
    c.negate_z, c.organized = bool(rng.random() < 0.5), bool(rng.random() < 0.35)
    c.src = _source(rng, c, c.shares, FORMATS[(c.index + c.seed) % 3], True)
    c.bgr_frames = c.n if rng.random() < 0.6 else 1
    c.bgr = rng.integers(0, 256, (c.bgr_frames, H, W, 3), dtype=np.uint8)
    c.bgr_off = int(rng.integers(0, 8)) if rng.random() < 0.5 else 0
    c.own_buffer = bool(rng.random() < 0.3)                   # the object-owned records, not the caller's
    c.valid_share = float(np.mean([CC.valid_mask(c.src.points[f], c.z_min, c.z_max).mean() for f in range(c.n)]))


def _want_cloud(c):
    c.want = [CC.statement(c.src.points[f], c.bgr[f if c.bgr_frames > 1 else 0], c.z_min, c.z_max, c.divisor, c.negate_z, c.organized)
              for f in range(c.n)]
    c.counts = [CC.count(c.src.points[f], c.z_min, c.z_max) for f in range(c.n)]


def _draw_error3d(rng, c):
    _draw_frames(rng, c, c.index)
    (W, H), n = c.size, c.n
    c.m = 1 + (c.index + c.seed) % 8
    c.max_candidates = int(rng.integers(c.m, 9))
    c.set_range = not (c.z_min == 50.0 and c.z_max == 15000.0) or bool(rng.random() < 0.5)
    c.truth_frames = n if rng.random() < 0.6 else 1
    shares = c.shares if c.truth_frames == n else c.shares[:1]
    keep, c.n = c.n, c.truth_frames
    c.truth = _source(rng, c, shares, str(rng.choice(FORMATS)), False)
    c.n = keep
    c.cands = []
    for j in range(c.m):                                      # the truth's surface, a few millimetres off, with its own invalid pixels
        fmt = str(rng.choice(FORMATS))
        t = c.truth.points[np.arange(n) % c.truth_frames]
        s = _source(rng, c, np.full(n, 0.93), fmt, False)
        own = CC.valid_mask(s.points, c.z_min, c.z_max) & CC.valid_mask(t, c.z_min, c.z_max)
        if fmt == "points":
            noisy = (t.astype(np.float64) + rng.normal(0.0, 3.0 + j, t.shape)).astype(F)
            s.points = np.where(own[..., None], noisy, s.points).astype(F)
            s.data = s.points
        else:
            z = (t[..., 2].astype(np.float64) + rng.normal(0.0, 3.0 + j, own.shape)).astype(F)
            z = np.where(own, np.clip(np.rint(z), 0, 65535).astype(F) if fmt == "u16" else z, s.points[..., 2])
            s.points = np.stack([CC.project(z[f], c.K) for f in range(n)]).astype(F)
            s.data = np.ascontiguousarray(z if fmt == "depth" else z.astype(np.uint16).view(np.int16))
        c.cands.append(s)
    t = c.truth.points[np.arange(n) % c.truth_frames]
    c.valid_share = float(EC.valid_mask(c.cands[0].points, t, c.z_min, c.z_max).mean())


def _want_error3d(c):
    c.want = [[EC.statement(s.points[f], c.truth.points[f % c.truth_frames], c.z_min, c.z_max) for s in c.cands] for f in range(c.n)]


# ---- tail: plane fit, projection and sweeps through kde_stage_spdsr_tail ---------------------------------------------------
TAIL_WIDTHS = (4, 5, 7, 63, 64, 65, 127, 128, 129)        # SetParametor admits no width below 4 (a window is >= 4 pixels)
TAIL_SWEEPS = (0, 1, 2, 3, 19, 20)
TAIL_INVALID = np.array([0.0, 30.0, 50.0, np.nextafter(F(50), F(100)), -500.0], F)
MIN_GAP = 1e-6
# the largest relative error of the float32 restatement (okde_projection_plane) against sweeps64 over the budget's calls of a
# sweep count; tests/test_output_sweep.py proves the table on the CPU, the bar on the device is 8 x the entry (check_sweeps)
TAIL_E32 = {0: 0.0, 1: 1.235e-06, 2: 1.885e-06, 3: 1.353e-06, 19: 4.190e-06, 20: 3.919e-06}


def _tail_geometry(rng, c):
    j = c.index - len(PIPE_PINNED)
    if j < 0:                                                 # the last table on LDS (1024) and the first in global memory (1056)
        W, H, c.rows, c.cols = PIPE_PINNED[c.index]
        c.size, c.n = (W, H), 1 + (c.seed + c.index) % 2
        return
    c.n = int(rng.integers(1, 5))
    while True:
        W = TAIL_WIDTHS[j] if j < len(TAIL_WIDTHS) else (2 * int(rng.integers(2, 132)) + 1 if j % 2 else int(rng.integers(4, MAX_W + 1)))
        H = 8 * int(rng.integers(1, MAX_H // 8 + 1)) if (j + c.seed) % 2 else int(rng.integers(6, MAX_H + 1))
        if j == len(TAIL_WIDTHS):                             # exactly 8 tiles of 64 x 8
            W, H, c.n = 64, 64, 1
        c.cols, c.rows = int(rng.integers(1, W // 4 + 1)), int(rng.integers(1, H // 4 + 1))
        if rng.random() < 0.12:
            c.rows = c.cols = 1
        if admitted(W, H, c.rows, c.cols) and ((j + c.seed) % 2 or H % 8 or j == len(TAIL_WIDTHS)):
            c.size = (W, H)
            return


def _tail_labels(rng, W, H, rows, cols, style):
    k = rows * cols
    perm = rng.permutation(k).astype(np.int32)
    y, x = np.mgrid[0:H, 0:W]
    if style in ("grid", "speckle"):
        lab = SC.block_labels(W, H, rows, cols, perm)
    elif style == "blobs":
        bw, bh = int(rng.integers(3, max(W // 3, 4) + 1)), int(rng.integers(3, max(H // 3, 4) + 1))
        lab = rng.integers(0, k, (-(-H // bh), -(-W // bw)))[y // bh, x // bw].astype(np.int32)
    else:                                                     # stripes two to five pixels wide (one pixel wide: collinear points)
        lab = perm[((x if rng.random() < 0.6 else y) // int(rng.integers(2, 6))) % k]
    lab = np.ascontiguousarray(lab, np.int32)
    if style == "speckle":
        hit = rng.random((H, W)) < 0.04
        lab[hit] = rng.integers(0, k, int(hit.sum()))
    if style == "grid" and k > 1 and H > 2:                   # two rows where the label changes at every pixel
        r = int(rng.integers(0, H - 1))
        lab[r, 0::2], lab[r, 1::2] = perm[0], perm[k - 1]
        lab[r + 1, 0::2], lab[r + 1, 1::2] = perm[k - 1], perm[0]
    return lab


def _tail_reference(c, call, f):
    """the binary64 reference of one frame: (planes64 or None, planes, plane-fitted z, projected, |den|, sweeps64)"""
    lab, pts = call.labels[f], call.points[f]
    ref = SC.planes64(lab, pts, c.k, nd_prev=None) if call.nd is None else None
    nd = ref["nd"] if ref is not None else call.nd[f]
    z, proj, den = SC.plane_fitted64(nd, lab, pts, c.tx, c.ty)
    with np.errstate(all="ignore"):
        pfz = z.astype(F)
    return ref, nd, pfz, proj, den, SC.sweeps64(pfz, pts[..., 2], call.sweeps)


def _tail_frame(rng, c, call, f):
    """one frame of a call, proposed until no decision of the binary64 reference is closer than 2 x MARGIN to its threshold"""
    (W, H), k = c.size, c.k
    # (a frame narrower than 8 pixels takes the compact styles: a blob that loses its outliers there is a column of points,
    #  and the plane fitted to it is far from the drawn one)
    style = str(rng.choice(ERS_STYLES if W >= 8 else ("grid", "stripes")))
    lab = _tail_labels(rng, W, H, c.rows, c.cols, style)
    fit = call.nd is None
    noise = 0.001 if fit else 0.003                           # inside the 1 % centre test; a fit of 16 points wants the smaller
    z, nd = SC._plane_points(rng, lab, k, c.tx, c.ty, noise, (800.0, 3000.0), c.tilt)
    out = rng.random((H, W)) < 0.06                           # outliers outside the 1 % centre test
    z[out] *= 1.0 + rng.choice([-1.0, 1.0], int(out.sum())) * rng.uniform(0.03, 0.05, int(out.sum()))
    # around the centre test: 0.8 .. 1.3 % off the plane, on either side (handed-in planes only: one such point turns a fitted 4 x 4 plane)
    if not fit:
        near = ~out & (rng.random((H, W)) < 0.04)
        z[near] *= 1.0 + rng.choice([-1.0, 1.0], int(near.sum())) * rng.uniform(0.008, 0.013, int(near.sum()))
    clean = z.copy()
    inv = rng.random((H, W)) < 0.05
    z[inv] = rng.choice(TAIL_INVALID, int(inv.sum()))
    # where the planes are fitted, outliers and invalid samples leave their clusters (1 % of a 4 x 4 cluster's points at z = 0
    # turn its plane); they stay taps and centres of the sweeps.  Handed-in planes keep the outliers and a fifth of the others
    lab[(inv | out) if fit else (inv & (rng.random((H, W)) < 0.8))] = -1
    r = rng.random((H, W))
    lab[r < 0.02] = k + int(rng.integers(0, 6))               # labels outside the table
    lab[(r > 0.02) & (r < 0.03)] = -1
    lab[(r > 0.03) & (r < 0.035)] = -7
    starved = {}
    for l in rng.permutation(k)[:int(rng.integers(0, min(k, 5) + 1))]:     # clusters of 0 .. 3 points
        idx = np.flatnonzero(lab.reshape(-1) == l)
        keep = int(rng.integers(0, 4))
        lab.reshape(-1)[rng.permutation(idx)[keep:]] = -1
        starved[int(l)] = min(keep, idx.size)
    item = None
    if rng.random() < 0.3:                                    # one non-finite item (spdsr_tail_cases.sweep_micro)
        # pf_inf needs a plane of its own.  huge is dealt where the planes are handed in: a fitted plane goes through a point
        # at 3e38, the pixel passes the centre test and its float32 numerator, 1.5 x 3e38, overflows where sweeps64 does not
        item = str(rng.choice([i for i in SC.MICRO_ITEMS if (i != "pf_inf" or k > 1) and (i not in ("pf_inf", "huge") or not fit)]))
    if not fit and f == 0:                                    # the first frame of handed-in planes: every item in turn
        item = SC.MICRO_ITEMS[(c.index // 2) % len(SC.MICRO_ITEMS)]
        item = item if item != "pf_inf" or k > 1 else "huge"
    call.styles.append(style)
    call.items.append(item)
    call.starved.append(starved)
    call.labels[f] = lab
    if call.nd is not None:
        call.nd[f] = nd
    at = (int(rng.integers(0, H)), int(rng.integers(0, W)))
    if item == "pf_inf":                                      # the pixel's cluster gets the plane whose denominator is 0
        l = int(lab[at]) if 0 <= lab[at] < k else 0
        call.nd[f][l] = (0.0, 0.0, 0.0, 1000.0)
        call.pf_inf.append((f, l))
    if item == "huge" and not 0 <= call.labels[f][at] < k:    # on a plane: an unlabelled pixel is its own plane-fitted point, passes
        call.labels[f][at] = 0                                # the centre test, and its float32 numerator 1.5 x 3e38 overflows
    for trial in range(200):
        pts = SC._points_from_z(z, c.tx, c.ty, SC.OFF_RAY)
        if item not in (None, "pf_inf"):
            pts[at] = (0.0, 0.0, dict(plus_inf=np.inf, minus_inf=-np.inf, nan=np.nan, huge=3.0e38, negative=-1000.0)[item])
        call.points[f] = pts
        close = _tail_reference(c, call, f)[5]["margin"] < 2.0 * SC.MARGIN
        if not close.any():
            return
        c.rejected += 1                                       # the next proposal: fresh noise on the pixels on a decision
        m = int(close.sum())
        z[close] = clean[close] * (1.0 + rng.uniform(-noise, noise, m))       # (an outlier or a pixel near the test keeps its offset)
    raise AssertionError("no proposal without a decision inside 2 x MARGIN")


def _tail_call(rng, c, n, fit, sweeps):
    (W, H), k = c.size, c.k
    call = SimpleNamespace(n=n, sweeps=sweeps, labels=np.zeros((n, H, W), np.int32), points=np.zeros((n, H, W, 3), F),
                           nd=None if fit else np.zeros((n, k, 4), F), styles=[], items=[], starved=[], pf_inf=[], want=None)
    for f in range(n):
        _tail_frame(rng, c, call, f)
    return call


def _draw_tail(rng, c):
    _tail_geometry(rng, c)
    (W, H), c.k = c.size, c.rows * c.cols
    c.max_batch = int(rng.integers(c.n, 5))
    c.tiles = -(-W // 64) * -(-H // 8) * c.n
    f = float(F(rng.uniform(0.9, 2.0) * max(W, H)))           # 0.9 W alone puts the denominator of a narrow tall frame near 0
    c.K = np.array([[f, 0, W // 2], [0, f, H // 2], [0, 0, 1]], np.float64)
    c.tx, c.ty = SC.rays(W, H, c.K)
    c.tilt = float(rng.uniform(0.05, 0.5))
    c.rejected = 0
    c.fit = bool((c.index + c.seed) % 2)
    sweeps = TAIL_SWEEPS[(c.index // 2 + c.seed) % len(TAIL_SWEEPS)]
    c.calls = [_tail_call(rng, c, c.n, c.fit, sweeps)]
    if rng.random() < 0.5:                                    # the used handle: the planes are fitted, the markers keep the w of call 0
        c.calls.append(_tail_call(rng, c, int(rng.integers(1, c.max_batch + 1)), True, int(rng.choice(TAIL_SWEEPS))))


def _want_tail(c):
    """per call and frame what needs no device: the reference's pieces, the clusters below the eigen-gap, the numbers of projected
    pixels and of those with |den| < 0.5 outside the pf_inf planes, the rewritten share, and e32 of the float32 restatement"""
    O = oracle()
    for call in c.calls:
        call.want = []
        for f in range(call.n):
            ref, nd, pfz, proj, den, sw = _tail_reference(c, call, f)
            skip = [] if ref is None else [int(l) for l in np.flatnonzero(ref["gap"] < MIN_GAP)]
            dealt = np.isin(call.labels[f], [l for g, l in call.pf_inf if g == f])      # the planes whose denominator is dealt as 0
            with np.errstate(invalid="ignore"):
                low = proj & ~dealt & ~(den >= 0.5)
            pf32, opt32 = (_f3(a) for a in O.projection_plane(nd, call.labels[f], call.points[f], c.K, call.sweeps))
            ref32 = SC.sweeps64(pf32[..., 2], call.points[f][..., 2], call.sweeps)
            e32 = SC.sweep_compare(opt32, ref32, call.points[f], c.tx, c.ty, "the float32 restatement")
            call.want.append(dict(skip=skip, low_den=int(low.sum()), projected=int(proj.sum()), rewritten=float(sw["rewritten"].mean()),
                                  min_margin=float(sw["margin"].min()), e32=e32, gap=None if ref is None else ref["gap"]))
    c.want = True


# ---- process: the tail as Process runs it --------------------------------------------------------------------------------
def _draw_process(rng, c):
    """the `spdsr` case of superpixel_sweep of the same seed and index (its own generator; that sweep holds the head)"""
    s = SS.draw("spdsr", c.seed, c.index)
    c.size, c.rows, c.cols, c.n, c.max_batch, c.grid, c.calls = s.size, s.rows, s.cols, s.n, s.max_batch, s.grid, s.calls
    c.k, c.K = c.rows * c.cols, camera_matrix(*c.size)
    c.tx, c.ty = SC.rays(*c.size, c.K)


def process_reference(c, lab, pts, prev):
    """one frame of the tail's input (refined labels, back-projected points) -> (planes64, the clusters below the eigen-gap,
    projected pixels, those of them with |den| < 0.5 on the reference's planes)"""
    ref = SC.planes64(lab, pts, c.k, nd_prev=prev)
    skip = [int(l) for l in np.flatnonzero(ref["gap"] < MIN_GAP)]
    z, proj, den = SC.plane_fitted64(ref["nd"], lab, pts, c.tx, c.ty)
    with np.errstate(invalid="ignore"):
        low = proj & ~np.isin(lab, skip) & ~(den >= 0.5)
    return ref, skip, int(proj.sum()), int(low.sum())


def _want_process(c):
    """per call and frame, on the ORACLE's head (the device's labels are held to it by superpixel_sweep): the numbers the conditions
    of tests/test_output_sweep.py are about.  run_case takes its references from the device's own labels and points"""
    O = oracle()
    for call in c.calls:
        call.tail = []
        for f in range(call.n):
            i = call.inputs
            rl, rd, rp = O.spdsr_head(i["depth"][f], i["points"][f], i["bgr"][f], c.rows, c.cols, c.K)
            ref, skip, projected, low = process_reference(c, rl, _f3(rp) if rp.dtype.names else np.asarray(rp, F).reshape(rl.shape + (3,)), None)
            fitted = int((~np.isnan(ref["gap"])).sum())
            call.tail.append(dict(skip=skip, fitted=fitted, markers=int((ref["nd"][:, 0] == 5).sum()), projected=projected, low_den=low,
                                  pixels=rl.size, finite=bool(np.isfinite(ref["nd"]).all())))
    c.want = True


_DRAW = dict(tail=_draw_tail, process=_draw_process, buffer2d=_draw_buffer2d, convert=_draw_convert, cloud=_draw_cloud, error3d=_draw_error3d)
_WANT = dict(tail=_want_tail, process=_want_process, buffer2d=_want_buffer2d, convert=_want_convert, cloud=_want_cloud, error3d=_want_error3d)


def draw(kind, seed, index):
    """the case without `want`"""
    rng = np.random.default_rng([seed, ALL_KINDS.index(kind), index])
    c = SimpleNamespace(kind=kind, seed=seed, index=index, want=None)
    _DRAW[kind](rng, c)
    return c


def want(c):
    """fills want from the oracle or the statement"""
    if c.want is None:
        _WANT[c.kind](c)
    return c


def case(kind, seed, index):
    return want(draw(kind, seed, index))


def describe(c):
    """what regenerates and explains a case"""
    keys = ("size", "cls", "n", "max_batch", "m", "max_candidates", "truth_frames", "z_min", "z_max", "divisor", "negate_z", "organized",
            "bgr_frames", "bgr_off", "own_buffer", "off", "valid_share")
    d = {k: getattr(c, k) for k in keys if hasattr(c, k)}
    if hasattr(c, "ops"):
        d["ops"] = [(o.op, o.off, o.get_off) + ((len(o.data),) if o.op == "update_seq" else ()) for o in c.ops]
    if hasattr(c, "src"):
        d["source"] = (c.src.fmt, c.src.off)
    if hasattr(c, "cands"):
        d["sources"] = [(s.fmt, s.off) for s in c.cands] + [("truth", c.truth.fmt, c.truth.off)]
    if hasattr(c, "K"):
        d["K"] = [round(float(v), 3) for v in (c.K[0, 0], c.K[1, 1], c.K[0, 2], c.K[1, 2])]
    return f"({c.kind!r}, seed {c.seed}, index {c.index}) {d}"


# ---- the device side: torch and kinectdepthmapenhancement_amd.filters are handed in -----------------------------------------
def _host(t):
    return t.detach().cpu().numpy()


def _space(torch, shape, dtype, off, fill=0):
    """a contiguous device tensor of the shape that starts `off` elements past a 16-byte boundary"""
    size = int(np.prod(shape))
    flat = torch.full((size + 16,), fill, dtype=dtype, device="cuda")
    assert flat.data_ptr() % 16 == 0
    return flat[off:off + size].view(tuple(shape))


def _dev_at(torch, a, off=0):
    """the array on the device, `off` elements past a 16-byte boundary"""
    src = torch.from_numpy(np.ascontiguousarray(a))
    view = _space(torch, src.shape, src.dtype, off)
    view.copy_(src)
    return view


def _floats(bad, tag, got, exp):
    k = same_floats(got, exp)
    if k:
        g, e = np.ascontiguousarray(got, F).reshape(-1), np.ascontiguousarray(exp, F).reshape(-1)
        with np.errstate(invalid="ignore"):
            at = int(np.flatnonzero((np.isnan(g) != np.isnan(e)) | (~np.isnan(g) & ~np.isnan(e) & (g.view(np.uint32) != e.view(np.uint32))))[0])
        bad.append(f"{tag}: {k} of {g.size} floats differ, the first at {at}: {g[at]!r} ({g.view(np.uint32)[at]:#010x}), the oracle "
                   f"{e[at]!r} ({e.view(np.uint32)[at]:#010x})")


def _run_buffer2d(torch, F_, c, bad, got):
    W, H = c.size
    gb = F_.Buffer2D(W, H)
    try:
        for j, (o, w) in enumerate(zip(c.ops, c.want)):
            tag = f"op {j} {o.op}"
            if o.op in ("update", "update_seq"):
                gb.updateData(_dev_at(torch, o.data, o.off))
            elif o.op in ("insert_depth", "insert_float2"):
                gb.insertData(_dev_at(torch, o.data, o.off))
            elif o.op == "insert_weighted":
                gb.insertWeighted(_dev_at(torch, o.data, o.off))
            dm = gb.getDepthMap(_space(torch, (H, W), torch.float32, o.get_off[0], -7.0))
            wm = gb.getWeightMap(_space(torch, (H, W), torch.float32, o.get_off[1], -7.0))
            g = got[tag] = dict(raw=_host(gb.getRawPointer()).copy(), depth=_host(dm).copy(), weight=_host(wm).copy())
            for name, exp in zip(("raw", "depth", "weight"), w):
                _floats(bad, f"{tag}, {name}", g[name], exp)
            if bad:                                           # everything after the first difference follows from it
                break
    finally:
        gb.close()


def _run_convert(torch, F_, c, bad, got):
    (W, H), n, w = c.size, c.n, c.want
    conv = F_.DimensionConvertor()
    try:
        conv.setCameraParameters(c.K, W, H)
        out = lambda: _space(torch, (n, H, W, 3), torch.float32, c.off["out"], -7.0)
        depth, points = _dev_at(torch, c.depth, c.off["depth"]), _dev_at(torch, c.points, c.off["points"])
        got["p2r_depth"] = conv.projectiveToReal(depth, out())
        got["r2p_chain"] = conv.realToProjective(got["p2r_depth"], out())          # chained on the device's own output
        got["p2r_chain"] = conv.projectiveToReal(got["r2p_chain"], out())
        got["interp"] = conv.projectiveToRealInterp(depth, out())
        got["r2p"] = conv.realToProjective(points, out())
        got["p2r_points"] = conv.projectiveToReal(points, out())
        got["z_f32"] = F_.points_to_depth(points, _space(torch, (n, H, W), torch.float32, c.off["zf"], -7.0))
        got["z_u16"] = F_.points_to_depth(points, _space(torch, (n, H, W), torch.int16, c.off["zu"], -7), dtype=torch.int16)
        for k in list(got):
            got[k] = _host(got[k]).copy()
        for k in ("p2r_depth", "r2p_chain", "p2r_chain", "interp", "r2p", "p2r_points", "z_f32"):
            _floats(bad, k, got[k], w[k])
        k = int((got["z_u16"].view(np.uint16) != w["z_u16"]).sum())
        if k:
            bad.append(f"z_u16: {k} of {w['z_u16'].size} samples differ")
    finally:
        conv.close()


_TORCH_OF = dict(points="float32", depth="float32", u16="int16")
SENTINEL = 0xA5


def _run_cloud(torch, F_, c, bad, got):
    (W, H), n = c.size, c.n
    px = W * H
    C = F_.PointCloudXYZRGB(W, H, max_batch=c.max_batch, z_min=c.z_min, z_max=c.z_max, divisor=c.divisor, negate_z=c.negate_z,
                            organized=c.organized)
    try:
        C.set_camera(c.K)
        src, bgr = _dev_at(torch, c.src.data, c.src.off), _dev_at(torch, c.bgr, c.bgr_off)
        if c.own_buffer:
            C.build(src, bgr)                                 # once to learn the buffer, which is then filled with the sentinel
            out = F_._view(C.points_device().data_ptr(), (c.max_batch, px, 16), torch.uint8, C)
            out.fill_(SENTINEL)
            C.build(src, bgr)
        else:
            out = torch.full((c.max_batch, px, 16), SENTINEL, dtype=torch.uint8, device="cuda")
            C.build(src, bgr, out[:n])
        counts = C.counts()
        raw = got["records"] = _host(out).copy()
        got["counts"] = counts
        host = C.points_host()
        if counts.tolist() != c.counts:
            bad.append(f"counts {counts.tolist()}, the statement {c.counts}")
        if np.array_equal(counts, c.counts) and C.offsets.tolist() != np.concatenate([[0], np.cumsum([r.size for r in c.want])]).tolist():
            bad.append(f"offsets {C.offsets.tolist()}")
        for f, rec in enumerate(c.want):
            if raw[f, :rec.size].tobytes() != rec.tobytes():
                g = raw[f, :rec.size].reshape(-1, 16)
                at = int(np.flatnonzero((g != rec.view(np.uint8).reshape(-1, 16)).any(1))[0])
                bad.append(f"frame {f}: {int((g != rec.view(np.uint8).reshape(-1, 16)).any(1).sum())} of {rec.size} records differ, the first "
                           f"at {at}: {g[at].view(CC.POINT)[0]}, the statement {rec[at]}")
            elif host[f].tobytes() != rec.tobytes():
                bad.append(f"frame {f}: points_host differs from the device's records")
            if not np.all(raw[f, rec.size:] == SENTINEL):
                bad.append(f"frame {f}: records behind count[f] were written")
        if not np.all(raw[n:] == SENTINEL):
            bad.append("a frame slot behind the batch was written")
    finally:
        C.close()


def _run_error3d(torch, F_, c, bad, got):
    (W, H), n = c.size, c.n
    E = F_.MeanError3D(W, H, max_batch=c.max_batch, max_candidates=c.max_candidates)
    try:
        E.set_camera(c.K)
        if c.set_range:
            E.set_range(c.z_min, c.z_max)
        E.compare([_dev_at(torch, s.data, s.off) for s in c.cands], _dev_at(torch, c.truth.data, c.truth.off))
        table = got["table"] = E.results_host()
        if table.shape != (n, c.m):
            bad.append(f"the table has shape {table.shape}")
            return
        for f in range(n):
            for j in range(c.m):
                g, st, tag = table[f, j], c.want[f][j], f"frame {f} candidate {j}"
                if int(g["count"]) != st["count"]:
                    bad.append(f"{tag}: count {int(g['count'])}, the statement {st['count']}")
                elif st["count"] == 0:
                    if not (g["sum"] == 0.0 and np.isnan(g["mean"])):
                        bad.append(f"{tag}: no valid pixel, sum {g['sum']}, mean {g['mean']}")
                else:
                    if not abs(float(g["sum"]) - st["sum"]) <= st["count"] * 2.0 ** -53 * st["sum"]:
                        bad.append(f"{tag}: sum {float(g['sum'])!r}, the exact sum {st['sum']!r}")
                    m = F(np.float64(g["sum"]) / np.float64(g["count"]))
                    if F(g["mean"]).view(np.uint32) != m.view(np.uint32):
                        bad.append(f"{tag}: mean {float(g['mean'])!r} is not the float conversion of sum / count {float(m)!r}")
    finally:
        E.close()


def _asserted(bad, where, fn, *a, **kw):
    """runs a bar written as assertions; a failure becomes a violation"""
    try:
        return fn(*a, **kw)
    except AssertionError as e:
        bad.append(f"{where}: {e}")
        return None


def _projection_bars(c, lab, pts, nd, pf, skip, bad, tag):
    """check_fit's bars on plane_fitted from the side's own planes: unprojected pixels are the input point to the bit, z within 8
    float32 ulps of the binary64 projection where |den| >= 0.5 (the clusters of `skip` apart), x, y = ray * z to the bit
    -> the largest deviation of z in ulps"""
    bits = lambda a: np.ascontiguousarray(a, F).view(np.uint32)
    z, proj, den = SC.plane_fitted64(nd, lab, pts, c.tx, c.ty)
    with np.errstate(all="ignore"):
        if not np.array_equal(bits(pf[~proj]), bits(pts[~proj])):
            bad.append(f"{tag}: an unprojected pixel of plane_fitted is not the input point")
        ok = proj & ~np.isin(lab, skip) & (den >= 0.5)
        du = float(SC.ulps32(pf[..., 2][ok], z[ok]).max()) if ok.any() else 0.0
        if not du <= 8.0:
            bad.append(f"{tag}: plane_fitted z is {du:.1f} ulps from the binary64 projection")
        if not (np.array_equal(pf[..., 0][proj], (c.tx * pf[..., 2])[proj], equal_nan=True)
                and np.array_equal(pf[..., 1][proj], (c.ty * pf[..., 2])[proj], equal_nan=True)):
            bad.append(f"{tag}: plane_fitted x, y are not ray * z")
    return du


def _tail_frame_check(c, call, f, w, nd, pf, opt, prev, bad, tag):
    """one frame of one call under the bars of tests/test_gpu_spdsr_tail.py (check_fit, check_sweeps)"""
    O = oracle()
    lab, pts, bits = call.labels[f], call.points[f], lambda a: np.ascontiguousarray(a, F).view(np.uint32)
    if call.nd is None:
        ref = SC.planes64(lab, pts, c.k, nd_prev=prev)
        _asserted(bad, tag, SC.planes_compare, nd, ref, "planes", w["skip"])
    elif not np.array_equal(bits(nd), bits(call.nd[f])):
        bad.append(f"{tag}: the planes handed in came back changed")
    pf32, opt32 = (_f3(a) for a in O.projection_plane(nd, lab, pts, c.K, call.sweeps))
    du = _projection_bars(c, lab, pts, nd, pf, w["skip"], bad, tag)
    with np.errstate(all="ignore"):
        held = ~np.isin(lab, w["skip"])                       # the classes of okde_projection_plane, for every denominator
        if not (np.array_equal(np.isfinite(pf)[held], np.isfinite(pf32)[held]) and np.array_equal(np.isnan(pf)[held], np.isnan(pf32)[held])):
            bad.append(f"{tag}: NaN / inf classes of plane_fitted differ from okde_projection_plane's")
    ref = SC.sweeps64(pf[..., 2], pts[..., 2], call.sweeps)   # from the device's own plane-fitted z: the sweeps alone
    err = _asserted(bad, tag, SC.sweep_compare, opt, ref, pts, c.tx, c.ty, "sweeps")
    if not (np.array_equal(np.isnan(opt), np.isnan(opt32)) and np.array_equal(np.isinf(opt), np.isinf(opt32))):
        bad.append(f"{tag}: NaN / inf masks of the optimized cloud differ from okde_projection_plane's")
    flagged = int(ref["flagged"].sum())
    if flagged > (SC.MAX_FLAGGED * ref["flagged"].size if call.sweeps > 1 else 0):
        bad.append(f"{tag}: {flagged} of {ref['flagged'].size} pixels within MARGIN of a decision")
    if err is not None and not err <= 8.0 * TAIL_E32[call.sweeps]:
        bad.append(f"{tag}: optimized z is {err:.3e} from sweeps64 (> 8 x e32 = {8 * TAIL_E32[call.sweeps]:.3e})")
    if call.sweeps == 0 and not np.array_equal(bits(opt), bits(pts)):
        bad.append(f"{tag}: no sweep, and the optimized cloud is not the input")
    return dict(err=err, flagged=flagged, pf_ulps=du)


def _run_tail(torch, F_, c, bad, got):
    from tools.hooks import stage
    (W, H), k = c.size, c.k
    outs = stage.spdsr_tail_calls(W, H, c.rows, c.cols, c.K, [dict(labels=call.labels, points=call.points, nd=call.nd, sweeps=call.sweeps)
                                                              for call in c.calls], c.max_batch)
    prev = np.zeros((c.max_batch, k, 4), F)                   # what the frame slots hold: zeros after SetParametor
    for j, (call, (nd, pf, opt)) in enumerate(zip(c.calls, outs)):
        got[f"call {j}"] = dict(nd=nd, plane_fitted=pf, optimized=opt, figures=[
            _tail_frame_check(c, call, f, call.want[f], nd[f], pf[f], opt[f], prev[f], bad, f"call {j} frame {f}") for f in range(call.n)])
        prev[:call.n] = nd


def _process_outputs(torch, F_, c):
    """the calls of the case on one SPDepthSuperResolution of the library in force -> per call (refined labels, edge-enhanced
    points, ClusterND, PlaneFitted3D, OptimizedPoints), each with a leading n"""
    (W, H), k, out = c.size, c.k, []
    o = SS.new_object(F_, c)
    try:
        for call in c.calls:
            SS._pipe_run(torch, o, call)
            n = call.n
            out.append((_host(o.getRefinedLabels_Device()).reshape(n, H, W).copy(), _host(o.getEdgeEnhanced3DPoints_Device()).reshape(n, H, W, 3).copy(),
                        _host(o.getClusterND_Device()).reshape(n, k, 4).copy(), _host(o.getPlaneFitted3D_Device()).reshape(n, H, W, 3).copy(),
                        _host(o.getOptimizedPoints_Device()).reshape(n, H, W, 3).copy()))
    finally:
        o.close()
    return out


def _run_process(torch, F_, c, bad, got):
    """Process in the product build and in the stage build.  Each build's planes and plane-fitted cloud are held to planes64 and
    the projection bars on its OWN refined labels and points; then the hook, on those labels and points with that build's
    ClusterND and 20 sweeps, must give PlaneFitted3D and OptimizedPoints of Process bit for bit"""
    from tools.hooks import stage
    (W, H), k = c.size, c.k
    bits = lambda a: np.ascontiguousarray(a, F).view(np.uint32)
    builds = [("product", _process_outputs(torch, F_, c))]
    with stage.stage_library():
        builds.append(("stage", _process_outputs(torch, F_, c)))
    for name, outs in builds:
        prev = np.zeros((c.max_batch, k, 4), F)               # what the frame slots hold: zeros after SetParametor
        for j, (call, (lab, pts, nd, pf, opt)) in enumerate(zip(c.calls, outs)):
            figures = []
            for f in range(call.n):
                tag = f"{name} build, call {j} frame {f}"
                ref, skip, projected, low = process_reference(c, lab[f], pts[f], prev[f])
                _asserted(bad, tag, SC.planes_compare, nd[f], ref, "planes", skip)
                figures.append(dict(pf_ulps=_projection_bars(c, lab[f], pts[f], nd[f], pf[f], skip, bad, tag), skip=len(skip), low_den=low, projected=projected))
            prev[:call.n] = nd
            hnd, hpf, hopt = stage.spdsr_tail_run(W, H, c.rows, c.cols, c.K, lab, pts, nd=nd, sweeps=20, max_batch=c.max_batch)
            for what, a, b in (("ClusterND", hnd, nd), ("PlaneFitted3D", hpf, pf), ("OptimizedPoints", hopt, opt)):
                d = int((bits(a) != bits(b)).sum())
                if d:
                    bad.append(f"{name} build, call {j}: the hook's {what} differs from Process's in {d} of {b.size} floats")
            got[f"{name} call {j}"] = dict(labels=lab, points=pts, nd=nd, plane_fitted=pf, optimized=opt, figures=figures)


_RUN = dict(tail=_run_tail, process=_run_process, buffer2d=_run_buffer2d, convert=_run_convert, cloud=_run_cloud, error3d=_run_error3d)


def run_case(torch, F_, c):
    """Builds the object of the drawn case c, fills want, runs the calls and compares.  Returns (violations, got): a list of
    strings -- empty: every bar holds -- and what the device gave (for a dump)."""
    bad, got = [], {}
    try:
        if c.kind != "process":                              # its references come from the device's own labels and points
            want(c)
        _RUN[c.kind](torch, F_, c, bad, got)
        torch.cuda.synchronize()
    except F_._native.KdeError as e:
        bad.append(f"create or a call refused an admitted configuration: {e}")
    except RuntimeError as e:                                 # torch reports a HIP error of an earlier launch
        bad.append(f"refused: {e}")
    return bad, got
