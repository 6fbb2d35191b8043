"""The five-argument Projection_GPU::PlaneProjection on the GPU (proj_kernels.hip) against the CPU restatement
tools/proj_ref.c, through the Python class.  The bar ("Plane projection (five-argument)"), every pixel checked:
plane-fitted points bit-identical; optimized points bit-identical with window_size = 1; with the filter on <= 1e-4 relative
with an identical zero mask where the pixel's own pre-filter z is > 50, <= 1e-4 on holes whose binary64 denominator is at
least 2^-120, and 0 or inside the window's valid range, widened by half a millimetre for the rounding of float32-denormal weights, on
the rest (BAND)."""
import numpy as np
import pytest

import proj_cases as PC
from gpu_util import dev
from proj_cases import F

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def R():
    from tools import proj_ref
    proj_ref.build()
    return proj_ref


@pytest.fixture(scope="module")
def T(torch_cuda):
    import torch
    torch.cuda.set_device(0)
    return torch


def params(**kw):
    from kinectdepthmapenhancement_amd import filters
    p = filters.PlaneProjection.default_params()
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def to_dev(T, case):
    nd, labels, variance, points, size, _ = case
    return [dev(T, np.ascontiguousarray(a, t)) for a, t in ((nd, F), (labels, np.int32), (variance, F), (points, F), (size, np.int32))]


def read_outputs(proj, frame=None):
    pick = (lambda t: t) if frame is None else (lambda t: t[frame])
    return {"plane_fitted": pick(proj.GetPlaneFitted3D_Device()).cpu().numpy(), "optimized": pick(proj.GetOptimized3D_Device()).cpu().numpy()}


def gpu_plane_projection(T, case, proj=None, **kw):
    from kinectdepthmapenhancement_amd import filters
    H, W = case[1].shape
    own = proj is None
    if own:
        proj = filters.PlaneProjection(W, H, case[5], params=params(**kw) if kw else None)
    proj.PlaneProjection(*to_dev(T, case))
    out = read_outputs(proj)
    T.cuda.synchronize()
    if own:
        proj.close()
    return out


def check(T, R, case, what, **kw):
    """filter on: the tolerance bar; window 1 on the same inputs: bit-identity of the pre-filter z"""
    exp = R.plane_projection(*case, **kw)
    got = gpu_plane_projection(T, case, **kw)
    cmp = R.compare(got["plane_fitted"], got["optimized"], exp, kw.get("window_size", R.WINDOW_SIZE))
    print(f"{what}: {cmp}")
    assert cmp["plane_fitted"] == 0 and cmp["strict"] == 0 and cmp["hole"] == 0 and cmp["band"] == 0 and cmp["xy"] == 0, f"{what}: {cmp}"
    return exp, got, cmp


def assert_same_bytes(a, b, what):
    for k in ("plane_fitted", "optimized"):
        n = int(R_differing(a[k], b[k]).sum())
        assert n == 0, f"{what}: {k} differs in {n} elements"


def R_differing(a, b):
    from tools import proj_ref
    return proj_ref.differing(a, b)


MAIN = [("70x50 nc20", dict(seed=1, W=70, H=50, nc=20)), ("33x25 nc1", dict(seed=2, W=33, H=25, nc=1)),
        ("96x64 nc2048", dict(seed=3, W=96, H=64, nc=2048))]


@pytest.mark.parametrize("name,kw", MAIN)
def test_parity_main_cases(T, R, name, kw):
    """depth 600-1250 mm: no BAND pixel by construction (asserted on the checker's side); min_size lowered so that both
    branches of .cu:204-208 fire; ragged against the 64 x 16 tile, the halo crosses every border"""
    case = PC.synthetic_case(**kw)
    ms = PC.min_size_for(kw["W"], kw["H"])
    exp, got, cmp = check(T, R, case, name, min_size=ms)
    assert cmp["n_band"] == 0 and cmp["n_hole"] > 0
    b = PC.branch_counts(exp, case[3], case[1], case[2], case[4], ms)
    assert b["projected"] and b["kept"] and b["replaced"] and b["blended"]
    # window 1 exposes the pre-filter z: bit-identical
    exp1 = R.plane_projection(*case, min_size=ms, window_size=1)
    got1 = gpu_plane_projection(T, case, min_size=ms, window_size=1)
    assert_same_bytes(got1, exp1, name + " window 1")
    assert int(R.differing(got1["optimized"][..., 2], np.where(exp["prefilter"][..., 2] > 50, exp["prefilter"][..., 2], F(0))).sum()) == 0


@pytest.mark.parametrize("window", (3, 5, 15))
def test_other_windows_take_the_run_time_kernel(T, R, window):
    case = PC.synthetic_case(seed=4, W=70, H=50, nc=20)
    check(T, R, case, f"window {window}", min_size=PC.min_size_for(70, 50), window_size=window, spatial_sigma=3.0, depth_sigma=40.0)


def test_reference_constants_on_the_golden_inputs(T, R):
    case = PC.golden_inputs()
    exp, got, cmp = check(T, R, case, "golden inputs, default parameters")
    b = PC.branch_counts(exp, case[3], case[1], case[2], case[4], PC.MIN_SIZE)
    assert cmp["n_band"] == 0 and b["replaced"] and b["blended"] and b["small_region"]


def test_deep_case_exercises_band(T, R):
    """depth up to 4000 mm: hardware exp and expf may flush differently below 2^-120; a BAND pixel must be 0 or inside its
    window's valid range"""
    case = PC.deep_case(5, 70, 50, 20)
    exp, got, cmp = check(T, R, case, "deep", min_size=PC.min_size_for(70, 50))
    holes = cmp["n_hole"] + cmp["n_band"]
    assert 0 < cmp["n_band"] < holes and cmp["n_band"] < 0.05 * 70 * 50


def test_denormal_weight_holes_stay_within_half_a_millimetre_of_their_tap(T, R):
    """found by the seeded sweep (proj_cases.denormal_weight_case, tests/test_proj_ref.py): a hole whose only tap weighs one
    unit of 2^-149.  The kernel's exp_denormal keeps such a weight, so the hole is filled, and what it is filled with is the
    tap's depth to the rounding of the denormal product (the BAND bar), or 0 where hardware exp flushes the weight"""
    case, kw = PC.denormal_weight_case()
    exp, got, cmp = check(T, R, case, "denormal weight", **kw)
    zg = got["optimized"][0, :, 2]
    print("denormal weight: device", zg.tolist(), "restatement", exp["optimized"][0, :, 2].tolist())
    assert cmp["n_band"] == 2 and zg[1] == PC.DENORMAL_TAP
    assert all(z == 0 or abs(float(z) - float(PC.DENORMAL_TAP)) <= 0.5 for z in zg[[0, 2]])


def test_micro_cases_inf_nan_and_table_edges(T, R):
    """the hand-worked frame of tests/test_proj_ref.py (proj_cases.micro_frame): label >= n_clusters, plane denominator 0 -> inf / NaN, variance 1,
    > 1 and NaN"""
    case = PC.micro_frame()
    for w in (1, 3):
        exp = R.plane_projection(*case, window_size=w)
        got = gpu_plane_projection(T, case, window_size=w)
        assert int(R.differing(got["plane_fitted"], exp["plane_fitted"]).sum()) == 0
        assert np.isinf(got["plane_fitted"][0, 7, 2]) and np.isnan(got["plane_fitted"][0, 7, 1])
        if w == 1:
            assert_same_bytes(got, exp, "micro window 1")
        else:
            cmp = R.compare(got["plane_fitted"], got["optimized"], exp, w)
            assert cmp["strict"] == cmp["hole"] == cmp["band"] == 0, cmp


def batch_inputs(T):
    W, H, nc = 96, 64, 20
    cases = [PC.synthetic_case(seed=10 + k, W=W, H=H, nc=nc) for k in range(3)]
    stack = lambda i, t: dev(T, np.stack([np.ascontiguousarray(c[i], t) for c in cases]))
    return W, H, cases, [stack(0, F), stack(1, np.int32), stack(2, F), stack(3, F), stack(4, np.int32)]


def test_batch_equals_single_calls_on_a_side_stream_and_a_used_handle(T, R):
    from kinectdepthmapenhancement_amd import filters
    W, H, cases, batch = batch_inputs(T)
    ms = PC.min_size_for(W, H)
    singles = [gpu_plane_projection(T, c, min_size=ms) for c in cases]
    proj = filters.PlaneProjection(W, H, cases[0][5], max_batch=3, params=params(min_size=ms))
    T.cuda.synchronize()
    s = T.cuda.Stream()
    with T.cuda.stream(s):
        proj.plane_projection_batch(*batch)
    s.synchronize()
    for k in range(3):
        assert_same_bytes(read_outputs(proj, k), singles[k], f"batch frame {k}")
    host = proj.GetOptimized3D_Host()
    assert host.shape == (3, H, W, 3) and int(R.differing(host[2], singles[2]["optimized"]).sum()) == 0
    assert int(R.differing(proj.GetPlaneFitted3D_Host()[1], singles[1]["plane_fitted"]).sum()) == 0
    # the used handle again with smaller n, other frames first
    proj.plane_projection_batch(*[t[[2, 0]].contiguous() for t in batch])
    T.cuda.synchronize()
    assert_same_bytes(read_outputs(proj, 0), singles[2], "second call, frame 0")
    assert_same_bytes(read_outputs(proj, 1), singles[0], "second call, frame 1")
    proj.PlaneProjection(*[t[1].contiguous() for t in batch])
    T.cuda.synchronize()
    assert_same_bytes(read_outputs(proj), singles[1], "third call, one frame")
    proj.close()


def test_graph_capture_replays_the_same_bytes(T, R):
    from kinectdepthmapenhancement_amd import filters
    W, H, cases, batch = batch_inputs(T)
    proj = filters.PlaneProjection(W, H, cases[0][5], max_batch=3, params=params(min_size=PC.min_size_for(W, H)))
    proj.plane_projection_batch(*batch)
    eager = [read_outputs(proj, k) for k in range(3)]
    T.cuda.synchronize()
    s = T.cuda.Stream()
    graph = T.cuda.CUDAGraph()
    with T.cuda.graph(graph, stream=s):
        proj.plane_projection_batch(*batch)
    for _ in range(2):
        proj.GetOptimized3D_Device().fill_(7)
        proj.GetPlaneFitted3D_Device().fill_(7)
        T.cuda.synchronize()
        graph.replay()
        T.cuda.synchronize()
        for k in range(3):
            assert_same_bytes(read_outputs(proj, k), eager[k], f"replay frame {k}")
    del graph
    proj.close()


def test_argument_checks(T):
    import ctypes as C
    from kinectdepthmapenhancement_amd import filters, _native
    K = PC.intrinsics(64, 48)
    for bad in (dict(window_size=4), dict(window_size=17), dict(window_size=0), dict(depth_sigma=0.0), dict(depth_sigma=-1.0),
                dict(spatial_sigma=0.0), dict(max_angle=float("nan"))):
        with pytest.raises(_native.KdeError):
            filters.PlaneProjection(64, 48, K, params=params(**bad))
    with pytest.raises(_native.KdeError):
        filters.PlaneProjection(64, 48, K, max_batch=0)
    lib = _native.lib()
    h = C.c_void_p()
    assert lib.kde_proj_create(C.byref(h), 64, 48, 1, None, None) == _native.KDE_ERR_INVALID and not h.value
    proj = filters.PlaneProjection(64, 48, K, max_batch=2)
    nd, lab = T.zeros((48, 64, 4), device="cuda"), T.zeros((48, 64), dtype=T.int32, device="cuda")
    var, pts, size = T.zeros(5, device="cuda"), T.zeros((48, 64, 3), device="cuda"), T.zeros(5, dtype=T.int32, device="cuda")
    ptrs = [nd.data_ptr(), lab.data_ptr(), var.data_ptr(), pts.data_ptr(), size.data_ptr()]
    for k in range(5):                                      # each NULL in turn
        a = list(ptrs)
        a[k] = None
        assert lib.kde_proj_plane_projection(proj._h, *a, 5, None) == _native.KDE_ERR_INVALID
    assert lib.kde_proj_plane_projection(proj._h, *ptrs, 0, None) == _native.KDE_ERR_INVALID
    assert lib.kde_proj_plane_projection_batch(proj._h, 3, *ptrs, 5, None) == _native.KDE_ERR_INVALID     # n > max_batch
    assert lib.kde_proj_plane_projection_batch(proj._h, 0, *ptrs, 5, None) == _native.KDE_ERR_INVALID
    assert lib.kde_proj_optimized_points_device(proj._h, None) == _native.KDE_ERR_INVALID
    with pytest.raises((_native.KdeError, ValueError)):
        proj.PlaneProjection(nd, lab, var, pts, T.zeros(6, dtype=T.int32, device="cuda"))
    if T.cuda.device_count() > 1:                           # a handle belongs to the device it was created on
        T.cuda.set_device(1)
        try:
            assert lib.kde_proj_plane_projection(proj._h, *ptrs, 5, None) == _native.KDE_ERR_INVALID
        finally:
            T.cuda.set_device(0)
    assert lib.kde_proj_plane_projection(proj._h, *ptrs, 5, None) == _native.KDE_OK
    T.cuda.synchronize()
    proj.close()
