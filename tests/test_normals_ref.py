"""The CPU checker of the normal-estimation stage (tools/normals_ref.c) on hand-checked cases, and the C ABI's argument
validation of kde_normals_* (no GPU needed)."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

from conftest import ROOT

F = np.float32
A = F(1.4)          # the reference's 1.4f


@pytest.fixture(scope="module")
def R():
    from tools import normals_ref
    normals_ref.build()
    return normals_ref


def dci_with_seeds(W, H, seeds):
    d = np.full((H, W), 255, np.uint8)
    for r, c in seeds:
        d[r, c] = 0
    return d


# ---- distance transform (SmoothingAreaMapGenerator.cu:40-92) ---------------------------------------------------------
def test_dt_single_seed(R):
    big = F(8)
    T = R.distance_transform(dci_with_seeds(4, 4, [(1, 1)]))
    exp = np.array([[big, big, big, big],
                    [big, 0, 1, 2],
                    [F(2), 1, A, F(1) + A],      # (2,0) comes from the backward sweep of row H-2 only
                    [big, 2, F(1) + A, A + A]], np.float32)
    np.testing.assert_array_equal(T, exp)


def test_dt_up_right_wraps_to_column_zero_of_the_current_row(R):
    # seed at (2, 0): at c = W-1 the forward pass reads previous_row[W] = current_row[0] as upRight
    W, H = 6, 3
    big = F(W + H)
    T = R.distance_transform(dci_with_seeds(W, H, [(2, 0)]))
    np.testing.assert_array_equal(T[2], np.array([0, 1, 2, 3, 4, A], np.float32))
    # backward sweep of row H-2 against row H-1; at c = 0 lowerLeft reads current_row[W-1] (= big + 1.4 here)
    np.testing.assert_array_equal(T[1], np.array([1, A, F(1) + A, F(2) + A, A + A, big], np.float32))
    np.testing.assert_array_equal(T[0], np.full(W, big, np.float32))


def test_dt_backward_pass_changes_only_row_h_minus_2(R):
    W, H = 7, 5
    T = R.distance_transform(dci_with_seeds(W, H, [(4, 3)]))
    assert (T[:3] == F(W + H)).all()          # a true backward pass would have reached these rows
    assert (T[3, :W - 1] < F(W + H)).all()    # row H-2, except its last column, which the sweep never visits
    assert T[3, W - 1] == F(W + H)
    assert T[3, 3] == 1 and T[3, 2] == A and T[3, 4] == A


@pytest.mark.parametrize("W,H", [(1, 1), (1, 6), (6, 1)])
def test_dt_degenerate_sizes_run_no_pass(R, W, H):
    d = dci_with_seeds(W, H, [(0, 0)])
    exp = np.where(d == 0, F(0), F(W + H)).astype(np.float32)
    np.testing.assert_array_equal(R.distance_transform(d), exp)


def test_dt_two_rows(R):
    # H = 2: the forward pass does row 1, the backward sweep row 0
    T = R.distance_transform(dci_with_seeds(4, 2, [(1, 1)]))
    np.testing.assert_array_equal(T[1], np.array([6, 0, 1, 2], np.float32))
    np.testing.assert_array_equal(T[0], np.array([A, 1, A, 6], np.float32))


# ---- depth-change map (definition N1) ----------------------------------------------------------------------------------
def test_dci_threshold(R):
    # thr = (0.05 * (|1| + 1)) * 2 = 0.2: 1.1 stays, 1.3 fires; the last row fires on its (out-of-frame) down neighbour
    v = np.zeros((3, 3, 3), np.float32)
    v[..., 2] = 1.0
    v[0, 1, 2] = 1.1
    d = R.dci_map(v)
    assert (d[:2] == 255).all() and (d[2] == 0).all()
    v[0, 1, 2] = 1.3
    d = R.dci_map(v)
    # (0,1) fires right and down: it, (0,2) and (1,1) are 0; (0,0)'s right test fires too
    assert d[0, 0] == 0 and d[0, 1] == 0 and d[0, 2] == 0 and d[1, 1] == 0
    assert d[1, 0] == 255 and d[1, 2] == 255


def test_dci_zero_depth_and_linear_wrap(R):
    W, H = 3, 3
    v = np.zeros((H, W, 3), np.float32)
    v[..., 2] = 2.0
    v[1, 0, 2] = 5.0        # the right neighbour of (0, 2) in the linear index
    d = R.dci_map(v)
    assert d[0, 2] == 0      # right test of (0,2) compares with (1,0)
    assert d[0, 0] == 0      # down test of (0,0) fires
    assert d[1, 0] == 0 and d[1, 1] == 0
    assert d[0, 1] == 255
    v[1, 0, 2] = 2.0
    v[0, 1, 2] = 0.0        # z == 0 fires both tests of its own and of its left / upper neighbours
    d = R.dci_map(v)
    assert d[0, 0] == 0 and d[0, 1] == 0 and d[0, 2] == 0 and d[1, 1] == 0
    assert d[1, 0] == 255


# ---- eigen solver (NormalMapGenerator.cu:135-242) -------------------------------------------------------------------
def test_eigen_diagonal(R):
    # the float-typed constants ((double)(1.0f/3.0f), (double)sqrtf(3.0f)) hold the roots to ~1e-7 of the scale
    ev, vec, code = R.eigen(np.diag([3.0, 2.0, 1.0]))
    assert abs(ev - 1.0) < 1e-6
    np.testing.assert_allclose(np.abs(vec), [0, 0, 1], atol=1e-6)
    assert not code & R.SMALL_C0


def test_eigen_plane_points(R):
    rng = np.random.default_rng(7)
    xy = rng.uniform(-0.3, 0.3, (400, 2))
    z = 0.5 * xy[:, 0] + 0.2 * xy[:, 1] + 3.0
    P = np.column_stack([xy, z])
    C = (P - P.mean(0)).T @ (P - P.mean(0))
    ev, vec, code = R.eigen(C)
    n = np.array([0.5, 0.2, -1.0]) / np.linalg.norm([0.5, 0.2, -1.0])
    assert abs(abs(vec @ n) - 1.0) < 1e-9
    assert abs(ev) < 1e-6 * np.abs(C).max()


def test_eigen_zero_matrix(R):
    ev, vec, code = R.eigen(np.zeros((3, 3)))
    assert code & R.SMALL_C0 and ev == 0.0
    assert np.isnan(vec).all()          # 0 / 0: the reference's normal is NaN there too


# ---- whole frames ------------------------------------------------------------------------------------------------------
# band census on synthetic VGA frames (seeds 1-3), measured with this checker: 1730, 983 and 587 pixels of 307200
BAND_BOUND_VGA = 2000


def vga_points(seed, W=640, H=480):
    from kinectdepthmapenhancement_amd import synth
    from oracle import oracle as O
    _, depth = synth.make_frame(seed, W, H)
    return O.p2r_depth(depth, synth.intrinsics(W, H)).view(np.float32).reshape(H, W, 3)


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_band_census_on_vga(R, seed):
    p = vga_points(seed)
    n, fs, band = R.normals(p, R.CM)
    bad = (n == -1).all(-1)
    assert 0 < band.sum() <= BAND_BOUND_VGA
    assert not (band & bad).any()
    # every non-bad CM normal is a unit vector
    ok = ~bad & ~np.isnan(n).any(-1)
    np.testing.assert_allclose(np.linalg.norm(n[ok], axis=-1), 1.0, atol=1e-5)
    assert fs.max() <= 20.0 + p[..., 2].max() / 1000.0 / 10.0 + 1e-3


def test_bilateral_restates_the_neighbour_cross_product(R):
    p = vga_points(1, 64, 48)
    n, _, _ = R.normals(p, R.BILATERAL)
    v = R.scale(p)
    # pixel (10, 10): r = +1, cross of (right - c) and (down - c), divided by -norm, then x and z negated
    c, rr, dd = v[10, 10], v[10, 11], v[11, 10]
    h, w = rr - c, dd - c
    m = np.array([h[2] * w[1] - h[1] * w[2], -(h[0] * w[2] - h[2] * w[0]), h[1] * w[0] - h[0] * w[1]], np.float32)
    m = m / -np.sqrt(np.float32((m * m).sum()))
    np.testing.assert_allclose(n[10, 10], [-m[0], m[1], -m[2]], rtol=1e-6, atol=1e-7)
    assert ((n == -1).all(-1) == (p[..., 2] == 0)).all()


@pytest.mark.skipif(shutil.which("gcc") is None, reason="gcc not available")
def test_checker_under_asan_and_ubsan(tmp_path):
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-g", "-O1"]
    exe = str(tmp_path / "normals_driver")
    subprocess.check_call(["gcc", "-std=c11", "-ffp-contract=off", *san, "-o", exe,
                           os.path.join(ROOT, "tests", "sanitize", "normals_driver.c"),
                           os.path.join(ROOT, "tools", "normals_ref.c"), "-lm"])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr
    assert "normals driver ok" in r.stdout


# ---- C ABI validation (before any HIP call) ---------------------------------------------------------------------------
def test_normals_create_validates_without_a_gpu():
    from kinectdepthmapenhancement_amd import _native as N
    lib = N.lib()
    p = N.NormalsParams()
    assert lib.kde_normals_default_params(ctypes.byref(p)) == N.KDE_OK
    assert (p.method, p.normal_smoothing_size) == (N.KDE_NORMALS_BILATERAL, 20.0)
    assert abs(p.max_depth_change_factor - 0.05) < 1e-9
    h = ctypes.c_void_p()
    for w, hh, b in [(0, 480, 1), (640, 0, 1), (640, 480, 0), (1 << 16, 1 << 15, 1), (640, 480, 70000)]:
        assert lib.kde_normals_create(ctypes.byref(h), w, hh, b, None) == N.KDE_ERR_INVALID
        assert not h.value
    p.method = N.KDE_NORMALS_SDC
    assert lib.kde_normals_create(ctypes.byref(h), 640, 480, 1, ctypes.byref(p)) == N.KDE_ERR_UNSUPPORTED
    assert b"SDC" in lib.kde_last_error_string()
    p.method = 7
    assert lib.kde_normals_create(ctypes.byref(h), 640, 480, 1, ctypes.byref(p)) == N.KDE_ERR_INVALID
    p.method, p.normal_smoothing_size = N.KDE_NORMALS_CM, float("inf")
    assert lib.kde_normals_create(ctypes.byref(h), 640, 480, 1, ctypes.byref(p)) == N.KDE_ERR_INVALID
    assert lib.kde_normals_set_method(None, N.KDE_NORMALS_CM) == N.KDE_ERR_INVALID
    assert lib.kde_normals_smoothing_map_device(None, None) == N.KDE_ERR_INVALID
    assert lib.kde_normals_destroy(None) == N.KDE_OK


def test_normals_header_is_c99():
    src = "#include \"kde_hip.h\"\nint main(void) { kde_normals_params p; (void)p; return KDE_NORMALS_CM; }\n"
    r = subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-fsyntax-only", "-I",
                        os.path.join(ROOT, "include"), "-x", "c", "-"], input=src, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
