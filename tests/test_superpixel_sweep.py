"""The conditions on the draw of tests/superpixel_sweep.py, on the CPU oracle alone (no GPU): everything here is asserted over
exactly the budget tests/test_gpu_superpixel_sweep.py runs, SEEDS x CASES_PER_KIND[kind] cases per kind, so that the GPU run cannot
pass by drawing nothing of interest and K10's BAND class cannot hide a failure; and the oracle's answer on the named inputs of the
GPU test is pinned here."""
import functools

import numpy as np
import pytest

import superpixel_sweep as S

KINDS = S.kinds()


@functools.lru_cache(maxsize=None)
def cases(kind):
    """the budget of a kind, made once and never written to"""
    return tuple(S.case(kind, seed, index) for seed, index in S.budget(kind))


def calls(kind):
    return [(c, call) for c in cases(kind) for call in c.calls]


def _bytes(c):
    return b"".join(np.ascontiguousarray(a).tobytes() for call in c.calls for a in call.inputs.values()) + repr(S.describe(c)).encode()


def _grids(c):
    """the (rows, cols) of every call of a dasp case: SetParametor may be called again"""
    out, g = [], (c.rows, c.cols)
    for call in c.calls:
        g = getattr(call, "regrid", None) or g
        out.append(g)
    return out


def test_the_kinds():
    assert KINDS == ("dasp", "ers", "rgbf", "spdsr") and set(S.CASES_PER_KIND) == set(KINDS)
    assert all(len(S.budget(k)) == len(S.SEEDS) * S.CASES_PER_KIND[k] for k in KINDS)


@pytest.mark.parametrize("kind", KINDS)
def test_a_case_depends_on_its_kind_seed_and_index_alone(kind):
    cs = cases(kind)
    picked = [cs[0], cs[3], cs[len(cs) // 2], cs[-1]]
    picked += [c for c in cs if len(c.calls) == 2][:1]                              # one with a second call
    picked += [c for c in cs if any(getattr(call, "regrid", None) for call in c.calls)][:1]      # dasp: and one with SetParametor again
    assert any(len(c.calls) == 2 for c in picked) and (kind != "dasp" or any(c.calls[-1].regrid for c in picked))
    for first in picked:
        again = S.case(kind, first.seed, first.index)         # made alone, after the whole budget
        assert _bytes(first) == _bytes(again) == _bytes(S.case(kind, first.seed, first.index)), S.describe(first)
        assert _bytes(first) != _bytes(S.draw(kind, first.seed, first.index + 1)) and _bytes(first) != _bytes(S.draw(kind, first.seed + 100, first.index))


def test_admitted_is_superpixel_geometry():
    """admitted() against the oracle's okde_dasp_check_geometry, the same four tests as csrc/kde_handles.h states them"""
    O = S.oracle()
    rng = np.random.default_rng(4)
    seen = set()
    for _ in range(4000):
        W, H, rows, cols = (int(v) for v in rng.integers(1, 80, 4))
        ok = O.lib().okde_dasp_check_geometry(W, H, rows, cols) == 0
        assert S.admitted(W, H, rows, cols) == ok, (W, H, rows, cols)
        seen.add(ok)
    assert seen == {False, True}
    assert not S.admitted(64, 48, 15, 20) and not S.admitted(40, 5, 1, 2) and S.admitted(260, 132, 33, 65)


@pytest.mark.parametrize("kind", KINDS)
def test_every_drawn_geometry_is_admitted(kind):
    for c in cases(kind):
        W, H = c.size
        assert 1 <= W <= S.MAX_W and 1 <= H <= S.MAX_H
        if kind == "ers":
            continue
        assert S.admitted(W, H, c.rows, c.cols), S.describe(c)
        for call in c.calls:
            if getattr(call, "regrid", None):
                assert S.admitted(W, H, *call.regrid) and call.regrid != (c.rows, c.cols)
            if hasattr(call, "sig"):
                with np.errstate(over="ignore"):              # finite sigmas; the sum, formed as the library forms it, is not 0
                    assert np.isfinite(call.sig).all() and np.float32(call.sig[1]) + np.float32(call.sig[0]) + np.float32(call.sig[2]) != 0, call.sig


# ---- dasp ---------------------------------------------------------------------------------------------------------------
def test_dasp_every_geometry_class_occurs():
    cs = cases("dasp")
    seen = [S.grid_classes(*c.size, *g) for c in cs for g in _grids(c)]
    for k in ("win4", "ragged", "1x1", "1xN", "Nx1", "small", "tile", "global", "NxN"):
        assert sum(k in s for s in seen) >= 2, k
    assert {c.grid for c in cs} == set(S.DASP_GRIDS) | {"pinned"}
    counts = {c.rows * c.cols for c in cs}
    assert {2048, 2145} <= counts and S.MAX_LDS_CLUSTERS == 2048      # the last table on LDS, the first in global memory
    sizes = [c.size for c in cs]
    assert {63, 64, 65} <= {w for w, _ in sizes} and any(h % 4 for _, h in sizes)
    assert any(c.rows < 4 and c.cols < 4 for c in cs) and any(c.rows >= 4 and c.cols >= 4 for c in cs)
    ragged = [c for c in cs if c.size[0] % (c.size[0] // c.cols)]                 # x / wx reaches cols on the last columns
    assert len(ragged) >= 10 and all((c.size[0] - 1) // (c.size[0] // c.cols) == c.cols for c in ragged)


def test_dasp_every_sigma_class_iteration_count_and_call_pattern_occurs():
    cs = cases("dasp")
    cl = calls("dasp")
    assert {call.sigmas for _, call in cl} == set(S.DASP_SIGMAS)
    assert {call.iteration for _, call in cl} == set(range(6))
    sig = {call.sigmas: call.sig for _, call in cl}
    assert (sig["sp"], sig["dasp"], sig["spdsr"]) == ((200.0, 40.0, 0.0), (100.0, 20.0, 200.0), (0.0, 10.0, 200.0))
    by = lambda name: [call.sig for _, call in cl if call.sigmas == name]
    zeros = lambda s: [v == 0 for v in s]
    assert {tuple(zeros(s)) for s in by("color0") + by("spatial0") + by("depth0")} == {(True, False, False), (False, True, False), (False, False, True)}
    assert all(sum(zeros(s)) == 2 for s in by("two0")) and len({tuple(zeros(s)) for s in by("two0")}) >= 2
    assert all(sum(v < 0 for v in s) == 1 for s in by("negative"))
    for s in by("tiny_sum"):                                  # the squared weights overflow
        total = np.float32(s[1]) + np.float32(s[0]) + np.float32(s[2])
        with np.errstate(over="ignore"):
            assert total != 0 and np.isinf([np.float32(v) / total * (np.float32(v) / total) for v in s]).any(), s
    with np.errstate(over="ignore"):
        assert all(max(np.abs(s)) >= 1e18 for s in by("large")) and any(np.isinf(np.float32(s[0]) + np.float32(s[1])) for s in by("large"))
    two = [c for c in cs if len(c.calls) == 2]
    assert 0.35 <= len(two) / len(cs) <= 0.7
    assert sum(c.calls[0].iteration > 0 and c.calls[1].iteration == 0 for c in two) >= 3      # 0 on a used handle
    assert sum(c.calls[0].iteration == 0 and c.calls[1].iteration > 0 for c in two) >= 3      # a count after 0
    assert sum(c.calls[1].regrid is not None for c in two) >= 3                                # SetParametor again
    assert all(c.calls[0].sigmas != c.calls[1].sigmas for c in two)


def test_dasp_every_special_value_occurs():
    cl = calls("dasp")
    z = [call.inputs["points"][..., 2] for _, call in cl]
    f50 = np.float32(50)
    tests = dict(hole=lambda a: (a == 0).any(), fifty=lambda a: (a == f50).any(), below50=lambda a: (a == np.nextafter(f50, np.float32(0))).any(),
                 above50=lambda a: (a == np.nextafter(f50, np.float32(100))).any(), negative=lambda a: (a < 0).any() & np.isfinite(a[a < 0]).any(),
                 pinf=lambda a: np.isposinf(a).any(), ninf=lambda a: np.isneginf(a).any(), nan=lambda a: np.isnan(a).any(),
                 huge=lambda a: (a == np.float32(3e38)).any())
    for name, t in tests.items():
        with np.errstate(invalid="ignore"):
            assert sum(bool(t(a)) for a in z) >= 3, name
    forms = {(k, v) for _, call in cl for k, v in call.what.get("specials", {}).items()}
    for k in S.DASP_SPECIALS:                                 # as a single pixel and as a patch that owns a cluster
        assert {v for kk, v in forms if kk == k} >= {"pixel", "patch"} or {v for kk, v in forms if kk == k} >= {"both"}, k
    assert {b for _, call in cl for b in call.what.get("below", [])} == {"far", "near"}
    assert {call.what["colour"] for _, call in cl if call.what} == set(S.DASP_COLOURS)
    black = [call for _, call in cl if not call.inputs["bgr"].any()]
    assert len(black) >= 3                                    # sumG / count is 0 / 0 for every candidate of every cluster


def test_dasp_the_cases_are_not_trivial():
    """on the oracle's output: the labels leave the initial grid, and distances, centres and rows leave the finite and the float-exact"""
    cs = cases("dasp")
    moved = [bool((c.calls[-1].want["labels"] != S.init_grid(*c.size, *_grids(c)[-1])).any()) for c in cs]
    assert np.mean(moved) >= 0.9, np.mean(moved)
    for seed in S.SEEDS:
        mine = [call.want for c in cs if c.seed == seed for call in c.calls]
        with np.errstate(invalid="ignore"):
            assert sum(bool((~np.isfinite(w["ld"]["d"])).any()) for w in mine) >= 1, seed
            assert sum(bool(np.isposinf(w["ld"]["d"]).any()) for w in mine) >= 1 and sum(bool(np.isnan(w["ld"]["d"]).any()) for w in mine) >= 1, seed
            assert sum(bool((~np.isfinite(np.ascontiguousarray(w["centers"]).view(np.float32))).any()) for w in mine) >= 1, seed
        assert sum(bool((w["mean"]["y"] >= (1 << 24)).any()) for w in mine) >= 1, seed
        assert sum(bool(((w["mean"]["y"] > 136) & (w["mean"]["y"] < (1 << 24))).any()) for w in mine) >= 1, seed
    zero = [(c, call) for c, call in calls("dasp") if call.iteration == 0]
    assert len(zero) >= 10
    for c, call in zero:                                      # LD is init_LD's grid
        assert (call.want["ld"]["d"] == np.float32(999999.9)).all()


# ---- ers ----------------------------------------------------------------------------------------------------------------
def test_ers_labels_lie_in_the_documented_domain_and_cover_it():
    cl = calls("ers")
    top_seen = minus_seen = 0
    for c, call in cl:
        W, H = c.size
        for key in ("color_labels", "depth_labels"):
            m = call.inputs[key]
            assert m.dtype == np.int32 and m.min() >= -1 and m.max() <= W * H - 1, S.describe(c)
            top_seen += bool((m == W * H - 1).any())
            minus_seen += bool((m == -1).any())
    assert top_seen >= 10 and minus_seen >= 10
    assert {call.style for _, call in cl} == set(S.ERS_STYLES) and {call.variant for _, call in cl} == {0, 1, 2, 3}
    assert all(call.variant == 3 for _, call in cl if call.hostile) and sum(bool(call.hostile) for _, call in cl) >= 5
    values = [v for _, call in cl for v in call.hostile.values()]
    assert any(np.isposinf(v) for v in values) and any(np.isnan(v) for v in values) and any(np.isfinite(v) and v > 2.0 ** 64 for v in values)
    for _, call in cl:
        if not call.hostile:
            assert np.isfinite(call.inputs["depth"]).all() and (call.inputs["depth"] >= 0).all()
    assert sum(bool((call.inputs["depth"] == 0).any()) for _, call in cl) == len(cl)                     # depth has holes
    sizes = [c.size for c in cases("ers")]
    assert {w % 64 for w, _ in sizes} >= {63, 0, 1} and {h % 8 for _, h in sizes} >= {7, 0, 1}            # either side of K10's 64 x 8 tile
    assert {len(c.calls) for c in cases("ers")} == {1, 2}


def test_ers_k9_changes_labels_and_depth_in_every_case():
    for c, call in calls("ers"):
        i, w = call.inputs, call.want
        assert (w["labels"] != i["depth_labels"]).any() and S.same_floats(w["edge_depth"], i["depth"]) > 0, S.describe(c)


def test_ers_band_census():
    """K10's BAND class at the oracle's own average, per case (the GPU cap is that count plus the larger of 2 pixels and 10 %)
    and pooled: at most 2 % of the pixels of the budget, the default cap of the existing tests, so that the class cannot hide a
    failure; and it is not empty, so that the cap is exercised"""
    band = sum(call.want["band"] for _, call in calls("ers"))
    pixels = sum(call.inputs["depth"].size for _, call in calls("ers"))
    assert 0 < band <= 0.02 * pixels, (band, pixels)
    for c, call in calls("ers"):
        w = call.want
        assert w["band_cap"] == w["band"] + max(2, -(-w["band"] // 10)) and w["band"] <= 0.02 * call.inputs["depth"].size, S.describe(c)


# ---- rgbf, spdsr ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["rgbf", "spdsr"])
def test_pipelines_draw_the_pinned_tables_batches_and_second_calls(kind):
    cs = cases(kind)
    counts = [c.rows * c.cols for c in cs]
    assert 1024 in counts and 1056 in counts and 2 * 1024 == S.MAX_LDS_CLUSTERS      # two tables: the last on LDS, the first in global memory
    cl = calls(kind)
    assert {call.n for _, call in cl} == {1, 2, 3} and {call.entry for _, call in cl} == {"single", "batch"}
    assert all(1 <= call.n <= c.max_batch for c, call in cl) and {len(c.calls) for c in cs} == {1, 2}
    assert any(c.rows * c.cols in (1024, 1056) and c.calls[0].n > 1 for c in cs)                        # a batch position other than 0
    for _, call in cl:
        assert np.isfinite(call.inputs["depth"]).all() and (call.inputs["depth"] >= 0).all()
    assert any(c.rows < 4 or c.cols < 4 for c in cs) and any(c.size[0] % (c.size[0] // c.cols) for c in cs)


def test_pipelines_the_labels_are_not_trivial():
    moved = [bool((w["dasp_labels"] != S.init_grid(*c.size, c.rows, c.cols)).any()) for c, call in calls("rgbf") for w in call.want]
    assert np.mean(moved) >= 0.8, np.mean(moved)
    differ = [bool((w["sp"] != w["dasp"]).any()) for c, call in calls("spdsr") for w in call.want]
    assert np.mean(differ) >= 0.8, np.mean(differ)


def test_spdsr_the_envelope_cannot_hide_a_failure():
    """test_spdsr_process_head_and_tail caps the pixels the float32 restatement's envelope flags (a tap on one of K10's
    decisions) at 1 % of the frame: every frame of the budget stays within it on the oracle alone, with room"""
    shares = [float(w["env"].flagged.mean()) for _, call in calls("spdsr") for w in call.want]
    assert len(shares) >= 30 and max(shares) <= 0.008, sorted(shares)[-5:]


def test_rgbf_band_census():
    """K10's BAND class at the oracle's own average on the pipeline's frames: assert_k10_stagewise's default cap is 2 % of a frame"""
    O = S.oracle()
    for c, call in calls("rgbf"):
        for f, w in enumerate(call.want):
            rl, rd9 = O.ers_edge_refining(w["sp_labels"], w["dasp_labels"], call.inputs["depth"][f])
            assert O.ers_stage(rd9, call.inputs["bgr"][f], rl).band.mean() <= 0.01, S.describe(c)


# ---- the named inputs of tests/test_gpu_superpixel_sweep.py: the oracle's answer ----------------------------------------
def test_named_no_iteration_case():
    c = S.want(S.iteration_zero_case())
    grid = S.init_grid(16, 8, 1, 2)
    assert set(np.unique(grid).tolist()) == {0, 1}
    for j in (0, 2):
        assert np.array_equal(c.calls[j].want["ld"]["l"], grid) and (c.calls[j].want["ld"]["d"] == np.float32(999999.9)).all()
        steps = S.oracle().dasp_steps(c.calls[j].inputs["bgr"], c.calls[j].inputs["points"], 1, 2)
        for f in ("r", "g", "b", "x", "y"):                   # the sampled clusters
            assert np.array_equal(c.calls[j].want["mean"][f], steps[1][f])
    assert not c.calls[0].want["labels"].any()                                   # a fresh handle: what SetParametor left
    assert np.array_equal(c.calls[2].want["labels"], c.calls[1].want["labels"]) and c.calls[1].want["labels"].any()
    assert np.array_equal(c.calls[2].want["mean"]["size"], c.calls[1].want["mean"]["size"]) and c.calls[1].want["mean"]["size"].all()


@pytest.mark.parametrize("depth_on", [True, False])
def test_named_infinite_pixel_case(depth_on):
    c = S.want(S.infinite_pixel_case(depth_on))
    w = c.calls[0].want
    assert S.init_grid(96, 64, 8, 12)[30, 40] == 41
    assert int(w["labels"][30, 40]) == 15 and int(w["ld"]["l"][30, 40]) == 15               # candidate 0: cell (1, 3) of the 8 x 12 grid
    assert np.isposinf(w["ld"]["d"][30, 40]) if depth_on else np.isnan(w["ld"]["d"][30, 40])
    with np.errstate(invalid="ignore"):
        assert int((~np.isfinite(w["ld"]["d"])).sum()) == 1


def test_named_infinite_centre_case():
    c = S.want(S.infinite_centre_case())
    w = c.calls[0].want
    cen = np.ascontiguousarray(w["centers"]).view(np.float32).reshape(-1, 3)
    assert np.isposinf(cen[18, 2])                            # nothing joined it, so analyzeClusters left the sampled centre
    own = (slice(16, 24), slice(16, 24))
    assert S.init_grid(64, 32, 4, 8)[own].tolist() == [[18] * 8] * 8
    assert (w["labels"][own] == 0).all() and np.isposinf(w["ld"]["d"][own]).all()      # candidate 0 of cell (2, 2) is cluster 0
