"""The conditions on the seeded draw of tests/output_sweep.py, held on the CPU over exactly the budget tests/test_gpu_output_sweep.py
runs, and the oracle's answer on every named case.  Nothing here needs a GPU."""
import hashlib
from types import SimpleNamespace

import numpy as np
import pytest

import output_sweep as S
import spdsr_tail_cases as SC
from superpixel_sweep import admitted

F = np.float32


def _digest(v, h=None):
    """a hash over every array, number and string a case holds"""
    top = h is None
    h = hashlib.sha256() if top else h
    if isinstance(v, SimpleNamespace):
        v = vars(v)
    if isinstance(v, dict):
        for k in sorted(v, key=str):
            if k not in ("want", "raised", "counts", "tail"):  # what want() adds
                h.update(str(k).encode())
                _digest(v[k], h)
    elif isinstance(v, (list, tuple)):
        for x in v:
            _digest(x, h)
    elif isinstance(v, np.ndarray):
        h.update(str((v.dtype, v.shape)).encode())
        h.update(np.ascontiguousarray(v).tobytes())
    else:
        h.update(repr(v).encode())
    return h.hexdigest() if top else None


@pytest.fixture(scope="module")
def cases():
    """the whole budget with its references: drawn once, shared, left unchanged"""
    return {kind: [S.case(kind, seed, index) for seed, index in S.budget(kind)] for kind in S.kinds()}


@pytest.mark.parametrize("kind", S.kinds())
def test_a_case_is_its_seed_kind_and_index_alone(kind, cases):
    """the same (kind, seed, index) gives the same bytes, whatever was drawn before"""
    for at in (0, 3, S.CASES_PER_KIND[kind] - 1):
        S.draw(kind, 2, (at + 1) % S.CASES_PER_KIND[kind])            # another case in between
        again = S.draw(kind, 1, at)
        assert _digest(again) == _digest(cases[kind][at]), (kind, at)
    assert len({_digest(c) for c in cases[kind]}) == len(cases[kind])
    assert all(S.describe(c).startswith(f"({kind!r}, seed {c.seed}, index {c.index})") for c in cases[kind])


def test_kind_numbers_and_budget():
    assert S.SEEDS == (1, 2) and set(S.kinds()) <= set(S.ALL_KINDS)
    assert [S.ALL_KINDS.index(k) for k in S.kinds()] == sorted(S.ALL_KINDS.index(k) for k in S.kinds())
    for kind in S.kinds():
        assert S.budget(kind) == [(s, i) for s in (1, 2) for i in range(S.CASES_PER_KIND[kind])]


# ---- tail ---------------------------------------------------------------------------------------------------------------------
def test_tail_geometry_is_admitted_and_dealt(cases):
    cs = cases["tail"]
    for c in cs:
        W, H = c.size
        assert admitted(W, H, c.rows, c.cols) and W <= S.MAX_W and H <= S.MAX_H, S.describe(c)
        assert 1 <= c.n <= c.max_batch <= 4 and all(1 <= call.n <= c.max_batch and call.sweeps >= 0 for call in c.calls)
        f = c.K[0, 0]
        assert 0.9 * max(W, H) - 1e-3 <= f <= 2.0 * max(W, H) and c.tilt <= 0.5
        for call in c.calls:
            assert call.labels.shape == (call.n, H, W) and call.points.shape == (call.n, H, W, 3)
            assert (call.labels < 0).any() and (call.labels >= c.k).any() or W * H < 200
    for seed in S.SEEDS:
        mine = [c for c in cs if c.seed == seed]
        assert {1024, 1056} <= {c.k for c in mine} and 1 in {c.k for c in mine}
        assert set(S.TAIL_WIDTHS) <= {c.size[0] for c in mine}
        assert any(c.size[0] % 2 and c.size[0] not in S.TAIL_WIDTHS for c in mine)
        assert any(c.size[1] % 8 == 0 for c in mine) and any(c.size[1] % 8 for c in mine)
        tiles = [c.tiles for c in mine]
        assert min(tiles) < 8 and 8 in tiles and any(t > 8 and t % 8 for t in tiles)
        assert any(c.max_batch > c.n for c in mine) and {c.n for c in mine} == {1, 2, 3, 4}
    sweeps = {call.sweeps for c in cs for call in c.calls}
    assert sweeps == set(S.TAIL_SWEEPS)
    assert {s for c in cs for call in c.calls for s in call.styles} == {"grid", "blobs", "stripes", "speckle"}
    assert {i for c in cs for call in c.calls for i in call.items} >= set(SC.MICRO_ITEMS)
    starved = [v for c in cs for call in c.calls for d in call.starved for v in d.values()]
    assert set(starved) == {0, 1, 2, 3}
    fits = [c.fit for c in cs]
    assert abs(sum(fits) - len(fits) / 2) <= 1
    second = [len(c.calls) == 2 for c in cs]
    assert 0.3 <= np.mean(second) <= 0.7 and all(c.calls[1].nd is None for c in cs if len(c.calls) == 2)
    values = np.concatenate([call.points[..., 2].reshape(-1) for c in cs for call in c.calls])
    for v in S.TAIL_INVALID:
        assert (values == v).any()


def test_tail_conditions_on_the_reference(cases):
    """no decision of the binary64 reference within 2 x MARGIN; at most 2 % of the projected pixels with |den| < 0.5; every
    fitted cluster but at most one per case has an eigen-gap >= 1e-6; at least 90 % of the cases that sweep rewrite more than
    30 % of their pixels; the e32 table is what okde_projection_plane gives"""
    cs = cases["tail"]
    e32, rewritten, rejected, gaps, worst = {}, [], 0, [], 0.0
    for c in cs:
        rejected += c.rejected
        skipped = 0
        share = []
        for call in c.calls:
            for w in call.want:
                assert w["min_margin"] >= 2.0 * SC.MARGIN, S.describe(c)
                skipped += len(w["skip"])
                if w["gap"] is not None:
                    gaps.extend(w["gap"][np.isfinite(w["gap"]) & (w["gap"] >= S.MIN_GAP)].tolist())
                e32[call.sweeps] = max(e32.get(call.sweeps, 0.0), w["e32"])
                if call.sweeps:
                    share.append(w["rewritten"])
        assert skipped <= 1, S.describe(c)
        low, projected = (sum(w[k] for call in c.calls for w in call.want) for k in ("low_den", "projected"))
        assert low <= 0.02 * projected, (S.describe(c), low, projected)       # outside the dealt pf_inf planes alone
        worst = max(worst, low / max(projected, 1))
        if share:
            rewritten.append(min(share))
    assert np.mean(np.array(rewritten) > 0.3) >= 0.9, sorted(rewritten)[:5]
    assert rejected <= 20, rejected
    print(f"tail: {rejected} proposals rejected; smallest held eigen-gap {min(gaps):.2e}; e32 per sweep count {e32}; "
          f"smallest rewritten share of a sweeping case {min(rewritten):.2f}; largest share of |den| < 0.5 in a case {worst:.4f}")
    assert set(e32) == set(S.TAIL_E32)
    for k, v in e32.items():
        assert abs(v - S.TAIL_E32[k]) <= 1e-3 * v, (k, v, S.TAIL_E32[k])


def test_tail_bars_hold_for_the_float32_restatement(cases):
    """what run_case asks of the device, asked of okde_projection_plane on the reference's planes: every bar of the kind can be met"""
    O = S.oracle()
    for c in cases["tail"]:
        prev = np.zeros((c.max_batch, c.k, 4), F)
        for j, call in enumerate(c.calls):
            nds = []
            for f in range(call.n):
                nd = SC.planes64(call.labels[f], call.points[f], c.k, nd_prev=prev[f])["nd"] if call.nd is None else call.nd[f]
                pf32, opt32 = (S._f3(a) for a in O.projection_plane(nd, call.labels[f], call.points[f], c.K, call.sweeps))
                bad = []
                fig = S._tail_frame_check(c, call, f, call.want[f], nd, pf32, opt32, prev[f], bad, f"call {j} frame {f}")
                assert not bad and fig["flagged"] == 0, (S.describe(c), bad)
                nds.append(nd)
            prev[:call.n] = np.stack(nds)


# ---- process -------------------------------------------------------------------------------------------------------------------
def test_process_draw_is_the_spdsr_draw_and_keeps_its_bars(cases):
    """the cases are superpixel_sweep's `spdsr` cases, input for input; on the oracle's head every frame has fitted clusters, the
    clusters below the eigen-gap (they lose the normals' bar) are at most 2 % of a frame's fitted ones or one, and the projected
    pixels with |den| < 0.5 (they lose the 8-ulp bar, nothing else) leave 75 % of a case's and 90 % of the budget's projected
    pixels under it"""
    import superpixel_sweep as SS
    cs = cases["process"]
    assert S.budget("process") == SS.budget("spdsr")
    low_all = projected_all = 0
    for c in cs:
        s = SS.draw("spdsr", c.seed, c.index)
        assert (c.size, c.rows, c.cols, c.n, c.max_batch) == (s.size, s.rows, s.cols, s.n, s.max_batch) and admitted(*c.size, c.rows, c.cols)
        assert len(c.calls) == len(s.calls) and all(_digest(a.inputs) == _digest(b.inputs) and a.entry == b.entry for a, b in zip(c.calls, s.calls))
        low = projected = 0
        for call in c.calls:
            assert len(call.tail) == call.n
            for w in call.tail:
                assert w["fitted"] >= 1 and len(w["skip"]) <= max(1, 0.02 * w["fitted"]), (S.describe(c), w)
                low, projected = low + w["low_den"], projected + w["projected"]
        assert low <= 0.25 * projected, (S.describe(c), low, projected)
        low_all, projected_all = low_all + low, projected_all + projected
    assert low_all <= 0.1 * projected_all, (low_all, projected_all)
    assert {1024, 1056} <= {c.k for c in cs} and any(c.max_batch > c.n for c in cs) and any(len(c.calls) == 2 for c in cs)
    assert any(w["markers"] for c in cs for call in c.calls for w in call.tail)
    print(f"process: {sum(call.n for c in cs for call in c.calls)} frames, {low_all} of {projected_all} projected pixels with |den| < 0.5, "
          f"{sum(len(w['skip']) for c in cs for call in c.calls for w in call.tail)} clusters below the eigen-gap of "
          f"{sum(w['fitted'] for c in cs for call in c.calls for w in call.tail)} fitted")


# ---- buffer2d ------------------------------------------------------------------------------------------------------------------
def test_buffer2d_draw(cases):
    cs = cases["buffer2d"]
    assert np.mean([c.raised >= 3 for c in cs]) >= 0.7
    for cls in S.BUF_CLASSES:
        mine = [c for c in cs if c.cls == cls]
        assert {c.size[0] * c.size[1] % 4 for c in mine} == {0, 1, 2, 3}, cls
    assert any(c.size[0] * c.size[1] < 4 for c in cs) and any(c.size[0] * c.size[1] % 2 for c in cs)
    assert all(3 <= len(c.ops) <= 8 and c.size[0] >= 1 and c.size[1] >= 1 for c in cs)
    assert {o.op for c in cs for o in c.ops} == set(S.BUF_OPS)
    assert {o.off for c in cs for o in c.ops} == {0, 1, 2, 3} == {g for c in cs for o in c.ops for g in o.get_off}
    assert {len(o.data) for c in cs for o in c.ops if o.op == "update_seq"} == {2, 3, 4, 5, 6}
    depth = np.concatenate([o.data.reshape(-1) for c in cs if c.cls == "hostile" for o in c.ops if o.op.startswith("update")])
    state = np.concatenate([o.data[..., 0].reshape(-1) for c in cs if c.cls == "hostile" for o in c.ops if o.op in ("insert_float2", "insert_weighted")])
    weight = np.concatenate([o.data[..., 1].reshape(-1) for c in cs if c.cls == "hostile" for o in c.ops if o.op == "insert_weighted"])
    for v in S.HOSTILE:
        for where in (depth, state):
            assert (np.isnan(where).any() if np.isnan(v) else ((where == v) & (np.signbit(where) == np.signbit(v))).any()), v
    for v in S.HOSTILE_W:
        assert np.isnan(weight).any() if np.isnan(v) else (weight == v).any(), v
    fifty = np.concatenate([o.data.reshape(-1) for c in cs if c.cls == "fifty" for o in c.ops if o.op.startswith("update")])
    assert (fifty == F(50)).any() and (fifty == np.nextafter(F(50), F(100))).any()


def test_buffer2d_limit_pairs_sit_on_either_side(cases):
    """the pairs of the `limit` class: neighbouring floats, the rule's comparison false for the lower and true for the upper, and
    the oracle averages exactly the records that got the upper one"""
    for k in (6, 11, 40):
        lo, hi = S.limit_pair(k)
        assert np.nextafter(lo, S.INF) == hi and not F(k) < F(lo * F(0.01)) and F(k) < F(hi * F(0.01))
    for c in [c for c in cases["buffer2d"] if c.cls == "limit"]:
        m = c.marked
        before, after = c.want[0][2], c.want[1][2]
        took_hi = c.ops[1].data[m] == c.pairs[1]
        assert took_hi.any() and (~took_hi).any() or m.sum() < 4
        assert np.array_equal(after[m] - before[m] == 1.0, took_hi), S.describe(c)


def test_buffer2d_int_min_difference_is_averaged():
    for n in (4, 3):
        c = S.want(S.int_min_difference_case(n))
        raw = c.want[1][0].reshape(-1, 2)
        assert raw[0].tolist() == [715827904.0, 2.0] and raw[1].tolist() == [np.inf, 3.0] and raw[2].tolist() == [-2.0 ** 31, 1.0]
        if n == 4:
            assert raw[3].tolist() == [float(F(3.0e38)), 2.0]


# ---- convert -------------------------------------------------------------------------------------------------------------------
def test_convert_draw(cases):
    cs = cases["convert"]
    assert {c.n for c in cs} == {1, 2, 3} and {c.size[0] * c.size[1] % 4 for c in cs} == {0, 1, 2, 3}
    for key in ("depth", "points", "out", "zf", "zu"):
        assert {c.off[key] for c in cs} == {0, 1, 2, 3}
    assert any(c.K[0, 2] < 0 for c in cs) and any(c.K[1, 2] > c.size[1] for c in cs) and all(c.K[0, 2] != int(c.K[0, 2]) for c in cs)
    z = np.concatenate([c.points[..., 2].reshape(-1) for c in cs])
    d = np.concatenate([c.depth.reshape(-1) for c in cs])
    for v in np.concatenate([S.HOSTILE, S.UNIT_Z]):
        for where in (z, d):
            assert (np.isnan(where).any() if np.isnan(v) else ((where == v) & (np.signbit(where) == np.signbit(v))).any()), v
    both = [(np.abs(c.want["r2p"][..., 2]) < 1).any() and (np.abs(c.want["r2p"][..., 2]) >= 1).any() for c in cs]
    assert np.mean(both) >= 0.8                 # both sides of realToProjective's |z| < 1 rule; a frame of a few pixels may miss one


def test_convert_reaches_every_streaming_form_in_every_seed(cases):
    """tests/test_gpu_streaming_forms.py runs the budget again with the cache threshold at 0 and asks every site of
    csrc/stream_kernels.hip for a streaming launch per seed.  The streaming forms are vector forms, so only the cases whose
    tensors lie on 16-byte boundaries reach them: counted here, per seed (seed 1, seed 2): p2r_depth 4, 4 of 32; points_map 18,
    16; points_to_depth float 11, 9; uint16 14, 10.  The p2r_depth cases hold a batch and a frame with a ragged last quad"""
    sites = ("p2r_depth", "points_map", "points_to_depth_f32", "points_to_depth_u16")
    for seed in S.SEEDS:
        reach = [S.convert_streaming_sites(c) for c in cases["convert"] if c.seed == seed]
        assert all(r <= set(sites) for r in reach)
        count = {s: sum(s in r for r in reach) for s in sites}
        assert count["p2r_depth"] >= 4 and count["points_map"] >= 16 and count["points_to_depth_f32"] >= 9 and count["points_to_depth_u16"] >= 10, (seed, count)
    p2r = [c for c in cases["convert"] if "p2r_depth" in S.convert_streaming_sites(c)]
    assert any(c.n > 1 for c in p2r) and any(c.n == 1 and c.size[0] * c.size[1] % 4 for c in p2r)
    assert all(c.n == 1 or c.size[0] * c.size[1] % 4 == 0 for c in p2r)


def test_convert_three_depth_frames_of_3x3():
    c = S.want(S.depth_stack_case())
    assert c.depth.shape == (3, 3, 3) and c.want["p2r_depth"].shape == (3, 3, 3, 3)
    assert c.want["p2r_depth"][0, 0, 0].tolist() == [-200.0, 200.0, 1000.0] and c.want["p2r_depth"][2, 2, 2].tolist() == [252.0, -252.0, 1260.0]


# ---- cloud, error3d ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["cloud", "error3d"])
def test_frames_draw(kind, cases):
    cs = cases[kind]
    share = np.array([c.valid_share for c in cs])
    assert np.mean((share >= 0.05) & (share <= 0.95)) >= 0.9
    for seed in S.SEEDS:
        mine = [c for c in cs if c.seed == seed]
        px = {c.size[0] * c.size[1] for c in mine}
        assert set(S.PIXELS) <= px | ({6144, 6150} if kind == "error3d" else set()), sorted(set(S.PIXELS) - px)
        big = [c for c in mine if c.size[0] * c.size[1] > S.SCAN_PASS * S.SEGMENT]
        assert len(big) == (1 if kind == "cloud" else 0)
        assert all(c.size[0] <= S.MAX_W and c.size[1] <= S.MAX_H for c in mine if c not in big)
    assert {2047, 2048, 2050} <= set(S.PIXELS) and {7, 8, 9} <= set(S.PIXELS)
    assert {c.n for c in cs} == {1, 2, 3, 4} and all(c.max_batch > c.n and np.isfinite([c.z_min, c.z_max]).all() and c.z_min < c.z_max for c in cs)
    empty = full = 0
    for c in cs:
        pts = c.src.points if kind == "cloud" else c.truth.points
        for f in range(pts.shape[0]):
            v = S.CC.valid_mask(pts[f], c.z_min, c.z_max).mean()
            empty, full = empty + (v == 0), full + (v == 1)
    assert empty >= 1 and full >= 1
    if kind == "cloud":
        assert {c.src.fmt for c in cs} == set(S.FORMATS) and {c.src.off for c in cs} == {0, 1, 2, 3}
        assert {c.organized for c in cs} == {False, True} == {c.negate_z for c in cs} == {c.own_buffer for c in cs}
        assert {c.bgr_frames == 1 for c in cs if c.n > 1} == {False, True} and all(c.divisor > 0 for c in cs)
        assert len({c.divisor for c in cs}) >= 4 and len({(c.z_min, c.z_max) for c in cs}) >= 4
    else:
        assert {c.m for c in cs} == set(range(1, 9)) and all(c.m <= c.max_candidates <= 8 for c in cs)
        assert {c.truth_frames == 1 for c in cs if c.n > 1} == {False, True}
        assert {s.fmt for c in cs for s in c.cands + [c.truth]} == set(S.FORMATS)
        assert all(np.isfinite(st["sum"]) for c in cs for row in c.want for st in row)
