"""The numpy statement of the DepthTemporalFilter rule (temporal_cases.py) checked on its own, without a GPU: against a scalar
per-pixel Python loop, against outputs worked by hand, and that cutting a sequence into calls changes nothing."""
import numpy as np
import pytest

import temporal_cases as TC

F = np.float32


def _bits(a):
    return np.ascontiguousarray(a).view({4: np.uint32, 2: np.uint16}[a.dtype.itemsize])


@pytest.mark.parametrize("guide", (False, True))
@pytest.mark.parametrize("name", TC.IDS)
def test_statement_equals_the_scalar_loop(name, guide):
    d, g = TC.frames(name)
    p = TC.params(name)
    n, h, w = d.shape
    r = TC.filter_sequence(d, g if guide else None, **p)
    step = max(1, (h * w) // 60)                             # every pixel of the tiny frames, a sixtieth of the others
    counts = np.zeros((n, 4), np.int64)
    for at in range(0, h * w, 1 if h * w <= 64 else step):
        y, x = divmod(at, w)
        outs, value, hist, cnt = TC.scalar_pixel(d[:, y, x], g[:, y, x] if guide else None, **p)
        assert _bits(np.array(outs, np.float32)).tolist() == _bits(r.out[:, y, x]).tolist(), (name, y, x)
        assert _bits(np.array([value], np.float32))[0] == _bits(r.value)[y, x] and hist == int(r.hist[y, x]), (name, y, x)
        counts += np.array(cnt)
    if h * w <= 64:
        assert counts.tolist() == np.stack([r.smoothed, r.jumped, r.held, r.changed], 1).tolist()
    assert r.out.dtype == np.float32 and r.hist.dtype == np.uint32 and r.smoothed.dtype == np.uint32
    r16 = TC.filter_sequence(d, g if guide else None, np.uint16, **p)
    assert r16.out.dtype == np.uint16 and r16.out.tobytes() == TC.depth_to_u16(r.out).tobytes()
    assert r16.value.tobytes() == r.value.tobytes()          # the state is the float, never the uint16 rounding


def test_threshold_by_hand():
    d, _ = TC.frames("threshold")
    r = TC.filter_sequence(d, None, **TC.params("threshold"))
    want = [[1024.0, 1024.0, 1024.0],
            [1156.0, 1289.0, 1155.75],                      # 264 = 8 + 0.25 * 1024: linked; 265: a jump; 263.5: linked
            [1222.0, 1289.0, 1221.625],
            [1123.0, 1024.0, 1221.625],                     # 265 > 8 + 0.25 * 1024 the other way round; a hole held behind 3 frames
            [1205.5, 1289.0, 1254.5625],
            [1246.75, 1289.0, 1271.03125],
            [1267.375, 1289.0, 1279.265625]]
    assert r.out[:, 0, :].tolist() == want
    assert r.smoothed.tolist() == [0, 2, 3, 1, 2, 3, 3]
    assert r.jumped.tolist() == [0, 1, 0, 1, 1, 0, 0]
    assert r.held.tolist() == [0, 0, 0, 1, 0, 0, 0]
    assert r.changed.tolist() == [0] * 7
    assert (r.hist[0] & 0xFF).tolist() == [0x7F, 0x7F, 0x77] and (r.hist >> 8).tolist() == [[0, 0, 0]]


def _one(samples, **kw):
    d = np.array(samples, np.float32).reshape(-1, 1, 1)
    r = TC.filter_sequence(d, None, **dict(TC.DEFAULTS, alpha=1.0, **kw))
    return r.out[:, 0, 0].tolist(), r.held.tolist(), int(r.hist[0, 0])


def test_dropout_by_hand():
    v = 2000.0
    # never hold
    assert _one([v, v, v, 0, 0], persist_min=0)[0] == [v, v, v, 0, 0]
    # one valid frame is enough, and the value is held for exactly eight frames
    out, held, hist = _one([v] + [0] * 10, persist_min=1)
    assert out == [v] + [v] * 8 + [0, 0] and held == [0] + [1] * 8 + [0, 0] and hist == 0
    # three of the last eight: two are not enough; three hold until the first of them leaves the history
    assert _one([v, v, 0, v], persist_min=3)[0] == [v, v, 0, v]
    assert _one([v, v, v] + [0] * 8, persist_min=3)[0] == [v] * 3 + [v] * 6 + [0, 0]
    assert _one([v] * 8 + [0] * 10, persist_min=3)[0] == [v] * 8 + [v] * 6 + [0] * 4
    # eight of eight: the popcount is taken BEFORE this frame's shift (after it, it would be seven and nothing would ever hold)
    assert _one([v] * 8 + [0, 0, v], persist_min=8)[0] == [v] * 8 + [v, 0, v]
    assert _one([v] * 7 + [0], persist_min=8)[0] == [v] * 7 + [0]
    # a held value is a state like any other: the next sample links to it
    r = TC.filter_sequence(np.array([v, v, v, 0, v + 5], np.float32).reshape(-1, 1, 1), None, **dict(TC.DEFAULTS, alpha=0.5))
    assert r.out[:, 0, 0].tolist() == [v, v, v, v, v + 2.5] and r.smoothed.tolist() == [0, 1, 1, 0, 1]
    # the case of the GPU test: pixel k holds a = k % 8 + 1 valid frames and then b = k // 8 + 1 holes
    d, _ = TC.frames("dropout_p1")
    r = TC.filter_sequence(d, None, **TC.params("dropout_p1"))
    flat = r.out.reshape(len(d), -1)
    for k in range(80):
        a, b = k % 8 + 1, k // 8 + 1
        gap = flat[a:a + b, k]
        assert (gap[:8] > 0).all() and (gap[8:] == 0).all(), (k, gap)


def test_colour_by_hand():
    d, g = TC.frames("colour_t48")
    n, h, w = d.shape
    x = np.arange(w)
    fired = (x % 4 == 2) | (x % 4 == 3)                     # 51 and 765 are above 48; 0 and 45 are not
    r = TC.filter_sequence(d, g, **TC.params("colour_t48"))
    assert r.changed.tolist() == [0, 0, 0, 0, int(fired.sum()) * h, 0, 0, 0, 0]    # the first frame fires on an empty state
    top, low = slice(0, h // 2), slice(h // 2, h)
    assert (r.out[4, top][:, fired] == d[4, top][:, fired]).all()                  # the surface starts again at the sample
    assert (r.out[4, top][:, ~fired] != d[4, top][:, ~fired]).all() and r.jumped.tolist() == [0] * n
    assert (r.out[3, low] > 0).all() and int(r.held[3]) == (h - h // 2) * w       # the hole opens: held everywhere
    assert (r.out[4:6, low][:, :, fired] == 0).all() and (r.out[4:6, low][:, :, ~fired] > 0).all()
    assert (r.out[6, low][:, fired] == d[6, low][:, fired]).all()                  # and after the hole the fired pixels start anew
    assert ((r.hist >> 8) == TC.pack_bgr(g[-1])).all()
    # 765: the guide is never consulted -- the depth of a call without a guide; only the stored colour differs
    off = TC.filter_sequence(d, g, **TC.params("colour_t765"))
    none = TC.filter_sequence(d, None, **TC.params("colour_t765"))
    assert off.out.tobytes() == none.out.tobytes() and off.changed.tolist() == [0] * n and (none.hist >> 8 == 0).all()
    # 764: only black to white (765) fires; 0: one level does
    assert TC.filter_sequence(d, g, **TC.params("colour_t764")).changed.tolist() == [0, 0, 0, 0, int((x % 4 == 3).sum()) * h, 0, 0, 0, 0]
    zero = TC.filter_sequence(d, g, **TC.params("colour_t0"))
    flicker = (x >= w // 2) & (x % 4 == 0)
    assert (zero.out[1:, top][:, :, flicker] == d[1:, top][:, :, flicker]).all() and min(zero.changed[1:]) >= int(flicker.sum()) * (h // 2)


@pytest.mark.parametrize("name", TC.IDS)
def test_the_statement_does_not_depend_on_the_cut(name):
    d, g = TC.frames(name)
    p = TC.params(name)
    n = len(d)
    whole = TC.filter_sequence(d, g, **p)
    for cuts in ([1] * n, [4, 1, 4, 8], [2, 7, 8]):
        state, parts, t = None, [], 0
        for c in cuts:
            if t >= n:
                break
            r = TC.filter_sequence(d[t:t + c], g[t:t + c], state=state, **p)
            state, t = (r.value, r.hist), t + c
            parts.append(r)
        assert np.concatenate([q.out for q in parts]).tobytes() == whole.out.tobytes()
        assert state[0].tobytes() == whole.value.tobytes() and state[1].tobytes() == whole.hist.tobytes()
        for k in TC.COUNTS:
            assert np.concatenate([getattr(q, k) for q in parts]).tolist() == getattr(whole, k).tolist()


def test_the_cases_cover_what_they_are_for():
    assert sorted({TC.CASES[k].n for k in TC.IDS}) == [1, 7, 9, 17]
    assert {TC.CASES[k].size for k in TC.IDS} == {(37, 19), (3, 1), (64, 8)}
    d, g = TC.frames("noise")
    r = TC.filter_sequence(d, g, **TC.params("noise"))
    # a contracted multiply-add differs from the three roundings on some of these samples
    prev = np.concatenate([np.zeros_like(r.out[:1]), r.out[:-1]])
    diff = (d - prev).astype(np.float32)
    fused = (prev.astype(np.float64) + np.float64(F(0.4)) * diff.astype(np.float64)).astype(np.float32)    # the product is exact in binary64
    linked = (d > 0) & (prev > 0) & (np.abs(diff) < 10)
    assert int(((fused != r.out) & linked).sum()) > 20
    assert min(r.smoothed[1:]) > 0 and int(r.held.sum()) > 0
    s = TC.filter_sequence(*TC.frames("step"), **TC.params("step"))
    assert int(s.jumped[TC.CASES["step"].n // 2]) > 100 and int(s.jumped[:TC.CASES["step"].n // 2].sum()) == 0
    k = TC.filter_sequence(*TC.frames("spike"), **TC.params("spike"))
    assert int(k.jumped[3]) > 0 and int(k.jumped[4]) > 0
    i, _ = TC.frames("invalid")
    assert np.isnan(i).any() and np.isinf(i).any() and (i < 0).any() and np.isnan(i[2]).all()
    ri = TC.filter_sequence(i, None, **TC.params("invalid"))
    assert np.isfinite(ri.out).all() and ((ri.out == 0) | ((ri.out > 500) & (ri.out < 4000))).all()
    assert TC.as_u16(i).dtype == np.uint16 and TC.as_u16(TC.frames("u16_edges")[0]).max() == 65535
