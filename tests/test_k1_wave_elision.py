"""K1's per-wavefront rule elision, the predicate alone (no GPU): tools/elision_census.py restates what jbf_pk_kernel decides
for a wavefront -- from the value ranges of the wavefront's pixels plus the window radius on every side -- and this test
holds it against a brute-force search over every (centre, tap) pair of the region:

  whenever the predicate calls a region free of a rule, no pair in the region trips that rule.

Colour rule: a tap's factor is skipped when its integer colour distance to the centre reaches cd_skip.  Depth rule: it is
skipped when t = fl(fl(d_q - avg_p) * sd) has t^2 >= fl(t_skip^2) (the packed kernels' form).  avg_p is a weighted mean of
the valid depths of p's window with weights the search does not know, rounded in float32: the search takes both ends of what
it can be, the smallest and the largest valid depth of the window, each moved outwards by the rounding bound of the sums,
(taps + 8) / 2 ulps of the largest depth.
Inputs: small random images with planted colour steps (on both sides of cd_skip), depth steps (on both sides of the depth
limit), holes and 50 mm samples; and the large-depth case of ADVICE r02 (1e4 mm at sigma_d = 1 mm), where the float32 rounding
of the average is of the order of the distance to the limit."""
import numpy as np
import pytest

from tools import elision_census as E

F32 = np.float32
FOOTPRINTS = ((32, 8), (64, 4), (16, 8), (8, 8))


def planted(seed, w=48, h=36, base_depth=1500.0, depth_step=400.0, noise=4.0):
    rng = np.random.default_rng(seed)
    bgr = (np.array([90, 140, 60]) + rng.integers(-2, 3, (h, w, 3))).astype(np.int64)
    depth = (base_depth + noise * rng.random((h, w))).astype(F32)
    for _ in range(2):                                     # colour steps: one far above cd_skip = 12170, one just below it
        x, y = rng.integers(0, w - 6), rng.integers(0, h - 6)
        bgr[y:y + 5, x:x + 6] += 100
    x, y = rng.integers(0, w - 4), rng.integers(0, h - 4)
    bgr[y:y + 3, x:x + 3] += np.array([60, 60, 60])        # 3 * 60^2 = 10800 < 12170 (+- the noise)
    x, y = rng.integers(0, w - 8), rng.integers(0, h - 8)
    depth[y:y + 6, x:x + 7] += F32(depth_step)             # a depth step beyond the limit ...
    x, y = rng.integers(0, w - 8), rng.integers(0, h - 8)
    depth[y:y + 4, x:x + 4] += F32(0.6 * depth_step)       # ... and one inside it
    depth[rng.random((h, w)) < 0.02] = 0.0                 # holes
    for _ in range(3):
        depth[rng.integers(0, h), rng.integers(0, w)] = 50.0    # the largest invalid value
    depth[rng.integers(0, h), rng.integers(0, w)] = np.nextafter(F32(50.0), F32(100.0))   # the smallest valid one: far from the rest
    return np.clip(bgr, 0, 255).astype(np.uint8), depth


def brute_force(bgr, depth, x0, y0, fw, fh, window, thr):
    """(some pair trips the colour rule, some pair can trip the depth rule) over the centres of the footprint and their taps"""
    h, w = depth.shape
    r = window // 2
    t2 = float(F32(thr["t_skip"]) * F32(thr["t_skip"]))
    sd = F32(thr["sd"])
    trip_c = trip_d = False
    c = bgr.astype(np.int64)
    for y in range(max(y0, 0), min(y0 + fh, h)):
        for x in range(max(x0, 0), min(x0 + fw, w)):
            ya, yb, xa, xb = max(y - r, 0), min(y + r + 1, h), max(x - r, 0), min(x + r + 1, w)
            cd = ((c[ya:yb, xa:xb] - c[y, x]) ** 2).sum(axis=-1)
            trip_c |= bool((cd >= thr["cd_skip"]).any())
            d = depth[ya:yb, xa:xb].ravel()
            d = d[d > 50.0]
            if d.size == 0:
                continue
            ulp = np.spacing(d.max())
            e = F32(0.5 * (window * window + 8)) * ulp
            for avg in (F32(d.min() - e), F32(d.max() + e)):
                t = (d - avg).astype(F32) * sd
                trip_d |= bool((t.astype(np.float64) ** 2 >= t2).any())
    return trip_c, trip_d


def check_image(bgr, depth, window, thr, footprints=FOOTPRINTS):
    h, w = depth.shape
    seen = {"c_free": 0, "c_need": 0, "d_free": 0, "d_need": 0}
    for fw, fh in footprints:
        grid_c, grid_d = E.census(bgr, depth, fw, fh, window, thr)
        for gy, y0 in enumerate(range(0, h, fh)):
            for gx, x0 in enumerate(range(0, w, fw)):
                need_c, need_d = E.region_needs_rules(bgr, depth, x0, y0, fw, fh, window, thr)
                assert (need_c, need_d) == (bool(grid_c[gy, gx]), bool(grid_d[gy, gx])), "census() and region_needs_rules() disagree"
                trip_c, trip_d = brute_force(bgr, depth, x0, y0, fw, fh, window, thr)
                assert need_c or not trip_c, f"window {window}, region {fw}x{fh} at ({x0}, {y0}): called colour-rule-free, but a pair trips it"
                assert need_d or not trip_d, f"window {window}, region {fw}x{fh} at ({x0}, {y0}): called depth-rule-free, but a pair trips it"
                seen["c_need" if need_c else "c_free"] += 1
                seen["d_need" if need_d else "d_free"] += 1
    return seen


def test_thresholds_are_the_library_s():
    thr = E.thresholds(7.65, 20.0)
    assert thr["cd_skip"] == 12170
    assert abs(float(thr["t_skip"]) / float(thr["sd"]) - 288.4) < 0.1       # the depth limit in mm (tests/k1_colour_cases.py)


@pytest.mark.parametrize("window", [9, 11, 19])
def test_rule_free_regions_hold_no_tripping_pair(window):
    thr = E.thresholds(7.65, 20.0)
    total = {"c_free": 0, "c_need": 0, "d_free": 0, "d_need": 0}
    for seed in range(3):
        bgr, depth = planted(100 * window + seed)
        for k, v in check_image(bgr, depth, window, thr).items():
            total[k] += v
    print(window, total)
    assert min(total.values()) > 0, f"the inputs do not exercise both answers of both predicates: {total}"


def test_regions_without_or_with_one_valid_depth():
    thr = E.thresholds(7.65, 20.0)
    bgr, depth = planted(7)
    depth[:] = 0.0
    assert not E.census(bgr, depth, 32, 8, 11, thr)[1].any()                 # no valid depth: no depth rule anywhere
    depth[10, 20] = 1234.0
    assert not E.census(bgr, depth, 32, 8, 11, thr)[1].any()                 # a single valid depth: range 0
    check_image(bgr, depth, 11, thr, footprints=((32, 8),))
    depth[30, 5] = 30.0                                                      # invalid values do not count
    assert not E.census(bgr, depth, 32, 8, 11, thr)[1].any()
    depth[11, 21] = 1234.0 + 300.0
    assert E.census(bgr, depth, 32, 8, 11, thr)[1].any()


def test_large_depths_small_sigma():
    """depths near 1e4 mm at sigma_d = 1 mm.  The limit is 14.4 mm; one ulp of the depths is 0.001 mm and the
    rounding of the window average up to 65 of them, so ranges within 0.1 mm of the limit must keep the rule."""
    thr = E.thresholds(7.65, 1.0)
    limit = float(thr["t_skip"]) / float(thr["sd"])
    assert 14.3 < limit < 14.5
    rng = np.random.default_rng(5)
    seen = {"d_free": 0, "d_need": 0}
    for k, spread in enumerate([limit - 1.0, limit - 0.2, limit - 0.05, limit - 0.01, limit - 0.001, limit, limit + 0.01]):
        h, w = 24, 40
        bgr = np.full((h, w, 3), 100, np.uint8)
        depth = (1.0e4 + spread * rng.random((h, w))).astype(F32)
        depth[3, 4], depth[15, 30] = F32(1.0e4), F32(1.0e4 + spread)         # the full spread inside one window
        depth[16, 25] = F32(1.0e4 + spread)
        depth[14, 27] = F32(1.0e4)
        s = check_image(bgr, depth, 11, thr, footprints=((32, 8), (16, 8)))
        seen["d_free"] += s["d_free"]
        seen["d_need"] += s["d_need"]
    assert seen["d_free"] > 0 and seen["d_need"] > 0, seen
