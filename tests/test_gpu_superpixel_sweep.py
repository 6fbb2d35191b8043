"""The superpixel side on the GPU -- DepthAdaptiveSuperpixel, EdgeRefinedSuperpixel, RegionGrowingBilateralFilter and the head of
SPDepthSuperResolution -- against the CPU oracle, on the seeded draw of tests/superpixel_sweep.py: SEEDS x CASES_PER_KIND[kind]
cases per kind, each with its own size, grid, sigmas, iteration count and one or two calls on the same object.

The bars are those of tests/test_gpu_dasp_ers.py, none new (superpixel_sweep's docstring lists them per kind).  A refusal by
create, SetParametor or a call fails the case: the draw holds admitted configurations only (tests/test_superpixel_sweep.py
holds the conditions on the draw, and pins the oracle's answer on the named inputs below).

A failure names (kind, seed, index) and the parameters; superpixel_sweep.case(kind, seed, index) makes that case again alone, and
tools/stress_superpixels.py --only KIND --seed S --case I runs it.  The named cases below are the smallest inputs of what the
sweep was written to find (EXPERIMENTS.md, "Superpixel sweep").

The oracle's share of the budget, measured on the CPU per kind, drawing the cases included: dasp (96 cases, two of 2048 and two
of 2145 clusters) 0.8 s, ers (64) 2.2 s, rgbf (24, two of 2 x 1024 and two of 2 x 1056 clusters) 1.3 s, spdsr (16) 4.3 s.  On an
MI355X the test of a kind, oracle and stage-wise restatements included: dasp 0.6 - 0.7 s, ers 3.0 s, rgbf 1.6 - 2.0 s, spdsr
2.7 - 3.9 s (the first test of a process that touches tools/hooks/libkde_hip_stage.so also pays for `make` looking at it)."""
import numpy as np
import pytest

import superpixel_sweep as S

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("kind", S.kinds())
def test_parity_on_the_seeded_draw(torch_cuda, kind):
    from kinectdepthmapenhancement_amd import filters as F_
    failures = []
    for seed, index in S.budget(kind):
        c = S.draw(kind, seed, index)
        bad, _ = S.run_case(torch_cuda, F_, c)
        if bad:
            failures.append(S.describe(c) + ": " + "; ".join(bad))
            if any("refused" in b for b in bad):              # a status that is not 0, a HIP error among them: nothing more is launched
                break
    assert not failures, (len(failures), "cases differ", failures[:5])


def test_dasp_no_iteration_leaves_the_initial_grid_in_ld(torch_cuda):
    """DESIGN.md listed it as an open defect: init_LD is folded into the first calculateLD, so a Segmentation of no iteration
    left LD as the call before had it.  16 x 8, two superpixels; no iteration on the fresh handle (labels 0, as SetParametor
    leaves them), two iterations, none again on the used handle (the labels of the call before)"""
    from kinectdepthmapenhancement_amd import filters as F_
    c = S.iteration_zero_case()
    bad, got = S.run_case(torch_cuda, F_, c)
    assert not bad, bad
    for tag in ("call 0", "call 2"):
        ld = got[tag]["ld"]
        assert (ld["d"] == np.float32(999999.9)).all() and set(np.unique(ld["l"]).tolist()) == {0, 1}
    assert not got["call 0"]["labels"].any() and np.array_equal(got["call 2"]["labels"], got["call 1"]["labels"])


@pytest.mark.parametrize("depth_on", [True, False])
def test_dasp_infinite_pixel_takes_the_trees_first_candidate(torch_cuda, depth_on):
    """one z = +inf: every candidate distance of the pixel is +inf (depth sigma 200) or inf * 0 = NaN (depth sigma 0).  The
    reference's tree starts from candidate 0 and a NaN neither replaces nor is replaced: label 15.  A scan that starts from
    (+inf, own cell) with a strict '<' returns the own cell, 41"""
    from kinectdepthmapenhancement_amd import filters as F_
    c = S.infinite_pixel_case(depth_on)
    bad, got = S.run_case(torch_cuda, F_, c)
    assert not bad, bad
    ld = got["call 0"]["ld"][30, 40]
    assert int(ld["l"]) == 15 and (np.isposinf(ld["d"]) if depth_on else np.isnan(ld["d"]))


def test_dasp_infinite_cluster_centre(torch_cuda):
    """a cluster whose sampled centre is +inf: every pixel that sees it has a +inf candidate, its own pixels a NaN one"""
    from kinectdepthmapenhancement_amd import filters as F_
    c = S.infinite_centre_case()
    bad, got = S.run_case(torch_cuda, F_, c)
    assert not bad, bad
