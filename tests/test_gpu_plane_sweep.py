"""The plane chain on the GPU -- NormalMapGenerator, NormalAdaptiveSuperpixel, LabelEquivalenceSeg, PlaneProjection and the
KinectDepthEnhancement object that composes them -- against the CPU restatements tools/normals_ref.c, nasp_ref.c, les_ref.c and
proj_ref.c, on the seeded draw of tests/plane_sweep.py: SEEDS x CASES_PER_KIND[kind] cases per kind, each with its own size, grid,
parameters, one or two calls on the same object and 1 .. 4 frames per call.

The bars are those of the stages' own tests, none new: normals_cases.check_cm (smoothing map, bad mask and rest normals bit for
bit, CM normals within 1e-4 outside the checker's band, no more pixels beyond than the band holds) and BILATERAL bit for bit;
every NASP output bit for bit; every LES output bit for bit; tools/proj_ref.compare with plane_fitted, strict, hole, band and xy
all 0, window 1 bit for bit.  A batch is compared frame by frame, a second call against the restatement and not against the
first.  A refusal by create, SetParametor or a call fails the case: the draw holds admitted configurations only
(tests/test_plane_sweep.py holds the conditions on the draw).

A failure names (kind, seed, index) and the parameters; plane_sweep.case(kind, seed, index) makes that case again alone, and
tools/stress_planes.py --only KIND --seed S --case I runs it.  The named cases below are the smallest inputs of what the sweep
found (EXPERIMENTS.md, "Plane-chain sweep").

The restatements of the budget, measured on the CPU per kind, drawing the cases included: normals (80 cases) 1.3 - 2.0 s, nasp
(32, two of 1536 and two of 1568 clusters) 4.3 - 5.6 s, les (80) 0.6 s, proj (60) 2.1 - 2.8 s, chain (20) 1.6 s for the draw
(its restatements read the device's results and run with the GPU test).  On an MI355X the test of a kind, restatements
included: normals 1.3 - 1.5 s, nasp 2.0 s, les 0.3 s, proj 1.0 - 1.1 s, chain 1.1 s."""
import numpy as np
import pytest

import plane_sweep as P

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("kind", P.kinds())
def test_parity_on_the_seeded_draw(torch_cuda, kind):
    from kinectdepthmapenhancement_amd import filters as F_
    failures = []
    for seed, index in P.budget(kind):
        c = P.draw(kind, seed, index)
        bad, _ = P.run_case(torch_cuda, F_, c)
        if bad:
            failures.append(P.describe(c) + ": " + "; ".join(bad))
    assert not failures, (len(failures), "cases differ", failures[:5])


def test_nasp_no_iteration_leaves_the_initial_grid_in_ld(torch_cuda):
    """found by the sweep (every drawn case with iteration = 0): initLD_NASP is folded into the first calculateLD_NASP, so a
    Segmentation of no iteration left LD as the call before had it (zeros on a fresh handle).  16 x 8, two superpixels; no
    iteration on the fresh handle, two iterations, none again on the used handle"""
    from kinectdepthmapenhancement_amd import filters as F_
    c = P.nasp_iteration_zero_case()
    bad, got = P.run_case(torch_cuda, F_, c)
    assert not bad, bad
    ld = got["call 2 (single, n 1)"][0]["ld"]
    assert (ld["d"] == np.float32(999999.9)).all() and set(np.unique(ld["l"]).tolist()) == {0, 1}


def test_proj_drawn_case_with_denormal_tap_weights(torch_cuda):
    """found by tools/stress_planes.py --seed 3: `proj`, index 0, a far frame under depth_sigma 150 and spatial_sigma 0.5.  A hole
    whose one tap weighs a unit of 2^-149 leaves its window's range by 0.42 mm in the restatement itself; the BAND bar was the
    range, and is now the range widened by what the rounding of a denormal product can give (tools/proj_ref.BAND_SLACK_MM).
    The smallest such input has its own tests in test_proj_ref.py and test_gpu_proj.py"""
    from kinectdepthmapenhancement_amd import filters as F_
    c = P.draw("proj", 3, 0)
    bad, got = P.run_case(torch_cuda, F_, c)
    assert not bad, (P.describe(c), bad)
    z = float(got["call 0 (batch, n 2)"]["optimized"][0][47, 126, 2])       # the restatement: 2139, under taps from 2139.418
    print(f"proj seed 3 index 0, frame 0 pixel (126, 47): device {z!r}")
