"""The output side on the GPU -- the tail of SPDepthSuperResolution through kde_stage_spdsr_tail and as Process runs it, Buffer2D, DimensionConvertor with
points_to_depth, PointCloudXYZRGB and MeanError3D -- against the CPU oracle and the numpy statements, on the seeded draw of
tests/output_sweep.py: SEEDS x CASES_PER_KIND[kind] cases per kind, each with its own size, parameters, pointer offsets and history.

The bars are those of tests/test_gpu_spdsr_tail.py, tests/test_gpu_stream.py, tests/test_gpu_cloud.py and
tests/test_gpu_error3d.py, none new (output_sweep's docstring lists them per kind).  A refusal by create, SetParametor or a call
fails the case: the draw holds admitted configurations only (tests/test_output_sweep.py holds the conditions on the draw, and pins
the oracle's answer on the named inputs below).

A failure names (kind, seed, index) and the parameters; output_sweep.case(kind, seed, index) makes that case again alone, and
tools/stress_outputs.py --only KIND --seed S --case I runs it.  The named cases below are the smallest inputs of what the sweep
found (EXPERIMENTS.md, "Output sweep").

The references' share of the budget, measured on the CPU per kind, drawing the cases included: tail (28 cases, 45 calls, 99
frames; one of 1024 and one of 1056 clusters per seed) 2.3 s, process (16 cases, 22 calls, 44 frames) 2.3 s, buffer2d (96) 0.1 s, convert (64) 0.1 s, cloud (64, two of 1024 x
520) 0.2 s, error3d (48) 0.3 s.  On an MI355X the test of a kind, references included: tail 2 s, process 0.8 s, buffer2d 0.25 s, convert
0.05 s, cloud 0.25 s, error3d 0.13 s (the first test of a process that touches tools/hooks/libkde_hip_stage.so also pays for
`make` looking at it: 18 - 20 s in a tree without object files)."""
import numpy as np
import pytest

import output_sweep as S

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("kind", S.kinds())
def test_parity_on_the_seeded_draw(torch_cuda, kind):
    from kinectdepthmapenhancement_amd import filters as F_
    failures = []
    for seed, index in S.budget(kind):
        c = S.draw(kind, seed, index)
        bad, _ = S.run_case(torch_cuda, F_, c)
        if bad:
            failures.append(S.describe(c) + ": " + "; ".join(bad[:4]))
            if any("refused" in b for b in bad):              # a status that is not 0, a HIP error among them: nothing more is launched
                break
    assert not failures, (len(failures), "cases differ", failures[:5])


@pytest.mark.parametrize("n", [4, 3])
def test_buffer2d_integer_difference_of_int_min(torch_cuda, n):
    """(int)-1.5 - (int)2^31 is INT_MIN, the reference's abs keeps it and its float is below every limit: the record is averaged.
    Four records take the packed form, three the scalar form, whose code converted the difference as unsigned (+2^31, no
    average) before this test"""
    from kinectdepthmapenhancement_amd import filters as F_
    c = S.int_min_difference_case(n)
    bad, got = S.run_case(torch_cuda, F_, c)
    assert not bad, bad
    raw = got["op 1 update"]["raw"].reshape(-1, 2)
    assert raw[0].tolist() == [715827904.0, 2.0] and raw[1].tolist() == [np.inf, 3.0] and raw[2].tolist() == [-2.0 ** 31, 1.0]


def test_convert_three_depth_frames_of_3x3(torch_cuda):
    """depth [3, 3, 3] with out [3, 3, 3, 3] is three frames, not one cloud"""
    from kinectdepthmapenhancement_amd import filters as F_
    c = S.depth_stack_case()
    bad, got = S.run_case(torch_cuda, F_, c)
    assert not bad, bad
    assert got["p2r_depth"][0, 0, 0].tolist() == [-200.0, 200.0, 1000.0] and got["p2r_depth"][2, 2, 2].tolist() == [252.0, -252.0, 1260.0]
