"""The seven depth-in / depth-out stages on the GPU against the numpy statements of their rules, on the seeded draw of
tests/stage_sweep.py: SEEDS x CASES_PER_KIND cases per kind, each with sizes, formats, placement and parameters of its own.

Per case: the bytes of every output frame (for speckle the labels, for holefill pass_of, for temporal the final state, for reg,
undist and decimate the colour call as well), every per-frame count (filled, mixed, removed, components, remaining, the four
temporal counts; speckle's capped is 0), the sentinel bytes in front of and behind the output and behind frame n of an object for
n + 1, and the input unchanged unless the call was in place.  No tolerance: both sides perform the same IEEE binary32 operations
in the same order.  A refusal by create or by a batch call fails the case: the draw holds admitted configurations only
(tests/test_stage_sweep.py creates every one of them and holds the conditions on the draw).

A failure names (kind, seed, index) and the parameters; stage_sweep.case(kind, seed, index) makes that case again alone, and
tools/stress_stages.py --only KIND --seed S --case I runs it.

The statements of the budget, measured on the CPU per kind (80 cases each, drawing them included): reg 0.9 s, undist 0.6 s,
upsample 2.6 s, holefill 4.4 s, speckle 0.5 s, temporal 0.3 s, decimate 0.4 s.  On an MI355X the test of a kind takes 0.3 to 2.2 s,
its statements included."""
import pytest

import stage_sweep as S

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("kind", S.kinds())
def test_byte_exact_on_the_seeded_draw(torch_cuda, kind):
    from kinectdepthmapenhancement_amd import filters as F_
    failures = []
    for seed in S.SEEDS:
        for index in range(S.CASES_PER_KIND):
            c = S.draw(kind, seed, index)
            bad, _ = S.run_case(torch_cuda, F_, c)
            if bad:
                failures.append(S.describe(c) + ": " + "; ".join(bad))
    assert not failures, (len(failures), "cases differ", failures[:5])
