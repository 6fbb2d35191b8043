"""The inputs of tests/test_gpu_k1_invalid_taps.py (tests/k1_invalid_cases.py) put no tap near a decision, checked on the CPU.

That test holds K1 to the stage-wise oracle bar with band_max = 0: no pixel may be excused to the interval of an open decision.
This only asks what the kernel can give if no tap of the inputs sits near the depth decision |d - avg| = 288.4 mm (sigma_d = 20)
or near the point just below it where a tap's weight S cf exp(-x) passes 2^-150.  Here: the binary64 oracle, at the float32
restatement's own first-pass average, flags no pixel BAND or GRID, and every valid tap of every window keeps 20 mm or more from
that zone -- four orders of magnitude above what a faithful float32 average may differ by (1500 mm x 1e-6)."""
import numpy as np
import pytest

import k1_invalid_cases as K
from oracle import oracle as O

WINDOWS = (3, 11, 19, 23)
X_SKIP = 150.0 * np.log(2.0)             # the depth factor exp(-x) is skipped from here on (it underflows in float32)


@pytest.mark.parametrize("si", range(len(K.SIZES)))
def test_no_tap_near_a_decision(si):
    dden = 2.0 * K.SIGMA_D ** 2
    hi = np.sqrt(dden * X_SKIP)
    assert abs(hi - 288.4) < 0.05
    smallest = np.inf
    for dk in K.DEPTHS:
        for gk in K.GUIDES:
            bgr, depth = K.make_case(si, dk, gk)
            d0 = depth[0]
            h, w = d0.shape
            ys, xs = np.nonzero(d0 > 50.0)
            for win in WINDOWS:
                st = O.jbf_stage(d0, bgr[0], win, K.SIGMA_S, K.SIGMA_C, K.SIGMA_D)
                assert not ((st.flags & (O.Stage.BAND | O.Stage.GRID | O.Stage.MISMATCH)) != 0).any(), (si, dk, gk, win)
                # the zone of |d - avg|: from where the lightest tap's weight (corner of the window, colours 12 apart) reaches
                # 2^-150 up to the depth decision
                r = win // 2
                lo = np.sqrt(dden * (X_SKIP - 2.0 * r * r / (2.0 * K.SIGMA_S ** 2) - 12.0 / (2.0 * K.SIGMA_C ** 2)))
                for ty, tx in zip(ys, xs):                       # every valid tap against the averages of the pixels that see it
                    a = st.avg32[max(0, ty - r):ty + r + 1, max(0, tx - r):tx + r + 1]
                    dd = np.abs(d0[ty, tx] - a[np.isfinite(a)])
                    gap = np.where(dd < lo, lo - dd, dd - hi)
                    smallest = min(smallest, float(gap.min()))
    print(f"frame set {si}: the nearest tap is {smallest:.1f} mm from the decision zone")
    assert smallest > 20.0
