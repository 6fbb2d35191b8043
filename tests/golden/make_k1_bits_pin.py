"""Records tests/golden/k1_bits_pin.npz on the GPU: K1's output bits for the launches of tests/k1_colour_cases.py, with the
inputs next to them.  The committed file was recorded from the commit BEFORE the packed-fma colour code went into
jbf_pk_kernel (one v_lshl_add_u32 per tap then); the change had to keep every bit, and tests/test_gpu_k1_colour_code.py holds
the kernel to these bits from then on.  Re-record only with a change that is meant to alter K1's results.

    python3 tests/golden/make_k1_bits_pin.py [output.npz]"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [ROOT, os.path.dirname(HERE)]


def main():
    import torch
    import k1_colour_cases as K
    from kinectdepthmapenhancement_amd import filters as F

    out = {}
    cases = [K.make_case(w, h) for (w, h) in K.SIZES]
    for si, (bgr, depth) in enumerate(cases):
        out[f"bgr_s{si}"], out[f"depth_s{si}"] = bgr, depth
    for key, si, win, v in K.runs(F.JointBilateralFilter.variants()):
        bgr, depth = cases[si]
        h, w = depth.shape
        p = F.JointBilateralFilter.default_params()
        p.window_size, p.spatial_sigma, p.color_sigma, p.depth_sigma, p.presmooth = win, K.SIGMA_S, K.SIGMA_C, K.SIGMA_D, 0
        jbf = F.JointBilateralFilter(w, h, p)
        jbf.set_variant(v)
        o = torch.empty((1, h, w), dtype=torch.float32, device="cuda")
        jbf.filter_batch(torch.from_numpy(depth[None]).cuda(), torch.from_numpy(bgr[None]).cuda(), o)
        out[key] = o.cpu().numpy()[0]
        print(key, jbf.active_variant(), "nonzero", int(np.count_nonzero(out[key])))
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "k1_bits_pin.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
