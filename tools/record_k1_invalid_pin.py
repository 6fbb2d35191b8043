"""Records tests/golden/k1_invalid_taps_pin.npz on the GPU: the sha256 of K1's output bits for every launch of
tests/test_gpu_k1_invalid_taps.py (inputs: tests/k1_invalid_cases.py, seeded generators), the whole output of two of them, and
the launches of the colour-sigma guard.  The committed file was recorded from the commit BEFORE invalid taps got their weight 0
through the colour code (they were removed by a validity factor in the accumulating fma then); the change had to keep every
bit.  Re-record only with a change that is meant to alter K1's results.

    python3 tools/record_k1_invalid_pin.py [output.npz]"""
import hashlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]


def sha(a):
    """sha256 of the float32 bits, as 32 bytes"""
    return np.frombuffer(hashlib.sha256(np.ascontiguousarray(a, np.float32).tobytes()).digest(), np.uint8)


def main():
    import torch
    import k1_invalid_cases as K
    from kinectdepthmapenhancement_amd import filters as F

    out, keys, digests = {}, [], []
    for si, dk, gk in K.case_keys():
        bgr, depth = K.make_case(si, dk, gk)
        for vkey, win, vname in K.VARIANTS:
            key = K.pin_key(si, vkey, dk, gk)
            _, name, got = K.launch(torch, F, bgr, depth, win, vname)
            assert name.startswith(f"w{win}-pk"), (key, name)
            keys.append(key)
            digests.append(sha(got))
            if key in K.FULL_OUTPUTS:
                out["full_" + key] = got
        print(f"s{si} {dk} {gk}: recorded {len(K.VARIANTS)} launches")
    for si in range(len(K.SIZES)):
        bgr, depth = K.make_case(si, "random", "split")
        for gname, sigma, tuned in K.GUARD_SIGMAS:
            _, name, got = K.launch(torch, F, bgr, depth, 11, None, color_sigma=sigma)
            assert name.startswith("w11-pk") == tuned, (gname, sigma, name)
            keys.append(f"guard_s{si}_{gname}")
            digests.append(sha(got))
            print(f"guard s{si} {gname} (sigma_c {sigma:.6g}): {name}, nonzero {int(np.count_nonzero(got))}")
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "tests", "golden", "k1_invalid_taps_pin.npz")
    # keys: one newline-joined string; digests[k] = sha256 of the launch keys[k]
    out["keys"], out["digests"] = np.array("\n".join(keys)), np.stack(digests)
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes,", len(keys), "launches")


if __name__ == "__main__":
    main()
