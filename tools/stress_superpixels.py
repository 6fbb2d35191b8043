#!/usr/bin/env python3
"""Randomised parity sweep of the superpixel side (dasp, ers, rgbf, spdsr) against the CPU oracle: the generator and the
comparison of tests/test_gpu_superpixel_sweep.py (tests/superpixel_sweep.py), for longer runs.  Case i of a kind is
superpixel_sweep.case(kind, seed, i), whatever else is run.  Prints one line per case and a summary; exit code 1 on any violation;
--dump DIR keeps the inputs of every call and what the GPU gave of every failing case as DIR/<kind>_s<seed>_i<index>.npz.  Usage
on the GPU box:
    python tools/stress_superpixels.py --cases 200 --seed 3 [--only KIND] [--case I] [--dump DIR] [--library PATH]
--cases N: N cases in all, dealt to the kinds in turn (indices 0 .. of each); with --only all N are KIND's.  --case I: index I alone,
of KIND or of every kind.  --library PATH: another build of libkde_hip.so (a parent commit's, or one with a mutation applied).
One process, no retries: the first status that is not 0 (a HIP error is a refusal, hence a violation) is the result."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def _flat(prefix, v, out):
    if isinstance(v, dict):
        for k, x in v.items():
            _flat(f"{prefix}_{k}", x, out)
    elif isinstance(v, (list, tuple)):
        for k, x in enumerate(v):
            _flat(f"{prefix}_{k}", x, out)
    elif isinstance(v, np.ndarray):
        out[prefix] = v.view(np.uint8) if v.dtype.names else v


def _dump(path, c, got):
    arrays = {}
    for j, call in enumerate(c.calls):
        _flat(f"in_{j}", call.inputs, arrays)
    for j, v in enumerate(got.values()):
        _flat(f"got_{j}", v, arrays)
    np.savez_compressed(path, **arrays)


def run(cases=100, seed=1, only="", case=None, dump="", library=""):
    """-> number of violating cases"""
    if library:
        from kinectdepthmapenhancement_amd import _native
        _native.use_library(library)
    import torch
    import superpixel_sweep as S
    from kinectdepthmapenhancement_amd import filters as F_
    assert torch.cuda.is_available(), "needs a GPU: the HIP path has no CPU fallback"
    kinds = [only] if only else list(S.kinds())
    assert all(k in S.kinds() for k in kinds), f"--only: one of {S.kinds()}"
    todo = [(k, case) for k in kinds] if case is not None else [(kinds[j % len(kinds)], j // len(kinds)) for j in range(cases)]
    violations, ran, t0 = 0, 0, time.time()
    for kind, index in todo:
        c = S.draw(kind, seed, index)
        bad, got = S.run_case(torch, F_, c)
        ran += 1
        print(f"{'FAIL' if bad else 'ok  '} {S.describe(c)}" + (": " + "; ".join(bad) if bad else ""), flush=True)
        if bad:
            violations += 1
            if dump:
                os.makedirs(dump, exist_ok=True)
                _dump(os.path.join(dump, f"{kind}_s{seed}_i{index}.npz"), c, got)
            if any("refused" in b for b in bad):              # a status that is not 0 (a HIP error among them): nothing more runs
                print("stress_superpixels: the library returned an error; stopping")
                break
    print(f"stress_superpixels: seed {seed}, {ran} cases ({', '.join(kinds)}), {violations} violations, {time.time() - t0:.0f} s")
    return violations


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--cases", type=int, default=100)
    ap.add_argument("--seed", type=int, default=3)
    ap.add_argument("--only", default="")
    ap.add_argument("--case", type=int, default=None)
    ap.add_argument("--dump", default="")
    ap.add_argument("--library", default="")
    a = ap.parse_args()
    sys.exit(1 if run(a.cases, a.seed, a.only, a.case, a.dump, a.library) else 0)
