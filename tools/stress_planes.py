#!/usr/bin/env python3
"""Randomised parity sweep of the plane chain (normals, nasp, les, proj, chain) against the CPU restatements tools/*_ref.c: the
generator and the comparison of tests/test_gpu_plane_sweep.py (tests/plane_sweep.py), for longer runs.  Case i of a kind is
plane_sweep.case(kind, seed, i), whatever else is run.  Prints one line per case and a summary; exit code 1 on any violation;
--dump DIR keeps the inputs of every call and what the GPU gave of every failing case as DIR/<kind>_s<seed>_i<index>.npz.  Usage on
the GPU box:
    python tools/stress_planes.py --cases 200 --seed 1 [--only KIND] [--case I] [--dump DIR]
--cases N: N cases in all, dealt to the kinds in turn (indices 0 .. of each); with --only all N are KIND's.  --case I: index I alone, of
KIND or of every kind."""
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


def run(cases=100, seed=1, only="", case=None, dump=""):
    """-> number of violating cases"""
    import torch
    import plane_sweep as P
    from kinectdepthmapenhancement_amd import filters as F_
    assert torch.cuda.is_available(), "needs a GPU: the HIP path has no CPU fallback"
    kinds = [only] if only else list(P.kinds())
    assert all(k in P.kinds() for k in kinds), f"--only: one of {P.kinds()}"
    todo = [(k, case) for k in kinds] if case is not None else [(kinds[j % len(kinds)], j // len(kinds)) for j in range(cases)]
    violations, ran, t0 = 0, 0, time.time()
    for kind, index in todo:
        c = P.draw(kind, seed, index)
        bad, got = P.run_case(torch, F_, c)
        ran += 1
        print(f"{'FAIL' if bad else 'ok  '} {P.describe(c)}" + (": " + "; ".join(bad) if bad else ""), flush=True)
        if bad:
            violations += 1
            if dump:
                os.makedirs(dump, exist_ok=True)
                _dump(os.path.join(dump, f"{kind}_s{seed}_i{index}.npz"), c, got)
    print(f"stress_planes: seed {seed}, {ran} cases ({', '.join(kinds)}), {violations} violations, {time.time() - t0:.0f} s")
    return violations


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--cases", type=int, default=100)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--only", default="")
    ap.add_argument("--case", type=int, default=None)
    ap.add_argument("--dump", default="")
    a = ap.parse_args()
    sys.exit(1 if run(a.cases, a.seed, a.only, a.case, a.dump) else 0)
