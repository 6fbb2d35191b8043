#!/usr/bin/env python3
"""Randomised parity sweep of the output side (tail, process, buffer2d, convert, cloud, error3d) against the CPU oracle and the numpy
statements: the generator and the comparison of tests/test_gpu_output_sweep.py (tests/output_sweep.py), for longer runs.  Case i
of a kind is output_sweep.case(kind, seed, i), whatever else is run.  Prints one line per case and a summary; exit code 1 on any
violation; --dump DIR keeps what the GPU gave of every failing case as DIR/<kind>_s<seed>_i<index>.npz.  Usage on the GPU box:
    python tools/stress_outputs.py --cases 200 --seed 3 [--only KIND] [--case I] [--budget] [--dump DIR] [--lib PATH] [--stage-lib PATH]
--cases N: N cases in all, dealt to the kinds in turn (indices 0 .. of each); with --only all N are KIND's.  --case I: index I alone,
of KIND or of every kind.  --budget: the budget of the test (every seed of output_sweep.SEEDS; --seed and --cases are ignored).
--lib PATH: another build of libkde_hip.so (a parent commit's, or one with a mutation applied); --stage-lib PATH: another build of
tools/hooks/libkde_hip_stage.so, which is what the `tail` kind and the hook of the `process` kind run.
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
            _flat(f"{prefix}_{k}".replace(" ", "_").replace(",", ""), x, out)
    elif isinstance(v, (list, tuple)):
        for k, x in enumerate(v):
            _flat(f"{prefix}_{k}", x, out)
    elif isinstance(v, np.ndarray):
        out[prefix] = v.view(np.uint8) if v.dtype.names else v


def run(cases=100, seed=1, only="", case=None, dump="", library="", whole_budget=False, stage_library=""):
    """-> number of violating cases"""
    if library:
        from kinectdepthmapenhancement_amd import _native
        _native.use_library(library)
    if stage_library:                                         # the `tail` kind runs through the stage build's hook
        from tools.hooks import stage
        stage.PATH = os.path.abspath(stage_library)
    import torch
    import output_sweep as S
    from kinectdepthmapenhancement_amd import filters as F_
    assert torch.cuda.is_available(), "needs a GPU: the HIP path has no CPU fallback"
    kinds = [only] if only else list(S.kinds())
    assert all(k in S.kinds() for k in kinds), f"--only: one of {S.kinds()}"
    if whole_budget:
        todo = [(k, s, i) for k in kinds for s, i in S.budget(k)]
    elif case is not None:
        todo = [(k, seed, case) for k in kinds]
    else:
        todo = [(kinds[j % len(kinds)], seed, j // len(kinds)) for j in range(cases)]
    violations, ran, t0, failing, tail = 0, 0, time.time(), {}, {}
    for kind, sd, index in todo:
        c = S.draw(kind, sd, index)
        bad, got = S.run_case(torch, F_, c)
        ran += 1
        for j, call in enumerate(getattr(c, "calls", [])):   # tail: the figures behind the bars, per sweep count
            for fig in got.get(f"call {j}", {}).get("figures", []):
                t = tail.setdefault(call.sweeps, dict(err=0.0, flagged=0, pf_ulps=0.0, frames=0))
                t.update(err=max(t["err"], fig["err"] or 0.0), flagged=max(t["flagged"], fig["flagged"]), pf_ulps=max(t["pf_ulps"], fig["pf_ulps"]),
                         frames=t["frames"] + 1)
        print(f"{'FAIL' if bad else 'ok  '} {S.describe(c)}" + (": " + "; ".join(bad[:4]) if bad else ""), flush=True)
        if bad:
            violations += 1
            failing.setdefault(kind, []).append((sd, index))
            if dump:
                os.makedirs(dump, exist_ok=True)
                arrays = {}
                _flat("got", got, arrays)
                np.savez_compressed(os.path.join(dump, f"{kind}_s{sd}_i{index}.npz"), **arrays)
            if any("refused" in b for b in bad):              # a status that is not 0 (a HIP error among them): nothing more runs
                print("stress_outputs: the library returned an error; stopping")
                break
    for sweeps, t in sorted(tail.items()):
        print(f"stress_outputs: tail x{sweeps}: {t['frames']} frames, largest relative error {t['err']:.3e} (bar {8 * S.TAIL_E32.get(sweeps, 0.0):.3e}), "
              f"most flagged pixels {t['flagged']}, plane_fitted z within {t['pf_ulps']:.2f} ulps")
    for kind, which in failing.items():
        print(f"stress_outputs: {kind}: {len(which)} cases fail: {which}")
    print(f"stress_outputs: {'the budget' if whole_budget else f'seed {seed}'}, {ran} cases ({', '.join(kinds)}), {violations} violations, "
          f"{time.time() - t0:.0f} s")
    return violations


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--cases", type=int, default=100)
    ap.add_argument("--seed", type=int, default=3)
    ap.add_argument("--only", default="")
    ap.add_argument("--case", type=int, default=None)
    ap.add_argument("--budget", action="store_true")
    ap.add_argument("--dump", default="")
    ap.add_argument("--lib", "--library", dest="lib", default="")
    ap.add_argument("--stage-lib", default="")
    a = ap.parse_args()
    sys.exit(1 if run(a.cases, a.seed, a.only, a.case, a.dump, a.lib, a.budget, a.stage_lib) else 0)
