"""The streaming (non-temporal) twins of the size-selected kernels at the shapes of the seeded sweeps.

Twelve launch sites (csrc/kde_internal.h: CacheSite; DESIGN.md, "Size-selected paths") launch another instantiation of their
kernel once a call moves more than 256 MiB: non-temporal loads and stores, nothing else.  Those are the kernels the benchmark
shapes run, and no frame a correctness test can afford reaches them.  The stage build (tools/hooks/libkde_hip_stage.so) takes
the threshold from kde_stage_set_cache_bytes and counts, per site, the launches of the streaming form, so the cases of the
sweeps -- ragged tails, misaligned frames of a batch, uint16 sources, hostile values -- run here once more with the threshold at 0:

  convert, cloud, error3d     tests/output_sweep.py, every (seed, index) of its budget
  reg, undist, temporal       tests/stage_sweep.py, likewise
  mesh                        the frames of mesh_cases.frames(w, h) at test_gpu_mesh.SMALL as tests/test_gpu_mesh.py runs them:
                              every named frame under the three diagonals (both links), the three source formats with the two
                              shifted maps, three frames at a misaligned place of a batch; a size stands for a seed

Per case, inside stage_library(): the case with the default threshold and again with threshold 0, both through the kind's own
run_case (the mesh: against the statement and the cloud call, as _build_and_check does) under its existing bars -- no new
tolerance; every array, count and table the two runs return equal byte for byte (NaN payloads, sentinel-filled slack); the first
case of every seed also on the product library, equal to the default run byte for byte (the rule of include/kde_test_hooks.h).
After every default run every counter is 0; after a seed's streaming runs exactly the kind's sites have counted, each at least
once.  The sites of csrc/stream_kernels.hip stream in their vector forms only: tests/test_output_sweep.py counts the `convert`
cases that reach them (4 of 32 per seed for launch_p2r_any).

A failure names (kind, seed, index); output_sweep.case / stage_sweep.case make the case again alone.

On an MI355X, statements included: convert 0.08 s, cloud 0.48 s, error3d 0.14 s, reg 0.73 s, undist 0.44 s, temporal 0.42 s, each
of the three temporal shapes 0.5 s, the mesh 0.25 s -- about twice the sweep's own test of the kind (the first test of a process that touches tools/hooks/libkde_hip_stage.so also
pays for `make` looking at it: 18 - 20 s in a tree without object files)."""
import numpy as np
import pytest

import cloud_cases as CC
import mesh_cases as MC
import output_sweep as OS
import stage_sweep as SS
import test_gpu_mesh as TM
from gpu_util import dev

pytestmark = pytest.mark.gpu

# kind -> (the sweep's module, the sites whose streaming form the kind launches: tools/hooks/stage.py SITES)
KINDS = {
    "convert": (OS, ("p2r_depth", "points_map", "points_to_depth_f32", "points_to_depth_u16")),
    "cloud": (OS, ("cloud",)),
    "error3d": (OS, ("error3d",)),
    "reg": (SS, ("reg", "reg_gather")),
    "undist": (SS, ("undist_color", "undist_depth")),
    "temporal": (SS, ("temporal",)),
}
MESH_SITES = ("cloud", "mesh")                                # launch_mesh takes its vertices from launch_cloud


def _budget(kind):
    S = KINDS[kind][0]
    return OS.budget(kind) if S is OS else [(seed, index) for seed in SS.SEEDS for index in range(SS.CASES_PER_KIND)]


def _differ(a, b, where="result"):
    """None, or where two results of run_case differ on their bytes"""
    if isinstance(a, dict) and isinstance(b, dict):
        if sorted(a, key=str) != sorted(b, key=str):
            return f"{where}: keys {sorted(a, key=str)} against {sorted(b, key=str)}"
        return next((d for d in (_differ(a[k], b[k], f"{where}[{k!r}]") for k in a) if d), None)
    if isinstance(a, (list, tuple)) and isinstance(b, (list, tuple)):
        if len(a) != len(b):
            return f"{where}: {len(a)} items against {len(b)}"
        return next((d for d in (_differ(x, y, f"{where}[{i}]") for i, (x, y) in enumerate(zip(a, b))) if d), None)
    if isinstance(a, np.ndarray) or isinstance(b, np.ndarray):
        a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
        if a.dtype != b.dtype or a.shape != b.shape:
            return f"{where}: {a.dtype} {a.shape} against {b.dtype} {b.shape}"
        if a.tobytes() != b.tobytes():
            raw = lambda v: np.frombuffer(v.tobytes(), np.uint8)
            at = np.flatnonzero(raw(a) != raw(b))
            return f"{where}: {at.size} of {a.nbytes} bytes differ, the first at byte {int(at[0])}"
        return None
    return None if a == b or (a != a and b != b) else f"{where}: {a!r} against {b!r}"


def _no_launch(counts):
    return [s for s, k in counts.items() if k]


def _run_budget(torch, F_, cases, run, describe, sites):
    """cases: [(seed, case)] in the order of the budget; run(case) -> (violations, got).  Per case the product library (the
    first of a seed only), the stage build with the default threshold and with threshold 0; the counters as the docstring says"""
    from tools.hooks import stage
    failures = []
    seeds = sorted({seed for seed, _ in cases})
    for seed in seeds:
        first = True
        with stage.stage_library() as ctl:
            ctl.streaming_launches()
        streamed = dict.fromkeys(stage.SITES, 0)
        for _, c in (sc for sc in cases if sc[0] == seed):
            bad = []
            product = run(c) if first else None
            with stage.stage_library() as ctl:
                default = run(c)
                counted = _no_launch(ctl.streaming_launches())
                if counted:
                    bad.append(f"the default threshold launched the streaming form of {counted}")
                ctl.set_cache_bytes(0)
                streaming = run(c)
                for s, k in ctl.streaming_launches().items():
                    streamed[s] += k
            for name, r in (("product", product), ("default", default), ("streaming", streaming)):
                bad += [f"{name}: {v}" for v in r[0][:3]] if r is not None else []
            d = _differ(default[1], streaming[1], "streaming against default")
            if d:
                bad.append(d)
            if first:
                d = _differ(product[1], default[1], "stage build against product")
                if d:
                    bad.append(d)
            first = False
            if bad:
                failures.append(describe(c) + ": " + "; ".join(bad))
                if any("refused" in b for b in bad):          # a status that is not 0, a HIP error among them: nothing more is launched
                    assert not failures, failures
        missed = [s for s in sites if streamed[s] < 1]
        other = [s for s in stage.SITES if s not in sites and streamed[s]]
        if missed or other:
            failures.append(f"seed {seed}: no streaming launch at {missed}, launches at {other} (of {streamed})")
    assert not failures, (len(failures), "cases differ", failures[:5])


@pytest.mark.parametrize("kind", list(KINDS))
def test_streaming_forms_on_the_seeded_draw(torch_cuda, kind):
    from kinectdepthmapenhancement_amd import filters as F_
    S, sites = KINDS[kind]
    cases = [(seed, S.draw(kind, seed, index)) for seed, index in _budget(kind)]
    _run_budget(torch_cuda, F_, cases, lambda c: S.run_case(torch_cuda, F_, c), S.describe, sites)


class _Shaped:
    """the filters module, whose DepthTemporalFilter objects run in a given shape (pixels per thread, frames loaded ahead)"""

    def __init__(self, F_, pixels, unroll):
        self._F, self._shape = F_, (pixels, unroll)

    def __getattr__(self, name):
        return getattr(self._F, name)

    def DepthTemporalFilter(self, *a, **kw):
        o = self._F.DepthTemporalFilter(*a, **kw)
        o.set_shape(*self._shape)
        return o


@pytest.mark.parametrize("pixels,unroll", [(2, 4), (4, 2), (8, 1)])
def test_streaming_stores_of_the_temporal_shapes(torch_cuda, pixels, unroll):
    """temporal_shape gives a thread one pixel until a frame has 512 000 of them, so the sweep's frames take the element stores
    and never the 8- and 16-byte streaming stores of 2, 4 and 8 pixels per thread, which 1080p runs (8 pixels).  The same budget
    with the shape set: whole groups on aligned frames take the vector store, ragged tails and the frames of a batch that start
    off a boundary the element stores"""
    from kinectdepthmapenhancement_amd import filters
    F_ = _Shaped(filters, pixels, unroll)
    cases = [(seed, SS.draw("temporal", seed, index)) for seed, index in _budget("temporal")]
    _run_budget(torch_cuda, F_, cases, lambda c: SS.run_case(torch_cuda, F_, c), SS.describe, KINDS["temporal"][1])


# ---- the mesh -----------------------------------------------------------------------------------------------------------
def _mesh_call(torch, F, w, h, g, src, bgr, mode, frames, tri_shift, what):
    """one kde_mesh_build_batch into sentinel-filled buffers under the comparisons of test_gpu_mesh._build_and_check: counts
    and vertex bytes against the cloud call on the same inputs, triangles and their counts against the statement, nothing
    written around them -> (violations, everything the call wrote)"""
    n = len(frames)
    slot = 2 * (w - 1) * (h - 1)
    bad = []
    M = F.OrganizedMesh(w, h, max_batch=n, diagonal=mode, **g["link"])
    try:
        M.set_camera(g["K"])
        vout = TM._sentinel(torch, (n, w * h, 16))
        flat = TM._sentinel(torch, (n * slot * 12 + 16,))
        tout = flat[tri_shift:tri_shift + n * slot * 12].view(n, slot, 12)
        M.build(src, bgr, vout, tout)
        counts, tri_counts = M.counts(), M.tri_counts()
        cloud, ccounts = TM._cloud_bytes(torch, F, w, h, src, bgr, n)
        got = dict(vertices=vout.cpu().numpy(), triangles=flat.cpu().numpy(), counts=counts, tri_counts=tri_counts, cloud=cloud.cpu().numpy())
        if not np.array_equal(counts, ccounts) or counts.tolist() != [int(MC.valid_mask(g["z"][f]).sum()) for f in frames]:
            bad.append(f"{what}: counts {counts.tolist()}, the cloud's {ccounts.tolist()}")
        if not torch.equal(vout, cloud):
            bad.append(f"{what}: the vertex bytes are not the cloud's")
        try:
            TM._check_triangles(tout.cpu().numpy(), tri_counts, [TM._want(g, mode)[f] for f in frames], what)
        except AssertionError as e:
            bad.append(f"{what}: {e}")
        if not (torch.all(flat[:tri_shift] == TM.SENTINEL) and torch.all(flat[tri_shift + n * slot * 12:] == TM.SENTINEL)):
            bad.append(f"{what}: bytes around the triangles were written")
    finally:
        M.close()
    return bad, got


def _mesh_cases(torch, w, h):
    """[(name, arguments of _mesh_call behind F, w, h)] of one size; the device tensors are made once and shared"""
    out = []
    for g in TM._inputs(w, h):                                # every named frame, both links, the three diagonals
        src, bgr = dev(torch, g["pts"]), dev(torch, g["bgr"])
        frames = list(range(len(g["names"])))
        out += [(f"named, link {g['link']}, diagonal {mode}", (g, src, bgr, mode, frames, 0)) for mode in TM.MODES]
    n = 3                                                     # the three source formats, the maps also one element off
    z = np.stack([MC.noisy(w, h, 40 + f) for f in range(n)])
    z[0].reshape(-1)[:3] = (0.0, 65535.0, 49.0)
    K = CC.camera(w, h)
    g = dict(link={}, names=[f"noisy{f}" for f in range(n)], z=z, K=K, want={})
    bgr = dev(torch, CC.bgr_images(3, n, h, w))
    u16 = z.astype(np.uint16).view(np.int16)
    sources = [dev(torch, np.stack([MC.as_points(zz, K) for zz in z])), dev(torch, z), dev(torch, u16),
               TM._shifted(torch, z, torch.float32), TM._shifted(torch, u16, torch.int16)]
    out += [(f"source {i} {src.dtype}", (g, src, bgr, MC.DIAG_ADAPTIVE, list(range(n)), 0)) for i, src in enumerate(sources)]
    g = TM._inputs(w, h)[0]                                   # a misaligned place of a batch: cloud, image and triangles shifted
    pick = [g["names"].index(name) for name in ("salt", "noisy0", "nan_inf")]
    pts, img = g["pts"][pick], g["bgr"][pick]
    out.append(("shifted", (g, TM._shifted(torch, pts, torch.float32), TM._shifted(torch, img, torch.uint8), MC.DIAG_ADAPTIVE, pick, 4)))
    out.append(("shifted by 8 bytes", (g, TM._shifted(torch, pts, torch.float32, 2), TM._shifted(torch, img, torch.uint8, 8), MC.DIAG_ADAPTIVE, pick, 8)))
    return out


def test_streaming_forms_of_the_mesh(torch_cuda):
    from kinectdepthmapenhancement_amd import filters as F
    torch = torch_cuda
    cases = [((w, h), (w, h, name, args)) for w, h in TM.SMALL for name, args in _mesh_cases(torch, w, h)]
    _run_budget(torch, F, cases, lambda c: _mesh_call(torch, F, c[0], c[1], *c[3], what=c[2]), lambda c: f"mesh {c[0]} x {c[1]}, {c[2]}", MESH_SITES)
