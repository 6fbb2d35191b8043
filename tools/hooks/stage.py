"""Loader of tools/hooks/libkde_hip_stage.so (include/kde_test_hooks.h): the product library's own sources compiled with
-DKDE_STAGE_HOOKS -- same ABI, plus kde_stage_set(), kde_stage_spdsr_tail(), kde_stage_set_cache_bytes() and
kde_stage_streaming_launches().  Test infrastructure only.

    with stage_library() as ctl:          # inside the block kinectdepthmapenhancement_amd.filters talks to the stage build
        ctl.set(jbf_avg=tensor)           # K1 dumps its first-pass average there
        ...run filters.JointBilateralFilter as usual...

Handles created inside the block must be closed inside it (a handle belongs to the library that made it).
"""
from __future__ import annotations

import contextlib
import ctypes as C
import os
import subprocess

_HERE = os.path.dirname(os.path.abspath(__file__))
PATH = os.path.join(_HERE, "libkde_hip_stage.so")
_lib = None


def lib() -> C.CDLL:
    global _lib
    if _lib is None:
        subprocess.check_call(["make", "-C", _HERE, "-s", "-j8", "libkde_hip_stage.so"])     # no-op when up to date
        from kinectdepthmapenhancement_amd import _native
        l = C.CDLL(PATH)
        for name, (res, args) in _native.SIGNATURES.items():
            fn = getattr(l, name)
            fn.restype = res
            fn.argtypes = args
        l.kde_stage_set.restype = C.c_int
        l.kde_stage_set.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]
        l.kde_stage_spdsr_tail.restype = C.c_int
        l.kde_stage_spdsr_tail.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
        l.kde_stage_set_cache_bytes.restype = C.c_int
        l.kde_stage_set_cache_bytes.argtypes = [C.c_size_t]
        l.kde_stage_streaming_launches.restype = C.c_int
        l.kde_stage_streaming_launches.argtypes = [C.POINTER(C.c_uint64), C.c_int]
        _lib = l
    return _lib


CACHE_BYTES = 256 << 20         # csrc/kde_internal.h: kCacheBytes
# enum kde_stage_site (include/kde_test_hooks.h), in its order
SITES = ("p2r_depth", "points_map", "points_to_depth_f32", "points_to_depth_u16", "cloud", "mesh", "error3d", "undist_color",
         "undist_depth", "reg", "reg_gather", "temporal")


class StageCtl:
    def __init__(self, l):
        self._l = l

    def set(self, jbf_avg=None, ers_avg=None, ers_dev=None, counters=None, force_full_rules=False):
        """torch CUDA tensors (float32 sinks, int32[8] counters) or None.
        counters[0..3]: how often each rule-specialised body ran (bit 0 = colour rule, bit 1 = depth rule).  K1's packed
        kernels count once per WAVEFRONT that owns at least one pixel (lane 0 of the wavefront; a wavefront wholly outside the
        image does not count) -- they decide per wavefront, so the total depends on the kernel variant's wavefront footprint.
        counters[4..7] are K10's, once per tile (include/kde_test_hooks.h)."""
        p = lambda t: None if t is None else t.data_ptr()
        rc = self._l.kde_stage_set(p(jbf_avg), p(ers_avg), p(ers_dev), p(counters), 1 if force_full_rules else 0)
        if rc:
            raise RuntimeError(f"kde_stage_set failed ({rc})")

    def set_cache_bytes(self, nbytes=CACHE_BYTES):
        """the threshold above which a call takes the streaming (non-temporal) twin of its kernels; 0: every call does"""
        rc = self._l.kde_stage_set_cache_bytes(nbytes)
        if rc:
            raise RuntimeError(f"kde_stage_set_cache_bytes failed ({rc})")

    def streaming_launches(self):
        """{site: launches of its streaming form since the last call}, all of SITES; zeroes the counters"""
        buf = (C.c_uint64 * len(SITES))()
        rc = self._l.kde_stage_streaming_launches(buf, len(SITES))
        if rc:
            raise RuntimeError(f"kde_stage_streaming_launches failed ({rc})")
        return dict(zip(SITES, (int(v) for v in buf)))

    def clear(self):
        self._l.kde_stage_set(None, None, None, None, 0)
        self._l.kde_stage_set_cache_bytes(CACHE_BYTES)
        self._l.kde_stage_streaming_launches(None, 0)


@contextlib.contextmanager
def stage_library():
    from kinectdepthmapenhancement_amd import _native
    l = lib()
    prev = _native._lib
    _native._lib = l
    ctl = StageCtl(l)
    try:
        yield ctl
    finally:
        ctl.clear()
        _native._lib = prev


def bits_equal(a, b) -> bool:
    """float32 arrays equal to the bit (NaN payloads included)"""
    import numpy as np
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def jbf_stage_run(params, depth, guide, variant=-1, force_full_rules=False):
    """K1 on the stage build: depth [n,H,W] f32, guide [n,H,W,3] u8 (numpy) -> (out, avg, counters) numpy.
    `guide` is the image K1 is guided by (the smoothed one when K0 runs in the product call)."""
    import numpy as np
    import torch
    from kinectdepthmapenhancement_amd import filters
    n, h, w = depth.shape
    d = torch.from_numpy(np.ascontiguousarray(depth, np.float32)).cuda()
    g = torch.from_numpy(np.ascontiguousarray(guide, np.uint8)).cuda()
    out = torch.empty((n, h, w), dtype=torch.float32, device="cuda")
    avg = torch.full((n, h, w), -1.0, dtype=torch.float32, device="cuda")
    cnt = torch.zeros(8, dtype=torch.int32, device="cuda")
    with stage_library() as ctl:
        jbf = filters.JointBilateralFilter(w, h, params, max_batch=n)
        try:
            jbf.set_variant(variant)
            ctl.set(jbf_avg=avg, counters=cnt, force_full_rules=force_full_rules)
            jbf.filter_batch(d, g, out)
            torch.cuda.synchronize()
        finally:
            jbf.close()
    return out.cpu().numpy(), avg.cpu().numpy(), cnt.cpu().numpy()


def ers_stage_run(color_labels, depth_labels, depth, bgr, variant=0, force_full_rules=False):
    """EdgeRefinedSuperpixel::EdgeRefining on the stage build -> dict(labels, edge_depth, depth, avg, dev, counters)"""
    import numpy as np
    import torch
    from kinectdepthmapenhancement_amd import filters
    h, w = depth.shape
    t = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a, dt)).cuda()
    avg = torch.full((h, w), -1.0, dtype=torch.float32, device="cuda")
    dev = torch.full((h, w), -1.0, dtype=torch.float32, device="cuda")
    cnt = torch.zeros(8, dtype=torch.int32, device="cuda")
    with stage_library() as ctl:
        ers = filters.EdgeRefinedSuperpixel(w, h)
        try:
            ers.set_variant(variant)
            ctl.set(ers_avg=avg, ers_dev=dev, counters=cnt, force_full_rules=force_full_rules)
            ers.EdgeRefining(t(color_labels, np.int32), t(depth_labels, np.int32), t(depth, np.float32), t(bgr, np.uint8))
            torch.cuda.synchronize()
            res = {"labels": ers.getRefinedLabels_Device().cpu().numpy(), "edge_depth": ers.getEdgeStageDepth_Device().cpu().numpy(),
                   "depth": ers.getRefinedDepth_Device().cpu().numpy()}
        finally:
            ers.close()
    res.update(avg=avg.cpu().numpy(), dev=dev.cpu().numpy(), counters=cnt.cpu().numpy())
    return res


def spdsr_tail_calls(width, height, rows, cols, K, calls, max_batch):
    """kde_stage_spdsr_tail (include/kde_test_hooks.h), the calls in order on ONE fresh SPDepthSuperResolution handle of the stage
    build.  A call is a dict: labels [n,H,W] int32, points [n,H,W,3] float32, nd None (fit the planes) or [n,k,4] float32 (use
    these), sweeps.  -> per call (nd [n,k,4], plane_fitted [n,H,W,3], optimized [n,H,W,3]) numpy, as the handle held them after
    that call (a marker (5,5,5) keeps the w the frame slot held before it)."""
    import numpy as np
    import torch
    from kinectdepthmapenhancement_amd import _native, filters
    t = lambda a: torch.from_numpy(a).cuda()
    k, out = rows * cols, []
    with stage_library():
        sp = filters.SPDepthSuperResolution(width, height, max_batch=max_batch)
        try:
            sp.SetParametor(rows, cols, K)
            for call in calls:
                lab = np.ascontiguousarray(call["labels"], np.int32).reshape((-1, height, width))
                n = lab.shape[0]
                pts = np.ascontiguousarray(call["points"], np.float32).reshape((n, height, width, 3))
                planes = call.get("nd")
                # the tensors stay referenced until the synchronize below
                args = [t(lab), t(pts)] + ([t(np.ascontiguousarray(planes, np.float32).reshape((n, k, 4)))] if planes is not None else [])
                _native.check(lib().kde_stage_spdsr_tail(sp._h, n, args[0].data_ptr(), args[1].data_ptr(),
                                                         args[2].data_ptr() if planes is not None else None, call["sweeps"], filters._stream()))
                sp._n = n
                torch.cuda.synchronize()
                out.append((sp.getClusterND_Device().cpu().numpy().reshape((n, k, 4)).copy(),
                            sp.getPlaneFitted3D_Device().cpu().numpy().reshape((n, height, width, 3)).copy(),
                            sp.getOptimizedPoints_Device().cpu().numpy().reshape((n, height, width, 3)).copy()))
        finally:
            sp.close()
    return out


def spdsr_tail_run(width, height, rows, cols, K, labels, points, nd=None, sweeps=20, max_batch=None, nd_prev_call=None):
    """spdsr_tail_calls for one call on a fresh handle:
    labels [H,W] or [n,H,W] int32, points [...,3] float32, nd None (fit the planes) or [k,4] / [n,k,4] float32 (use these).
    nd_prev_call = {"labels": ..., "points": ...} of a first call on the SAME handle with the planes fitted and no sweeps;
    its planes are stored under nd_prev_call["nd"] (the (5,5,5) marker of the second call keeps that call's w).
    -> (nd, plane_fitted, optimized) numpy, with a leading n only when labels has one."""
    import numpy as np
    lab = np.ascontiguousarray(labels, np.int32)
    batched = lab.ndim == 3
    lab = lab.reshape((-1, height, width))
    n = lab.shape[0]
    calls = [dict(labels=lab, points=points, nd=nd, sweeps=sweeps)]
    if nd_prev_call is not None:
        calls.insert(0, dict(labels=nd_prev_call["labels"], points=nd_prev_call["points"], nd=None, sweeps=0))
    res = spdsr_tail_calls(width, height, rows, cols, K, calls, n if max_batch is None else max_batch)
    if nd_prev_call is not None:
        first = res[0][0]
        nd_prev_call["nd"] = first[0] if first.shape[0] == 1 else first
    return tuple(r if batched else r[0] for r in res[-1])
