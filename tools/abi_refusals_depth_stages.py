#!/usr/bin/env python3
"""The refusals of the four depth-in/depth-out stages (kde_reg_*, kde_undist_*, kde_upsample_*, kde_holefill_*), recorded like
tools/abi_refusals_new.py records its entry points.

    python tools/abi_refusals_depth_stages.py [LIBRARY]    prints the records as JSON (default: the built product library)

Their typed handles keep these entry points out of the enumeration of tools/abi_refusals.py, so they are listed HERE.  The output
for the library as it was before the four families were folded onto one shared core (csrc/kde_depth_stage.h) is
tests/golden/abi_refusals_depth_stages.json; tests/test_depth_stage_refusals.py replays it.  Argument validation precedes every
HIP call and never dereferences a device pointer, so fake addresses serve (0x1000; 0x1001 is no uint16, 0x1002 no float) and
this runs without a GPU.  The order is part of the record: a call that succeeds leaves the previous call's message in place.

  zero    every entry point of the four families with all arguments zero: KDE_ERR_INVALID, except *_destroy(NULL)
  create  each create parameter out of range, one at a time, with a valid out-pointer
  handle  on handles made here, for 4 frames: the calibrations' refusals, the getters before a batch call, a table getter with
          too small a capacity, and every refusal of the batch calls in turn (n, formats, alignments, bgr_frames, the missing
          calibration of reg and undist, holefill's overlap of out_dev with depth_dev)
  valid   one fully valid call of each batch function.  Made only where kde_device_count reports no device: the handle was
          then created without buffers and the answer is KDE_ERR_HIP, "created on a host without a device".  On a host with a
          device these calls would launch kernels on the fake addresses, so they are left out there (tests/test_gpu_*.py make
          them for real).
"""
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tools.abi_refusals import zero_args  # noqa: E402

FAMILIES = ("kde_reg_", "kde_undist_", "kde_upsample_", "kde_holefill_")
A, ODD, HALF = 0x1000, 0x1001, 0x1002       # aligned for both formats; no uint16; a uint16 but no float
FLT_MAX = 3.4028234663852886e38
NAN, INF = float("nan"), float("inf")


def records(path=None):
    from kinectdepthmapenhancement_amd import _native as N
    if path:
        N.use_library(path)
    lib = N.lib()
    F32, U16 = N.KDE_DEPTH_F32, N.KDE_DEPTH_U16
    count = C.c_int(0)
    no_device = lib.kde_device_count(C.byref(count)) != N.KDE_OK or count.value == 0
    out = []

    def record(mode, name, *argv):
        rc = getattr(lib, name)(*argv)
        out.append({"mode": mode, "name": name, "rc": rc, "message": lib.kde_last_error_string().decode()})
        return rc

    def valid(name, *argv):
        if no_device:
            record("valid", name, *argv)

    for name, (_, args) in N.SIGNATURES.items():
        if name.startswith(FAMILIES):
            record("zero", name, *zero_args(args))

    def doubles(*v):
        return (C.c_double * len(v))(*v)

    K = (500.0, 0.0, 10.0, 0.0, 500.0, 6.0, 0.0, 0.0, 1.0)
    I3 = (1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0)

    def with_(k, i, v):
        return doubles(*(k[:i] + (v,) + k[i + 1:]))

    p = C.c_void_p()
    table = (C.c_float * 766)()

    def getters(prefix, h, extra=()):
        for what in ("depth", "filled") + tuple(extra):
            record("handle", f"{prefix}{what}_device", h, C.byref(p))
            record("handle", f"{prefix}{what}_host", h, None, C.byref(p))

    # ---- DepthRegistration ----------------------------------------------------------------------------
    h = N.RegHandle()

    def reg_create(dw=20, dh=13, cw=24, ch=16, batch=4, params=None):
        return record("create", "kde_reg_create", C.byref(h), dw, dh, cw, ch, batch, None if params is None else C.byref(params))

    reg_create(dw=0)
    reg_create(batch=0)
    reg_create(batch=65536)
    reg_create(cw=0)
    reg_create(ch=-1)
    reg_create(dw=(1 << 24) + 1, dh=1)
    reg_create(cw=1, ch=(1 << 24) + 1)
    for params in (N.RegParams(-1.0, FLT_MAX, 0), N.RegParams(NAN, FLT_MAX, 0), N.RegParams(INF, FLT_MAX, 0), N.RegParams(5.0, 5.0, 0),
                   N.RegParams(0.0, NAN, 0), N.RegParams(0.0, FLT_MAX, -1), N.RegParams(0.0, FLT_MAX, 17)):
        reg_create(params=params)
    assert h.value is None and reg_create(params=N.RegParams(100.0, 5000.0, 2)) == N.KDE_OK
    getters("kde_reg_", h)

    def reg_batch(n=2, src=A, dfmt=F32, ofmt=F32, dst=None, mode="handle"):
        argv = ("kde_reg_register_batch", h, n, src, dfmt, ofmt, dst, None)
        return valid(*argv) if mode == "valid" else record(mode, *argv)

    def reg_gather(n=2, src=A, dfmt=F32, bgr=A, frames=1, dst=A, mode="handle"):
        argv = ("kde_reg_color_to_depth_batch", h, n, src, dfmt, bgr, frames, dst, None)
        return valid(*argv) if mode == "valid" else record(mode, *argv)

    reg_batch()                                      # not calibrated ...
    reg_batch(ofmt=7)                                # ... which register_batch reports before a bad output format
    reg_batch(dfmt=7)                                # ... and after a bad depth format
    reg_gather()
    reg_gather(frames=3)
    cal = "kde_reg_set_calibration"
    record("handle", cal, h, None, doubles(*K), doubles(*I3), doubles(0.0, 0.0, 0.0))
    record("handle", cal, h, with_(K, 1, NAN), doubles(*K), doubles(*I3), doubles(0.0, 0.0, 0.0))
    record("handle", cal, h, doubles(*K), with_(K, 8, INF), doubles(*I3), doubles(0.0, 0.0, 0.0))
    record("handle", cal, h, doubles(*K), doubles(*K), with_(I3, 4, 1e300), doubles(0.0, 0.0, 0.0))   # finite, not as a float
    record("handle", cal, h, doubles(*K), doubles(*K), doubles(*I3), doubles(0.0, NAN, 0.0))
    record("handle", cal, h, doubles(*K), doubles(*K), doubles(*I3), doubles(0.0, 0.0, -1e300))
    record("handle", cal, h, with_(K, 0, 1e300), doubles(*K), doubles(*I3), doubles(0.0, 0.0, 0.0))
    record("handle", cal, h, with_(K, 0, 0.0), doubles(*K), doubles(*I3), doubles(0.0, 0.0, 0.0))
    record("handle", cal, h, doubles(*K), with_(K, 4, -500.0), doubles(*I3), doubles(0.0, 0.0, 0.0))
    reg_batch()                                      # still not calibrated
    assert record("handle", cal, h, doubles(*K), doubles(*K), doubles(*I3), doubles(25.0, 0.0, 0.0)) == N.KDE_OK
    reg_batch(src=None)
    for n in (0, -1, 5):
        reg_batch(n=n)
        reg_gather(n=n)
    for fmt in (2, -1):
        reg_batch(dfmt=fmt)
        reg_batch(ofmt=fmt)
        reg_gather(dfmt=fmt)
    reg_batch(src=HALF)
    reg_batch(src=ODD, dfmt=U16)
    reg_batch(dst=HALF)
    reg_batch(dst=ODD, ofmt=U16)
    reg_batch(src=ODD, dfmt=U16, ofmt=7, dst=HALF)   # several things wrong: the first of them
    reg_batch(n=9, src=HALF, ofmt=7)
    reg_gather(src=HALF)
    reg_gather(src=ODD, dfmt=U16)
    reg_gather(bgr=None)
    reg_gather(dst=None)
    for frames in (0, 3, 4, -1):
        reg_gather(frames=frames)
    reg_gather(n=9, frames=3)
    getters("kde_reg_", h)                           # still no call went through
    reg_batch(mode="valid")
    reg_batch(dfmt=U16, ofmt=U16, dst=A, mode="valid")
    reg_gather(frames=2, mode="valid")
    getters("kde_reg_", h)
    record("handle", "kde_reg_destroy", h)

    # ---- LensUndistortion -----------------------------------------------------------------------------
    h = N.UndistHandle()

    def undist_create(sw=20, sh=13, ow=24, oh=16, batch=4, params=None):
        return record("create", "kde_undist_create", C.byref(h), sw, sh, ow, oh, batch, None if params is None else C.byref(params))

    undist_create(sh=0)
    undist_create(batch=0)
    undist_create(ow=-2)
    undist_create(sw=(1 << 24) + 1, sh=1)
    undist_create(ow=(1 << 24) + 1, oh=1)
    for params in (N.UndistParams(-1.0, FLT_MAX, 0, 0.0), N.UndistParams(NAN, FLT_MAX, 0, 0.0), N.UndistParams(7.0, 6.0, 0, 0.0),
                   N.UndistParams(0.0, NAN, 0, 0.0), N.UndistParams(0.0, FLT_MAX, 2, 50.0), N.UndistParams(0.0, FLT_MAX, -1, 50.0),
                   N.UndistParams(0.0, FLT_MAX, 1, 0.0), N.UndistParams(0.0, FLT_MAX, 1, -5.0), N.UndistParams(0.0, FLT_MAX, 1, NAN),
                   N.UndistParams(0.0, FLT_MAX, 1, INF)):
        undist_create(params=params)
    assert h.value is None and undist_create(params=N.UndistParams(100.0, 5000.0, 1, 40.0)) == N.KDE_OK
    getters("kde_undist_", h)

    def undist_batch(n=2, src=A, dfmt=F32, ofmt=F32, dst=None, mode="handle"):
        argv = ("kde_undist_depth_batch", h, n, src, dfmt, ofmt, dst, None)
        return valid(*argv) if mode == "valid" else record(mode, *argv)

    def undist_color(n=2, bgr=A, frames=1, dst=A, mode="handle"):
        argv = ("kde_undist_color_batch", h, n, bgr, frames, dst, None)
        return valid(*argv) if mode == "valid" else record(mode, *argv)

    undist_batch()                                   # not calibrated ...
    undist_batch(ofmt=7)                             # ... which depth_batch reports after a bad output format
    undist_batch(dst=HALF)
    undist_color()
    undist_color(frames=3)                           # ... and color_batch after bgr_frames
    record("handle", "kde_undist_map_device", h, None, C.byref(p))
    cal = "kde_undist_set_calibration"
    D8 = (0.1, -0.05, 0.001, 0.002, 0.01, 0.0, 0.0, 0.0)
    record("handle", cal, h, doubles(*K), None, None)
    record("handle", cal, h, with_(K, 3, NAN), doubles(*D8), None)
    record("handle", cal, h, doubles(*K), doubles(*D8), with_(K, 7, -INF))
    record("handle", cal, h, doubles(*K), with_(D8, 2, NAN), None)
    record("handle", cal, h, doubles(*K), with_(D8, 7, 1e300), None)            # finite, not as a float
    record("handle", cal, h, with_(K, 4, 1e300), doubles(*D8), None)
    record("handle", cal, h, with_(K, 4, 0.0), doubles(*D8), None)
    record("handle", cal, h, doubles(*K), doubles(*D8), with_(K, 0, -1.0))
    undist_batch()                                   # still not calibrated
    assert record("handle", cal, h, doubles(*K), doubles(*D8), None) == N.KDE_OK
    undist_batch(src=None)
    undist_color(bgr=None)
    undist_color(dst=None)
    for n in (0, -1, 5):
        undist_batch(n=n)
        undist_color(n=n)
    for fmt in (2, -1):
        undist_batch(dfmt=fmt)
        undist_batch(ofmt=fmt)
    undist_batch(src=HALF)
    undist_batch(src=ODD, dfmt=U16)
    undist_batch(dst=HALF)
    undist_batch(dst=ODD, ofmt=U16)
    undist_batch(src=ODD, dfmt=U16, ofmt=7, dst=HALF)
    undist_batch(n=9, src=HALF, ofmt=7)
    for frames in (0, 3, 4, -1):
        undist_color(frames=frames)
    undist_color(n=9, frames=3)
    record("handle", "kde_undist_map_device", h, None, None)
    getters("kde_undist_", h)
    undist_batch(mode="valid")
    undist_batch(dfmt=U16, ofmt=U16, dst=A, mode="valid")
    undist_color(frames=2, mode="valid")
    valid("kde_undist_map_device", h, None, C.byref(p))
    getters("kde_undist_", h)
    record("handle", "kde_undist_destroy", h)

    # ---- GuidedDepthUpsampling ------------------------------------------------------------------------
    h = N.UpsampleHandle()

    def upsample_create(sw=10, sh=7, ow=24, oh=16, batch=4, params=None):
        return record("create", "kde_upsample_create", C.byref(h), sw, sh, ow, oh, batch, None if params is None else C.byref(params))

    def upsample_params(radius=2, sigma_color=30.0, max_gap=0.0, z_min=0.0, z_max=FLT_MAX):
        return N.UpsampleParams(radius, sigma_color, max_gap, z_min, z_max)

    upsample_create(sw=0)
    upsample_create(batch=0)
    upsample_create(oh=0)
    upsample_create(sw=(1 << 24) + 1, sh=1, ow=(1 << 24) + 1, oh=1)
    upsample_create(ow=(1 << 24) + 1, oh=1)
    upsample_create(ow=9)
    upsample_create(oh=6)
    for kw in (dict(radius=0), dict(radius=5), dict(sigma_color=0.0), dict(sigma_color=-30.0), dict(sigma_color=NAN), dict(sigma_color=INF),
               dict(max_gap=-1.0), dict(max_gap=NAN), dict(max_gap=INF), dict(z_min=-1.0), dict(z_min=NAN), dict(z_min=INF),
               dict(z_min=9.0, z_max=9.0), dict(z_max=NAN), dict(radius=0, sigma_color=0.0, max_gap=-1.0, z_min=-1.0)):
        upsample_create(params=upsample_params(**kw))
    assert h.value is None and upsample_create(params=upsample_params(3, 12.0, 80.0, 100.0, 5000.0)) == N.KDE_OK
    getters("kde_upsample_", h)
    record("handle", "kde_upsample_range_table", h, None, 766)
    for capacity in (765, 0, -1):
        record("handle", "kde_upsample_range_table", h, table, capacity)
    assert record("handle", "kde_upsample_range_table", h, table, 766) == N.KDE_OK

    def upsample_batch(n=2, src=A, dfmt=F32, bgr=A, frames=1, ofmt=F32, dst=None, mode="handle"):
        argv = ("kde_upsample_depth_batch", h, n, src, dfmt, bgr, frames, ofmt, dst, None)
        return valid(*argv) if mode == "valid" else record(mode, *argv)

    upsample_batch(src=None)
    upsample_batch(bgr=None)
    for n in (0, -1, 5):
        upsample_batch(n=n)
    for frames in (0, 2, 4, -1):
        upsample_batch(n=3, frames=frames)
    for fmt in (2, -1):
        upsample_batch(dfmt=fmt)
        upsample_batch(ofmt=fmt)
    upsample_batch(src=HALF)
    upsample_batch(src=ODD, dfmt=U16)
    upsample_batch(dst=HALF)
    upsample_batch(dst=ODD, ofmt=U16)
    upsample_batch(n=9, src=ODD, dfmt=U16, frames=3, ofmt=7, dst=HALF)     # several things wrong: the first of them
    upsample_batch(src=ODD, dfmt=U16, frames=3, ofmt=7, dst=HALF)
    upsample_batch(src=ODD, dfmt=U16, ofmt=7, dst=HALF)
    upsample_batch(dfmt=U16, ofmt=7, dst=HALF)
    getters("kde_upsample_", h)
    upsample_batch(mode="valid")
    upsample_batch(dfmt=U16, frames=2, ofmt=U16, dst=A, mode="valid")
    upsample_batch(dst=A, mode="valid")                                    # in place is this stage's to allow
    getters("kde_upsample_", h)
    record("handle", "kde_upsample_destroy", h)

    # ---- DepthHoleFilling -----------------------------------------------------------------------------
    h = N.HolefillHandle()
    defaults = dict(radius=2, iterations=8, min_taps=3, sigma_space=2.0, sigma_color=30.0, max_gap=0.0, gap_rule=0, z_min=0.0, z_max=FLT_MAX,
                    passes_per_launch=0)

    def holefill_create(w=20, hgt=13, batch=4, params=None, **kw):
        if kw:
            params = N.HolefillParams(*{**defaults, **kw}.values())
        return record("create", "kde_holefill_create", C.byref(h), w, hgt, batch, None if params is None else C.byref(params))

    holefill_create(w=0)
    holefill_create(batch=0)
    holefill_create(w=(1 << 24) + 1, hgt=1)
    holefill_create(w=1, hgt=(1 << 24) + 1)
    for kw in (dict(radius=0), dict(radius=4), dict(iterations=0), dict(iterations=65), dict(min_taps=0), dict(min_taps=25),
               dict(radius=1, min_taps=9), dict(sigma_space=0.0), dict(sigma_space=NAN), dict(sigma_space=INF), dict(sigma_color=0.0),
               dict(sigma_color=-30.0), dict(sigma_color=NAN), dict(max_gap=-1.0), dict(max_gap=NAN), dict(max_gap=INF), dict(gap_rule=2),
               dict(gap_rule=-1), dict(z_min=-1.0), dict(z_min=NAN), dict(z_min=9.0, z_max=9.0), dict(z_max=NAN), dict(passes_per_launch=-1),
               dict(passes_per_launch=5), dict(radius=0, iterations=0, min_taps=0, sigma_space=0.0, sigma_color=0.0, max_gap=-1.0, gap_rule=2,
                                               z_min=-1.0, passes_per_launch=5)):
        holefill_create(**kw)
    assert h.value is None
    assert holefill_create(radius=3, iterations=5, min_taps=2, sigma_space=1.5, sigma_color=12.0, max_gap=80.0, gap_rule=1, z_min=100.0,
                           z_max=5000.0, passes_per_launch=2) == N.KDE_OK
    getters("kde_holefill_", h, ("remaining",))
    k = C.c_int()
    record("handle", "kde_holefill_passes_per_launch", h, None)
    assert record("handle", "kde_holefill_passes_per_launch", h, C.byref(k)) == N.KDE_OK
    record("handle", "kde_holefill_space_table", h, None, 49)
    record("handle", "kde_holefill_range_table", h, None, 766)
    for capacity in (48, 0, -1):
        record("handle", "kde_holefill_space_table", h, table, capacity)
    for capacity in (765, 0, -1):
        record("handle", "kde_holefill_range_table", h, table, capacity)
    assert record("handle", "kde_holefill_space_table", h, table, 49) == N.KDE_OK
    assert record("handle", "kde_holefill_range_table", h, table, 766) == N.KDE_OK

    def holefill_batch(n=2, src=A, dfmt=F32, bgr=A, frames=1, ofmt=F32, dst=None, pass_of=None, mode="handle"):
        argv = ("kde_holefill_fill_batch", h, n, src, dfmt, bgr, frames, ofmt, dst, pass_of, None)
        return valid(*argv) if mode == "valid" else record(mode, *argv)

    holefill_batch(src=None)
    holefill_batch(bgr=None)
    for n in (0, -1, 5):
        holefill_batch(n=n)
    for frames in (0, 2, 4, -1):
        holefill_batch(n=3, frames=frames)
    for fmt in (2, -1):
        holefill_batch(dfmt=fmt)
        holefill_batch(ofmt=fmt)
    holefill_batch(src=HALF)
    holefill_batch(src=ODD, dfmt=U16)
    holefill_batch(dst=0x10002)
    holefill_batch(dst=0x10001, ofmt=U16)
    frame = 20 * 13
    for dst in (A, A + 4 * frame, A - 4 * (2 * frame - 1), A + 4 * (2 * frame - 1)):       # in place, and partial overlaps
        holefill_batch(dst=dst)
    holefill_batch(dfmt=U16, ofmt=U16, dst=A)
    holefill_batch(dfmt=U16, dst=A + 2 * 2 * frame - 4)                                    # the last two uint16 under the first float
    holefill_batch(n=9, src=ODD, dfmt=U16, frames=3, ofmt=7, dst=ODD)                      # several things wrong: the first of them
    holefill_batch(src=ODD, dfmt=U16, frames=3, ofmt=7, dst=ODD)
    holefill_batch(src=ODD, dfmt=U16, ofmt=7, dst=ODD)
    holefill_batch(dfmt=U16, ofmt=7, dst=ODD)
    holefill_batch(dfmt=U16, ofmt=U16, dst=ODD)
    getters("kde_holefill_", h, ("remaining",))
    holefill_batch(mode="valid")
    holefill_batch(dfmt=U16, frames=2, ofmt=U16, dst=0x10000, pass_of=0x20000, mode="valid")
    holefill_batch(dst=A + 4 * 2 * frame, mode="valid")                                    # the frames just do not overlap
    getters("kde_holefill_", h, ("remaining",))
    record("handle", "kde_holefill_destroy", h)
    return out


if __name__ == "__main__":
    json.dump(records(sys.argv[1] if len(sys.argv) > 1 else None), sys.stdout, indent=1)
    print()
