#!/usr/bin/env python3
"""The calls libkde_hip.so refuses before it touches HIP, with the return code and the message each one leaves.

    python tools/abi_refusals.py [LIBRARY]        prints the records as JSON (default: the built product library)

Argument validation precedes every HIP call, so this runs without a GPU.  tests/golden/abi_refusals.json is the output
for the library as it was before the entry points were split into several files; tests/test_capi_symbols.py replays the
same calls, in the same order, against the library under test and requires the same codes and the same messages.
The order is part of the record: a call that succeeds leaves the previous call's message in place.

  zero    every int-returning entry point whose first argument is a handle or an out-pointer, all arguments zero, in
          the order of _native.SIGNATURES
  create  every *_create* entry point with a valid out-pointer and every other argument zero (the size check)
  batch   every *_create* entry point that takes (out, width, height, max_batch, ...), for a 64 x 48 frame with
          max_batch = 0 and every other argument zero (the batch check)
"""
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def zero_args(args):
    return [0 if a in (C.c_int, C.c_size_t) else 0.0 if a is C.c_float else None for a in args]


def records(path=None):
    from kinectdepthmapenhancement_amd import _native as N
    if path:
        N.use_library(path)
    lib = N.lib()
    handle_first = (C.c_void_p, C.POINTER(C.c_void_p))
    names = [n for n, (res, args) in N.SIGNATURES.items() if res is C.c_int and args and args[0] in handle_first]
    out = []

    def record(mode, name, argv):
        rc = getattr(lib, name)(*argv)
        out.append({"mode": mode, "name": name, "rc": rc, "message": lib.kde_last_error_string().decode()})
        return rc

    for name in names:
        record("zero", name, zero_args(N.SIGNATURES[name][1]))
    for name in names:
        if "_create" not in name:
            continue
        h = C.c_void_p()
        rc = record("create", name, [C.byref(h)] + zero_args(N.SIGNATURES[name][1][1:]))
        if rc == N.KDE_OK:          # kde_dimconv_create has nothing to refuse
            getattr(lib, name.split("_create")[0] + "_destroy")(h)
    for name in names:
        args = N.SIGNATURES[name][1]
        if "_create" in name and args[1:4] == [C.c_int] * 3:
            h = C.c_void_p()
            record("batch", name, [C.byref(h), 64, 48, 0] + zero_args(args[4:]))
    return out


if __name__ == "__main__":
    json.dump(records(sys.argv[1] if len(sys.argv) > 1 else None), sys.stdout, indent=1)
    print()
