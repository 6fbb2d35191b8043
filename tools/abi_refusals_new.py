#!/usr/bin/env python3
"""The refusals of the entry points added after tests/golden/abi_refusals.json was frozen, recorded the same way.

    python tools/abi_refusals_new.py [LIBRARY]    prints the records as JSON (default: the built product library)

tools/abi_refusals.py enumerates the _native.SIGNATURES entries whose first argument is c_void_p or POINTER(c_void_p), and
tests/test_capi_symbols.py pins that enumeration to the calls it held when the record was made.  Entry points added since
are bound so that the enumeration does not see them -- kde_points_to_depth leads with its size_t count, the kde_enh_feed_*
functions take the typed handle _native.EnhFeedHandle -- and are listed HERE by name instead.  The output for the library
that introduced them is tests/golden/abi_refusals_enh_feed.json; tests/test_enh_feed_abi.py replays it.  Argument
validation precedes every HIP call, so this runs without a GPU.  The order is part of the record: a call that succeeds
leaves the previous call's message in place.

  zero    every entry point of NEW with all arguments zero.  KDE_ERR_INVALID, except *_destroy(NULL) (a no-op like
          free(NULL)) and kde_points_to_depth, whose all-zero call is its n_points == 0 case: KDE_OK, nothing launched
  create  kde_enh_feed_create with a valid out-pointer and every other argument zero
  one     kde_points_to_depth for one point with null pointers; for one point with an unknown format
"""
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tools.abi_refusals import zero_args  # noqa: E402

NEW = ("kde_points_to_depth", "kde_enh_feed_create", "kde_enh_feed_destroy", "kde_enh_feed_process", "kde_enh_feed_last_stats")


def records(path=None):
    from kinectdepthmapenhancement_amd import _native as N
    if path:
        N.use_library(path)
    lib = N.lib()
    out = []

    def record(mode, name, argv):
        rc = getattr(lib, name)(*argv)
        out.append({"mode": mode, "name": name, "rc": rc, "message": lib.kde_last_error_string().decode()})
        return rc

    for name in NEW:
        record("zero", name, zero_args(N.SIGNATURES[name][1]))
    h = N.EnhFeedHandle()
    record("create", "kde_enh_feed_create", [C.byref(h)] + zero_args(N.SIGNATURES["kde_enh_feed_create"][1][1:]))
    record("one", "kde_points_to_depth", [1, None, N.KDE_DEPTH_U16, None, None])
    record("one", "kde_points_to_depth", [1, None, 7, None, None])
    return out


if __name__ == "__main__":
    json.dump(records(sys.argv[1] if len(sys.argv) > 1 else None), sys.stdout, indent=1)
    print()
