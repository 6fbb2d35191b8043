"""CPU sanitizer leg for LabelEquivalenceSeg: the checker tools/les_ref.c and the library's host-side arithmetic
(csrc/kde_host_math.h: the L6 threshold) built with -fsanitize=address,undefined, the checker run on small and ragged frames
with labels outside the table and bad, NaN and (-1,-1,z) normals (as tests/test_nasp_sanitize.py does; device code is
covered by the parity tests), the library's thresholds compared with the checker's."""
import os
import shutil
import subprocess

import pytest

from conftest import ROOT

SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-g", "-O1"]
ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")


@pytest.mark.skipif(shutil.which("gcc") is None, reason="gcc not available")
def test_les_checker_under_asan_and_ubsan(tmp_path):
    exe = str(tmp_path / "les_driver")
    subprocess.check_call(["gcc", "-std=c11", "-ffp-contract=off", *SAN, "-o", exe, os.path.join(ROOT, "tests", "sanitize", "les_driver.c"),
                           os.path.join(ROOT, "tools", "les_ref.c"), "-lm"])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600, env=ENV)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-4000:]
    assert "les driver ok" in r.stdout


@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not available")
def test_library_threshold_equals_the_checkers(tmp_path):
    """L6: the library (csrc/kde_host_math.h) and the checker (tools/les_ref.c) each derive the acos threshold themselves;
    here the two are compared bit for bit, the library's side under ASan/UBSan"""
    import numpy as np
    from tools import les_ref as R
    exe = str(tmp_path / "les_host_driver")
    subprocess.check_call(["g++", "-std=c++17", "-ffp-contract=off", *SAN, "-o", exe,
                           os.path.join(ROOT, "tests", "sanitize", "les_host_driver.cpp"), "-lm"])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600, env=ENV)
    assert r.returncode == 0 and "les host driver ok" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-4000:]
    rows = [ln.split() for ln in r.stdout.splitlines() if ln.startswith("threshold")]
    assert len(rows) == 12
    for _, ab, tb in rows:
        angle = np.array([int(ab, 16)], np.uint32).view(np.float32)[0]
        assert int(R.acos_threshold(angle).view(np.uint32)) == int(tb, 16), (angle, tb)
    assert int(rows[0][2], 16) == int(R.acos_threshold().view(np.uint32)) and rows[1][2] == "3f000000"
    assert [ln for ln in r.stdout.splitlines() if ln.startswith("nasp")] == ["nasp 3f000000"]
