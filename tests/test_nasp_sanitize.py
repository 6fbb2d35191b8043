"""CPU sanitizer leg for NormalAdaptiveSuperpixel: the checker tools/nasp_ref.c and the library's host-side arithmetic
(csrc/kde_host_math.h: acos threshold, weight tables) built with -fsanitize=address,undefined, the checker run on ragged and
smallest-accepted geometries with holes, bad and NaN normals and zero sigmas (as tests/test_sanitizers.py does for the
oracle; device code is covered by the parity tests), the library's tables compared with the checker's weights."""
import os
import shutil
import subprocess

import pytest

from conftest import ROOT

SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-g", "-O1"]
ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")


@pytest.mark.skipif(shutil.which("gcc") is None, reason="gcc not available")
def test_nasp_checker_under_asan_and_ubsan(tmp_path):
    exe = str(tmp_path / "nasp_driver")
    subprocess.check_call(["gcc", "-std=c11", "-ffp-contract=off", *SAN, "-o", exe, os.path.join(ROOT, "tests", "sanitize", "nasp_driver.c"),
                           os.path.join(ROOT, "tools", "nasp_ref.c"), "-lm"])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600, env=ENV)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-4000:]
    assert "nasp driver ok" in r.stdout


@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not available")
def test_library_threshold_and_weight_tables_equal_the_checkers(tmp_path):
    """NA3 / NA4: the library (csrc/kde_host_math.h) and the checker (tools/nasp_ref.c) each derive the acos threshold and
    the weights themselves; here the two are compared bit for bit, the library's side under ASan/UBSan"""
    import numpy as np
    from tools import nasp_ref as R
    exe = str(tmp_path / "nasp_host_driver")
    subprocess.check_call(["g++", "-std=c++17", "-ffp-contract=off", *SAN, "-o", exe,
                           os.path.join(ROOT, "tests", "sanitize", "nasp_host_driver.cpp"), "-lm"])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600, env=ENV)
    assert r.returncode == 0 and "nasp host driver ok" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-4000:]
    lines = r.stdout.splitlines()
    bits = lambda v: int(np.array([v], np.float32).view(np.uint32)[0])
    assert int(lines[0].split()[1], 16) == bits(R.acos_threshold()) == 0x3F000000
    tables = [ln.split() for ln in lines if ln.startswith("table")]
    assert len(tables) == 5
    for tok in tables:
        sigma, n, zero = float(tok[1]), int(tok[2]), int(tok[3])
        checked = 0
        for item in tok[4:]:
            i, b = item.split(":")
            w = R.weight(int(i), sigma)
            assert bits(w) == int(b, 16) or (np.isnan(w) and (int(b, 16) & 0x7FFFFFFF) > 0x7F800000), (sigma, i)
            checked += 1
        assert checked > 0 or n == 0
        # truncated exactly where the weight first becomes 0 (or never, for a sigma that keeps every weight positive)
        if zero:
            assert R.weight(n, sigma) == 0.0 and (n == 0 or R.weight(n - 1, sigma) != 0.0)
        else:
            assert n == 3 * 255 * 255 + 1 and R.weight(n - 1, sigma) > 0.0
    assert [int(t[2]) for t in tables][3] == 1        # sigma 0: [NaN], then -x/0 = -inf -> 0
