"""CPU sanitizer leg for the five-argument PlaneProjection: the checker tools/proj_ref.c built with
-fsanitize=address,undefined into a stand-alone program and run on small and ragged frames with labels outside the tables,
zero plane denominators, NaN depth and every odd window up to 15 (as tests/test_les_sanitize.py does; device code is
covered by the parity tests)."""
import os
import subprocess

from conftest import ROOT

SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-g", "-O1"]
ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")


def test_proj_checker_under_asan_and_ubsan(tmp_path):
    exe = str(tmp_path / "proj_driver")
    subprocess.check_call(["gcc", "-std=c11", "-ffp-contract=off", *SAN, "-o", exe, os.path.join(ROOT, "tests", "sanitize", "proj_driver.c"),
                           os.path.join(ROOT, "tools", "proj_ref.c"), "-lm"])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600, env=ENV)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-4000:]
    assert "proj driver ok" in r.stdout
