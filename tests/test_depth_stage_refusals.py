"""The refusals of the four depth-in/depth-out stages (kde_reg_*, kde_undist_*, kde_upsample_*, kde_holefill_*) against the
record made before they were folded onto csrc/kde_depth_stage.h: tests/golden/abi_refusals_depth_stages.json, written by
tools/abi_refusals_depth_stages.py.  Without a GPU, in a few seconds."""
import json
import os
import re
import subprocess
import sys

import pytest

from conftest import GOLDEN, ROOT

TOOL = os.path.join(ROOT, "tools", "abi_refusals_depth_stages.py")
CSRC = os.path.join(ROOT, "kinectdepthmapenhancement_amd", "csrc")
SOURCES = ("kde_api_reg.cpp", "kde_api_undist.cpp", "kde_api_upsample.cpp", "kde_api_holefill.cpp", "kde_depth_stage.h")
# message formats no call of the record can reach: a failed allocation, a failed HIP call, and the refusal kde_upsample_create
# itself marks as never met
UNREACHED = ("%s: out of host memory",
             "%s: the range table could not be copied to the device",
             "%s: the space table could not be copied to the device",
             "%s: the nearest-pixel tables could not be copied to the device",
             "%s: a tile's tap window exceeds %d x %d")


@pytest.fixture(scope="module")
def golden():
    return json.load(open(os.path.join(GOLDEN, "abi_refusals_depth_stages.json")))


@pytest.mark.timeout(300)
def test_refused_calls_answer_as_recorded(golden):
    """The same calls in the same order, in a child process, give the same codes and the same messages.  The `valid` records
    (a fully valid batch call answers KDE_ERR_HIP, "created on a host without a device") are made only where there is no device:
    on a host with one the tool leaves those calls out, since they would launch kernels on its fake addresses, and every other
    record must still be equal.

    Not in the record, because no call reaches them without a failed allocation, a failed HIP call or a successful launch:
      "%s: out of host memory"
      "%s: the range table could not be copied to the device"
      "%s: the space table could not be copied to the device"
      "%s: the nearest-pixel tables could not be copied to the device"
      "%s: a tile's tap window exceeds %d x %d"                        (never met, as kde_upsample_create says)
      "... the object-owned output buffer, which out_dev == NULL selects, overlaps depth_dev ..."   (needs a launch before it)
      "%s failed: %s (%s:%d)", "hipMalloc(...) failed", "hipHostMalloc(...) failed"  and the wrong-device refusal of kde_handles.h"""
    assert all(r["name"] in r["message"] for r in golden if r["rc"] != 0)
    valid = [r for r in golden if r["mode"] == "valid"]
    assert len(valid) == 13 and all(r["rc"] == 2 and r["message"] == r["name"] + ": the handle was created on a host without a device"
                                    for r in valid)
    r = subprocess.run([sys.executable, TOOL], capture_output=True, text=True, timeout=280)
    assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
    got = json.loads(r.stdout)
    want = golden if any(x["mode"] == "valid" for x in got) else [x for x in golden if x["mode"] != "valid"]
    assert len(got) == len(want)
    for i, (a, b) in enumerate(zip(got, want)):
        assert a == b, (i, a, b)


def _formats():
    """the message formats of the four stages' host code: the string literals that open with "%s: " or with a function's name"""
    found = set()
    for name in SOURCES:
        path = os.path.join(CSRC, name)
        if os.path.exists(path):
            found.update(re.findall(r'"((?:%s|kde_(?:reg|undist|upsample|holefill)_\w+): (?:[^"\\]|\\.)*)"', open(path).read()))
    return found


def _pattern(fmt):
    out = re.escape(fmt)
    for spec, rx in ((r"%s", r".*"), (r"%d", r"-?\d+"), (r"%g", r"\S+")):
        out = out.replace(re.escape(spec), rx)
    return re.compile(out + r"\Z", re.S)


@pytest.mark.timeout(120)
def test_the_record_holds_every_message_format(golden):
    """every message format of the four kde_api_*.cpp files and of the core they share occurs in the record, except UNREACHED:
    a stage that grows a refusal grows the record with it"""
    formats = _formats()
    assert len(formats) >= 30 and set(UNREACHED) <= formats, sorted(set(UNREACHED) - formats)
    messages = {r["message"] for r in golden}
    missing = [f for f in sorted(formats - set(UNREACHED)) if not any(_pattern(f).match(m) for m in messages)]
    assert missing == []
