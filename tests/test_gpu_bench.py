"""bench.py's plain run and --dump-outputs on the GPU: the line of a plain run, and the outputs of its last timed step,
which must equal the product path called directly on the same frames and be the same from run to run."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT


def _plain(extra, timeout=600):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1"] + extra, capture_output=True, text=True,
                       timeout=timeout)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout
    return json.loads(lines[0])


@pytest.mark.gpu
def test_dump_outputs_are_the_last_timed_steps_outputs(torch_cuda, synth, tmp_path):
    torch = torch_cuda
    from kinectdepthmapenhancement_amd import filters
    n, w, h = 16, 640, 480          # 16 frames of 4.9 MB do not fit in the dump's budget: a seeded sample of whole frames
    args = ["--steps", "3", "--warmup", "1", "--wakeup-ms", "0", "--frames-per-gpu", str(n), "--width", str(w), "--height", str(h)]
    dumps = []
    for k in range(2):
        d = tmp_path / f"run{k}"
        j = _plain(args + ["--dump-outputs", str(d)])
        assert j["steps"] == 3 and j["ms_per_step"] > 0 and j["value"] > 0 and j["full"] is False
        assert "roofline" not in j and "verified" not in j and "cpu_baseline" not in j and "also" not in j
        assert sorted(j["dumped_outputs"]["files"]) == ["filtered_depth.npy", "frame_index.npy", "smoothed_bgr.npy"]
        files = sorted(os.listdir(d))
        assert files == sorted(j["dumped_outputs"]["files"])
        assert sum(os.path.getsize(d / f) for f in files) <= 64 * 2**20
        dumps.append({f[:-4]: np.load(d / f) for f in files})
    a, b = dumps
    idx = a["frame_index"]
    assert a["filtered_depth"].dtype == np.float32 and a["smoothed_bgr"].dtype == np.float32 and idx.dtype == np.float64
    assert 1 <= len(idx) < n and np.all(np.diff(idx) > 0) and idx[0] >= 0 and idx[-1] < n
    assert a["filtered_depth"].shape == (len(idx), h, w) and a["smoothed_bgr"].shape == (len(idx), h, w, 3)
    for name in a:                  # same arguments, same inputs, same outputs, to the bit
        assert a[name].tobytes() == b[name].tobytes(), name

    # the product path called directly on bench.py's frames (8 distinct synthetic frames from seed 0, tiled to the batch)
    bgr, depth = synth.make_batch(0, 8, w, h)
    bgr, depth = np.tile(bgr, (2, 1, 1, 1))[:n], np.tile(depth, (2, 1, 1))[:n]
    p = filters.JointBilateralFilter.default_params()
    p.window_size, p.spatial_sigma, p.color_sigma, p.depth_sigma = 11, 3.0, 7.65, 20.0
    jbf = filters.JointBilateralFilter(w, h, p, max_batch=n)
    out = torch.empty((n, h, w), dtype=torch.float32, device="cuda")
    jbf.process_batch(torch.from_numpy(depth).cuda(), torch.from_numpy(bgr).cuda(), out)
    sel = idx.astype(np.int64)
    got_depth = out.cpu().numpy()[sel]
    got_smooth = jbf.getSmoothImage_Device(n).cpu().numpy()[sel].astype(np.float32)
    jbf.close()
    assert got_depth.tobytes() == a["filtered_depth"].tobytes()
    assert np.array_equal(got_smooth, a["smoothed_bgr"])
