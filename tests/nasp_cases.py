"""Shared by tests/test_gpu_nasp.py and tests/plane_sweep.py (not a test module): reading every output of a
NormalAdaptiveSuperpixel object as the dict tools/nasp_ref.py gives, and the bit-identity bar of DESIGN.md ("Normal-adaptive
superpixels")."""
import numpy as np


def read_outputs(R, sp, frame=None):
    """every output of the handle as the checker's dict (frame f of a batch, or the single frame)"""
    pick = (lambda t: t) if frame is None else (lambda t: t[frame])
    H, W = sp.height, sp.width
    return {"labels": pick(sp.getLabelDevice()).cpu().numpy(),
            "ld": pick(sp.getLDDevice()).cpu().numpy().reshape(H, W, 8).view(R.LABEL_DISTANCE).reshape(H, W),
            "mean": pick(sp.getMeanDataDevice()).cpu().numpy().view(R.SUPERPIXEL).reshape(-1),
            "centers": pick(sp.getCentersDevice()).cpu().numpy(),
            "normals": pick(sp.getNormalsDevice()).cpu().numpy(),
            "variance": pick(sp.getNormalsVarianceDevice()).cpu().numpy()}


def ubits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def differing(got, exp):
    """number of float elements that differ in their bits, NaNs compared by position"""
    got, exp = np.asarray(got, np.float32), np.asarray(exp, np.float32)
    assert got.shape == exp.shape
    return int(((ubits(got) != ubits(exp)) & ~(np.isnan(got) & np.isnan(exp))).sum())


def assert_identical(got, exp, what):
    counts = {
        "labels": int((got["labels"] != exp["labels"]).sum()),
        "ld.l": int((got["ld"]["l"] != exp["ld"]["l"]).sum()),
        "ld.d": differing(got["ld"]["d"], exp["ld"]["d"]),
        "mean": int((got["mean"].view(np.uint8).reshape(-1, 16) != exp["mean"].view(np.uint8).reshape(-1, 16)).any(-1).sum()),
        "centers": differing(got["centers"], exp["centers"]),
        "normals": differing(got["normals"], exp["normals"]),
        "variance": differing(got["variance"], exp["variance"]),
    }
    print(f"{what}: differing elements {counts}; NaN distances {int(np.isnan(exp['ld']['d']).sum())}, "
          f"labels -1 {int((exp['labels'] == -1).sum())}, clusters with NaN normal {int(np.isnan(exp['normals']).any(-1).sum())}")
    assert not any(counts.values()), f"{what}: {counts}"
