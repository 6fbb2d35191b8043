"""The *_host getters of the C ABI against the device buffers they mirror, through _native.lib(): the bytes a getter hands
out are those behind the matching *_device getter after the same call, and `count` is the number of entries mirrored.  The
expected values are device buffers read back, so there is no tolerance.  Frames are 64 x 48 with 3 x 4 superpixels (16 x 16
windows): the smallest grid NormalAdaptiveSuperpixel's 8 x 8 minimum leaves room for twice over."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

W, H, ROWS, COLS = 64, 48, 3, 4


@pytest.fixture(scope="module")
def T(torch_cuda):
    import torch
    torch.cuda.set_device(0)
    return torch


def device_inputs(T, n):
    """n synthetic frames on the device: colour [n,H,W,3], millimetre points [n,H,W,3] and the intrinsics"""
    from kinectdepthmapenhancement_amd import filters, synth
    bgr, depth = synth.make_batch(1, n, W, H)
    K = synth.intrinsics(W, H)
    conv = filters.DimensionConvertor()
    conv.setCameraParameters(K, W, H)
    pts = T.empty((n, H, W, 3), dtype=T.float32, device="cuda")
    conv.projectiveToReal(T.from_numpy(depth).cuda(), pts)
    return T.from_numpy(bgr).cuda(), pts, K


def host_bytes(fn, handle, nbytes, with_count):
    """the first nbytes behind the pointer a *_host getter returns (and its count, where it has one)"""
    from kinectdepthmapenhancement_amd import _native, filters
    p, cnt = C.c_void_p(), C.c_int(-1)
    args = (handle, filters._stream(), C.byref(p)) + ((C.byref(cnt),) if with_count else ())
    _native.check(getattr(_native.lib(), fn)(*args))
    a = np.ctypeslib.as_array(C.cast(p, C.POINTER(C.c_uint8)), shape=(nbytes,)).copy()
    return (a, cnt.value) if with_count else a


def dev_bytes(t):
    return t.contiguous().cpu().numpy().view(np.uint8).reshape(-1)


def test_dasp_host_getters_mirror_one_frame(T):
    from kinectdepthmapenhancement_amd import filters
    bgr, pts, K = device_inputs(T, 1)
    sp = filters.DepthAdaptiveSuperpixel(W, H)
    sp.SetParametor(ROWS, COLS, K)
    sp.Segmentation(bgr[0], pts[0], 100.0, 20.0, 200.0, 1)
    labels = dev_bytes(sp.getLabelDevice())
    mean = dev_bytes(sp.getMeanDataDevice())
    assert labels.size == W * H * 4 and mean.size == ROWS * COLS * 16
    assert labels.view(np.int32).max() > labels.view(np.int32).min()       # a label map, not a cleared buffer
    assert np.array_equal(host_bytes("kde_dasp_labels_host", sp._h, labels.size, False), labels)
    got, count = host_bytes("kde_dasp_mean_host", sp._h, mean.size, True)
    assert count == ROWS * COLS == 12
    assert np.array_equal(got, mean)
    sp.close()


def test_nasp_host_getters_mirror_the_frames_of_the_last_call(T):
    """max_batch = 3: after a call with n frames the getters mirror n frames of the max_batch allocation"""
    from kinectdepthmapenhancement_amd import filters
    bgr, pts, K = device_inputs(T, 3)
    gen = filters.NormalMapGenerator(W, H, max_batch=3)
    gen.generateNormalMapBatch(3, pts)
    nrm = gen.getNormalMap().clone()
    sp = filters.NormalAdaptiveSuperpixel(W, H, max_batch=3)
    sp.SetParametor(ROWS, COLS, K)
    nc = ROWS * COLS
    for n, first in ((3, 0), (2, 1)):          # the second call's two frames are not the first call's first two
        sl = slice(first, first + n)
        sp.segmentation_batch(bgr[sl].contiguous(), pts[sl].contiguous(), nrm[sl].contiguous(), 10.0, 50.0, 50.0, 150.0, 1)
        labels = dev_bytes(sp.getLabelDevice())
        assert labels.size == n * W * H * 4
        assert labels.view(np.int32).max() > labels.view(np.int32).min()
        assert np.array_equal(host_bytes("kde_nasp_labels_host", sp._h, labels.size, False), labels)
        for fn, dev in (("kde_nasp_centers_host", sp.getCentersDevice()), ("kde_nasp_mean_host", sp.getMeanDataDevice()),
                        ("kde_nasp_normals_host", sp.getNormalsDevice()),
                        ("kde_nasp_normals_variance_host", sp.getNormalsVarianceDevice())):
            exp = dev_bytes(dev)
            got, count = host_bytes(fn, sp._h, exp.size, True)
            assert count == n * nc, (fn, n, count)             # 36 entries, then 24
            assert np.array_equal(got, exp), (fn, n)
    sp.close()
    gen.close()
