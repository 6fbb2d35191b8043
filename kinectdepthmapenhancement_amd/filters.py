"""Python mirror of the reference's class surface for the hot path, over the C ABI.

Same class and member names as the reference (JointBilateralFilter::Process, getFiltered_Device,
RegionGrowingBilateralFilter::SetParametor [sic], ...); cv::gpu::GpuMat becomes a CUDA uint8 tensor
[H,W,3] (packed BGR), float*/float3*/int* device pointers become CUDA tensors, cv::Mat_<double>
becomes a 3x3 array.  torch is used for device memory and streams only; every computation goes
through libkde_hip.so and raises if that fails.
"""
from __future__ import annotations

import ctypes as C
from typing import Optional

import numpy as np
import torch

from . import _native
from ._native import JbfParams, LesParams, NormalsParams, ProjParams, check, lib


def _stream() -> int:
    return torch.cuda.current_stream().cuda_stream


def _ptr(t: Optional[torch.Tensor]) -> Optional[int]:
    return None if t is None else t.data_ptr()


def _req(t: torch.Tensor, dtype, shape, name: str) -> torch.Tensor:
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise TypeError(f"{name}: expected a CUDA tensor")
    if t.dtype != dtype or tuple(t.shape) != tuple(shape) or not t.is_contiguous():
        raise ValueError(f"{name}: expected contiguous {dtype} {tuple(shape)}, got {t.dtype} {tuple(t.shape)}")
    return t


class _DeviceView:
    """Zero-copy torch view of an object-owned device buffer (valid while `owner` lives)."""

    def __init__(self, ptr: int, shape, typestr: str, owner):
        self.owner = owner
        self.__cuda_array_interface__ = {"shape": tuple(shape), "typestr": typestr, "data": (ptr, False),
                                         "version": 2, "strides": None}


def _view(ptr: int, shape, dtype: torch.dtype, owner) -> torch.Tensor:
    typestr = {torch.float32: "<f4", torch.int32: "<i4", torch.uint8: "|u1"}[dtype]
    holder = _DeviceView(ptr, shape, typestr, owner)
    t = torch.as_tensor(holder, device="cuda")
    t._kde_owner = holder   # keep the handle alive as long as the view
    return t


def _K9(K) -> np.ndarray:
    k = np.ascontiguousarray(np.asarray(K, np.float64).reshape(9))
    return k


class _Handle:
    _destroy = None
    _handle_type = C.c_void_p       # the ctypes type of the handle (a subclass where _native declares one)

    def __init__(self):
        self._h = self._handle_type()
        self._owner_lib = lib()     # a handle is destroyed by the library that created it

    def close(self):
        if getattr(self, "_h", None) is not None and self._h.value:
            getattr(self._owner_lib, self._destroy)(self._h)
            self._h = self._handle_type()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class JointBilateralFilter(_Handle):
    """JointBilateralFilter/JointBilateralFilter.h:9-36."""
    _destroy = "kde_jbf_destroy"

    def __init__(self, width: int, height: int, params: Optional[JbfParams] = None, max_batch: int = 1):
        super().__init__()
        self.Width, self.Height, self.max_batch = width, height, max_batch
        self.params = params if params is not None else self.default_params()
        check(lib().kde_jbf_create(C.byref(self._h), width, height, max_batch, C.byref(self.params)))

    @staticmethod
    def default_params() -> JbfParams:
        p = JbfParams()
        check(lib().kde_jbf_default_params(C.byref(p)))
        return p

    # void Process(float* depth_device, cv::gpu::GpuMat color_image)
    def Process(self, depth_device: torch.Tensor, color_image: torch.Tensor) -> None:
        _req(depth_device, torch.float32, (self.Height, self.Width), "depth_device")
        _req(color_image, torch.uint8, (self.Height, self.Width, 3), "color_image")
        check(lib().kde_jbf_process(self._h, depth_device.data_ptr(), color_image.data_ptr(),
                                    self.Width * 3, _stream()))

    def process_batch(self, depth: torch.Tensor, color: torch.Tensor, out: Optional[torch.Tensor] = None):
        n = depth.shape[0]
        _req(depth, torch.float32, (n, self.Height, self.Width), "depth")
        _req(color, torch.uint8, (n, self.Height, self.Width, 3), "color")
        if out is not None:
            _req(out, torch.float32, (n, self.Height, self.Width), "out")
        check(lib().kde_jbf_process_batch(self._h, n, depth.data_ptr(), color.data_ptr(), _ptr(out), _stream()))
        return out if out is not None else self.getFiltered_Device(n)

    def presmooth_batch(self, color: torch.Tensor, out: torch.Tensor):
        n = color.shape[0]
        _req(color, torch.uint8, (n, self.Height, self.Width, 3), "color")
        _req(out, torch.uint8, (n, self.Height, self.Width, 3), "out")
        check(lib().kde_jbf_presmooth_batch(self._h, n, color.data_ptr(), out.data_ptr(), _stream()))
        return out

    def filter_batch(self, depth: torch.Tensor, guide: torch.Tensor, out: torch.Tensor):
        n = depth.shape[0]
        _req(depth, torch.float32, (n, self.Height, self.Width), "depth")
        _req(guide, torch.uint8, (n, self.Height, self.Width, 3), "guide")
        _req(out, torch.float32, (n, self.Height, self.Width), "out")
        check(lib().kde_jbf_filter_batch(self._h, n, depth.data_ptr(), guide.data_ptr(), out.data_ptr(), _stream()))
        return out

    def getFiltered_Device(self, n: int = 1) -> torch.Tensor:
        p = C.c_void_p()
        check(lib().kde_jbf_filtered_device(self._h, C.byref(p)))
        shape = (self.Height, self.Width) if n == 1 else (n, self.Height, self.Width)
        return _view(p.value, shape, torch.float32, self)

    def getFiltered_Host(self) -> np.ndarray:
        p = C.c_void_p()
        check(lib().kde_jbf_filtered_host(self._h, _stream(), C.byref(p)))
        arr = np.ctypeslib.as_array(C.cast(p, C.POINTER(C.c_float)), shape=(self.Height, self.Width))
        return arr.copy()

    def getSmoothImage_Device(self, n: int = 1) -> torch.Tensor:
        p = C.c_void_p()
        check(lib().kde_jbf_smooth_device(self._h, C.byref(p)))
        shape = (self.Height, self.Width, 3) if n == 1 else (n, self.Height, self.Width, 3)
        return _view(p.value, shape, torch.uint8, self)

    def spatial_table(self) -> np.ndarray:
        w = self.params.window_size
        t = np.empty((w, w), np.float32)
        check(lib().kde_jbf_spatial_table(self._h, t.ctypes.data, w * w))
        return t

    def set_variant(self, v: int) -> None:
        check(lib().kde_jbf_set_variant(self._h, v))

    def active_variant(self) -> str:
        """name of the kernel this handle's parameters and variant setting select ("generic-32x8-1px" when no tuned one applies)"""
        v = C.c_int(-1)
        check(lib().kde_jbf_active_variant(self._h, C.byref(v)))
        return lib().kde_jbf_variant_name(v.value).decode()

    @staticmethod
    def variants():
        n = lib().kde_jbf_variant_count()
        return [lib().kde_jbf_variant_name(i).decode() for i in range(n)]


def _host_array(a, dtypes, shape, name: str):
    """(data pointer, numpy dtype) of a host numpy array or CPU torch tensor (pinned or not): contiguous, of one of `dtypes`
    (numpy dtypes), of `shape`"""
    if isinstance(a, torch.Tensor):
        if a.is_cuda:
            raise TypeError(f"{name}: expected host memory (numpy array or CPU tensor), got a CUDA tensor")
        tdt = {torch.float32: np.dtype(np.float32), torch.uint8: np.dtype(np.uint8)}
        if hasattr(torch, "uint16"):
            tdt[torch.uint16] = np.dtype(np.uint16)
        dt, contiguous = tdt.get(a.dtype), a.is_contiguous()
    elif isinstance(a, np.ndarray):
        dt, contiguous = a.dtype, a.flags.c_contiguous
    else:
        raise TypeError(f"{name}: expected a numpy array or a CPU torch tensor, got {type(a).__name__}")
    if dt not in [np.dtype(d) for d in dtypes] or tuple(a.shape) != tuple(shape) or not contiguous:
        want = " or ".join(np.dtype(d).name for d in dtypes)
        raise ValueError(f"{name}: expected contiguous {want} {tuple(shape)}, got {getattr(a, 'dtype', None)} {tuple(a.shape)}")
    return (a.data_ptr() if isinstance(a, torch.Tensor) else a.ctypes.data), dt


class JointBilateralFilterFeed(_Handle):
    """Host-fed JointBilateralFilter::Process (kde_jbf_feed_*): frames in host memory in, filtered depth in host memory out,
    in chunks of `chunk_frames` with the copies overlapped with the kernels.  Borrows `jbf` (kept alive by this object) and
    leaves its device buffers untouched; `jbf` must not be used while process() runs.  A blocking call on the feed's own
    streams, not on torch's current stream."""
    _destroy = "kde_jbf_feed_destroy"

    def __init__(self, jbf: JointBilateralFilter, chunk_frames: int = 8):
        super().__init__()
        self.jbf = jbf
        self.Width, self.Height, self.chunk_frames = jbf.Width, jbf.Height, chunk_frames
        check(lib().kde_jbf_feed_create(C.byref(self._h), jbf._h, chunk_frames))

    def process(self, depth, color, out=None):
        """depth [n,H,W] float32 or uint16 (mm, 0 = invalid), color [n,H,W,3] uint8 BGR, out [n,H,W] float32 (allocated
        as a numpy array when None): numpy arrays or CPU torch tensors, pinned or pageable.  Returns out."""
        n = depth.shape[0] if len(depth.shape) == 3 else -1
        dptr, ddt = _host_array(depth, (np.float32, np.uint16), (n, self.Height, self.Width), "depth")
        cptr, _ = _host_array(color, (np.uint8,), (n, self.Height, self.Width, 3), "color")
        if out is None:
            out = np.empty((n, self.Height, self.Width), np.float32)
        optr, _ = _host_array(out, (np.float32,), (n, self.Height, self.Width), "out")
        fmt = _native.KDE_DEPTH_U16 if ddt == np.uint16 else _native.KDE_DEPTH_F32
        check(lib().kde_jbf_feed_process(self._h, n, dptr, fmt, cptr, optr))
        return out

    def last_stats(self) -> dict:
        st = _native.FeedStats()
        check(lib().kde_jbf_feed_last_stats(self._h, C.byref(st)))
        return {name: getattr(st, name) for name, _ in st._fields_}


class MarkovRandomField(_Handle):
    """MarkovRandomField/MarkovRandomField.h (sibling filter, same signature as JBF)."""
    _destroy = "kde_mrf_destroy"

    def __init__(self, width: int, height: int, max_batch: int = 1, window: int = 0,
                 color_sigma: float = -1.0, smooth_sigma: float = -1.0):
        super().__init__()
        self.Width, self.Height, self.max_batch = width, height, max_batch
        check(lib().kde_mrf_create(C.byref(self._h), width, height, max_batch, window, color_sigma, smooth_sigma))

    def Process(self, depth_device: torch.Tensor, color_image: torch.Tensor) -> None:
        _req(depth_device, torch.float32, (self.Height, self.Width), "depth_device")
        _req(color_image, torch.uint8, (self.Height, self.Width, 3), "color_image")
        check(lib().kde_mrf_process_batch(self._h, 1, depth_device.data_ptr(), color_image.data_ptr(), None, _stream()))

    def process_batch(self, depth, color, out):
        n = depth.shape[0]
        check(lib().kde_mrf_process_batch(self._h, n, depth.data_ptr(), color.data_ptr(), out.data_ptr(), _stream()))
        return out

    def getFiltered_Device(self) -> torch.Tensor:
        p = C.c_void_p()
        check(lib().kde_mrf_filtered_device(self._h, C.byref(p)))
        return _view(p.value, (self.Height, self.Width), torch.float32, self)

    def getFiltered_Host(self) -> np.ndarray:
        """MarkovRandomField.h:16"""
        p = C.c_void_p()
        check(lib().kde_mrf_filtered_host(self._h, _stream(), C.byref(p)))
        return np.ctypeslib.as_array(C.cast(p, C.POINTER(C.c_float)), shape=(self.Height, self.Width)).copy()


class NormalMapGenerator(_Handle):
    """NormalEstimation/NormalMapGenerator.h: per-pixel normals of float32 points [H, W, 3] in millimetres (what
    DimensionConvertor.projectiveToReal writes); normals are float32 [H, W, 3], a bad point is (-1, -1, -1)."""
    _destroy = "kde_normals_destroy"
    SDC, CM, BILATERAL = _native.KDE_NORMALS_SDC, _native.KDE_NORMALS_CM, _native.KDE_NORMALS_BILATERAL

    def __init__(self, width: int, height: int, max_batch: int = 1, params: Optional[NormalsParams] = None):
        super().__init__()
        self.Width, self.Height, self.max_batch = width, height, max_batch
        check(lib().kde_normals_create(C.byref(self._h), width, height, max_batch, None if params is None else C.byref(params)))
        self._n = self._n_fs = 1   # frames of the last call in the object-owned normal map / smoothing map

    @staticmethod
    def default_params() -> NormalsParams:
        p = NormalsParams()
        check(lib().kde_normals_default_params(C.byref(p)))
        return p

    def setNormalEstimationMethods(self, method: int) -> None:
        check(lib().kde_normals_set_method(self._h, int(method)))

    def generateNormalMap(self, points: torch.Tensor) -> None:
        """void generateNormalMap(float3* vertices_device) (NormalMapGenerator.cu:513-524)"""
        _req(points, torch.float32, (self.Height, self.Width, 3), "points")
        check(lib().kde_normals_generate_batch(self._h, 1, points.data_ptr(), None, _stream()))
        self._n = self._n_fs = 1

    def generateNormalMapBatch(self, n: int, points: torch.Tensor, out: Optional[torch.Tensor] = None):
        """n frames [n, H, W, 3]; out=None writes the object-owned map (getNormalMap returns all n frames)"""
        _req(points, torch.float32, (n, self.Height, self.Width, 3), "points")
        if out is not None:
            _req(out, torch.float32, (n, self.Height, self.Width, 3), "out")
        check(lib().kde_normals_generate_batch(self._h, n, points.data_ptr(), _ptr(out), _stream()))
        self._n_fs = n
        if out is None:
            self._n = n
        return out

    def _shape(self, n, trailing=()):
        lead = (n,) if n > 1 else ()
        return lead + (self.Height, self.Width) + tuple(trailing)

    def getNormalMap(self) -> torch.Tensor:
        """float3* getNormalMap() (NormalMapGenerator.cpp:47-49): object-owned [H, W, 3] ([n, H, W, 3] after a batch)"""
        p = C.c_void_p()
        check(lib().kde_normals_normal_map_device(self._h, C.byref(p)))
        return _view(p.value, self._shape(self._n, (3,)), torch.float32, self)

    def getNormalMap_Host(self) -> np.ndarray:
        p = C.c_void_p()
        check(lib().kde_normals_normal_map_host(self._h, _stream(), C.byref(p)))
        shape = self._shape(self._n, (3,))
        return np.ctypeslib.as_array(C.cast(p, C.POINTER(C.c_float)), shape=shape).copy()

    def getSmoothingMap(self) -> torch.Tensor:
        """the final smoothing map of the last call, if it ran CM (SmoothingAreaMapGenerator::getFinalSmoothingMap):
        [H, W] ([n, H, W] after a batch, whichever buffer took the normals)"""
        p = C.c_void_p()
        check(lib().kde_normals_smoothing_map_device(self._h, C.byref(p)))
        return _view(p.value, self._shape(self._n_fs), torch.float32, self)


class DimensionConvertor(_Handle):
    """DimensionConvertor/DimensionConvertor.h:152-171.  float3 buffers are float32 tensors [..., 3]."""
    _destroy = "kde_dimconv_destroy"

    def __init__(self):
        super().__init__()
        check(lib().kde_dimconv_create(C.byref(self._h)))
        self.Width = self.Height = 0

    def setCameraParameters(self, intrinsic, width: int, height: int) -> None:
        k = _K9(intrinsic)
        check(lib().kde_dimconv_set_camera(self._h, k.ctypes.data, width, height))
        self.Width, self.Height = width, height

    def _n(self, t: torch.Tensor, trailing) -> int:
        lead = t.shape[:t.dim() - len(trailing) - 2]
        n = int(np.prod(lead)) if len(lead) else 1
        exp = tuple(lead) + (self.Height, self.Width) + tuple(trailing)
        if tuple(t.shape) != exp or t.dtype != torch.float32 or not t.is_cuda or not t.is_contiguous():
            raise ValueError(f"expected contiguous CUDA float32 {exp}, got {t.dtype} {tuple(t.shape)}")
        return n

    def projectiveToReal(self, data: torch.Tensor, out: torch.Tensor) -> torch.Tensor:
        """both overloads: float* depth -> float3* (DimensionConvertor.cu:3-23) or float3* -> float3* (:25-33).  The float3
        overload is the one whose `out` has the rank of `data`: three depth frames of 3 x 3 have the shape of one 3 x 3 cloud."""
        if data.shape[-1] == 3 and data.dim() >= 3 and tuple(data.shape[-3:-1]) == (self.Height, self.Width) and out.dim() == data.dim():
            n = self._n(data, (3,))
            self._n(out, (3,))
            check(lib().kde_dimconv_projective_to_real_points(self._h, n, data.data_ptr(), out.data_ptr(), _stream()))
        else:
            n = self._n(data, ())
            self._n(out, (3,))
            check(lib().kde_dimconv_projective_to_real_depth(self._h, n, data.data_ptr(), out.data_ptr(), _stream()))
        return out

    def projectiveToRealInterp(self, data: torch.Tensor, out: torch.Tensor) -> torch.Tensor:
        n = self._n(data, ())
        self._n(out, (3,))
        check(lib().kde_dimconv_projective_to_real_interp(self._h, n, data.data_ptr(), out.data_ptr(), _stream()))
        return out

    def realToProjective(self, data: torch.Tensor, out: torch.Tensor) -> torch.Tensor:
        n = self._n(data, (3,))
        self._n(out, (3,))
        check(lib().kde_dimconv_real_to_projective(self._h, n, data.data_ptr(), out.data_ptr(), _stream()))
        return out


class Buffer2D(_Handle):
    """ArrayBuffer/Buffer2D.h:9-37 (the OpenNI DepthMetaData overload is out of scope)."""
    _destroy = "kde_buffer2d_destroy"

    def __init__(self, width: int, height: int):
        super().__init__()
        self.width, self.height = width, height
        check(lib().kde_buffer2d_create(C.byref(self._h), width, height))

    def insertData(self, data: torch.Tensor) -> None:
        """float* [H,W]; float2* [H,W,2] (d = .x, w = row index [sic]); weighted_d* is insertWeighted."""
        if data.dim() == 3 and data.shape[-1] == 2:
            _req(data, torch.float32, (self.height, self.width, 2), "data")
            check(lib().kde_buffer2d_insert_float2(self._h, data.data_ptr(), _stream()))
        else:
            _req(data, torch.float32, (self.height, self.width), "data")
            check(lib().kde_buffer2d_insert_depth(self._h, data.data_ptr(), _stream()))

    def insertWeighted(self, data: torch.Tensor) -> None:
        _req(data, torch.float32, (self.height, self.width, 2), "data")
        check(lib().kde_buffer2d_insert_weighted(self._h, data.data_ptr(), _stream()))

    def getDepthMap(self, out: torch.Tensor) -> torch.Tensor:
        _req(out, torch.float32, (self.height, self.width), "out")
        check(lib().kde_buffer2d_get_depth_map(self._h, out.data_ptr(), _stream()))
        return out

    def getWeightMap(self, out: torch.Tensor) -> torch.Tensor:
        _req(out, torch.float32, (self.height, self.width), "out")
        check(lib().kde_buffer2d_get_weight_map(self._h, out.data_ptr(), _stream()))
        return out

    def updateData(self, data: torch.Tensor) -> None:
        if data.dim() == 3:   # a sequence of frames [F,H,W], fused into one pass
            _req(data, torch.float32, (data.shape[0], self.height, self.width), "data")
            check(lib().kde_buffer2d_update_sequence(self._h, data.shape[0], data.data_ptr(), _stream()))
        else:
            _req(data, torch.float32, (self.height, self.width), "data")
            check(lib().kde_buffer2d_update(self._h, data.data_ptr(), _stream()))

    def getRawPointer(self) -> torch.Tensor:
        p = C.c_void_p()
        check(lib().kde_buffer2d_raw_pointer(self._h, C.byref(p)))
        return _view(p.value, (self.height, self.width, 2), torch.float32, self)


class DepthAdaptiveSuperpixel(_Handle):
    """SuperpixelSegmentation/DepthAdaptiveSuperpixel.h:15-28."""
    _destroy = "kde_dasp_destroy"

    def __init__(self, width: int, height: int):
        super().__init__()
        self.width, self.height = width, height
        self.rows = self.cols = 0
        check(lib().kde_dasp_create(C.byref(self._h), width, height))

    def SetParametor(self, rows: int, cols: int, intrinsic) -> None:
        k = _K9(intrinsic)
        check(lib().kde_dasp_set_parameters(self._h, rows, cols, k.ctypes.data))
        self.rows, self.cols = rows, cols

    def Segmentation(self, color_image: torch.Tensor, points3d_device: torch.Tensor, color_sigma: float,
                     spatial_sigma: float, depth_sigma: float, iteration: int) -> None:
        _req(color_image, torch.uint8, (self.height, self.width, 3), "color_image")
        _req(points3d_device, torch.float32, (self.height, self.width, 3), "points3d_device")
        check(lib().kde_dasp_segmentation(self._h, color_image.data_ptr(), points3d_device.data_ptr(),
                                          color_sigma, spatial_sigma, depth_sigma, iteration, _stream()))

    def _get(self, fn, shape, dtype):
        p = C.c_void_p()
        check(getattr(lib(), fn)(self._h, C.byref(p)))
        return _view(p.value, shape, dtype, self)

    def getLabelDevice(self) -> torch.Tensor:
        return self._get("kde_dasp_labels_device", (self.height, self.width), torch.int32)

    def getMeanDataDevice(self) -> torch.Tensor:
        """superpixel records as raw bytes [rows*cols, 16] (r,g,b,pad, x:int32, y:int32, size:int32)."""
        return self._get("kde_dasp_mean_device", (self.rows * self.cols, 16), torch.uint8)

    def getCentersDevice(self) -> torch.Tensor:
        return self._get("kde_dasp_centers_device", (self.rows * self.cols, 3), torch.float32)

    def getLDDevice(self) -> torch.Tensor:
        """label_distance records as raw bytes [H,W,8] (d:float32, l:int32)."""
        return self._get("kde_dasp_ld_device", (self.height, self.width, 8), torch.uint8)


class NormalAdaptiveSuperpixel(_Handle):
    """SuperpixelSegmentation/NormalAdaptiveSuperpixel.h:15-38: superpixels on colour, position, depth and surface normal.
    After segmentation_batch the getters return the n frames of the call ([n, ...]); after Segmentation one frame."""
    _destroy = "kde_nasp_destroy"

    def __init__(self, width: int, height: int, max_batch: int = 1):
        super().__init__()
        self.width, self.height, self.max_batch = width, height, max_batch
        self.rows = self.cols = 0
        self._n = 1
        check(lib().kde_nasp_create(C.byref(self._h), width, height, max_batch))

    def SetParametor(self, rows: int, cols: int, intrinsic) -> None:
        k = _K9(intrinsic)
        check(lib().kde_nasp_set_parameters(self._h, rows, cols, k.ctypes.data))
        self.rows, self.cols = rows, cols

    def Segmentation(self, color_image: torch.Tensor, points3d_device: torch.Tensor, normals_device: torch.Tensor,
                     color_sigma: float, spatial_sigma: float, depth_sigma: float, normal_sigma: float, iteration: int) -> None:
        hw = (self.height, self.width)
        _req(color_image, torch.uint8, hw + (3,), "color_image")
        _req(points3d_device, torch.float32, hw + (3,), "points3d_device")
        _req(normals_device, torch.float32, hw + (3,), "normals_device")
        check(lib().kde_nasp_segmentation(self._h, color_image.data_ptr(), points3d_device.data_ptr(), normals_device.data_ptr(),
                                          color_sigma, spatial_sigma, depth_sigma, normal_sigma, iteration, _stream()))
        self._n = 1

    def segmentation_batch(self, color: torch.Tensor, points: torch.Tensor, normals: torch.Tensor, color_sigma: float,
                           spatial_sigma: float, depth_sigma: float, normal_sigma: float, iteration: int) -> None:
        """n independent frames back to back ([n,H,W,3] each); each frame's result is bit-identical to its Segmentation"""
        n = color.shape[0]
        hw = (self.height, self.width)
        _req(color, torch.uint8, (n,) + hw + (3,), "color")
        _req(points, torch.float32, (n,) + hw + (3,), "points")
        _req(normals, torch.float32, (n,) + hw + (3,), "normals")
        check(lib().kde_nasp_segmentation_batch(self._h, n, color.data_ptr(), points.data_ptr(), normals.data_ptr(), color_sigma,
                                                spatial_sigma, depth_sigma, normal_sigma, iteration, _stream()))
        self._n = n

    def _lead(self):
        return () if self._n == 1 else (self._n,)

    def _get(self, fn, shape, dtype):
        p = C.c_void_p()
        check(getattr(lib(), fn)(self._h, C.byref(p)))
        return _view(p.value, self._lead() + tuple(shape), dtype, self)

    def getLabelDevice(self) -> torch.Tensor:
        return self._get("kde_nasp_labels_device", (self.height, self.width), torch.int32)

    def getMeanDataDevice(self) -> torch.Tensor:
        """superpixel records as raw bytes [rows*cols, 16] (r,g,b,pad, x:int32, y:int32, size:int32)."""
        return self._get("kde_nasp_mean_device", (self.rows * self.cols, 16), torch.uint8)

    def getCentersDevice(self) -> torch.Tensor:
        return self._get("kde_nasp_centers_device", (self.rows * self.cols, 3), torch.float32)

    def getNormalsDevice(self) -> torch.Tensor:
        return self._get("kde_nasp_normals_device", (self.rows * self.cols, 3), torch.float32)

    def getNormalsVarianceDevice(self) -> torch.Tensor:
        return self._get("kde_nasp_normals_variance_device", (self.rows * self.cols,), torch.float32)

    def getLDDevice(self) -> torch.Tensor:
        """label_distance records as raw bytes [H,W,8] (d:float32, l:int32)."""
        return self._get("kde_nasp_ld_device", (self.height, self.width, 8), torch.uint8)

    def _host(self, fn, ctype, per, dtype):
        p, cnt = C.c_void_p(), C.c_int()
        check(getattr(lib(), fn)(self._h, _stream(), C.byref(p), C.byref(cnt)))
        a = np.ctypeslib.as_array(C.cast(p, C.POINTER(ctype)), shape=(cnt.value * per,)).copy()
        return a.view(dtype).reshape(self._lead() + (self.rows * self.cols, -1))

    def getLabelsHost(self) -> np.ndarray:
        p = C.c_void_p()
        check(lib().kde_nasp_labels_host(self._h, _stream(), C.byref(p)))
        return np.ctypeslib.as_array(C.cast(p, C.POINTER(C.c_int32)), shape=self._lead() + (self.height, self.width)).copy()

    def getMeanDataHost(self) -> np.ndarray:
        """records as raw bytes [rows*cols, 16]"""
        return self._host("kde_nasp_mean_host", C.c_uint8, 16, np.uint8)

    def getCentersHost(self) -> np.ndarray:
        return self._host("kde_nasp_centers_host", C.c_float, 3, np.float32)

    def getNormalsHost(self) -> np.ndarray:
        return self._host("kde_nasp_normals_host", C.c_float, 3, np.float32)

    def getNormalsVarianceHost(self) -> np.ndarray:
        return self._host("kde_nasp_normals_variance_host", C.c_float, 1, np.float32)[..., 0]

    def getNormalImg(self) -> np.ndarray:
        """NormalAdaptiveSuperpixel.cpp:38-54: per pixel its superpixel's normal as (unsigned char)(255*(n+1)/2); a pixel
        without a superpixel (label -1) or with a label outside the table is black"""
        labels, nrm = self.getLabelsHost(), self.getNormalsHost()
        k = self.rows * self.cols
        labels, nrm = labels.reshape(-1, self.height, self.width), nrm.reshape(-1, k, 3)
        img = np.zeros(labels.shape + (3,), np.uint8)
        for f in range(labels.shape[0]):
            ok = (labels[f] >= 0) & (labels[f] < k)
            v = np.float32(255.0) * (nrm[f][np.where(ok, labels[f], 0)] + np.float32(1.0)) / np.float32(2.0)
            v = np.where(np.isfinite(v), v, 0.0)
            img[f] = np.where(ok[..., None], np.clip(np.trunc(v), -2147483648, 2147483647).astype(np.int64) & 0xFF, 0).astype(np.uint8)
        return img.reshape(self._lead() + (self.height, self.width, 3))


class LabelEquivalenceSeg(_Handle):
    """LabelEquivalenceSeg/LabelEquivalenceSeg.h: merges 4-adjacent superpixels with similar plane parameters into regions
    and gives each region an averaged plane (n, d), a size and a normal-agreement variance.  The number of superpixels is
    the length of the normals tensor ([k, 3] for labelImage, [n, k, 3] for label_image_batch).  After label_image_batch the
    getters return the n frames of the call ([n, ...]); after labelImage one frame."""
    _destroy = "kde_les_destroy"

    def __init__(self, width: int, height: int, max_batch: int = 1, params: Optional[LesParams] = None):
        super().__init__()
        self.width, self.height, self.max_batch = width, height, max_batch
        self._n, self._k = 1, 0
        check(lib().kde_les_create(C.byref(self._h), width, height, max_batch, C.byref(params) if params is not None else None))

    @staticmethod
    def default_params() -> LesParams:
        p = LesParams()
        check(lib().kde_les_default_params(C.byref(p)))
        return p

    def labelImage(self, cluster_normals_device: torch.Tensor, cluster_label_device: torch.Tensor,
                   cluster_centers_device: torch.Tensor, variance_device: Optional[torch.Tensor] = None) -> None:
        """LabelEquivalenceSeg.cu:228-282; variance_device is dead in the reference and never read"""
        if not isinstance(cluster_normals_device, torch.Tensor) or cluster_normals_device.dim() != 2:
            raise ValueError("cluster_normals_device: expected a [k, 3] tensor")
        k = cluster_normals_device.shape[0]
        _req(cluster_normals_device, torch.float32, (k, 3), "cluster_normals_device")
        _req(cluster_label_device, torch.int32, (self.height, self.width), "cluster_label_device")
        _req(cluster_centers_device, torch.float32, (k, 3), "cluster_centers_device")
        check(lib().kde_les_label_image(self._h, cluster_normals_device.data_ptr(), cluster_label_device.data_ptr(),
                                        cluster_centers_device.data_ptr(), _ptr(variance_device), k, _stream()))
        self._n, self._k = 1, k

    def label_image_batch(self, normals: torch.Tensor, labels: torch.Tensor, centers: torch.Tensor,
                          variance: Optional[torch.Tensor] = None) -> None:
        """n independent frames back to back ([n, k, 3], [n, H, W], [n, k, 3]); each frame's result is bit-identical to its
        labelImage"""
        if not isinstance(normals, torch.Tensor) or normals.dim() != 3:
            raise ValueError("normals: expected a [n, k, 3] tensor")
        n, k = normals.shape[0], normals.shape[1]
        _req(normals, torch.float32, (n, k, 3), "normals")
        _req(labels, torch.int32, (n, self.height, self.width), "labels")
        _req(centers, torch.float32, (n, k, 3), "centers")
        check(lib().kde_les_label_image_batch(self._h, n, normals.data_ptr(), labels.data_ptr(), centers.data_ptr(),
                                              _ptr(variance), k, _stream()))
        self._n, self._k = n, k

    def _lead(self):
        return () if self._n == 1 else (self._n,)

    def _get(self, fn, shape, dtype):
        p = C.c_void_p()
        check(getattr(lib(), fn)(self._h, C.byref(p)))
        return _view(p.value, self._lead() + tuple(shape), dtype, self)

    def getMergedClusterLabel_Device(self) -> torch.Tensor:
        return self._get("kde_les_merged_label_device", (self.height, self.width), torch.int32)

    def getMergedClusterND_Device(self) -> torch.Tensor:
        return self._get("kde_les_merged_nd_device", (self.height, self.width, 4), torch.float32)

    def getMergedClusterVariance_Device(self) -> torch.Tensor:
        """indexed by merged label, one entry per superpixel of the last call"""
        return self._get("kde_les_merged_variance_device", (self._k,), torch.float32)

    def getMergedClusterSize_Device(self) -> torch.Tensor:
        """indexed by merged label, one entry per superpixel of the last call"""
        return self._get("kde_les_merged_size_device", (self._k,), torch.int32)

    def getMergedClusterLabel_Host(self) -> np.ndarray:
        p = C.c_void_p()
        check(lib().kde_les_merged_label_host(self._h, _stream(), C.byref(p)))
        return np.ctypeslib.as_array(C.cast(p, C.POINTER(C.c_int32)), shape=self._lead() + (self.height, self.width)).copy()

    def getMergedClusterND_Host(self) -> np.ndarray:
        p = C.c_void_p()
        check(lib().kde_les_merged_nd_host(self._h, _stream(), C.byref(p)))
        return np.ctypeslib.as_array(C.cast(p, C.POINTER(C.c_float)), shape=self._lead() + (self.height, self.width, 4)).copy()

    def getNormalImg(self) -> np.ndarray:
        """LabelEquivalenceSeg.cpp:109-124: per pixel its region's normal as (unsigned char)(255*(n+1)/2), black where
        the merged label is -1"""
        labels, nd = self.getMergedClusterLabel_Host(), self.getMergedClusterND_Host()
        v = np.float32(255.0) * (nd[..., :3] + np.float32(1.0)) / np.float32(2.0)
        v = np.where(np.isfinite(v), v, 0.0)
        img = (np.clip(np.trunc(v), -2147483648, 2147483647).astype(np.int64) & 0xFF).astype(np.uint8)
        return np.where((labels > -1)[..., None], img, 0).astype(np.uint8)

    def getSegmentResult(self) -> np.ndarray:
        """LabelEquivalenceSeg.cpp:87-108: one colour per merged label from a fixed-seed palette (the reference
        draws them with rand()), black where the merged label is -1"""
        labels = self.getMergedClusterLabel_Host()
        palette = np.random.default_rng(12345).integers(0, 256, (max(self._k, 1), 3)).astype(np.uint8)
        return np.where((labels > -1)[..., None], palette[np.clip(labels, 0, max(self._k, 1) - 1)], 0).astype(np.uint8)


class PlaneProjection(_Handle):
    """Projection_GPU/Projection_GPU.h, the five-argument PlaneProjection: projects every pixel of an agreeing region onto
    the region's plane, replaces or blends the measured depth where the two are close and the region is large, and smooths
    with a depth-bilateral filter.  Takes what LabelEquivalenceSeg's four *_Device getters return.  After
    plane_projection_batch the getters return the n frames of the call ([n, ...]); after PlaneProjection one frame."""
    _destroy = "kde_proj_destroy"

    def __init__(self, width: int, height: int, intrinsic, max_batch: int = 1, params: Optional[ProjParams] = None):
        super().__init__()
        self.width, self.height, self.max_batch = width, height, max_batch
        self._n = 1
        k = _K9(intrinsic)
        check(lib().kde_proj_create(C.byref(self._h), width, height, max_batch, k.ctypes.data,
                                    C.byref(params) if params is not None else None))

    @staticmethod
    def default_params() -> ProjParams:
        p = ProjParams()
        check(lib().kde_proj_default_params(C.byref(p)))
        return p

    def PlaneProjection(self, nd_device: torch.Tensor, labels_device: torch.Tensor, variance_device: torch.Tensor,
                        points3d_device: torch.Tensor, size_device: torch.Tensor) -> None:
        """Projection_GPU.cu:248-272; the number of table entries is the length of variance_device"""
        if not isinstance(variance_device, torch.Tensor) or variance_device.dim() != 1:
            raise ValueError("variance_device: expected a [k] tensor")
        k, hw = variance_device.shape[0], (self.height, self.width)
        _req(nd_device, torch.float32, hw + (4,), "nd_device")
        _req(labels_device, torch.int32, hw, "labels_device")
        _req(variance_device, torch.float32, (k,), "variance_device")
        _req(points3d_device, torch.float32, hw + (3,), "points3d_device")
        _req(size_device, torch.int32, (k,), "size_device")
        check(lib().kde_proj_plane_projection(self._h, nd_device.data_ptr(), labels_device.data_ptr(), variance_device.data_ptr(),
                                              points3d_device.data_ptr(), size_device.data_ptr(), k, _stream()))
        self._n = 1

    def plane_projection_batch(self, nd: torch.Tensor, labels: torch.Tensor, variance: torch.Tensor, points: torch.Tensor,
                               size: torch.Tensor) -> None:
        """n independent frames back to back ([n, H, W, 4], [n, H, W], [n, k], [n, H, W, 3], [n, k]); each frame's result is
        bit-identical to its PlaneProjection"""
        if not isinstance(variance, torch.Tensor) or variance.dim() != 2:
            raise ValueError("variance: expected a [n, k] tensor")
        n, k = variance.shape
        hw = (self.height, self.width)
        _req(nd, torch.float32, (n,) + hw + (4,), "nd")
        _req(labels, torch.int32, (n,) + hw, "labels")
        _req(variance, torch.float32, (n, k), "variance")
        _req(points, torch.float32, (n,) + hw + (3,), "points")
        _req(size, torch.int32, (n, k), "size")
        check(lib().kde_proj_plane_projection_batch(self._h, n, nd.data_ptr(), labels.data_ptr(), variance.data_ptr(),
                                                    points.data_ptr(), size.data_ptr(), k, _stream()))
        self._n = n

    def _lead(self):
        return () if self._n == 1 else (self._n,)

    def _device(self, fn):
        p = C.c_void_p()
        check(getattr(lib(), fn)(self._h, C.byref(p)))
        return _view(p.value, self._lead() + (self.height, self.width, 3), torch.float32, self)

    def _host(self, fn):
        p = C.c_void_p()
        check(getattr(lib(), fn)(self._h, _stream(), C.byref(p)))
        return np.ctypeslib.as_array(C.cast(p, C.POINTER(C.c_float)), shape=self._lead() + (self.height, self.width, 3)).copy()

    def GetOptimized3D_Device(self) -> torch.Tensor:
        return self._device("kde_proj_optimized_points_device")

    def GetOptimized3D_Host(self) -> np.ndarray:
        return self._host("kde_proj_optimized_points_host")

    def GetPlaneFitted3D_Device(self) -> torch.Tensor:
        return self._device("kde_proj_plane_fitted_points_device")

    def GetPlaneFitted3D_Host(self) -> np.ndarray:
        return self._host("kde_proj_plane_fitted_points_host")


class KinectDepthEnhancement(_Handle):
    """KinectDepthEnhancement.h: the reference's "PROPOSED" method (main.cpp:198-202).  Process = JointBilateralFilter,
    projectiveToReal, NormalMapGenerator (CM), NormalAdaptiveSuperpixel (10, 50, 50, 150, 1), LabelEquivalenceSeg and the
    five-argument PlaneProjection (KinectDepthEnhancement.cpp:56-81).  getRefinedDepth_* is not built: it returns a buffer
    Process never writes; points_to_depth(getOptimizedPoints_Device()) is the enhanced depth map, and
    KinectDepthEnhancementFeed runs Process on frames in host memory and returns it in the sensor's own format."""
    _destroy = "kde_enh_destroy"

    def __init__(self, width: int, height: int, max_batch: int = 1):
        super().__init__()
        self.width, self.height, self.max_batch = width, height, max_batch
        self._n = 1
        check(lib().kde_enh_create(C.byref(self._h), width, height, max_batch))

    def SetParametor(self, rows: int, cols: int, intrinsic) -> None:
        k = _K9(intrinsic)
        check(lib().kde_enh_set_parameters(self._h, rows, cols, k.ctypes.data))

    def Process(self, depth_device: torch.Tensor, color_device: torch.Tensor) -> None:
        _req(depth_device, torch.float32, (self.height, self.width), "depth_device")
        _req(color_device, torch.uint8, (self.height, self.width, 3), "color_device")
        check(lib().kde_enh_process_batch(self._h, 1, depth_device.data_ptr(), color_device.data_ptr(), _stream()))
        self._n = 1

    def process_batch(self, depth: torch.Tensor, color: torch.Tensor) -> None:
        """n independent frames back to back ([n, H, W] and [n, H, W, 3])"""
        n = depth.shape[0]
        _req(depth, torch.float32, (n, self.height, self.width), "depth")
        _req(color, torch.uint8, (n, self.height, self.width, 3), "color")
        check(lib().kde_enh_process_batch(self._h, n, depth.data_ptr(), color.data_ptr(), _stream()))
        self._n = n

    def _get(self, fn, trailing, dtype):
        p = C.c_void_p()
        check(getattr(lib(), fn)(self._h, C.byref(p)))
        lead = () if self._n == 1 else (self._n,)
        return _view(p.value, lead + (self.height, self.width) + trailing, dtype, self)

    def getOptimizedPoints_Device(self) -> torch.Tensor:
        return self._get("kde_enh_optimized_points_device", (3,), torch.float32)

    def getOptimizedPoints_Host(self) -> np.ndarray:
        p = C.c_void_p()
        check(lib().kde_enh_optimized_points_host(self._h, _stream(), C.byref(p)))
        lead = () if self._n == 1 else (self._n,)
        return np.ctypeslib.as_array(C.cast(p, C.POINTER(C.c_float)), shape=lead + (self.height, self.width, 3)).copy()

    def getLabelDevice(self) -> torch.Tensor:
        """NASP->getLabelDevice(): the superpixel labels before merging"""
        return self._get("kde_enh_nasp_labels_device", (), torch.int32)

    def getMergedClusterLabel_Device(self) -> torch.Tensor:
        return self._get("kde_enh_merged_labels_device", (), torch.int32)

    def getEdgeEnhanced3DPoints_Device(self) -> torch.Tensor:
        return self._get("kde_enh_edge_enhanced_points_device", (3,), torch.float32)


_U16 = getattr(torch, "uint16", None)     # torch builds before 2.3 have no uint16


def points_to_depth(points: torch.Tensor, out: Optional[torch.Tensor] = None, dtype=torch.float32) -> torch.Tensor:
    """kde_points_to_depth on torch's current stream: the z of packed points [..., 3] (CUDA float32, contiguous) as a depth
    map of shape points.shape[:-1].  dtype torch.float32 copies the bits of z; torch.uint16 gives the sensor's format
    (millimetres rounded half to even, 0 = invalid: NaN, +-inf, z < 0.5, z >= 65535.5).  Where the torch build has no
    uint16 (before 2.3), pass dtype=torch.int16: the result is an int16 tensor holding the uint16 bits
    (`.cpu().numpy().view(numpy.uint16)`); an int16 `out` is accepted as such a view on every build."""
    if not isinstance(points, torch.Tensor) or not points.is_cuda:
        raise TypeError("points: expected a CUDA tensor")
    if points.dtype != torch.float32 or points.dim() < 1 or points.shape[-1] != 3 or not points.is_contiguous():
        raise ValueError(f"points: expected contiguous torch.float32 [..., 3], got {points.dtype} {tuple(points.shape)}")
    if dtype == torch.float32:
        fmt, store = _native.KDE_DEPTH_F32, (torch.float32,)
    elif dtype is not None and dtype in (_U16, torch.int16):
        fmt, store = _native.KDE_DEPTH_U16, tuple(t for t in (_U16, torch.int16) if t is not None)
    else:
        raise ValueError(f"dtype: expected torch.float32 or torch.uint16, got {dtype}")
    shape = tuple(points.shape[:-1])
    if out is None:
        out = torch.empty(shape, dtype=dtype, device=points.device)
    elif not isinstance(out, torch.Tensor) or not out.is_cuda:
        raise TypeError("out: expected a CUDA tensor")
    elif out.dtype not in store or tuple(out.shape) != shape or not out.is_contiguous() or out.device != points.device:
        raise ValueError(f"out: expected contiguous {store[0]} {shape} on {points.device}, got {out.dtype} {tuple(out.shape)}")
    with torch.cuda.device(points.device):
        check(lib().kde_points_to_depth(out.numel(), points.data_ptr(), fmt, out.data_ptr(), _stream()))
    return out


def _source_of(width: int, height: int, t, name: str):
    """(kde_error3d_source, frames) of a contiguous CUDA tensor [f,H,W,3] float32 or [f,H,W] float32 / uint16 / int16"""
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise TypeError(f"{name}: expected a CUDA tensor")
    hw = (height, width)
    if t.dtype == torch.float32 and t.dim() == 4 and tuple(t.shape[1:]) == hw + (3,):
        fmt = _native.KDE_SRC_POINTS_F32
    elif t.dtype == torch.float32 and t.dim() == 3 and tuple(t.shape[1:]) == hw:
        fmt = _native.KDE_SRC_DEPTH_F32
    elif t.dtype in (torch.int16, _U16) and t.dim() == 3 and tuple(t.shape[1:]) == hw:
        fmt = _native.KDE_SRC_DEPTH_U16
    else:
        raise ValueError(f"{name}: expected float32 [n,{hw[0]},{hw[1]},3] (points) or float32 / uint16 [n,{hw[0]},{hw[1]}] "
                         f"(depth), got {t.dtype} {tuple(t.shape)}")
    if not t.is_contiguous():
        raise ValueError(f"{name}: expected a contiguous tensor")
    return _native.Error3dSource(t.data_ptr(), fmt), t.shape[0]


class MeanError3D(_Handle):
    """The reference's quality figure (main.cpp:220-308) on the device (kde_error3d_*): the mean 3-D distance of up to
    `max_candidates` results from one ground truth over the pixels where both are valid, for up to `max_batch` frames in
    one call.  A source is a cloud ([n,H,W,3] float32) or a depth map ([n,H,W] float32, or uint16 / int16 holding the
    sensor's uint16), which stands for the cloud DimensionConvertor.projectiveToReal makes of it with the camera of
    set_camera.  The table holds, per frame and candidate, the binary64 sum of the float32 terms, the number of valid
    pixels and mean = float32(sum / count) (NaN when count is 0); it is deterministic to the bit."""
    _destroy = "kde_error3d_destroy"
    _handle_type = _native.Error3dHandle
    RESULT_DTYPE = np.dtype([("sum", "<f8"), ("count", "<u4"), ("mean", "<f4")])

    def __init__(self, width: int, height: int, max_batch: int = 1, max_candidates: int = 8):
        super().__init__()
        self.width, self.height, self.max_batch, self.max_candidates = width, height, max_batch, max_candidates
        self._n = self._m = 0
        check(lib().kde_error3d_create(C.byref(self._h), width, height, max_batch, max_candidates))

    def set_camera(self, K) -> None:
        k = _K9(K)
        check(lib().kde_error3d_set_camera(self._h, k.ctypes.data))

    def set_range(self, z_min: float, z_max: float) -> None:
        check(lib().kde_error3d_set_range(self._h, z_min, z_max))

    def _source(self, t, name: str):
        return _source_of(self.width, self.height, t, name)

    def compare(self, candidates, truth: torch.Tensor) -> None:
        """candidates: a sequence of 1..max_candidates tensors of n frames each; truth: n frames or 1 (the same truth for
        every frame).  Asynchronous on torch's current stream; no allocation, copy or synchronisation on the device."""
        cands = list(candidates)
        if not cands:
            raise ValueError("candidates: expected at least one tensor")
        srcs = (_native.Error3dSource * len(cands))()
        n = None
        for i, t in enumerate(cands):
            srcs[i], frames = self._source(t, f"candidates[{i}]")
            if n is not None and frames != n:
                raise ValueError(f"candidates[{i}]: {frames} frames, candidates[0] has {n}")
            n = frames
        tsrc, tframes = self._source(truth, "truth")
        check(lib().kde_error3d_compare_batch(self._h, n, len(cands), srcs, C.byref(tsrc), tframes, _stream()))
        self._n, self._m = n, len(cands)

    def results_device(self) -> torch.Tensor:
        """the [n, m] table of the last compare as raw bytes [n, m, 16] (sum: float64, count: uint32, mean: float32), a view
        of the object-owned buffer"""
        p = C.c_void_p()
        check(lib().kde_error3d_results_device(self._h, C.byref(p)))
        return _view(p.value, (self._n, self._m, 16), torch.uint8, self)

    def results_host(self) -> np.ndarray:
        """the [n, m] table as a numpy structured array (RESULT_DTYPE); synchronises torch's current stream"""
        p = C.c_void_p()
        check(lib().kde_error3d_results_host(self._h, _stream(), C.byref(p)))
        raw = np.ctypeslib.as_array(C.cast(p, C.POINTER(C.c_uint8)), shape=(self._n * self._m * 16,)).copy()
        return raw.view(self.RESULT_DTYPE).reshape(self._n, self._m)


class PointCloudXYZRGB(_Handle):
    """The output step of the reference (main.cpp:211-300) on the device (kde_cloud_*): a method's result and the colour
    image become the coloured cloud the reference pushes into a pcl::PointCloud<pcl::PointXYZRGB>, for up to `max_batch`
    frames in one call.  A source is a cloud ([n,H,W,3] float32, millimetres) or a depth map ([n,H,W] float32, or uint16 /
    int16 holding the sensor's uint16), which stands for the cloud DimensionConvertor.projectiveToReal makes of it with the
    camera of set_camera.  A pixel is valid iff z_min < z < z_max; its record is (x / divisor, y / divisor, -z / divisor,
    (r << 16) | (g << 8) | b).  Dense mode (the default) leaves the valid records of frame f, in raster order, in the first
    counts()[f] records of the frame's slot of W * H records and writes nothing behind them; organized=True writes every
    pixel, the invalid ones as three NaNs with their colour."""
    _destroy = "kde_cloud_destroy"
    _handle_type = _native.CloudHandle
    POINT_DTYPE = np.dtype([("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("rgb", "<u4")])

    def __init__(self, width: int, height: int, max_batch: int = 1, z_min: float = 50.0, z_max: float = 15000.0,
                 divisor: float = 1000.0, negate_z: bool = True, organized: bool = False):
        super().__init__()
        self.width, self.height, self.max_batch, self.organized = width, height, max_batch, bool(organized)
        self._n = 0
        p = _native.CloudParams(z_min, z_max, divisor, int(bool(negate_z)), int(bool(organized)))
        check(lib().kde_cloud_create(C.byref(self._h), width, height, max_batch, C.byref(p)))

    @staticmethod
    def default_params() -> "_native.CloudParams":
        p = _native.CloudParams()
        check(lib().kde_cloud_default_params(C.byref(p)))
        return p

    def set_camera(self, K) -> None:
        k = _K9(K)
        check(lib().kde_cloud_set_camera(self._h, k.ctypes.data))

    def build(self, source: torch.Tensor, bgr: torch.Tensor, out: Optional[torch.Tensor] = None) -> None:
        """source: n frames; bgr: uint8 [n,H,W,3] or [1,H,W,3] (one image for every frame); out: uint8 [n, H*W, 16] for the
        records, or None for the object-owned buffer.  Asynchronous on torch's current stream; no allocation, copy or
        synchronisation on the device."""
        src, n = _source_of(self.width, self.height, source, "source")
        if not isinstance(bgr, torch.Tensor) or bgr.dim() != 4 or bgr.shape[0] not in (1, n):
            raise ValueError(f"bgr: expected [1 or {n},{self.height},{self.width},3] uint8")
        _req(bgr, torch.uint8, (bgr.shape[0], self.height, self.width, 3), "bgr")
        if out is not None:
            _req(out, torch.uint8, (n, self.height * self.width, 16), "out")
        check(lib().kde_cloud_build_batch(self._h, n, C.byref(src), bgr.data_ptr(), bgr.shape[0], _ptr(out), _stream()))
        self._n = n

    def counts(self) -> np.ndarray:
        """the number of valid pixels per frame of the last build, uint32 [n]; synchronises torch's current stream"""
        p = C.c_void_p()
        check(lib().kde_cloud_counts_host(self._h, _stream(), C.byref(p)))
        return np.ctypeslib.as_array(C.cast(p, C.POINTER(C.c_uint32)), shape=(self._n,)).copy()

    def counts_device(self) -> torch.Tensor:
        """the same on the device, as raw bytes [n, 4] (uint32), a view of the object-owned buffer"""
        p = C.c_void_p()
        check(lib().kde_cloud_counts_device(self._h, C.byref(p)))
        return _view(p.value, (self._n, 4), torch.uint8, self)

    def points_device(self) -> torch.Tensor:
        """the records of the last build as raw bytes [n, H*W, 16] (POINT_DTYPE): `out` of that call or the object-owned
        buffer.  In dense mode only the first counts()[f] records of frame f are defined."""
        p = C.c_void_p()
        check(lib().kde_cloud_points_device(self._h, C.byref(p)))
        return _view(p.value, (self._n, self.height * self.width, 16), torch.uint8, self)

    def points_host(self) -> list:
        """one structured array (POINT_DTYPE) per frame: counts()[f] records in dense mode, H*W in organised mode;
        synchronises torch's current stream"""
        p, off = C.c_void_p(), C.c_void_p()
        check(lib().kde_cloud_points_host(self._h, _stream(), C.byref(p), C.byref(off)))
        offsets = np.ctypeslib.as_array(C.cast(off, C.POINTER(C.c_uint64)), shape=(self._n + 1,)).copy()
        self.offsets = offsets
        total = int(offsets[-1])
        if total == 0:
            return [np.empty(0, self.POINT_DTYPE) for _ in range(self._n)]
        raw = np.ctypeslib.as_array(C.cast(p, C.POINTER(C.c_uint8)), shape=(total * 16,)).copy().view(self.POINT_DTYPE)
        return [raw[int(offsets[f]):int(offsets[f + 1])] for f in range(self._n)]


class OrganizedMesh(_Handle):
    """The surface of main.cpp:211-300 as a triangle mesh of the organised grid (kde_mesh_*), for up to `max_batch` frames in
    one call.  A source is what PointCloudXYZRGB takes.  The vertices are exactly that class's dense cloud (the same bytes);
    the vertex index of a valid pixel is its rank in raster order.  Pixel (x, y), x < W-1, y < H-1, owns the quad a = (x, y),
    b = (x+1, y), c = (x, y+1), d = (x+1, y+1); a triangle is emitted iff its corners are valid and its edges linked,
    |za - zb| <= max_diff + rel_diff * min(za, zb) on the source's z in millimetres.  Four valid corners are cut along a-d
    (diagonal = DIAG_AD), b-c (DIAG_BC) or the shorter of the two in z (DIAG_ADAPTIVE, the default; a tie goes to a-d); three
    valid corners give their one triangle.  Triangles are 12-byte records of three uint32, ordered by owning pixel, the first
    tri_counts()[f] records of frame f's slot of 2 (W-1) (H-1); nothing is written behind them."""
    _destroy = "kde_mesh_destroy"
    _handle_type = _native.MeshHandle
    POINT_DTYPE = np.dtype([("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("rgb", "<u4")])
    TRIANGLE_DTYPE = np.dtype([("v0", "<u4"), ("v1", "<u4"), ("v2", "<u4")])
    DIAG_AD, DIAG_BC, DIAG_ADAPTIVE = _native.KDE_MESH_DIAG_AD, _native.KDE_MESH_DIAG_BC, _native.KDE_MESH_DIAG_ADAPTIVE

    def __init__(self, width: int, height: int, max_batch: int = 1, z_min: float = 50.0, z_max: float = 15000.0,
                 divisor: float = 1000.0, negate_z: bool = True, max_diff: float = 10.0, rel_diff: float = 0.02,
                 diagonal: int = _native.KDE_MESH_DIAG_ADAPTIVE, flip_winding: bool = False):
        super().__init__()
        self.width, self.height, self.max_batch = width, height, max_batch
        self.tri_slot = 2 * (width - 1) * (height - 1)
        self._n = 0
        p = _native.MeshParams(z_min, z_max, divisor, int(bool(negate_z)), max_diff, rel_diff, int(diagonal), int(bool(flip_winding)))
        check(lib().kde_mesh_create(C.byref(self._h), width, height, max_batch, C.byref(p)))

    @staticmethod
    def default_params() -> "_native.MeshParams":
        p = _native.MeshParams()
        check(lib().kde_mesh_default_params(C.byref(p)))
        return p

    def set_camera(self, K) -> None:
        k = _K9(K)
        check(lib().kde_mesh_set_camera(self._h, k.ctypes.data))

    def build(self, source: torch.Tensor, bgr: torch.Tensor, vertices_out: Optional[torch.Tensor] = None,
              triangles_out: Optional[torch.Tensor] = None) -> None:
        """source: n frames; bgr: uint8 [n,H,W,3] or [1,H,W,3]; vertices_out: uint8 [n, H*W, 16], triangles_out: uint8
        [n, 2(W-1)(H-1), 12] (on a 4-byte boundary), or None for the object-owned buffers.  Asynchronous on torch's current
        stream; no allocation, copy or synchronisation on the device."""
        src, n = _source_of(self.width, self.height, source, "source")
        if not isinstance(bgr, torch.Tensor) or bgr.dim() != 4 or bgr.shape[0] not in (1, n):
            raise ValueError(f"bgr: expected [1 or {n},{self.height},{self.width},3] uint8")
        _req(bgr, torch.uint8, (bgr.shape[0], self.height, self.width, 3), "bgr")
        if vertices_out is not None:
            _req(vertices_out, torch.uint8, (n, self.height * self.width, 16), "vertices_out")
        if triangles_out is not None:
            _req(triangles_out, torch.uint8, (n, self.tri_slot, 12), "triangles_out")
        check(lib().kde_mesh_build_batch(self._h, n, C.byref(src), bgr.data_ptr(), bgr.shape[0], _ptr(vertices_out),
                                         _ptr(triangles_out), _stream()))
        self._n = n

    def _u32_host(self, name: str) -> np.ndarray:
        p = C.c_void_p()
        check(getattr(lib(), name)(self._h, _stream(), C.byref(p)))
        return np.ctypeslib.as_array(C.cast(p, C.POINTER(C.c_uint32)), shape=(self._n,)).copy()

    def counts(self) -> np.ndarray:
        """the number of vertices per frame of the last build, uint32 [n]; synchronises torch's current stream"""
        return self._u32_host("kde_mesh_counts_host")

    def tri_counts(self) -> np.ndarray:
        """the number of triangles per frame of the last build, uint32 [n]; synchronises torch's current stream"""
        return self._u32_host("kde_mesh_tri_counts_host")

    def _device(self, name: str, shape) -> torch.Tensor:
        p = C.c_void_p()
        check(getattr(lib(), name)(self._h, C.byref(p)))
        return _view(p.value, shape, torch.uint8, self)

    def counts_device(self) -> torch.Tensor:
        """counts() on the device, as raw bytes [n, 4] (uint32), a view of the object-owned buffer"""
        return self._device("kde_mesh_counts_device", (self._n, 4))

    def tri_counts_device(self) -> torch.Tensor:
        """tri_counts() on the device, as raw bytes [n, 4] (uint32), a view of the object-owned buffer"""
        return self._device("kde_mesh_tri_counts_device", (self._n, 4))

    def vertices_device(self) -> torch.Tensor:
        """the vertex records of the last build as raw bytes [n, H*W, 16] (POINT_DTYPE); only the first counts()[f] of frame f
        are defined"""
        return self._device("kde_mesh_vertices_device", (self._n, self.height * self.width, 16))

    def triangles_device(self) -> torch.Tensor:
        """the triangle records of the last build as raw bytes [n, 2(W-1)(H-1), 12] (TRIANGLE_DTYPE); only the first
        tri_counts()[f] of frame f are defined"""
        return self._device("kde_mesh_triangles_device", (self._n, self.tri_slot, 12))

    def _packed_host(self, name: str, dtype) -> tuple:
        p, off = C.c_void_p(), C.c_void_p()
        check(getattr(lib(), name)(self._h, _stream(), C.byref(p), C.byref(off)))
        offsets = np.ctypeslib.as_array(C.cast(off, C.POINTER(C.c_uint64)), shape=(self._n + 1,)).copy()
        total = int(offsets[-1])
        if total == 0:
            return [np.empty(0, dtype) for _ in range(self._n)], offsets
        raw = np.ctypeslib.as_array(C.cast(p, C.POINTER(C.c_uint8)), shape=(total * dtype.itemsize,)).copy().view(dtype)
        return [raw[int(offsets[f]):int(offsets[f + 1])] for f in range(self._n)], offsets

    def vertices_host(self) -> list:
        """one structured array (POINT_DTYPE) of counts()[f] records per frame (offsets in self.offsets); synchronises"""
        frames, self.offsets = self._packed_host("kde_mesh_vertices_host", self.POINT_DTYPE)
        return frames

    def triangles_host(self) -> list:
        """one structured array (TRIANGLE_DTYPE) of tri_counts()[f] records per frame (offsets in self.tri_offsets);
        synchronises"""
        frames, self.tri_offsets = self._packed_host("kde_mesh_triangles_host", self.TRIANGLE_DTYPE)
        return frames


class _DepthStage(_Handle):
    """What the depth-in / depth-out stages share (csrc/kde_depth_stage.h in the library): n depth frames in as float32 or
    uint16, n frames out in either format, the results of the last batch call.  A subclass names its C prefix and its
    parameter struct, sets self._out_hw = (height, width) of an output frame in __init__ and records every batch call
    with _finished()."""
    _prefix = None                  # "kde_reg_", ...: default_params and the getters are this plus their name
    _params_type = None

    def __init__(self, max_batch: int):
        super().__init__()
        self.max_batch = max_batch
        self._n, self._fmt = 0, _native.KDE_DEPTH_F32

    @classmethod
    def default_params(cls):
        p = cls._params_type()
        check(getattr(lib(), cls._prefix + "default_params")(C.byref(p)))
        return p

    def _fn(self, name: str):
        return getattr(lib(), self._prefix + name)

    @staticmethod
    def _check_depth(depth: torch.Tensor, height: int, width: int):
        """(n, KDE_DEPTH_*) of an input depth tensor [n,height,width]"""
        if not isinstance(depth, torch.Tensor) or not depth.is_cuda:
            raise TypeError("depth: expected a CUDA tensor")
        if depth.dim() != 3 or tuple(depth.shape[1:]) != (height, width) or not depth.is_contiguous() or \
                depth.dtype not in (torch.float32, torch.int16, _U16):
            raise ValueError(f"depth: expected contiguous float32 / uint16 [n,{height},{width}], got "
                             f"{depth.dtype} {tuple(depth.shape)}")
        return depth.shape[0], (_native.KDE_DEPTH_F32 if depth.dtype == torch.float32 else _native.KDE_DEPTH_U16)

    def _out_format(self, out: Optional[torch.Tensor], out_format, n: int) -> int:
        """KDE_DEPTH_* of a batch call's output: the dtype of `out` [n, output frame], or out_format where out is None"""
        dt = out.dtype if isinstance(out, torch.Tensor) else out_format
        if dt == torch.float32:
            ofmt = _native.KDE_DEPTH_F32
        elif dt is not None and dt in (torch.int16, _U16):
            ofmt = _native.KDE_DEPTH_U16
        else:
            raise ValueError(f"out_format: expected torch.float32 or torch.uint16, got {dt}")
        if out is not None:
            _req(out, dt, (n,) + self._out_hw, "out")
        return ofmt

    @staticmethod
    def _check_guide(bgr: torch.Tensor, n: int, height: int, width: int) -> None:
        if not isinstance(bgr, torch.Tensor) or bgr.dim() != 4 or bgr.shape[0] not in (1, n):
            raise ValueError(f"bgr: expected [1 or {n},{height},{width},3] uint8")
        _req(bgr, torch.uint8, (bgr.shape[0], height, width, 3), "bgr")

    def _finished(self, n: int, ofmt: int, out: Optional[torch.Tensor]) -> torch.Tensor:
        self._n, self._fmt = n, ofmt
        return out if out is not None else self.depth_device()

    def depth_device(self) -> torch.Tensor:
        """the frames of the last batch call: `out` of that call or the object-owned buffer, [n,Ho,Wo] float32, or int16
        holding the uint16 bits (`.cpu().numpy().view(numpy.uint16)`)"""
        p = C.c_void_p()
        check(self._fn("depth_device")(self._h, C.byref(p)))
        h, w = self._out_hw
        if self._fmt == _native.KDE_DEPTH_F32:
            return _view(p.value, (self._n, h, w), torch.float32, self)
        return _view(p.value, (self._n, h, w * 2), torch.uint8, self).view(torch.int16)

    def depth_host(self) -> np.ndarray:
        """the same as a numpy array, float32 or uint16; synchronises torch's current stream"""
        p = C.c_void_p()
        check(self._fn("depth_host")(self._h, _stream(), C.byref(p)))
        ctype, dtype = (C.c_float, np.float32) if self._fmt == _native.KDE_DEPTH_F32 else (C.c_uint16, np.uint16)
        return np.ctypeslib.as_array(C.cast(p, C.POINTER(ctype)), shape=(self._n,) + self._out_hw).astype(dtype, copy=True)

    def _count_host(self, fn) -> np.ndarray:
        p = C.c_void_p()
        check(fn(self._h, _stream(), C.byref(p)))
        return np.ctypeslib.as_array(C.cast(p, C.POINTER(C.c_uint32)), shape=(self._n,)).copy()

    def _count_device(self, fn) -> torch.Tensor:
        p = C.c_void_p()
        check(fn(self._h, C.byref(p)))
        return _view(p.value, (self._n, 4), torch.uint8, self)

    def filled(self) -> np.ndarray:
        """the number of pixels per frame the last batch call gave a depth, uint32 [n]; synchronises torch's current stream"""
        return self._count_host(self._fn("filled_host"))

    def filled_device(self) -> torch.Tensor:
        """the same on the device, as raw bytes [n, 4] (uint32), a view of the object-owned buffer"""
        return self._count_device(self._fn("filled_device"))


class DepthRegistration(_DepthStage):
    """What Kinect::InitAllData (Kinect.cpp:71-75) asks OpenNI for, on the device (kde_reg_*): depth frames warped into the
    colour camera's view, so that depth pixel (x, y) and colour pixel (x, y) look along the same ray, as every other class
    here assumes.  depth_size and color_size are (width, height); params is a RegParams (z_min, z_max, max_splat) or None
    for the defaults (0, FLT_MAX, point mode).  The rule is stated in include/kde_hip.h: a scatter through a z-buffer, the
    nearest source pixel wins, deterministic to the bit; cx and cy are kept as floats, there is no lens distortion."""
    _destroy, _prefix = "kde_reg_destroy", "kde_reg_"
    _handle_type, _params_type = _native.RegHandle, _native.RegParams

    def __init__(self, depth_size, color_size, max_batch: int = 1, params: Optional["_native.RegParams"] = None):
        super().__init__(max_batch)
        (self.depth_width, self.depth_height), (self.color_width, self.color_height) = depth_size, color_size
        self._out_hw = (self.color_height, self.color_width)
        check(lib().kde_reg_create(C.byref(self._h), self.depth_width, self.depth_height, self.color_width, self.color_height,
                                   max_batch, None if params is None else C.byref(params)))

    def set_calibration(self, Kd, Kc, R, t) -> None:
        """Kd, Kc, R: 3 x 3 (row-major); t: 3 values in millimetres; P_colour = R * P_depth + t"""
        kd, kc, r = _K9(Kd), _K9(Kc), _K9(R)
        tt = np.ascontiguousarray(np.asarray(t, np.float64).reshape(3))
        check(lib().kde_reg_set_calibration(self._h, kd.ctypes.data, kc.ctypes.data, r.ctypes.data, tt.ctypes.data))

    def register(self, depth: torch.Tensor, out: Optional[torch.Tensor] = None, out_format=torch.float32) -> torch.Tensor:
        """depth: [n,Hd,Wd] float32, or uint16 / int16 holding the sensor's uint16.  out: [n,Hc,Wc] float32 or uint16 / int16
        (its dtype is the output format), or None for the object-owned buffer in out_format (torch.float32, torch.uint16 or
        torch.int16).  Returns the registered frames (0 where no source pixel came).  Asynchronous on torch's current stream;
        no allocation, copy or synchronisation on the device."""
        n, fmt = self._check_depth(depth, self.depth_height, self.depth_width)
        ofmt = self._out_format(out, out_format, n)
        check(lib().kde_reg_register_batch(self._h, n, depth.data_ptr(), fmt, ofmt, _ptr(out), _stream()))
        return self._finished(n, ofmt, out)

    def color_to_depth(self, depth: torch.Tensor, bgr: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """the companion gather: bgr uint8 [n,Hc,Wc,3] or [1,Hc,Wc,3] as the depth camera sees it, uint8 [n,Hd,Wd,3]: the colour
        at the point-mode target of each valid depth pixel, (0, 0, 0) elsewhere.  No occlusion test."""
        n, fmt = self._check_depth(depth, self.depth_height, self.depth_width)
        self._check_guide(bgr, n, self.color_height, self.color_width)
        if out is None:
            out = torch.empty((n, self.depth_height, self.depth_width, 3), dtype=torch.uint8, device=depth.device)
        else:
            _req(out, torch.uint8, (n, self.depth_height, self.depth_width, 3), "out")
        check(lib().kde_reg_color_to_depth_batch(self._h, n, depth.data_ptr(), fmt, bgr.data_ptr(), bgr.shape[0], out.data_ptr(),
                                                 _stream()))
        return out


class LensUndistortion(_DepthStage):
    """Frames of a camera with lens distortion resampled into the pinhole view every other class here assumes, on the device
    (kde_undist_*): OpenCV's rational model (k1, k2, p1, p2, k3, k4, k5, k6; zeros for k4..k6 give Brown-Conrady), no
    rectifying rotation.  src_size and out_size are (width, height); params is an UndistParams (z_min, z_max, depth_interp,
    max_gap) or None for the defaults (0, FLT_MAX, nearest).  The rule is stated in include/kde_hip.h: colour is bilinear
    with (0, 0, 0) outside the source, depth is the nearest valid sample or, with depth_interp 1, bilinear where the four
    taps are valid and within max_gap of each other; deterministic to the bit."""
    _destroy, _prefix = "kde_undist_destroy", "kde_undist_"
    _handle_type, _params_type = _native.UndistHandle, _native.UndistParams

    def __init__(self, src_size, out_size=None, max_batch: int = 1, params: Optional["_native.UndistParams"] = None):
        super().__init__(max_batch)
        self.src_width, self.src_height = src_size
        self.out_width, self.out_height = out_size if out_size is not None else src_size
        self._out_hw = (self.out_height, self.out_width)
        check(lib().kde_undist_create(C.byref(self._h), self.src_width, self.src_height, self.out_width, self.out_height,
                                      max_batch, None if params is None else C.byref(params)))

    def set_calibration(self, K, dist, K_new=None) -> None:
        """K, K_new: 3 x 3 (row-major), K_new None for K; dist: k1, k2, p1, p2, k3[, k4, k5, k6] (4, 5 or 8 values as OpenCV
        hands them out; the missing ones are 0)"""
        d = np.asarray(dist, np.float64).reshape(-1)
        if d.size not in (4, 5, 8):
            raise ValueError(f"dist: expected 4, 5 or 8 coefficients, got {d.size}")
        d8 = np.zeros(8, np.float64)
        d8[:d.size] = d
        k = _K9(K)
        kn = None if K_new is None else _K9(K_new)
        check(lib().kde_undist_set_calibration(self._h, k.ctypes.data, d8.ctypes.data, None if kn is None else kn.ctypes.data))

    def color(self, bgr: torch.Tensor, n: Optional[int] = None, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """bgr: uint8 [n,Hs,Ws,3], or [1,Hs,Ws,3] with n given (one image for every frame).  Returns uint8 [n,Ho,Wo,3].
        Asynchronous on torch's current stream."""
        if not isinstance(bgr, torch.Tensor) or bgr.dim() != 4:
            raise ValueError(f"bgr: expected [n,{self.src_height},{self.src_width},3] uint8")
        n = bgr.shape[0] if n is None else n
        if bgr.shape[0] not in (1, n):
            raise ValueError(f"bgr: expected 1 or {n} frames, got {bgr.shape[0]}")
        _req(bgr, torch.uint8, (bgr.shape[0], self.src_height, self.src_width, 3), "bgr")
        if out is None:
            out = torch.empty((n, self.out_height, self.out_width, 3), dtype=torch.uint8, device=bgr.device)
        else:
            _req(out, torch.uint8, (n, self.out_height, self.out_width, 3), "out")
        check(lib().kde_undist_color_batch(self._h, n, bgr.data_ptr(), bgr.shape[0], out.data_ptr(), _stream()))
        return out

    def depth(self, depth: torch.Tensor, out: Optional[torch.Tensor] = None, out_format=torch.float32) -> torch.Tensor:
        """depth: [n,Hs,Ws] float32, or uint16 / int16 holding the sensor's uint16.  out: [n,Ho,Wo] float32 or uint16 / int16
        (its dtype is the output format), or None for the object-owned buffer in out_format (torch.float32, torch.uint16 or
        torch.int16).  Returns the undistorted frames (0 where a pixel got no depth).  Asynchronous on torch's current stream;
        no allocation, copy or synchronisation on the device."""
        n, fmt = self._check_depth(depth, self.src_height, self.src_width)
        ofmt = self._out_format(out, out_format, n)
        check(lib().kde_undist_depth_batch(self._h, n, depth.data_ptr(), fmt, ofmt, _ptr(out), _stream()))
        return self._finished(n, ofmt, out)

    def map(self) -> torch.Tensor:
        """(us, vs) of every output pixel, float32 [Ho,Wo,2]: the source point it shows, OpenCV's initUndistortRectifyMap
        product for this calibration.  A view of the object-owned buffer, computed on torch's current stream at the first
        request after set_calibration()."""
        p = C.c_void_p()
        check(lib().kde_undist_map_device(self._h, _stream(), C.byref(p)))
        return _view(p.value, (self.out_height, self.out_width, 2), torch.float32, self)


class GuidedDepthUpsampling(_DepthStage):
    """A low-resolution depth frame brought to the size of its colour image on the device (kde_upsample_*): joint bilateral
    upsampling, low-resolution samples weighted by a tent of radius `radius` around the output pixel and by the resemblance
    of the guide colour at the output pixel to the guide colour at the sample.  src_size and out_size are (width, height),
    out_size no smaller than src_size; params is an UpsampleParams (radius, sigma_color, max_gap, z_min, z_max) or None for the
    defaults (2, 30, no guard, every finite positive depth).  The rule is stated in include/kde_hip.h; deterministic to the
    bit."""
    _destroy, _prefix = "kde_upsample_destroy", "kde_upsample_"
    _handle_type, _params_type = _native.UpsampleHandle, _native.UpsampleParams

    def __init__(self, src_size, out_size, max_batch: int = 1, params: Optional["_native.UpsampleParams"] = None):
        super().__init__(max_batch)
        self.src_width, self.src_height = src_size
        self.out_width, self.out_height = out_size
        self._out_hw = (self.out_height, self.out_width)
        check(lib().kde_upsample_create(C.byref(self._h), self.src_width, self.src_height, self.out_width, self.out_height,
                                        max_batch, None if params is None else C.byref(params)))

    def range_table(self) -> np.ndarray:
        """range[k] for k = |db| + |dg| + |dr| = 0 .. 765 as the kernel reads it, float32 [766]; needs no device"""
        t = np.empty(766, np.float32)
        check(lib().kde_upsample_range_table(self._h, t.ctypes.data, t.size))
        return t

    def upsample(self, depth: torch.Tensor, bgr: torch.Tensor, out: Optional[torch.Tensor] = None,
                 out_format=torch.float32) -> torch.Tensor:
        """depth: [n,Hs,Ws] float32, or uint16 / int16 holding the sensor's uint16.  bgr: the guide, uint8 [n,Ho,Wo,3], or
        [1,Ho,Wo,3] for one guide for every frame.  out: [n,Ho,Wo] float32 or uint16 / int16 (its dtype is the output
        format), or None for the object-owned buffer in out_format (torch.float32, torch.uint16 or torch.int16).  Returns
        the upsampled frames (0 where a pixel got no depth).  Asynchronous on torch's current stream; no allocation, copy
        or synchronisation on the device."""
        n, fmt = self._check_depth(depth, self.src_height, self.src_width)
        self._check_guide(bgr, n, self.out_height, self.out_width)
        ofmt = self._out_format(out, out_format, n)
        check(lib().kde_upsample_depth_batch(self._h, n, depth.data_ptr(), fmt, bgr.data_ptr(), bgr.shape[0], ofmt, _ptr(out), _stream()))
        return self._finished(n, ofmt, out)


class DepthHoleFilling(_DepthStage):
    """The holes of a depth frame filled on the device under the guide of its colour image (kde_holefill_*): `iterations`
    passes, each of which gives the hole pixels with at least `min_taps` usable neighbours within `radius` the mean of those
    neighbours, weighted by distance and by the resemblance of the guide colour; iterations * radius bounds how far a fill
    reaches.  size is (width, height); params is a HolefillParams (radius, iterations, min_taps, sigma_space, sigma_color,
    max_gap, gap_rule, z_min, z_max, passes_per_launch) or None for the defaults (2, 8, 3, 2, 30, no guard, every finite
    positive depth, the library's passes per launch).  The rule is stated in include/kde_hip.h; deterministic to the bit."""
    _destroy, _prefix = "kde_holefill_destroy", "kde_holefill_"
    _handle_type, _params_type = _native.HolefillHandle, _native.HolefillParams

    def __init__(self, size, max_batch: int = 1, params: Optional["_native.HolefillParams"] = None):
        super().__init__(max_batch)
        self.width, self.height = size
        self._out_hw = (self.height, self.width)
        check(lib().kde_holefill_create(C.byref(self._h), self.width, self.height, max_batch, None if params is None else C.byref(params)))
        self.radius = (self.default_params() if params is None else params).radius

    def space_table(self) -> np.ndarray:
        """space[dy + r][dx + r] as the kernel reads it, float32 [2r + 1, 2r + 1]; needs no device"""
        side = 2 * self.radius + 1
        t = np.empty((side, side), np.float32)
        check(lib().kde_holefill_space_table(self._h, t.ctypes.data, t.size))
        return t

    def range_table(self) -> np.ndarray:
        """range[k] for k = |db| + |dg| + |dr| = 0 .. 765 as the kernel reads it, float32 [766]; needs no device"""
        t = np.empty(766, np.float32)
        check(lib().kde_holefill_range_table(self._h, t.ctypes.data, t.size))
        return t

    def passes_per_launch(self) -> int:
        """the number of passes one launch performs: passes_per_launch of the parameters, or the library's choice"""
        k = C.c_int()
        check(lib().kde_holefill_passes_per_launch(self._h, C.byref(k)))
        return k.value

    def fill(self, depth: torch.Tensor, bgr: torch.Tensor, out: Optional[torch.Tensor] = None, out_format=torch.float32,
             pass_of: Optional[torch.Tensor] = None) -> torch.Tensor:
        """depth: [n,H,W] float32, or uint16 / int16 holding the sensor's uint16.  bgr: the guide, uint8 [n,H,W,3], or
        [1,H,W,3] for one guide for every frame.  out: [n,H,W] float32 or uint16 / int16 (its dtype is the output format),
        or None for the object-owned buffer in out_format (torch.float32, torch.uint16 or torch.int16); what is written
        must not overlap depth, so a result returned by fill(..., out=None) goes back in only with an `out` for the new one.  pass_of: uint8 [n,H,W] or None: 0 for an original pixel, p for one filled in pass p, 255 for one that is
        still a hole.  Returns the filled frames (0 where a hole remains).  Asynchronous on torch's current stream; no
        allocation, copy or synchronisation on the device."""
        n, fmt = self._check_depth(depth, self.height, self.width)
        self._check_guide(bgr, n, self.height, self.width)
        ofmt = self._out_format(out, out_format, n)
        if pass_of is not None:
            _req(pass_of, torch.uint8, (n, self.height, self.width), "pass_of")
        check(lib().kde_holefill_fill_batch(self._h, n, depth.data_ptr(), fmt, bgr.data_ptr(), bgr.shape[0], ofmt, _ptr(out), _ptr(pass_of),
                                            _stream()))
        return self._finished(n, ofmt, out)

    def remaining(self) -> np.ndarray:
        """the number of pixels per frame that are still holes after the last fill(), uint32 [n]; synchronises"""
        return self._count_host(lib().kde_holefill_remaining_host)

    def remaining_device(self) -> torch.Tensor:
        """remaining on the device, as raw bytes [n, 4] (uint32), a view of the object-owned buffer"""
        return self._count_device(lib().kde_holefill_remaining_device)


class DepthSpeckleFilter(_DepthStage):
    """Wrong depth taken away on the device (kde_speckle_*): the connected components of a frame under a depth-difference
    link, those smaller than `min_size` set to 0 -- flying pixels, speckles, background showing through a registered
    foreground.  It sits behind registration, undistortion and upsampling and in front of DepthHoleFilling: invalidate
    first, then fill.  size is (width, height); params is a SpeckleParams (min_size, max_diff, rel_diff, connectivity,
    z_min, z_max) or None for the defaults (64, 10 mm, 0.02, 4, every finite positive depth).  The rule is stated in
    include/kde_hip.h; deterministic to the bit.  This stage fills nothing: its counts are removed(), components() and
    capped()."""
    _destroy, _prefix = "kde_speckle_destroy", "kde_speckle_"
    _handle_type, _params_type = _native.SpeckleHandle, _native.SpeckleParams

    def __init__(self, size, max_batch: int = 1, params: Optional["_native.SpeckleParams"] = None):
        super().__init__(max_batch)
        self.width, self.height = size
        self._out_hw = (self.height, self.width)
        check(lib().kde_speckle_create(C.byref(self._h), self.width, self.height, max_batch, None if params is None else C.byref(params)))

    def filter(self, depth: torch.Tensor, out: Optional[torch.Tensor] = None, out_format=torch.float32,
               labels: Optional[torch.Tensor] = None) -> torch.Tensor:
        """depth: [n,H,W] float32, or uint16 / int16 holding the sensor's uint16.  out: [n,H,W] float32 or uint16 / int16 (its
        dtype is the output format), or None for the object-owned buffer in out_format (torch.float32, torch.uint16 or
        torch.int16); `out` may be `depth` itself (in place) and must not overlap it otherwise.  labels: int32 [n,H,W] or
        None: the smallest raster index of a kept pixel's component, -1 where the output is 0.  Returns the filtered frames.
        Asynchronous on torch's current stream; no allocation, copy or synchronisation on the device."""
        n, fmt = self._check_depth(depth, self.height, self.width)
        ofmt = self._out_format(out, out_format, n)
        if labels is not None:
            _req(labels, torch.int32, (n, self.height, self.width), "labels")
        check(lib().kde_speckle_filter_batch(self._h, n, depth.data_ptr(), fmt, ofmt, _ptr(out), _ptr(labels), _stream()))
        return self._finished(n, ofmt, out)

    def filled(self):
        raise AttributeError("DepthSpeckleFilter fills nothing: removed(), components() and capped() are its counts")

    filled_device = filled

    def removed(self) -> np.ndarray:
        """the number of pixels per frame that had a depth and lost it in the last filter(), uint32 [n]; synchronises"""
        return self._count_host(lib().kde_speckle_removed_host)

    def removed_device(self) -> torch.Tensor:
        """removed on the device, as raw bytes [n, 4] (uint32), a view of the object-owned buffer"""
        return self._count_device(lib().kde_speckle_removed_device)

    def components(self) -> np.ndarray:
        """the number of components per frame the last filter() kept, uint32 [n]; synchronises"""
        return self._count_host(lib().kde_speckle_components_host)

    def components_device(self) -> torch.Tensor:
        return self._count_device(lib().kde_speckle_components_device)

    def capped(self) -> np.ndarray:
        """uint32 [n]: 0; anything else is a defect of the library and the frame is not to be trusted; synchronises"""
        return self._count_host(lib().kde_speckle_capped_host)

    def capped_device(self) -> torch.Tensor:
        return self._count_device(lib().kde_speckle_capped_device)


class DepthTemporalFilter(_DepthStage):
    """Motion-aware smoothing of a depth sequence on the device (kde_temporal_*): each sample is blended into a per-pixel
    running value while it stays on the same surface, starts the value again where it jumps, the value is held over short
    dropouts and forgotten where the colour guide says the scene changed.  The frames of a call are consecutive in time and
    the object carries the state from one call to the next; reset() starts a new sequence.  It sits beside
    DepthSpeckleFilter and in front of DepthHoleFilling.  size is (width, height); params is a TemporalParams (alpha,
    max_diff, rel_diff, persist_min, color_thresh, z_min, z_max) or None for the defaults.  The rule is stated in
    include/kde_hip.h; deterministic to the bit, however the sequence is cut into calls.  This stage fills nothing: its
    counts are smoothed(), jumped(), held() and changed()."""
    _destroy, _prefix = "kde_temporal_destroy", "kde_temporal_"
    _handle_type, _params_type = _native.TemporalHandle, _native.TemporalParams

    def __init__(self, size, max_batch: int = 1, params: Optional["_native.TemporalParams"] = None):
        super().__init__(max_batch)
        self.width, self.height = size
        self._out_hw = (self.height, self.width)
        check(lib().kde_temporal_create(C.byref(self._h), self.width, self.height, max_batch, None if params is None else C.byref(params)))

    def filter(self, depth: torch.Tensor, bgr: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None,
               out_format=torch.float32) -> torch.Tensor:
        """depth: the next n frames of the sequence, [n,H,W] float32, or uint16 / int16 holding the sensor's uint16.  bgr:
        uint8 [n,H,W,3] or None (no guide).  out: [n,H,W] float32 or uint16 / int16 (its dtype is the output format), or None
        for the object-owned buffer in out_format; `out` may be `depth` itself (in place) and must not overlap it otherwise.
        Returns the filtered frames.  Asynchronous on torch's current stream; no allocation, copy or synchronisation on the
        device."""
        n, fmt = self._check_depth(depth, self.height, self.width)
        ofmt = self._out_format(out, out_format, n)
        if bgr is not None:
            if not isinstance(bgr, torch.Tensor) or bgr.dim() != 4 or bgr.shape[0] != n:
                raise ValueError(f"bgr: expected [{n},{self.height},{self.width},3] uint8 (a frame of guide per frame of depth)")
            _req(bgr, torch.uint8, (n, self.height, self.width, 3), "bgr")
        check(lib().kde_temporal_filter_batch(self._h, n, depth.data_ptr(), fmt, _ptr(bgr), ofmt, _ptr(out), _stream()))
        return self._finished(n, ofmt, out)

    def reset(self) -> None:
        """the state of every pixel becomes empty, as after construction: the next frame starts a sequence.  A launch on
        torch's current stream; the counts and depth_device() ask for a filter() again."""
        check(lib().kde_temporal_reset(self._h, _stream()))
        self._n = 0

    def state(self):
        """(value float32 [H,W], hist int32 [H,W] holding the uint32 bits): views of the object-owned state.  Cloning them
        between calls checkpoints a stream; copying into them restores one, or moves it to another object."""
        v, k = C.c_void_p(), C.c_void_p()
        check(lib().kde_temporal_state_device(self._h, C.byref(v), C.byref(k)))
        return _view(v.value, self._out_hw, torch.float32, self), _view(k.value, self._out_hw, torch.int32, self)

    def set_shape(self, pixels_per_thread: int = 0, unroll: int = 0) -> None:
        """a measurement knob: the pixels a thread owns and the frames it loads ahead (0, 0: the library's choice); the bytes
        of every result are the same"""
        check(lib().kde_temporal_set_shape(self._h, pixels_per_thread, unroll))

    def shape(self, n: int):
        """(pixels per thread, frames loaded ahead) a call of n frames would run"""
        p, u = C.c_int(), C.c_int()
        check(lib().kde_temporal_shape(self._h, n, C.byref(p), C.byref(u)))
        return p.value, u.value

    def filled(self):
        raise AttributeError("DepthTemporalFilter fills nothing: smoothed(), jumped(), held() and changed() are its counts")

    filled_device = filled

    def smoothed(self) -> np.ndarray:
        """the pixels per frame of the last filter() whose sample was blended into the running value, uint32 [n]; synchronises"""
        return self._count_host(lib().kde_temporal_smoothed_host)

    def smoothed_device(self) -> torch.Tensor:
        """smoothed on the device, as raw bytes [n, 4] (uint32), a view of the object-owned buffer"""
        return self._count_device(lib().kde_temporal_smoothed_device)

    def jumped(self) -> np.ndarray:
        """the pixels per frame whose valid sample left the surface of the running value, uint32 [n]; synchronises"""
        return self._count_host(lib().kde_temporal_jumped_host)

    def jumped_device(self) -> torch.Tensor:
        return self._count_device(lib().kde_temporal_jumped_device)

    def held(self) -> np.ndarray:
        """the hole pixels per frame that kept the running value, uint32 [n]; synchronises"""
        return self._count_host(lib().kde_temporal_held_host)

    def held_device(self) -> torch.Tensor:
        return self._count_device(lib().kde_temporal_held_device)

    def changed(self) -> np.ndarray:
        """the pixels per frame whose running value the guide's colour change forgot, uint32 [n]; synchronises"""
        return self._count_host(lib().kde_temporal_changed_host)

    def changed_device(self) -> torch.Tensor:
        return self._count_device(lib().kde_temporal_changed_device)


class DepthDecimation(_DepthStage):
    """Depth frames and their colour guides made `factor` times smaller each way on the device (kde_decimate_*): an output pixel
    is the lower median (KDE_DECIMATE_MEDIAN) or the guarded mean (KDE_DECIMATE_MEAN) of the valid samples of its factor x
    factor block, 0 where fewer than min_valid are valid; the guide is the block's mean colour rounded half up.  The step down
    of a multi-resolution chain: decimate, enhance at the small size, GuidedDepthUpsampling back under the full-resolution
    guide.  src_size is (width, height); params is a DecimateParams (factor, mode, min_valid, max_gap, z_min, z_max) or None for
    the defaults (2, median, 1, no guard, every finite positive depth).  The rule is stated in include/kde_hip.h;
    deterministic to the bit.  Its counts are filled() and mixed()."""
    _destroy, _prefix = "kde_decimate_destroy", "kde_decimate_"
    _handle_type, _params_type = _native.DecimateHandle, _native.DecimateParams

    def __init__(self, src_size, max_batch: int = 1, params: Optional["_native.DecimateParams"] = None):
        super().__init__(max_batch)
        self.src_width, self.src_height = src_size
        check(lib().kde_decimate_create(C.byref(self._h), self.src_width, self.src_height, max_batch, None if params is None else C.byref(params)))
        w, h = C.c_int(), C.c_int()
        check(lib().kde_decimate_out_size(self._h, C.byref(w), C.byref(h)))
        self.out_width, self.out_height = w.value, h.value
        self._out_hw = (self.out_height, self.out_width)

    @property
    def out_size(self):
        """(width, height) of an output frame: ceil(src / factor) each way"""
        return self.out_width, self.out_height

    def decimate(self, depth: torch.Tensor, out: Optional[torch.Tensor] = None, out_format=None) -> torch.Tensor:
        """depth: [n,Hs,Ws] float32, or uint16 / int16 holding the sensor's uint16.  out: [n,Ho,Wo] float32 or uint16 / int16 (its
        dtype is the output format), or None for the object-owned buffer in out_format (torch.float32, torch.uint16 or
        torch.int16; None: the format of depth); what is written must not overlap depth.  Returns the decimated frames (0
        where a block had fewer than min_valid valid samples).  Asynchronous on torch's current stream; no allocation, copy or
        synchronisation on the device."""
        n, fmt = self._check_depth(depth, self.src_height, self.src_width)
        if out is None and out_format is None:
            out_format = torch.float32 if fmt == _native.KDE_DEPTH_F32 else torch.int16
        ofmt = self._out_format(out, out_format, n)
        check(lib().kde_decimate_depth_batch(self._h, n, depth.data_ptr(), fmt, ofmt, _ptr(out), _stream()))
        return self._finished(n, ofmt, out)

    def decimate_color(self, bgr: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """bgr: uint8 [n,Hs,Ws,3].  Returns uint8 [n,Ho,Wo,3], the mean colour of each block rounded half up.  Asynchronous on
        torch's current stream; it leaves the results of the last decimate() alone."""
        if not isinstance(bgr, torch.Tensor) or bgr.dim() != 4:
            raise ValueError(f"bgr: expected [n,{self.src_height},{self.src_width},3] uint8")
        n = bgr.shape[0]
        _req(bgr, torch.uint8, (n, self.src_height, self.src_width, 3), "bgr")
        if out is None:
            out = torch.empty((n, self.out_height, self.out_width, 3), dtype=torch.uint8, device=bgr.device)
        else:
            _req(out, torch.uint8, (n, self.out_height, self.out_width, 3), "out")
        check(lib().kde_decimate_color_batch(self._h, n, bgr.data_ptr(), out.data_ptr(), _stream()))
        return out

    def intrinsics(self, K) -> np.ndarray:
        """the 3 x 3 camera matrix of the small image for K of the source image, float64: fx / k, fy / k, (cx + 0.5) / k - 0.5,
        (cy + 0.5) / k - 0.5; needs no device"""
        k = _K9(K)
        r = np.empty(9, np.float64)
        check(lib().kde_decimate_intrinsics(self._h, k.ctypes.data, r.ctypes.data))
        return r.reshape(3, 3)

    def mixed(self) -> np.ndarray:
        """the output pixels per frame of the last decimate() whose block spans more than max_gap, uint32 [n] (0 without a
        guard); synchronises torch's current stream"""
        return self._count_host(lib().kde_decimate_mixed_host)

    def mixed_device(self) -> torch.Tensor:
        """mixed on the device, as raw bytes [n, 4] (uint32), a view of the object-owned buffer"""
        return self._count_device(lib().kde_decimate_mixed_device)


COMPARE_METHODS = ("input", "jbf", "mrf", "rgbf", "kde")


def compare_methods(depth: torch.Tensor, bgr: torch.Tensor, truth_depth: torch.Tensor, K, rows: int, cols: int,
                    methods=COMPARE_METHODS) -> dict:
    """The comparison of the reference's main.cpp on a batch: every method of `methods` on depth [n,H,W] float32 and bgr
    [n,H,W,3] uint8 (main.cpp:159-202: INPUT, JointBilateralFilter, MarkovRandomField, RegionGrowingBilateralFilter and
    KinectDepthEnhancement with rows x cols superpixels, each result as the cloud projectiveToReal makes of it), then the
    mean 3-D error of each against the cloud of truth_depth ([n,H,W] or [1,H,W]) in ONE MeanError3D.compare call
    (main.cpp:220-308).  Returns {name: results[n]} (MeanError3D.RESULT_DTYPE)."""
    methods = tuple(methods)
    unknown = [m for m in methods if m not in COMPARE_METHODS]
    if unknown or not methods or len(set(methods)) != len(methods):
        raise ValueError(f"methods: expected distinct names of {COMPARE_METHODS}, got {methods}")
    if not isinstance(depth, torch.Tensor) or depth.dim() != 3:
        raise ValueError("depth: expected a [n, H, W] tensor")
    n, h, w = depth.shape
    _req(depth, torch.float32, (n, h, w), "depth")
    _req(bgr, torch.uint8, (n, h, w, 3), "bgr")
    conv = DimensionConvertor()
    conv.setCameraParameters(K, w, h)

    def cloud(d):
        return conv.projectiveToReal(d.reshape(n, h, w), torch.empty((n, h, w, 3), dtype=torch.float32, device=depth.device))

    keep, cands = [], []          # the stage objects own some of the compared buffers: alive until the table is read
    for name in methods:
        if name == "input":
            cands.append(cloud(depth))                                            # main.cpp:168
        elif name == "jbf":
            o = JointBilateralFilter(w, h, max_batch=n)
            cands.append(cloud(o.process_batch(depth, bgr)))                      # :179-182
        elif name == "mrf":
            o = MarkovRandomField(w, h, max_batch=n)
            cands.append(cloud(o.process_batch(depth, bgr, torch.empty_like(depth))))   # :186-189
        elif name == "rgbf":
            o = RegionGrowingBilateralFilter(w, h, max_batch=n)
            o.SetParametor(rows, cols, K)
            o.process_batch(depth, cloud(depth), bgr)                             # :193
            cands.append(cloud(o.getRefinedDepth_Device()))                       # :196
        else:
            o = KinectDepthEnhancement(w, h, max_batch=n)
            o.SetParametor(rows, cols, K)
            o.process_batch(depth, bgr)                                           # :200
            cands.append(o.getOptimizedPoints_Device().reshape(n, h, w, 3))       # :202
        if name != "input":
            keep.append(o)
    err = MeanError3D(w, h, max_batch=n, max_candidates=len(methods))
    err.set_camera(K)
    err.compare(cands, truth_depth)                                               # the truth as a depth map: :175
    table = err.results_host()
    for o in keep + [err, conv]:
        o.close()
    return {name: table[:, i].copy() for i, name in enumerate(methods)}


class KinectDepthEnhancementFeed(_Handle):
    """Host-fed KinectDepthEnhancement::Process (kde_enh_feed_*): frames in host memory in, the enhanced result in host
    memory out, in chunks of `chunk_frames` <= enh.max_batch (default: enh.max_batch) with the copies overlapped with the
    kernels.  Borrows `enh` (kept alive by this object) and RUNS it: afterwards enh's getters show the last chunk of the
    last call, and `enh` must not be used while process() runs.  SetParametor must have been called on `enh`.  A blocking
    call on the feed's own streams, not on torch's current stream."""
    _destroy = "kde_enh_feed_destroy"
    _handle_type = _native.EnhFeedHandle
    _OUTPUTS = {"points": (_native.KDE_OUT_POINTS_F32, np.float32, (3,)), "depth": (_native.KDE_OUT_DEPTH_F32, np.float32, ()),
                "depth_u16": (_native.KDE_OUT_DEPTH_U16, np.uint16, ())}

    def __init__(self, enh: KinectDepthEnhancement, chunk_frames: Optional[int] = None):
        super().__init__()
        self.enh = enh
        self.Width, self.Height = enh.width, enh.height
        self.chunk_frames = enh.max_batch if chunk_frames is None else chunk_frames
        check(lib().kde_enh_feed_create(C.byref(self._h), enh._h, self.chunk_frames))

    def process(self, depth, color, out=None, output: str = "points"):
        """depth [n,H,W] float32 or uint16 (mm, 0 = invalid), color [n,H,W,3] uint8 BGR; numpy arrays or CPU torch tensors,
        pinned or pageable.  output = "points" ([n,H,W,3] float32: the optimized cloud), "depth" ([n,H,W] float32: its z) or
        "depth_u16" ([n,H,W] uint16: its z as the sensor's format).  out: a host buffer of that shape and type (a numpy
        array is allocated when None).  Returns out."""
        if output not in self._OUTPUTS:
            raise ValueError(f"output: expected one of {sorted(self._OUTPUTS)}, got {output!r}")
        ofmt, odt, trailing = self._OUTPUTS[output]
        n = depth.shape[0] if len(depth.shape) == 3 else -1
        dptr, ddt = _host_array(depth, (np.float32, np.uint16), (n, self.Height, self.Width), "depth")
        cptr, _ = _host_array(color, (np.uint8,), (n, self.Height, self.Width, 3), "color")
        if out is None:
            out = np.empty((n, self.Height, self.Width) + trailing, odt)
        optr, _ = _host_array(out, (odt,), (n, self.Height, self.Width) + trailing, "out")
        fmt = _native.KDE_DEPTH_U16 if ddt == np.uint16 else _native.KDE_DEPTH_F32
        check(lib().kde_enh_feed_process(self._h, n, dptr, fmt, cptr, ofmt, optr))
        cf = min(self.chunk_frames, n)
        self.enh._n = n - (-(-n // cf) - 1) * cf        # enh's getters now show the last chunk
        return out

    def last_stats(self) -> dict:
        st = _native.FeedStats()
        check(lib().kde_enh_feed_last_stats(self._h, C.byref(st)))
        return {name: getattr(st, name) for name, _ in st._fields_}


class EdgeRefinedSuperpixel(_Handle):
    """EdgeRefinedSuperpixel/EdgeRefinedSuperpixel.h:14-45."""
    _destroy = "kde_ers_destroy"

    def __init__(self, width: int, height: int):
        super().__init__()
        self.Width, self.Height = width, height
        check(lib().kde_ers_create(C.byref(self._h), width, height))

    def EdgeRefining(self, color_label_device, depth_label_device, depth_device, color_image) -> None:
        hw = (self.Height, self.Width)
        _req(color_label_device, torch.int32, hw, "color_label_device")
        _req(depth_label_device, torch.int32, hw, "depth_label_device")
        _req(depth_device, torch.float32, hw, "depth_device")
        _req(color_image, torch.uint8, hw + (3,), "color_image")
        check(lib().kde_ers_edge_refining(self._h, color_label_device.data_ptr(), depth_label_device.data_ptr(),
                                          depth_device.data_ptr(), color_image.data_ptr(), _stream()))

    def set_variant(self, v: int) -> None:
        """0 = built-in choice, 1 = packed-pair, 2 = scalar tuned, 3 = generic depthmap_enhancement kernel"""
        check(lib().kde_ers_set_variant(self._h, int(v)))

    def _get(self, fn, dtype):
        p = C.c_void_p()
        check(getattr(lib(), fn)(self._h, C.byref(p)))
        return _view(p.value, (self.Height, self.Width), dtype, self)

    def getRefinedLabels_Device(self):
        return self._get("kde_ers_refined_labels_device", torch.int32)

    def getRefinedDepth_Device(self):
        return self._get("kde_ers_refined_depth_device", torch.float32)

    def getEdgeStageDepth_Device(self):
        """depth after edge_refining, before depthmap_enhancement (for per-kernel parity tests)."""
        return self._get("kde_ers_stage_edge_depth_device", torch.float32)

    def getRefinedLabels_Host(self) -> np.ndarray:
        p = C.c_void_p()
        check(lib().kde_ers_refined_labels_host(self._h, _stream(), C.byref(p)))
        return np.ctypeslib.as_array(C.cast(p, C.POINTER(C.c_int32)), shape=(self.Height, self.Width)).copy()

    def getRefinedDepth_Host(self) -> np.ndarray:
        p = C.c_void_p()
        check(lib().kde_ers_refined_depth_host(self._h, _stream(), C.byref(p)))
        return np.ctypeslib.as_array(C.cast(p, C.POINTER(C.c_float)), shape=(self.Height, self.Width)).copy()


class _PipelineBase(_Handle):
    _prefix = ""

    def __init__(self, width: int, height: int, max_batch: int = 1):
        super().__init__()
        self.Width, self.Height, self.max_batch = width, height, max_batch
        if max_batch == 1:
            check(getattr(lib(), f"{self._prefix}_create")(C.byref(self._h), width, height))
        else:
            check(getattr(lib(), f"{self._prefix}_create_batch")(C.byref(self._h), width, height, max_batch))
        self._n = 1

    def process_batch(self, depth: torch.Tensor, points: torch.Tensor, color: torch.Tensor) -> None:
        """n independent frames back to back ([n,H,W], [n,H,W,3], [n,H,W,3]); the getters then return n frames"""
        n = depth.shape[0]
        hw = (self.Height, self.Width)
        _req(depth, torch.float32, (n,) + hw, "depth")
        _req(points, torch.float32, (n,) + hw + (3,), "points")
        _req(color, torch.uint8, (n,) + hw + (3,), "color")
        check(getattr(lib(), f"{self._prefix}_process_batch")(self._h, n, depth.data_ptr(), points.data_ptr(), color.data_ptr(), _stream()))
        self._n = n

    def _lead(self):
        return () if self._n == 1 else (self._n,)

    def SetParametor(self, rows: int, cols: int, intrinsic) -> None:
        k = _K9(intrinsic)
        check(getattr(lib(), f"{self._prefix}_set_parameters")(self._h, rows, cols, k.ctypes.data))
        self.sp_rows, self.sp_cols = rows, cols

    def Process(self, depth_device: torch.Tensor, points_device: torch.Tensor, color_device: torch.Tensor) -> None:
        hw = (self.Height, self.Width)
        _req(depth_device, torch.float32, hw, "depth_device")
        _req(points_device, torch.float32, hw + (3,), "points_device")
        _req(color_device, torch.uint8, hw + (3,), "color_device")
        check(getattr(lib(), f"{self._prefix}_process")(self._h, depth_device.data_ptr(), points_device.data_ptr(),
                                                        color_device.data_ptr(), _stream()))
        self._n = 1

    def _get(self, fn, shape, dtype):
        p = C.c_void_p()
        check(getattr(lib(), f"{self._prefix}_{fn}")(self._h, C.byref(p)))
        return _view(p.value, shape, dtype, self)

    def getRefinedDepth_Device(self) -> torch.Tensor:
        return self._get("refined_depth_device", self._lead() + (self.Height, self.Width), torch.float32)

    def getRefinedLabels_Device(self) -> torch.Tensor:
        return self._get("refined_labels_device", self._lead() + (self.Height, self.Width), torch.int32)

    def getRefinedDepth_Host(self) -> np.ndarray:
        p = C.c_void_p()
        check(getattr(lib(), f"{self._prefix}_refined_depth_host")(self._h, _stream(), C.byref(p)))
        return np.ctypeslib.as_array(C.cast(p, C.POINTER(C.c_float)), shape=self._lead() + (self.Height, self.Width)).copy()


class RegionGrowingBilateralFilter(_PipelineBase):
    """RegionGrowingBilateralFilter.h:11-27."""
    _destroy = "kde_rgbf_destroy"
    _prefix = "kde_rgbf"

    def getSPLabels_Device(self):
        return self._get("sp_labels_device", self._lead() + (self.Height, self.Width), torch.int32)

    def getDASPLabels_Device(self):
        return self._get("dasp_labels_device", self._lead() + (self.Height, self.Width), torch.int32)


class SPDepthSuperResolution(_PipelineBase):
    """SPDepthSuperResolution.h:17-46."""
    _destroy = "kde_spdsr_destroy"
    _prefix = "kde_spdsr"

    def getEdgeEnhanced3DPoints_Device(self):
        return self._get("edge_enhanced_points_device", self._lead() + (self.Height, self.Width, 3), torch.float32)

    def getOptimizedPoints_Device(self):
        return self._get("optimized_points_device", self._lead() + (self.Height, self.Width, 3), torch.float32)

    def getOptimizedPoints_Host(self) -> np.ndarray:
        p = C.c_void_p()
        check(lib().kde_spdsr_optimized_points_host(self._h, _stream(), C.byref(p)))
        return np.ctypeslib.as_array(C.cast(p, C.POINTER(C.c_float)), shape=self._lead() + (self.Height, self.Width, 3)).copy()

    def getPlaneFitted3D_Device(self):
        return self._get("plane_fitted_points_device", self._lead() + (self.Height, self.Width, 3), torch.float32)

    def getClusterND_Device(self):
        return self._get("cluster_nd_device", self._lead() + (self.sp_rows * self.sp_cols, 4), torch.float32)
