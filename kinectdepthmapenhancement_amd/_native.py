"""ctypes binding of libkde_hip.so (include/kde_hip.h).

The product path has no CPU fallback: if the HIP library is missing or a call fails, this module
raises.  Nothing here imports, links or calls the CPU oracle.
"""
from __future__ import annotations

import ctypes as C
import os
import subprocess

_PKG = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_PKG, "libkde_hip.so")
CSRC = os.path.join(_PKG, "csrc")

KDE_OK, KDE_ERR_INVALID, KDE_ERR_HIP, KDE_ERR_NOMEM, KDE_ERR_UNSUPPORTED = range(5)


class KdeError(RuntimeError):
    def __init__(self, code: int, message: str):
        super().__init__(f"libkde_hip error {code}: {message}")
        self.code = code


class JbfParams(C.Structure):
    """kde_jbf_params (defaults = JointBilateralFilter.cpp:3-6 and the call at JointBilateralFilter.cu:285)."""
    _fields_ = [("window_size", C.c_int), ("spatial_sigma", C.c_float), ("color_sigma", C.c_float),
                ("depth_sigma", C.c_float), ("presmooth", C.c_int), ("presmooth_kernel_size", C.c_int),
                ("presmooth_sigma_color", C.c_float), ("presmooth_sigma_spatial", C.c_float)]


KDE_DEPTH_F32, KDE_DEPTH_U16 = 0, 1
KDE_OUT_POINTS_F32, KDE_OUT_DEPTH_F32, KDE_OUT_DEPTH_U16 = 0, 1, 2
KDE_SRC_POINTS_F32, KDE_SRC_DEPTH_F32, KDE_SRC_DEPTH_U16 = 0, 1, 2
KDE_NORMALS_SDC, KDE_NORMALS_CM, KDE_NORMALS_BILATERAL = 0, 1, 2


class NormalsParams(C.Structure):
    """kde_normals_params (defaults = NormalMapGenerator.cpp:15, SmoothingAreaMapGenerator.cpp:15-16)."""
    _fields_ = [("method", C.c_int), ("max_depth_change_factor", C.c_float), ("normal_smoothing_size", C.c_float)]


class LesParams(C.Structure):
    """kde_les_params (defaults = LabelEquivalenceSeg.cu:235, :40, :42)."""
    _fields_ = [("iterations", C.c_int), ("max_angle", C.c_float), ("max_plane_distance", C.c_float)]


class ProjParams(C.Structure):
    """kde_proj_params (defaults = Projection_GPU.cpp:3-5, Projection_GPU.cu:38, :203)."""
    _fields_ = [("window_size", C.c_int), ("spatial_sigma", C.c_float), ("depth_sigma", C.c_float), ("max_angle", C.c_float),
                ("min_size", C.c_int)]


class FeedStats(C.Structure):
    """kde_feed_stats: what the last kde_jbf_feed_process / kde_enh_feed_process call did."""
    _fields_ = [("frames", C.c_int), ("chunks", C.c_int), ("chunk_frames", C.c_int), ("inputs_staged", C.c_int),
                ("outputs_staged", C.c_int), ("wall_ms", C.c_float), ("h2d_ms", C.c_float), ("compute_ms", C.c_float),
                ("d2h_ms", C.c_float), ("h2d_bytes", C.c_size_t), ("d2h_bytes", C.c_size_t)]


class EnhFeedHandle(C.c_void_p):
    """kde_enh_feed*: a ctypes type of its own, so that an argument declared as EnhFeedHandle takes None or an EnhFeedHandle
    and refuses a plain c_void_p (any other handle) with a TypeError.  It also keeps the kde_enh_feed_* entry points out of
    the frozen record tools/abi_refusals.py enumerates (first argument c_void_p or POINTER(c_void_p)); their refusals are
    recorded by tools/abi_refusals_new.py instead."""


class Error3dHandle(C.c_void_p):
    """kde_error3d*: a ctypes type of its own, like EnhFeedHandle, which keeps the kde_error3d_* entry points out of the
    frozen record tools/abi_refusals.py enumerates; tests/test_error3d_abi.py checks their refusals."""


class Error3dSource(C.Structure):
    """kde_error3d_source: a device pointer to [frames][H][W] elements and their KDE_SRC_* format."""
    _fields_ = [("data_dev", C.c_void_p), ("format", C.c_int)]


class Error3dResult(C.Structure):
    """kde_error3d_result (16 bytes): the binary64 sum of the terms, the number of valid pixels, (float)(sum / count)."""
    _fields_ = [("sum", C.c_double), ("count", C.c_uint32), ("mean", C.c_float)]


class CloudHandle(C.c_void_p):
    """kde_cloud*: a ctypes type of its own, like Error3dHandle, which keeps the kde_cloud_* entry points out of the frozen
    record tools/abi_refusals.py enumerates; tests/test_cloud_abi.py checks their refusals."""


class CloudParams(C.Structure):
    """kde_cloud_params (defaults = the literals of main.cpp:227-230: 50, 15000, 1000, negated z; dense)."""
    _fields_ = [("z_min", C.c_float), ("z_max", C.c_float), ("divisor", C.c_float), ("negate_z", C.c_int), ("organized", C.c_int)]


class CloudPoint(C.Structure):
    """kde_cloud_point (16 bytes): x, y, z and PCL's packed rgb, (r << 16) | (g << 8) | b."""
    _fields_ = [("x", C.c_float), ("y", C.c_float), ("z", C.c_float), ("rgb", C.c_uint32)]


KDE_MESH_DIAG_AD, KDE_MESH_DIAG_BC, KDE_MESH_DIAG_ADAPTIVE = 0, 1, 2


class MeshHandle(C.c_void_p):
    """kde_mesh*: a ctypes type of its own, like CloudHandle, which keeps the kde_mesh_* entry points out of the frozen
    record tools/abi_refusals.py enumerates; tests/test_mesh_abi.py checks their refusals."""


class MeshParams(C.Structure):
    """kde_mesh_params (defaults = the cloud's 50, 15000, 1000, negated z; the speckle filter's link 10, 0.02; the adaptive
    cut; winding as it is)."""
    _fields_ = [("z_min", C.c_float), ("z_max", C.c_float), ("divisor", C.c_float), ("negate_z", C.c_int),
                ("max_diff", C.c_float), ("rel_diff", C.c_float), ("diagonal", C.c_int), ("flip_winding", C.c_int)]


class MeshTriangle(C.Structure):
    """kde_mesh_triangle (12 bytes): three frame-local vertex indices."""
    _fields_ = [("v0", C.c_uint32), ("v1", C.c_uint32), ("v2", C.c_uint32)]


class RegHandle(C.c_void_p):
    """kde_reg*: a ctypes type of its own, like CloudHandle, which keeps the kde_reg_* entry points out of the frozen record
    tools/abi_refusals.py enumerates; tests/test_reg_abi.py checks their refusals."""


class RegParams(C.Structure):
    """kde_reg_params (defaults: 0, FLT_MAX, 0 -- every finite positive depth, one target pixel per source pixel)."""
    _fields_ = [("z_min", C.c_float), ("z_max", C.c_float), ("max_splat", C.c_int)]


class UndistHandle(C.c_void_p):
    """kde_undist*: a ctypes type of its own, like CloudHandle and RegHandle, which keeps the kde_undist_* entry points out of
    the frozen record tools/abi_refusals.py enumerates; tests/test_undist_abi.py checks their refusals."""


class UndistParams(C.Structure):
    """kde_undist_params (defaults: 0, FLT_MAX, 0, 0 -- every finite positive depth, the nearest sample)."""
    _fields_ = [("z_min", C.c_float), ("z_max", C.c_float), ("depth_interp", C.c_int), ("max_gap", C.c_float)]


class UpsampleHandle(C.c_void_p):
    """kde_upsample*: a ctypes type of its own, like CloudHandle, RegHandle and UndistHandle, which keeps the kde_upsample_*
    entry points out of the frozen record tools/abi_refusals.py enumerates; tests/test_upsample_abi.py checks their refusals."""


class UpsampleParams(C.Structure):
    """kde_upsample_params (defaults: 2, 30, 0, 0, FLT_MAX -- a 4 x 4 tent, K0's colour constant, no guard, every finite
    positive depth)."""
    _fields_ = [("radius", C.c_int), ("sigma_color", C.c_float), ("max_gap", C.c_float), ("z_min", C.c_float), ("z_max", C.c_float)]


class HolefillHandle(C.c_void_p):
    """kde_holefill*: a ctypes type of its own, like CloudHandle, RegHandle, UndistHandle and UpsampleHandle, which keeps the
    kde_holefill_* entry points out of the frozen record tools/abi_refusals.py enumerates; tests/test_holefill_abi.py checks
    their refusals."""


class HolefillParams(C.Structure):
    """kde_holefill_params (defaults: 2, 8, 3, 2, 30, 0, 0, 0, FLT_MAX, 0 -- a 5 x 5 window, 8 passes, 3 taps, K0's colour
    constant, no guard, every finite positive depth, the library's passes per launch)."""
    _fields_ = [("radius", C.c_int), ("iterations", C.c_int), ("min_taps", C.c_int), ("sigma_space", C.c_float),
                ("sigma_color", C.c_float), ("max_gap", C.c_float), ("gap_rule", C.c_int), ("z_min", C.c_float), ("z_max", C.c_float),
                ("passes_per_launch", C.c_int)]


class SpeckleHandle(C.c_void_p):
    """kde_speckle*: a ctypes type of its own, like HolefillHandle, which keeps the kde_speckle_* entry points out of the frozen
    record tools/abi_refusals.py enumerates; tests/test_speckle_abi.py checks their refusals."""


class SpeckleParams(C.Structure):
    """kde_speckle_params (defaults: 64, 10, 0.02, 4, 0, FLT_MAX -- components below 64 pixels go, a link holds within 10 mm
    + 2 % of the nearer depth, 4-connected, every finite positive depth)."""
    _fields_ = [("min_size", C.c_int), ("max_diff", C.c_float), ("rel_diff", C.c_float), ("connectivity", C.c_int),
                ("z_min", C.c_float), ("z_max", C.c_float)]


class TemporalHandle(C.c_void_p):
    """kde_temporal*: a ctypes type of its own, like SpeckleHandle, which keeps the kde_temporal_* entry points out of the
    frozen record tools/abi_refusals.py enumerates; tests/test_temporal_abi.py checks their refusals."""


class TemporalParams(C.Structure):
    """kde_temporal_params (defaults: 0.4, 10, 0.02, 3, 48, 0, FLT_MAX -- 0.4 of a linked sample, a link holds within 10 mm
    + 2 % of the nearer depth, a hole is held behind 3 valid frames of the last 8, a colour step above 48 forgets, every
    finite positive depth)."""
    _fields_ = [("alpha", C.c_float), ("max_diff", C.c_float), ("rel_diff", C.c_float), ("persist_min", C.c_int),
                ("color_thresh", C.c_int), ("z_min", C.c_float), ("z_max", C.c_float)]


class DecimateHandle(C.c_void_p):
    """kde_decimate*: a ctypes type of its own, like TemporalHandle, which keeps the kde_decimate_* entry points out of the
    frozen record tools/abi_refusals.py enumerates; tests/test_decimate_abi.py checks their refusals."""


class DecimateParams(C.Structure):
    """kde_decimate_params (defaults: 2, KDE_DECIMATE_MEDIAN, 1, 0, 0, FLT_MAX -- half the size each way, the lower median of
    at least one valid sample, no guard, every finite positive depth)."""
    _fields_ = [("factor", C.c_int), ("mode", C.c_int), ("min_valid", C.c_int), ("max_gap", C.c_float), ("z_min", C.c_float),
                ("z_max", C.c_float)]


KDE_DECIMATE_MEDIAN, KDE_DECIMATE_MEAN = 0, 1


def build(force: bool = False) -> str:
    """Compile libkde_hip.so for gfx950 with hipcc (cross-compiles without a GPU)."""
    if force:
        subprocess.check_call(["make", "-C", CSRC, "clean", "-s"])
    subprocess.check_call(["make", "-C", CSRC, "-s", "-j8"])
    return LIB_PATH


_lib = None

# name -> (restype, argtypes); every symbol include/kde_hip.h declares
_vp, _i, _f, _sz = C.c_void_p, C.c_int, C.c_float, C.c_size_t
_pp = C.POINTER(C.c_void_p)
SIGNATURES = {
    "kde_abi_version": (_i, []),
    "kde_last_error_string": (C.c_char_p, []),
    "kde_device_count": (_i, [C.POINTER(_i)]),
    "kde_set_device": (_i, [_i]),
    "kde_device_info": (_i, [C.c_char_p, _sz, C.POINTER(_i)]),
    "kde_device_pci_bus_id": (_i, [C.c_char_p, _sz]),
    "kde_jbf_default_params": (_i, [C.POINTER(JbfParams)]),
    "kde_jbf_create": (_i, [_pp, _i, _i, _i, C.POINTER(JbfParams)]),
    "kde_jbf_destroy": (_i, [_vp]),
    "kde_jbf_process": (_i, [_vp, _vp, _vp, _sz, _vp]),
    "kde_jbf_process_batch": (_i, [_vp, _i, _vp, _vp, _vp, _vp]),
    "kde_jbf_presmooth_batch": (_i, [_vp, _i, _vp, _vp, _vp]),
    "kde_jbf_filter_batch": (_i, [_vp, _i, _vp, _vp, _vp, _vp]),
    "kde_jbf_filtered_device": (_i, [_vp, _pp]),
    "kde_jbf_filtered_host": (_i, [_vp, _vp, _pp]),
    "kde_jbf_smooth_device": (_i, [_vp, _pp]),
    "kde_jbf_spatial_table": (_i, [_vp, _vp, _i]),
    "kde_jbf_set_variant": (_i, [_vp, _i]),
    "kde_jbf_active_variant": (_i, [_vp, C.POINTER(_i)]),
    "kde_jbf_variant_count": (_i, []),
    "kde_jbf_variant_name": (C.c_char_p, [_i]),
    "kde_jbf_feed_create": (_i, [_pp, _vp, _i]),
    "kde_jbf_feed_destroy": (_i, [_vp]),
    "kde_jbf_feed_process": (_i, [_vp, _i, _vp, _i, _vp, _vp]),
    "kde_jbf_feed_last_stats": (_i, [_vp, C.POINTER(FeedStats)]),
    "kde_mrf_create": (_i, [_pp, _i, _i, _i, _i, _f, _f]),
    "kde_mrf_destroy": (_i, [_vp]),
    "kde_mrf_process_batch": (_i, [_vp, _i, _vp, _vp, _vp, _vp]),
    "kde_mrf_filtered_device": (_i, [_vp, _pp]),
    "kde_mrf_filtered_host": (_i, [_vp, _vp, _pp]),
    "kde_dimconv_create": (_i, [_pp]),
    "kde_dimconv_destroy": (_i, [_vp]),
    "kde_dimconv_set_camera": (_i, [_vp, _vp, _i, _i]),
    "kde_dimconv_projective_to_real_depth": (_i, [_vp, _i, _vp, _vp, _vp]),
    "kde_dimconv_projective_to_real_points": (_i, [_vp, _i, _vp, _vp, _vp]),
    "kde_dimconv_projective_to_real_interp": (_i, [_vp, _i, _vp, _vp, _vp]),
    "kde_dimconv_real_to_projective": (_i, [_vp, _i, _vp, _vp, _vp]),
    "kde_buffer2d_create": (_i, [_pp, _i, _i]),
    "kde_buffer2d_destroy": (_i, [_vp]),
    "kde_buffer2d_insert_depth": (_i, [_vp, _vp, _vp]),
    "kde_buffer2d_insert_float2": (_i, [_vp, _vp, _vp]),
    "kde_buffer2d_insert_weighted": (_i, [_vp, _vp, _vp]),
    "kde_buffer2d_get_depth_map": (_i, [_vp, _vp, _vp]),
    "kde_buffer2d_get_weight_map": (_i, [_vp, _vp, _vp]),
    "kde_buffer2d_update": (_i, [_vp, _vp, _vp]),
    "kde_buffer2d_update_sequence": (_i, [_vp, _i, _vp, _vp]),
    "kde_buffer2d_raw_pointer": (_i, [_vp, _pp]),
    "kde_dasp_create": (_i, [_pp, _i, _i]),
    "kde_dasp_destroy": (_i, [_vp]),
    "kde_dasp_set_parameters": (_i, [_vp, _i, _i, _vp]),
    "kde_dasp_segmentation": (_i, [_vp, _vp, _vp, _f, _f, _f, _i, _vp]),
    "kde_dasp_labels_device": (_i, [_vp, _pp]),
    "kde_dasp_mean_device": (_i, [_vp, _pp]),
    "kde_dasp_centers_device": (_i, [_vp, _pp]),
    "kde_dasp_ld_device": (_i, [_vp, _pp]),
    "kde_dasp_mean_host": (_i, [_vp, _vp, _pp, C.POINTER(_i)]),
    "kde_dasp_labels_host": (_i, [_vp, _vp, _pp]),
    "kde_ers_create": (_i, [_pp, _i, _i]),
    "kde_ers_destroy": (_i, [_vp]),
    "kde_ers_edge_refining": (_i, [_vp, _vp, _vp, _vp, _vp, _vp]),
    "kde_ers_set_variant": (_i, [_vp, _i]),
    "kde_ers_stage_edge_depth_device": (_i, [_vp, _pp]),
    "kde_ers_refined_labels_device": (_i, [_vp, _pp]),
    "kde_ers_refined_depth_device": (_i, [_vp, _pp]),
    "kde_ers_refined_labels_host": (_i, [_vp, _vp, _pp]),
    "kde_ers_refined_depth_host": (_i, [_vp, _vp, _pp]),
    "kde_rgbf_create": (_i, [_pp, _i, _i]),
    "kde_rgbf_destroy": (_i, [_vp]),
    "kde_rgbf_set_parameters": (_i, [_vp, _i, _i, _vp]),
    "kde_rgbf_process": (_i, [_vp, _vp, _vp, _vp, _vp]),
    "kde_rgbf_create_batch": (_i, [_pp, _i, _i, _i]),
    "kde_rgbf_process_batch": (_i, [_vp, _i, _vp, _vp, _vp, _vp]),
    "kde_rgbf_refined_depth_device": (_i, [_vp, _pp]),
    "kde_rgbf_refined_depth_host": (_i, [_vp, _vp, _pp]),
    "kde_rgbf_refined_labels_device": (_i, [_vp, _pp]),
    "kde_rgbf_sp_labels_device": (_i, [_vp, _pp]),
    "kde_rgbf_dasp_labels_device": (_i, [_vp, _pp]),
    "kde_spdsr_create": (_i, [_pp, _i, _i]),
    "kde_spdsr_destroy": (_i, [_vp]),
    "kde_spdsr_set_parameters": (_i, [_vp, _i, _i, _vp]),
    "kde_spdsr_process": (_i, [_vp, _vp, _vp, _vp, _vp]),
    "kde_spdsr_create_batch": (_i, [_pp, _i, _i, _i]),
    "kde_spdsr_process_batch": (_i, [_vp, _i, _vp, _vp, _vp, _vp]),
    "kde_spdsr_refined_depth_device": (_i, [_vp, _pp]),
    "kde_spdsr_refined_depth_host": (_i, [_vp, _vp, _pp]),
    "kde_spdsr_refined_labels_device": (_i, [_vp, _pp]),
    "kde_spdsr_edge_enhanced_points_device": (_i, [_vp, _pp]),
    "kde_spdsr_optimized_points_device": (_i, [_vp, _pp]),
    "kde_spdsr_optimized_points_host": (_i, [_vp, _vp, _pp]),
    "kde_spdsr_plane_fitted_points_device": (_i, [_vp, _pp]),
    "kde_spdsr_cluster_nd_device": (_i, [_vp, _pp]),
    "kde_normals_default_params": (_i, [C.POINTER(NormalsParams)]),
    "kde_normals_create": (_i, [_pp, _i, _i, _i, C.POINTER(NormalsParams)]),
    "kde_normals_destroy": (_i, [_vp]),
    "kde_normals_set_method": (_i, [_vp, _i]),
    "kde_normals_generate_batch": (_i, [_vp, _i, _vp, _vp, _vp]),
    "kde_normals_normal_map_device": (_i, [_vp, _pp]),
    "kde_normals_normal_map_host": (_i, [_vp, _vp, _pp]),
    "kde_normals_smoothing_map_device": (_i, [_vp, _pp]),
    "kde_nasp_create": (_i, [_pp, _i, _i, _i]),
    "kde_nasp_destroy": (_i, [_vp]),
    "kde_nasp_set_parameters": (_i, [_vp, _i, _i, _vp]),
    "kde_nasp_segmentation": (_i, [_vp, _vp, _vp, _vp, _f, _f, _f, _f, _i, _vp]),
    "kde_nasp_segmentation_batch": (_i, [_vp, _i, _vp, _vp, _vp, _f, _f, _f, _f, _i, _vp]),
    "kde_nasp_labels_device": (_i, [_vp, _pp]),
    "kde_nasp_mean_device": (_i, [_vp, _pp]),
    "kde_nasp_centers_device": (_i, [_vp, _pp]),
    "kde_nasp_normals_device": (_i, [_vp, _pp]),
    "kde_nasp_normals_variance_device": (_i, [_vp, _pp]),
    "kde_nasp_ld_device": (_i, [_vp, _pp]),
    "kde_nasp_labels_host": (_i, [_vp, _vp, _pp]),
    "kde_nasp_mean_host": (_i, [_vp, _vp, _pp, C.POINTER(_i)]),
    "kde_nasp_centers_host": (_i, [_vp, _vp, _pp, C.POINTER(_i)]),
    "kde_nasp_normals_host": (_i, [_vp, _vp, _pp, C.POINTER(_i)]),
    "kde_nasp_normals_variance_host": (_i, [_vp, _vp, _pp, C.POINTER(_i)]),
    "kde_les_default_params": (_i, [C.POINTER(LesParams)]),
    "kde_les_create": (_i, [_pp, _i, _i, _i, C.POINTER(LesParams)]),
    "kde_les_destroy": (_i, [_vp]),
    "kde_les_label_image": (_i, [_vp, _vp, _vp, _vp, _vp, _i, _vp]),
    "kde_les_label_image_batch": (_i, [_vp, _i, _vp, _vp, _vp, _vp, _i, _vp]),
    "kde_les_merged_label_device": (_i, [_vp, _pp]),
    "kde_les_merged_nd_device": (_i, [_vp, _pp]),
    "kde_les_merged_variance_device": (_i, [_vp, _pp]),
    "kde_les_merged_size_device": (_i, [_vp, _pp]),
    "kde_les_merged_label_host": (_i, [_vp, _vp, _pp]),
    "kde_les_merged_nd_host": (_i, [_vp, _vp, _pp]),
    "kde_proj_default_params": (_i, [C.POINTER(ProjParams)]),
    "kde_proj_create": (_i, [_pp, _i, _i, _i, _vp, C.POINTER(ProjParams)]),
    "kde_proj_destroy": (_i, [_vp]),
    "kde_proj_plane_projection": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _i, _vp]),
    "kde_proj_plane_projection_batch": (_i, [_vp, _i, _vp, _vp, _vp, _vp, _vp, _i, _vp]),
    "kde_proj_optimized_points_device": (_i, [_vp, _pp]),
    "kde_proj_optimized_points_host": (_i, [_vp, _vp, _pp]),
    "kde_proj_plane_fitted_points_device": (_i, [_vp, _pp]),
    "kde_proj_plane_fitted_points_host": (_i, [_vp, _vp, _pp]),
    "kde_enh_create": (_i, [_pp, _i, _i, _i]),
    "kde_enh_destroy": (_i, [_vp]),
    "kde_enh_set_parameters": (_i, [_vp, _i, _i, _vp]),
    "kde_enh_process_batch": (_i, [_vp, _i, _vp, _vp, _vp]),
    "kde_enh_optimized_points_device": (_i, [_vp, _pp]),
    "kde_enh_optimized_points_host": (_i, [_vp, _vp, _pp]),
    "kde_enh_nasp_labels_device": (_i, [_vp, _pp]),
    "kde_enh_merged_labels_device": (_i, [_vp, _pp]),
    "kde_enh_edge_enhanced_points_device": (_i, [_vp, _pp]),
    "kde_points_to_depth": (_i, [_sz, _vp, _i, _vp, _vp]),
    "kde_enh_feed_create": (_i, [C.POINTER(EnhFeedHandle), _vp, _i]),
    "kde_enh_feed_destroy": (_i, [EnhFeedHandle]),
    "kde_enh_feed_process": (_i, [EnhFeedHandle, _i, _vp, _i, _vp, _i, _vp]),
    "kde_enh_feed_last_stats": (_i, [EnhFeedHandle, C.POINTER(FeedStats)]),
    "kde_error3d_create": (_i, [C.POINTER(Error3dHandle), _i, _i, _i, _i]),
    "kde_error3d_destroy": (_i, [Error3dHandle]),
    "kde_error3d_set_camera": (_i, [Error3dHandle, _vp]),
    "kde_error3d_set_range": (_i, [Error3dHandle, _f, _f]),
    "kde_error3d_compare_batch": (_i, [Error3dHandle, _i, _i, C.POINTER(Error3dSource), C.POINTER(Error3dSource), _i, _vp]),
    "kde_error3d_results_device": (_i, [Error3dHandle, _pp]),
    "kde_error3d_results_host": (_i, [Error3dHandle, _vp, _pp]),
    "kde_cloud_default_params": (_i, [C.POINTER(CloudParams)]),
    "kde_cloud_create": (_i, [C.POINTER(CloudHandle), _i, _i, _i, C.POINTER(CloudParams)]),
    "kde_cloud_destroy": (_i, [CloudHandle]),
    "kde_cloud_set_camera": (_i, [CloudHandle, _vp]),
    "kde_cloud_build_batch": (_i, [CloudHandle, _i, C.POINTER(Error3dSource), _vp, _i, _vp, _vp]),
    "kde_cloud_points_device": (_i, [CloudHandle, _pp]),
    "kde_cloud_counts_device": (_i, [CloudHandle, _pp]),
    "kde_cloud_counts_host": (_i, [CloudHandle, _vp, _pp]),
    "kde_cloud_points_host": (_i, [CloudHandle, _vp, _pp, _pp]),
    "kde_mesh_default_params": (_i, [C.POINTER(MeshParams)]),
    "kde_mesh_create": (_i, [C.POINTER(MeshHandle), _i, _i, _i, C.POINTER(MeshParams)]),
    "kde_mesh_destroy": (_i, [MeshHandle]),
    "kde_mesh_set_camera": (_i, [MeshHandle, _vp]),
    "kde_mesh_build_batch": (_i, [MeshHandle, _i, C.POINTER(Error3dSource), _vp, _i, _vp, _vp, _vp]),
    "kde_mesh_vertices_device": (_i, [MeshHandle, _pp]),
    "kde_mesh_triangles_device": (_i, [MeshHandle, _pp]),
    "kde_mesh_counts_device": (_i, [MeshHandle, _pp]),
    "kde_mesh_tri_counts_device": (_i, [MeshHandle, _pp]),
    "kde_mesh_counts_host": (_i, [MeshHandle, _vp, _pp]),
    "kde_mesh_tri_counts_host": (_i, [MeshHandle, _vp, _pp]),
    "kde_mesh_vertices_host": (_i, [MeshHandle, _vp, _pp, _pp]),
    "kde_mesh_triangles_host": (_i, [MeshHandle, _vp, _pp, _pp]),
    "kde_reg_default_params": (_i, [C.POINTER(RegParams)]),
    "kde_reg_create": (_i, [C.POINTER(RegHandle), _i, _i, _i, _i, _i, C.POINTER(RegParams)]),
    "kde_reg_destroy": (_i, [RegHandle]),
    "kde_reg_set_calibration": (_i, [RegHandle, _vp, _vp, _vp, _vp]),
    "kde_reg_register_batch": (_i, [RegHandle, _i, _vp, _i, _i, _vp, _vp]),
    "kde_reg_color_to_depth_batch": (_i, [RegHandle, _i, _vp, _i, _vp, _i, _vp, _vp]),
    "kde_reg_depth_device": (_i, [RegHandle, _pp]),
    "kde_reg_depth_host": (_i, [RegHandle, _vp, _pp]),
    "kde_reg_filled_device": (_i, [RegHandle, _pp]),
    "kde_reg_filled_host": (_i, [RegHandle, _vp, _pp]),
    "kde_undist_default_params": (_i, [C.POINTER(UndistParams)]),
    "kde_undist_create": (_i, [C.POINTER(UndistHandle), _i, _i, _i, _i, _i, C.POINTER(UndistParams)]),
    "kde_undist_destroy": (_i, [UndistHandle]),
    "kde_undist_set_calibration": (_i, [UndistHandle, _vp, _vp, _vp]),
    "kde_undist_color_batch": (_i, [UndistHandle, _i, _vp, _i, _vp, _vp]),
    "kde_undist_depth_batch": (_i, [UndistHandle, _i, _vp, _i, _i, _vp, _vp]),
    "kde_undist_depth_device": (_i, [UndistHandle, _pp]),
    "kde_undist_depth_host": (_i, [UndistHandle, _vp, _pp]),
    "kde_undist_filled_device": (_i, [UndistHandle, _pp]),
    "kde_undist_filled_host": (_i, [UndistHandle, _vp, _pp]),
    "kde_undist_map_device": (_i, [UndistHandle, _vp, _pp]),
    "kde_upsample_default_params": (_i, [C.POINTER(UpsampleParams)]),
    "kde_upsample_create": (_i, [C.POINTER(UpsampleHandle), _i, _i, _i, _i, _i, C.POINTER(UpsampleParams)]),
    "kde_upsample_destroy": (_i, [UpsampleHandle]),
    "kde_upsample_depth_batch": (_i, [UpsampleHandle, _i, _vp, _i, _vp, _i, _i, _vp, _vp]),
    "kde_upsample_depth_device": (_i, [UpsampleHandle, _pp]),
    "kde_upsample_depth_host": (_i, [UpsampleHandle, _vp, _pp]),
    "kde_upsample_filled_device": (_i, [UpsampleHandle, _pp]),
    "kde_upsample_filled_host": (_i, [UpsampleHandle, _vp, _pp]),
    "kde_upsample_range_table": (_i, [UpsampleHandle, _vp, _i]),
    "kde_holefill_default_params": (_i, [C.POINTER(HolefillParams)]),
    "kde_holefill_create": (_i, [C.POINTER(HolefillHandle), _i, _i, _i, C.POINTER(HolefillParams)]),
    "kde_holefill_destroy": (_i, [HolefillHandle]),
    "kde_holefill_fill_batch": (_i, [HolefillHandle, _i, _vp, _i, _vp, _i, _i, _vp, _vp, _vp]),
    "kde_holefill_depth_device": (_i, [HolefillHandle, _pp]),
    "kde_holefill_depth_host": (_i, [HolefillHandle, _vp, _pp]),
    "kde_holefill_filled_device": (_i, [HolefillHandle, _pp]),
    "kde_holefill_filled_host": (_i, [HolefillHandle, _vp, _pp]),
    "kde_holefill_remaining_device": (_i, [HolefillHandle, _pp]),
    "kde_holefill_remaining_host": (_i, [HolefillHandle, _vp, _pp]),
    "kde_holefill_passes_per_launch": (_i, [HolefillHandle, C.POINTER(_i)]),
    "kde_holefill_space_table": (_i, [HolefillHandle, _vp, _i]),
    "kde_holefill_range_table": (_i, [HolefillHandle, _vp, _i]),
    "kde_speckle_default_params": (_i, [C.POINTER(SpeckleParams)]),
    "kde_speckle_create": (_i, [C.POINTER(SpeckleHandle), _i, _i, _i, C.POINTER(SpeckleParams)]),
    "kde_speckle_destroy": (_i, [SpeckleHandle]),
    "kde_speckle_filter_batch": (_i, [SpeckleHandle, _i, _vp, _i, _i, _vp, _vp, _vp]),
    "kde_speckle_depth_device": (_i, [SpeckleHandle, _pp]),
    "kde_speckle_depth_host": (_i, [SpeckleHandle, _vp, _pp]),
    "kde_speckle_removed_device": (_i, [SpeckleHandle, _pp]),
    "kde_speckle_removed_host": (_i, [SpeckleHandle, _vp, _pp]),
    "kde_speckle_components_device": (_i, [SpeckleHandle, _pp]),
    "kde_speckle_components_host": (_i, [SpeckleHandle, _vp, _pp]),
    "kde_speckle_capped_device": (_i, [SpeckleHandle, _pp]),
    "kde_speckle_capped_host": (_i, [SpeckleHandle, _vp, _pp]),
    "kde_temporal_default_params": (_i, [C.POINTER(TemporalParams)]),
    "kde_temporal_create": (_i, [C.POINTER(TemporalHandle), _i, _i, _i, C.POINTER(TemporalParams)]),
    "kde_temporal_destroy": (_i, [TemporalHandle]),
    "kde_temporal_filter_batch": (_i, [TemporalHandle, _i, _vp, _i, _vp, _i, _vp, _vp]),
    "kde_temporal_reset": (_i, [TemporalHandle, _vp]),
    "kde_temporal_state_device": (_i, [TemporalHandle, _pp, _pp]),
    "kde_temporal_set_shape": (_i, [TemporalHandle, _i, _i]),
    "kde_temporal_shape": (_i, [TemporalHandle, _i, C.POINTER(_i), C.POINTER(_i)]),
    "kde_temporal_depth_device": (_i, [TemporalHandle, _pp]),
    "kde_temporal_depth_host": (_i, [TemporalHandle, _vp, _pp]),
    "kde_temporal_smoothed_device": (_i, [TemporalHandle, _pp]),
    "kde_temporal_smoothed_host": (_i, [TemporalHandle, _vp, _pp]),
    "kde_temporal_jumped_device": (_i, [TemporalHandle, _pp]),
    "kde_temporal_jumped_host": (_i, [TemporalHandle, _vp, _pp]),
    "kde_temporal_held_device": (_i, [TemporalHandle, _pp]),
    "kde_temporal_held_host": (_i, [TemporalHandle, _vp, _pp]),
    "kde_temporal_changed_device": (_i, [TemporalHandle, _pp]),
    "kde_temporal_changed_host": (_i, [TemporalHandle, _vp, _pp]),
    "kde_decimate_default_params": (_i, [C.POINTER(DecimateParams)]),
    "kde_decimate_create": (_i, [C.POINTER(DecimateHandle), _i, _i, _i, C.POINTER(DecimateParams)]),
    "kde_decimate_destroy": (_i, [DecimateHandle]),
    "kde_decimate_out_size": (_i, [DecimateHandle, C.POINTER(_i), C.POINTER(_i)]),
    "kde_decimate_depth_batch": (_i, [DecimateHandle, _i, _vp, _i, _i, _vp, _vp]),
    "kde_decimate_color_batch": (_i, [DecimateHandle, _i, _vp, _vp, _vp]),
    "kde_decimate_intrinsics": (_i, [DecimateHandle, _vp, _vp]),
    "kde_decimate_depth_device": (_i, [DecimateHandle, _pp]),
    "kde_decimate_depth_host": (_i, [DecimateHandle, _vp, _pp]),
    "kde_decimate_filled_device": (_i, [DecimateHandle, _pp]),
    "kde_decimate_filled_host": (_i, [DecimateHandle, _vp, _pp]),
    "kde_decimate_mixed_device": (_i, [DecimateHandle, _pp]),
    "kde_decimate_mixed_host": (_i, [DecimateHandle, _vp, _pp]),
}


def use_library(path: str) -> None:
    """Bind to another build of the same sources instead of libkde_hip.so -- the measurement build under tools/hooks/
    (libkde_hip_stage.so).  Must be called before the first lib(); the product never calls it."""
    global LIB_PATH
    if _lib is not None and os.path.abspath(path) != os.path.abspath(LIB_PATH):
        raise RuntimeError(f"{LIB_PATH} is already loaded")
    LIB_PATH = os.path.abspath(path)


def lib() -> C.CDLL:
    """Load libkde_hip.so; raises if it is not built (no fallback)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise FileNotFoundError(
                f"{LIB_PATH} is missing: build it with `make -C {CSRC}` (or __graft_entry__.build()). "
                "There is no CPU fallback for the product path.")
        l = C.CDLL(LIB_PATH)
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(l, name)   # AttributeError if the ABI lost a symbol
            fn.restype = res
            fn.argtypes = args
        _lib = l
    return _lib


def check(rc: int) -> None:
    if rc != KDE_OK:
        raise KdeError(rc, lib().kde_last_error_string().decode("utf-8", "replace"))
