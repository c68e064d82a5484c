"""ctypes binding of libpt_amd.so (the C ABI declared in include/pt_amd.h).

This is plumbing for the Python-side drivers (bench.py, tests, multi-GPU launcher);
all rendering happens in the HIP library.  There is NO CPU fallback: if the shared
library is missing, or no HIP device is present when a render entry point is
called, an exception is raised.
"""
from __future__ import annotations

import ctypes as C
import math
import os
from typing import Optional, Sequence, Tuple

import numpy as np

_PKG = os.path.dirname(os.path.abspath(__file__))
# PT_AMD_LIB lets experiment tooling (tools/ab*.sh, tools/pmc_*.sh) load an A/B build from elsewhere instead of
# overwriting the in-tree product library.
LIB_PATH = os.environ.get("PT_AMD_LIB") or os.path.join(_PKG, "libpt_amd.so")
PT_MAX_DEPTH = 64
ARITH = {"exact": 0, "fma": 1, "fast": 2}  # PT_ARITH_* (include/pt_amd.h)
ARITH_NAMES = {v: k for k, v in ARITH.items()}
FEATURE_PLANES = 3            # PT_FEATURE_PLANES
NOISE_PLANES = 2              # PT_NOISE_PLANES
NOISE_PIXELS_PER_PARTIAL = 1024  # PT_NOISE_PIXELS_PER_PARTIAL
CONVERGENCE_WAVES = 16        # PT_CONVERGENCE_WAVES
CONVERGENCE_CAPACITY = 65536  # PT_CONVERGENCE_CAPACITY: iterations the convergence metric keeps a value for
FLT_MAX = float(np.finfo(np.float32).max)


class PtGeom(C.Structure):
    _fields_ = [("type", C.c_int32), ("materialid", C.c_int32), ("transform", C.c_float * 16),
                ("inverseTransform", C.c_float * 16), ("invTranspose", C.c_float * 16)]


class PtMaterial(C.Structure):
    _fields_ = [("color", C.c_float * 3), ("specular_exponent", C.c_float), ("specular_color", C.c_float * 3),
                ("hasReflective", C.c_float), ("hasRefractive", C.c_float), ("indexOfRefraction", C.c_float),
                ("emittance", C.c_float)]


class PtCamera(C.Structure):
    _fields_ = [("resolution", C.c_int32 * 2), ("position", C.c_float * 3), ("lookAt", C.c_float * 3),
                ("view", C.c_float * 3), ("up", C.c_float * 3), ("right", C.c_float * 3), ("fov", C.c_float * 2),
                ("pixelLength", C.c_float * 2)]


class PtBVHNode(C.Structure):
    _fields_ = [("bmin", C.c_float * 3), ("bmax", C.c_float * 3), ("left", C.c_int32), ("right", C.c_int32),
                ("geomIndex", C.c_int32)]


class PtGridInfo(C.Structure):
    _fields_ = [("res", C.c_int32 * 3), ("origin", C.c_float * 3), ("cell_size", C.c_float * 3), ("pad", C.c_float),
                ("num_cells", C.c_int32), ("num_records", C.c_int32), ("num_leaves", C.c_int32)]


class PtGridRecord(C.Structure):
    _fields_ = [("bmin", C.c_float * 3), ("bmax", C.c_float * 3), ("leaf", C.c_int32), ("neighbours", C.c_int32)]


class PtCameraGridResult(C.Structure):
    """What pt_stage_camera_grid and pt_camera_grid_host report (include/pt_amd.h): status 0 built, PT_DEVICE_TABLES_LIST,
    PT_DEVICE_TABLES_CELLS or PT_CAMERA_GRID_NONE."""
    _fields_ = [("res", C.c_int32 * 3), ("origin", C.c_float * 3), ("cell_size", C.c_float * 3), ("inv_cell_size", C.c_float * 3), ("pad", C.c_float),
                ("guard", C.c_uint32), ("num_cells", C.c_int64), ("refs", C.c_uint64), ("longest", C.c_uint32), ("status", C.c_int32)]


class PtSceneDesc(C.Structure):
    _fields_ = [("geoms", C.POINTER(PtGeom)), ("num_geoms", C.c_int32), ("materials", C.POINTER(PtMaterial)),
                ("num_materials", C.c_int32), ("camera", PtCamera), ("trace_depth", C.c_int32)]


class PtOptions(C.Structure):
    _fields_ = [("device", C.c_int32), ("pixel_begin", C.c_int32), ("pixel_count", C.c_int32),
                ("iters_per_batch", C.c_int32), ("num_queues", C.c_int32), ("blocks_per_cu", C.c_int32),
                ("time_kernels", C.c_int32), ("legacy_traversal", C.c_int32), ("debug_flags", C.c_int32), ("unfused_primary", C.c_int32), ("unfused_bounces", C.c_int32), ("stripe_pixels", C.c_int32), ("stripe_stride", C.c_int32),
                ("arith", C.c_int32), ("aa_jitter", C.c_int32), ("convergence", C.c_int32),
                ("lds_table_kb", C.c_int32), ("primary_pieces", C.c_int32), ("paths_pieces", C.c_int32), ("paths_min_piece", C.c_int32)]


class PtStats(C.Structure):
    _fields_ = [("samples", C.c_int64), ("live_rays", C.c_int64 * PT_MAX_DEPTH), ("intersect_launches", C.c_int64),
                ("intersect_ms", C.c_double), ("render_ms", C.c_double), ("num_cus", C.c_int32),
                ("grid_blocks", C.c_int32), ("num_queues", C.c_int32), ("iters_per_batch", C.c_int32),
                ("device_bytes", C.c_int64), ("primary_fused", C.c_int32), ("bounces_fused", C.c_int32),
                ("arith", C.c_int32), ("grid_cells", C.c_int32), ("tight_leaves", C.c_int32), ("paths_waves", C.c_int32), ("record_form", C.c_int32),
                ("gather_form", C.c_int32), ("primary_launches", C.c_int64), ("inline_gathers", C.c_int64)]


class PtDenoiseOptions(C.Structure):
    """Options of the edge-avoiding filter (include/pt_amd.h); 0 in a field = its default (5 levels, sigmas 4 / 0.5 / 1, demodulate)."""
    _fields_ = [("levels", C.c_int32), ("sigma_color", C.c_float), ("sigma_normal", C.c_float), ("sigma_position", C.c_float),
                ("keep_albedo", C.c_int32)]


class PtHistoryOptions(C.Structure):
    """Options of the reprojected sample history (include/pt_amd.h); 0 in a field = its default (cap 32, normal dot 0.9, plane
    tolerance 0.02, reflective geoms carry nothing); a negative min_normal_dot / plane_tol switches that test off."""
    _fields_ = [("cap", C.c_float), ("min_normal_dot", C.c_float), ("plane_tol", C.c_float), ("keep_view_dependent", C.c_int32)]


class PtHistoryRoundOptions(C.Structure):
    """Options of the history round (include/pt_amd.h: pt_history_round); 0 in a field = its default (min_history 4 samples,
    max_fraction 1)."""
    _fields_ = [("min_history", C.c_float), ("max_fraction", C.c_float)]


class PtHistoryProbeOptions(C.Structure):
    """Options of the history probes' check (include/pt_amd.h: pt_history_probe_check); 0 in a field = its default (radius 0: the
    pixel's own probe cell, gain 0.25); radius -1 = 0."""
    _fields_ = [("radius", C.c_int32), ("gain", C.c_float)]


class PtHistoryFeedbackOptions(C.Structure):
    """Options of the feedback (include/pt_amd.h: pt_history_denoise_feedback); 0 in a field = its default (level 1, rule 1); variance
    -1 = rule 0."""
    _fields_ = [("level", C.c_int32), ("variance", C.c_int32)]


class PtSetupTimes(C.Structure):
    """Host wall-clock times of a renderer's setup and of its last camera move, ms (include/pt_amd.h: pt_get_setup_times)."""
    _fields_ = [("tables_ms", C.c_double), ("upload_ms", C.c_double), ("buffers_ms", C.c_double), ("probe_ms", C.c_double),
                ("set_camera_ms", C.c_double), ("set_camera_calls", C.c_int32)]


class PtSetCameraTimes(C.Structure):
    """Host wall-clock times of a renderer's last camera move, ms, and which build made its tables (include/pt_amd.h:
    pt_get_set_camera_times): path 0 host / 1 device, fallback 0 or PT_DEVICE_TABLES_LIST / PT_DEVICE_TABLES_CELLS."""
    _fields_ = [("tables_ms", C.c_double), ("rearm_ms", C.c_double), ("total_ms", C.c_double), ("path", C.c_int32), ("fallback", C.c_int32)]


class PtSetMaterialsTimes(C.Structure):
    """Host wall-clock times of a renderer's last pt_set_materials, ms (include/pt_amd.h: pt_get_set_materials_times)."""
    _fields_ = [("upload_ms", C.c_double), ("rearm_ms", C.c_double), ("total_ms", C.c_double)]


class PtSetGeomsTimes(C.Structure):
    """Host wall-clock times of a renderer's last pt_set_geoms, ms (include/pt_amd.h: pt_get_set_geoms_times)."""
    _fields_ = [("build_ms", C.c_double), ("upload_ms", C.c_double), ("rearm_ms", C.c_double), ("total_ms", C.c_double)]


PT_SET_CAMERA_DEVICE_TABLES = 1
PT_DEVICE_TABLES_LIST, PT_DEVICE_TABLES_CELLS = 1, 2
PT_CAMERA_GRID_NONE = 3
# PtTableNode and PtGridRecord, 32 bytes each (csrc/pt_device.h ptd::Node)
TABLE_NODE = np.dtype([("bmin", np.float32, 3), ("bmax", np.float32, 3), ("skip", np.int32), ("geom", np.int32)])
TABLE_NAMES = ("nodes", "nodes_b", "top", "top_b", "grid_start", "grid_items", "grid_items_b", "cull_margin", "geoms")  # pt_stage_read_tables' `which`


class PtError(RuntimeError):
    pass


_lib: Optional[C.CDLL] = None
_fp = C.POINTER(C.c_float)
_ip = C.POINTER(C.c_int32)


def lib() -> C.CDLL:
    """Load libpt_amd.so; fail loudly when it has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise PtError(f"{LIB_PATH} not found: run `python -c 'import __graft_entry__ as g; g.build()'` "
                      "(hipcc --offload-arch=gfx950).  There is no CPU fallback.")
    L = C.CDLL(LIB_PATH)
    L.pt_last_error.restype = C.c_char_p
    L.pt_scene_load.argtypes = [C.c_char_p, C.c_int, C.c_int, C.POINTER(C.c_void_p)]
    L.pt_scene_free.argtypes = [C.c_void_p]
    L.pt_scene_free.restype = None
    L.pt_scene_desc.argtypes = [C.c_void_p, C.POINTER(PtSceneDesc)]
    L.pt_scene_iterations.argtypes = [C.c_void_p]
    L.pt_scene_image_name.argtypes = [C.c_void_p]
    L.pt_scene_image_name.restype = C.c_char_p
    L.pt_build_bvh.argtypes = [C.POINTER(PtGeom), C.c_int, C.POINTER(PtBVHNode), C.c_int]
    L.pt_build_grid.argtypes = [C.POINTER(PtGeom), C.c_int, C.c_int, C.POINTER(PtGridInfo), C.POINTER(C.c_uint32), C.POINTER(PtGridRecord)]
    if hasattr(L, "pt_selfcheck_ieee"):
        L.pt_selfcheck_ieee.argtypes = [C.c_int, C.c_int, C.c_uint64, C.c_uint64, C.c_uint32, C.POINTER(C.c_uint64)]
    if hasattr(L, "pt_selfcheck_fast_math"):
        L.pt_selfcheck_fast_math.argtypes = [C.c_int, C.c_int, C.c_uint64, C.c_uint64, C.POINTER(C.c_double)]
    if hasattr(L, "pt_traversal_boxes"):  # absent from older A/B builds of the library (tools/build_rev.sh)
        L.pt_traversal_boxes.argtypes = [C.POINTER(PtGeom), C.c_int, _fp, _fp]
    if hasattr(L, "pt_center_half_box"):
        L.pt_center_half_box.argtypes = [_fp, _fp, C.c_int, C.c_float, _fp, _fp]
        L.pt_center_half_box.restype = None
    L.pt_build_transform.argtypes = [_fp, _fp, _fp, _fp]
    L.pt_init.argtypes = [C.POINTER(PtSceneDesc), C.POINTER(PtOptions)]
    L.pt_render.argtypes = [C.c_int, C.c_int]
    L.pt_readback.argtypes = [_fp]
    L.pt_readback_device.argtypes = [C.c_void_p]
    L.pt_preview_rgba8.argtypes = [C.c_int, C.POINTER(C.c_uint8)]
    L.pt_preview_rgba8_device.argtypes = [C.c_int, C.c_void_p]
    L.pt_get_stats.argtypes = [C.POINTER(PtStats)]
    L.pt_stage_generate.argtypes = [C.c_int, C.c_int, _fp, _fp]
    L.pt_stage_intersect.argtypes = [C.c_int, _fp, _fp, _fp, _fp, _ip, _fp]
    if hasattr(L, "pt_stage_intersect_grid"):  # absent only in older A/B builds loaded through PT_AMD_LIB (tools/build_rev.sh)
        L.pt_stage_intersect_grid.argtypes = [C.c_int, _fp, _fp, C.c_int, _fp, _fp, _ip, _fp]
        L.pt_stage_grid_info.argtypes = [C.POINTER(PtGridInfo), C.POINTER(C.c_int32)]
    L.pt_stage_shade.argtypes = [C.c_int, C.c_int, _ip, _ip, _fp, _fp, _ip, _fp, _fp, _fp, _fp, _ip]
    _u8p = C.POINTER(C.c_uint8)
    L.pt_save_u8.argtypes = [C.c_float, _u8p]
    L.pt_stage_save_u8.argtypes = [C.c_int, C.c_int, C.c_float, _fp, _u8p]
    L.pt_ctx_create.argtypes = [C.POINTER(PtSceneDesc), C.POINTER(PtOptions), C.POINTER(C.c_void_p)]
    L.pt_ctx_destroy.argtypes = [C.c_void_p]
    L.pt_ctx_render.argtypes = [C.c_void_p, C.c_int, C.c_int]
    L.pt_ctx_sync.argtypes = [C.c_void_p]
    L.pt_ctx_readback.argtypes = [C.c_void_p, _fp]
    L.pt_ctx_readback_device.argtypes = [C.c_void_p, C.c_void_p]
    L.pt_ctx_save_u8.argtypes = [C.c_void_p, C.c_float, _u8p]
    L.pt_ctx_get_stats.argtypes = [C.c_void_p, C.POINTER(PtStats)]
    L.pt_ctx_reset_stats.argtypes = [C.c_void_p]
    L.pt_ctx_clear.argtypes = [C.c_void_p]
    L.pt_ctx_pixel_count.argtypes = [C.c_void_p]
    L.pt_group_create.argtypes = [C.POINTER(PtSceneDesc), C.POINTER(PtOptions), _ip, C.c_int, C.POINTER(C.c_void_p)]
    if hasattr(L, "pt_group_create_ex"):  # absent only in older A/B builds loaded through PT_AMD_LIB (tools/build_rev.sh)
        L.pt_group_create_ex.argtypes = [C.POINTER(PtSceneDesc), C.POINTER(PtOptions), _ip, C.c_int, C.c_int, C.POINTER(C.c_void_p)]
        L.pt_group_transport.argtypes = [C.c_void_p]
    L.pt_group_destroy.argtypes = [C.c_void_p]
    L.pt_group_size.argtypes = [C.c_void_p]
    L.pt_group_context.argtypes = [C.c_void_p, C.c_int]
    L.pt_group_context.restype = C.c_void_p
    L.pt_group_render.argtypes = [C.c_void_p, C.c_int, C.c_int]
    L.pt_group_sync.argtypes = [C.c_void_p]
    L.pt_group_gather.argtypes = [C.c_void_p, _fp]
    L.pt_group_gather_u8.argtypes = [C.c_void_p, C.c_float, _u8p]
    L.pt_group_preview_rgba8.argtypes = [C.c_void_p, C.c_int, _u8p]
    L.pt_write_png_rgb8.argtypes = [C.c_char_p, _u8p, C.c_int, C.c_int]
    L.pt_output_basename.argtypes = [C.c_char_p, C.c_int, C.c_char_p, C.c_int]
    L.pt_save_png.argtypes = [C.c_char_p, _fp, C.c_int, C.c_int, C.c_float]
    L.pt_save_hdr.argtypes = [C.c_char_p, _fp, C.c_int, C.c_int, C.c_float]
    L.pt_save_pfm.argtypes = [C.c_char_p, _fp, C.c_int, C.c_int, C.c_float]
    L.pt_load_pfm.argtypes = [C.c_char_p, _fp, C.c_int, _ip, _ip, C.c_float]
    _dp = C.POINTER(C.c_double)
    L.pt_psnr_from_sse.argtypes = [C.c_double, C.c_int64]
    L.pt_psnr_from_sse.restype = C.c_float
    L.pt_set_reference.argtypes = [_fp]
    L.pt_get_convergence.argtypes = [C.c_int, C.c_int, _dp]
    L.pt_iterations_to_clean.argtypes = [C.c_float, _ip]
    L.pt_ctx_set_reference.argtypes = [C.c_void_p, _fp]
    L.pt_ctx_get_convergence.argtypes = [C.c_void_p, C.c_int, C.c_int, _dp]
    L.pt_ctx_iterations_to_clean.argtypes = [C.c_void_p, C.c_float, _ip]
    L.pt_group_set_reference.argtypes = [C.c_void_p, _fp]
    L.pt_group_get_convergence.argtypes = [C.c_void_p, C.c_int, C.c_int, _dp]
    L.pt_group_iterations_to_clean.argtypes = [C.c_void_p, C.c_float, _ip]
    if hasattr(L, "pt_render_features"):  # absent from older A/B builds of the library (tools/build_rev.sh)
        L.pt_render_features.argtypes = [C.c_int, C.c_int]
        L.pt_readback_features.argtypes = [_fp]
        L.pt_ctx_render_features.argtypes = [C.c_void_p, C.c_int, C.c_int]
        L.pt_ctx_readback_features.argtypes = [C.c_void_p, _fp]
        L.pt_ctx_device_features.argtypes = [C.c_void_p]
        L.pt_ctx_device_features.restype = C.c_void_p
        L.pt_group_render_features.argtypes = [C.c_void_p, C.c_int, C.c_int]
        L.pt_group_gather_features.argtypes = [C.c_void_p, _fp]
    if hasattr(L, "pt_denoise"):  # absent from older A/B builds of the library (tools/build_rev.sh)
        _dno = C.POINTER(PtDenoiseOptions)
        L.pt_denoise.argtypes = [C.c_float, _dno, _fp]
        L.pt_ctx_denoise.argtypes = [C.c_void_p, C.c_float, _dno, _fp]
        L.pt_ctx_denoise_device.argtypes = [C.c_void_p, C.c_float, _dno, C.POINTER(C.c_void_p)]
        L.pt_group_denoise.argtypes = [C.c_void_p, C.c_float, _dno, _fp]
        L.pt_stage_denoise.argtypes = [C.c_int, C.c_int, _fp, _fp, C.c_float, _dno, _fp]
        L.pt_denoise_host.argtypes = [C.c_int, C.c_int, _fp, _fp, C.c_float, _dno, _fp]
    if hasattr(L, "pt_denoise_guided"):  # absent from older A/B builds of the library (tools/build_rev.sh)
        _dno = C.POINTER(PtDenoiseOptions)
        _guided = [C.c_int, C.c_int, _fp, _fp, _fp, C.c_int, C.c_int64, _dno]
        L.pt_denoise_guided.argtypes = [_dno, _fp]
        L.pt_ctx_denoise_guided.argtypes = [C.c_void_p, _dno, _fp]
        L.pt_ctx_denoise_guided_device.argtypes = [C.c_void_p, _dno, C.POINTER(C.c_void_p)]
        L.pt_group_denoise_guided.argtypes = [C.c_void_p, _dno, _fp]
        L.pt_stage_denoise_guided.argtypes = _guided + [_fp]
        L.pt_denoise_guided_host.argtypes = _guided + [_fp]
        L.pt_denoise_guided_variance_host.argtypes = _guided + [_fp, _fp]
    if hasattr(L, "pt_noise_fold"):  # absent from older A/B builds of the library (tools/build_rev.sh)
        _until = [C.c_int, C.c_int, C.c_int, C.c_float, _ip, _fp]
        L.pt_noise_fold.argtypes = []
        L.pt_get_noise.argtypes = [_dp, _ip, _ip]
        L.pt_readback_noise.argtypes = [_fp]
        L.pt_render_until.argtypes = _until
        L.pt_ctx_noise_fold.argtypes = [C.c_void_p]
        L.pt_ctx_get_noise.argtypes = [C.c_void_p, _dp, _ip, _ip]
        L.pt_ctx_readback_noise.argtypes = [C.c_void_p, _fp]
        L.pt_ctx_render_until.argtypes = [C.c_void_p] + _until
        L.pt_ctx_device_noise.argtypes = [C.c_void_p]
        L.pt_ctx_device_noise.restype = C.c_void_p
        L.pt_group_noise_fold.argtypes = [C.c_void_p]
        L.pt_group_get_noise.argtypes = [C.c_void_p, _dp, _ip, _ip]
        L.pt_group_render_until.argtypes = [C.c_void_p] + _until
        L.pt_noise_fold_host.argtypes = [C.c_int, _fp, _fp, C.c_int, C.c_int, C.c_int64, _dp]
    if hasattr(L, "pt_adaptive_round"):  # absent from older A/B builds of the library (tools/build_rev.sh)
        _i64p = C.POINTER(C.c_int64)
        _adaptive = [C.c_int, C.c_int, C.c_int, C.c_float, C.c_float, _ip, _i64p, _fp]
        L.pt_adaptive_round.argtypes = [C.c_int, C.c_int, C.c_float]
        L.pt_render_adaptive.argtypes = _adaptive
        L.pt_readback_adaptive.argtypes = [_ip]
        L.pt_resolve.argtypes = [_fp]
        L.pt_ctx_adaptive_round.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_float]
        L.pt_ctx_render_adaptive.argtypes = [C.c_void_p] + _adaptive
        L.pt_ctx_readback_adaptive.argtypes = [C.c_void_p, _ip]
        L.pt_ctx_resolve.argtypes = [C.c_void_p, _fp]
        L.pt_ctx_resolve_device.argtypes = [C.c_void_p, C.POINTER(C.c_void_p)]
        L.pt_adaptive_select_host.argtypes = [C.c_int, C.c_int, _fp, _ip, C.c_int, _ip]
        L.pt_stage_adaptive_select.argtypes = [C.c_int, C.c_int, _fp, _ip, C.c_int, _ip]
        L.pt_adaptive_merge_host.argtypes = [C.c_int, _fp, _fp, _ip, _ip, C.c_int, _fp, C.c_int, _dp]
        L.pt_stage_render_list.argtypes = [_ip, C.c_int, C.c_int, C.c_int, _fp]
    if hasattr(L, "pt_adaptive_round_threshold"):  # absent from older A/B builds of the library (tools/build_rev.sh)
        _i64p = C.POINTER(C.c_int64)
        _threshold = [C.c_int, C.c_int, C.c_int, C.c_float, C.c_float, C.c_int, _ip, _i64p, _ip]
        _select_thr = [C.c_int, C.c_int, _fp, _ip, C.c_float, C.c_int, _ip, _ip, _ip]
        L.pt_adaptive_round_threshold.argtypes = [C.c_int, C.c_int, C.c_float, C.c_float, _ip, _ip]
        L.pt_render_threshold.argtypes = _threshold
        L.pt_ctx_adaptive_round_threshold.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_float, C.c_float, _ip, _ip]
        L.pt_ctx_render_threshold.argtypes = [C.c_void_p] + _threshold
        L.pt_adaptive_select_threshold_host.argtypes = _select_thr
        L.pt_stage_adaptive_select_threshold.argtypes = _select_thr
        L.pt_stage_render_list_capacity.argtypes = [_ip, C.c_int, C.c_int, C.c_int, C.c_int, _fp]
    if hasattr(L, "pt_denoise_adaptive"):  # absent from older A/B builds of the library (tools/build_rev.sh)
        _dno = C.POINTER(PtDenoiseOptions)
        _dn_adaptive = [C.c_int, C.c_int, _fp, _fp, _fp, _ip, _dno]
        L.pt_denoise_adaptive.argtypes = [_dno, _fp]
        L.pt_ctx_denoise_adaptive.argtypes = [C.c_void_p, _dno, _fp]
        L.pt_ctx_denoise_adaptive_device.argtypes = [C.c_void_p, _dno, C.POINTER(C.c_void_p)]
        L.pt_stage_denoise_adaptive.argtypes = _dn_adaptive + [_fp]
        L.pt_denoise_adaptive_host.argtypes = _dn_adaptive + [_fp]
        L.pt_denoise_adaptive_variance_host.argtypes = _dn_adaptive + [_fp, _fp]
    if hasattr(L, "pt_group_adaptive_round_threshold"):  # absent from older A/B builds of the library (tools/build_rev.sh)
        _i64p = C.POINTER(C.c_int64)
        _dno = C.POINTER(PtDenoiseOptions)
        _partition = [C.c_int, C.c_int, C.c_int, _ip, C.c_int, _ip, _ip]
        L.pt_adaptive_round_list.argtypes = [C.c_int, C.c_int, _ip, C.c_int, C.c_int]
        L.pt_ctx_adaptive_round_list.argtypes = [C.c_void_p, C.c_int, C.c_int, _ip, C.c_int, C.c_int]
        L.pt_ctx_adaptive_round_list_device.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int]
        L.pt_ctx_device_counts.argtypes = [C.c_void_p]
        L.pt_ctx_device_counts.restype = C.c_void_p
        L.pt_group_adaptive_round_threshold.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_float, C.c_float, _ip, _ip]
        L.pt_group_render_threshold.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_float, C.c_float, C.c_int, _ip, _i64p, _ip]
        L.pt_group_gather_adaptive.argtypes = [C.c_void_p, _ip]
        L.pt_group_resolve.argtypes = [C.c_void_p, _fp]
        L.pt_group_denoise_adaptive.argtypes = [C.c_void_p, _dno, _fp]
        L.pt_group_partition_host.argtypes = _partition
        L.pt_stage_group_partition.argtypes = _partition
    if hasattr(L, "pt_set_camera"):
        _cam = C.POINTER(PtCamera)
        L.pt_set_camera.argtypes = [_cam]
        L.pt_ctx_set_camera.argtypes = [C.c_void_p, _cam]
        L.pt_group_set_camera.argtypes = [C.c_void_p, _cam]
        L.pt_get_setup_times.argtypes = [C.POINTER(PtSetupTimes)]
        L.pt_ctx_get_setup_times.argtypes = [C.c_void_p, C.POINTER(PtSetupTimes)]
        L.pt_camera_tables_host.argtypes = [C.POINTER(PtSceneDesc), _cam, C.c_int, C.c_int, _ip, _ip, _ip]
        L.pt_scene_orbit.argtypes = [C.c_void_p, C.c_float, C.c_float, C.c_float]
    if hasattr(L, "pt_set_camera_ex"):
        _cam = C.POINTER(PtCamera)
        L.pt_set_camera_ex.argtypes = [_cam, C.c_uint32]
        L.pt_ctx_set_camera_ex.argtypes = [C.c_void_p, _cam, C.c_uint32]
        L.pt_group_set_camera_ex.argtypes = [C.c_void_p, _cam, C.c_uint32]
        L.pt_get_set_camera_times.argtypes = [C.POINTER(PtSetCameraTimes)]
        L.pt_ctx_get_set_camera_times.argtypes = [C.c_void_p, C.POINTER(PtSetCameraTimes)]
        L.pt_stage_read_tables.argtypes = [C.c_int, C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64)]
        L.pt_selfcheck_camera_math.argtypes = [C.c_int, C.c_uint64, C.c_uint32, C.POINTER(C.c_uint64)]
        if hasattr(L, "pt_stage_camera_grid"):  # absent from older A/B builds of the library (tools/build_rev.sh)
            _grid = [C.c_void_p, C.c_int, _ip, C.c_int, _fp, _fp, C.c_double, _ip, C.c_int, C.POINTER(PtCameraGridResult), C.c_void_p, C.c_uint64,
                     C.c_void_p, C.c_void_p, C.c_uint64]
            L.pt_stage_camera_grid.argtypes = _grid
            L.pt_camera_grid_host.argtypes = _grid
        L.pt_scene_camera.argtypes = [C.c_void_p, _cam]
        L.pt_scene_orbit_state.argtypes = [C.c_void_p, _fp, _fp, _fp]
    if hasattr(L, "pt_history_capture"):  # absent from older A/B builds of the library (tools/build_rev.sh)
        _hio, _cam, _u8 = C.POINTER(PtHistoryOptions), C.POINTER(PtCamera), C.POINTER(C.c_uint8)
        _reproject = [C.c_int, C.c_int, C.c_int, _cam, _fp, _fp, _u8, C.c_int, _hio, _fp]
        L.pt_history_capture.argtypes = [C.c_float]
        L.pt_history_reproject.argtypes = [_hio]
        L.pt_history_resolve.argtypes = [C.c_float, _fp]
        L.pt_readback_history.argtypes = [_fp, _fp]
        L.pt_history_drop.argtypes = []
        L.pt_ctx_history_capture.argtypes = [C.c_void_p, C.c_float]
        L.pt_ctx_history_reproject.argtypes = [C.c_void_p, _hio]
        L.pt_ctx_history_resolve.argtypes = [C.c_void_p, C.c_float, _fp]
        L.pt_ctx_history_resolve_device.argtypes = [C.c_void_p, C.c_float, C.POINTER(C.c_void_p)]
        L.pt_ctx_readback_history.argtypes = [C.c_void_p, _fp, _fp]
        L.pt_ctx_history_drop.argtypes = [C.c_void_p]
        L.pt_history_capture_host.argtypes = [C.c_int, _fp, _fp, _fp, C.c_float, _fp]
        L.pt_history_reproject_host.argtypes = _reproject
        L.pt_stage_history_reproject.argtypes = _reproject
        L.pt_history_blend_host.argtypes = [C.c_int, _fp, C.c_float, _fp, _fp]
    if hasattr(L, "pt_history_denoise"):  # absent from older A/B builds of the library (tools/build_rev.sh)
        _hio = C.POINTER(PtHistoryOptions)
        _dno = C.POINTER(PtDenoiseOptions)
        _reproject_var = [C.c_int, C.c_int, C.c_int, C.POINTER(PtCamera), _fp, _fp, _u8p, C.c_int, _hio, _fp, _fp, _fp]
        _hdn = [C.c_int, C.c_int, _fp, _fp, _fp, C.c_int, C.c_int64, C.c_float, _fp, _fp, _dno, _fp]
        L.pt_history_capture_ex.argtypes = [C.c_float, C.c_uint32]
        L.pt_history_reproject_ex.argtypes = [_hio, C.c_uint32]
        L.pt_history_denoise.argtypes = [C.c_float, _dno, _fp]
        L.pt_readback_history_variance.argtypes = [_fp, _fp]
        L.pt_ctx_history_capture_ex.argtypes = [C.c_void_p, C.c_float, C.c_uint32]
        L.pt_ctx_history_reproject_ex.argtypes = [C.c_void_p, _hio, C.c_uint32]
        L.pt_ctx_history_denoise.argtypes = [C.c_void_p, C.c_float, _dno, _fp]
        L.pt_ctx_history_denoise_device.argtypes = [C.c_void_p, C.c_float, _dno, C.POINTER(C.c_void_p)]
        L.pt_ctx_readback_history_variance.argtypes = [C.c_void_p, _fp, _fp]
        L.pt_history_capture_variance_host.argtypes = [C.c_int, _fp, C.c_int, C.c_int64, C.c_float, _fp, _fp, _fp]
        L.pt_history_reproject_variance_host.argtypes = _reproject_var
        L.pt_stage_history_reproject_variance.argtypes = _reproject_var
        L.pt_history_denoise_host.argtypes = _hdn
        L.pt_stage_history_denoise.argtypes = _hdn
    if hasattr(L, "pt_history_denoise_ex"):  # absent from older A/B builds of the library (tools/build_rev.sh)
        _mdn = [C.c_int, C.c_int, _fp, _fp, C.c_float, _fp, _fp, _dno]
        L.pt_history_denoise_ex.argtypes = [C.c_float, _dno, C.c_uint32, _fp]
        L.pt_ctx_history_denoise_ex.argtypes = [C.c_void_p, C.c_float, _dno, C.c_uint32, _fp]
        L.pt_ctx_history_denoise_ex_device.argtypes = [C.c_void_p, C.c_float, _dno, C.c_uint32, C.POINTER(C.c_void_p)]
        L.pt_history_capture_moments_host.argtypes = [C.c_int, _fp, C.c_float, _fp, _fp, _fp]
        L.pt_history_reproject_moments_host.argtypes = _reproject_var
        L.pt_stage_history_reproject_moments.argtypes = _reproject_var
        L.pt_history_denoise_moments_host.argtypes = _mdn + [_fp, _fp, _u8p]
        L.pt_stage_history_denoise_moments.argtypes = _mdn + [_fp]
    if hasattr(L, "pt_history_round"):  # absent from older A/B builds of the library (tools/build_rev.sh)
        _hro, _dno = C.POINTER(PtHistoryRoundOptions), C.POINTER(PtDenoiseOptions)
        _select = [C.c_int, C.c_int, _fp, _fp, _u8p, C.c_int, _hro, _ip, _ip, _ip]
        _merge = [C.c_int, _fp, _fp, _ip, C.c_int, _fp, C.c_int]
        L.pt_history_round.argtypes = [C.c_int, C.c_int, _hro, _ip, _ip]
        L.pt_ctx_history_round.argtypes = [C.c_void_p, C.c_int, C.c_int, _hro, _ip, _ip]
        L.pt_readback_history_extra.argtypes = [_fp]
        L.pt_ctx_readback_history_extra.argtypes = [C.c_void_p, _fp]
        L.pt_history_select_host.argtypes = _select
        L.pt_stage_history_select.argtypes = _select
        L.pt_history_merge_host.argtypes = _merge
        L.pt_stage_history_merge.argtypes = _merge
        L.pt_history_blend_counted_host.argtypes = [C.c_int, _fp, C.c_float, _fp, _fp, _fp]
        L.pt_history_capture_counted_host.argtypes = [C.c_int, _fp, _fp, _fp, C.c_float, _fp, _fp]
        L.pt_history_capture_moments_counted_host.argtypes = [C.c_int, _fp, C.c_float, _fp, _fp, _fp, _fp]
        L.pt_history_denoise_moments_counted_host.argtypes = [C.c_int, C.c_int, _fp, _fp, C.c_float, _fp, _fp, _fp, _dno, _fp, _fp, _u8p]
    if hasattr(L, "pt_set_geoms"):  # absent from older A/B builds of the library (tools/build_rev.sh)
        _gp, _cam, _hio = C.POINTER(PtGeom), C.POINTER(PtCamera), C.POINTER(PtHistoryOptions)
        _reproject_motion = [C.c_int, C.c_int, C.c_int, _cam, _fp, _fp, _u8p, C.c_int, _hio, _fp, _fp, _u8p, C.c_uint32, _fp, _fp]
        L.pt_set_geoms.argtypes = [_gp, C.c_int]
        L.pt_ctx_set_geoms.argtypes = [C.c_void_p, _gp, C.c_int]
        L.pt_group_set_geoms.argtypes = [C.c_void_p, _gp, C.c_int]
        L.pt_get_set_geoms_times.argtypes = [C.POINTER(PtSetGeomsTimes)]
        L.pt_ctx_get_set_geoms_times.argtypes = [C.c_void_p, C.POINTER(PtSetGeomsTimes)]
        L.pt_scene_geom_trs.argtypes = [C.c_void_p, C.c_int, _fp]
        L.pt_scene_set_geom_trs.argtypes = [C.c_void_p, C.c_int, _fp]
        L.pt_history_motion_host.argtypes = [_gp, _gp, C.c_int, _fp, _u8p]
        L.pt_history_reproject_motion_host.argtypes = _reproject_motion
        L.pt_stage_history_reproject_motion.argtypes = _reproject_motion
    if hasattr(L, "pt_set_materials"):  # absent from older A/B builds of the library (tools/build_rev.sh)
        _mp, _gp, _cam, _hio = C.POINTER(PtMaterial), C.POINTER(PtGeom), C.POINTER(PtCamera), C.POINTER(PtHistoryOptions)
        _reproject_materials = [C.c_int, C.c_int, C.c_int, _cam, _fp, _fp, _u8p, C.c_int, _hio, _fp, _fp, _u8p, _fp, _u8p, C.c_uint32, _fp, _fp]
        L.pt_set_materials.argtypes = [_mp, C.c_int]
        L.pt_ctx_set_materials.argtypes = [C.c_void_p, _mp, C.c_int]
        L.pt_group_set_materials.argtypes = [C.c_void_p, _mp, C.c_int]
        L.pt_get_set_materials_times.argtypes = [C.POINTER(PtSetMaterialsTimes)]
        L.pt_ctx_get_set_materials_times.argtypes = [C.c_void_p, C.POINTER(PtSetMaterialsTimes)]
        L.pt_scene_material.argtypes = [C.c_void_p, C.c_int, _mp]
        L.pt_scene_set_material.argtypes = [C.c_void_p, C.c_int, _mp]
        L.pt_history_recolor_host.argtypes = [_mp, _mp, C.c_int, _gp, C.c_int, _fp, _u8p]
        L.pt_history_reproject_materials_host.argtypes = _reproject_materials
        L.pt_stage_history_reproject_materials.argtypes = _reproject_materials
    if hasattr(L, "pt_history_probe_keep"):  # absent from older A/B builds of the library (tools/build_rev.sh)
        _hpo = C.POINTER(PtHistoryProbeOptions)
        L.pt_history_probe_keep.argtypes = [C.c_int, C.c_int, C.c_int]
        L.pt_history_probe_check.argtypes = [_hpo, _ip, _ip, _ip]
        L.pt_readback_history_probe.argtypes = [_fp, _fp, _ip]
        L.pt_ctx_history_probe_keep.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int]
        L.pt_ctx_history_probe_check.argtypes = [C.c_void_p, _hpo, _ip, _ip, _ip]
        L.pt_ctx_readback_history_probe.argtypes = [C.c_void_p, _fp, _fp, _ip]
        L.pt_history_probe_list_host.argtypes = [C.c_int, C.c_int, C.c_int, _ip, _ip]
        L.pt_history_probe_keep_host.argtypes = [C.c_int, C.c_int, C.c_int, _fp, _fp, _fp]
        L.pt_history_probe_gradient_host.argtypes = [C.c_int, C.c_int, C.c_int, _fp, _fp, _fp, _u8p, C.c_int, _fp, _ip, _ip]
        L.pt_history_probe_apply_host.argtypes = [C.c_int, C.c_int, C.c_int, _fp, _fp, _u8p, C.c_int, _hpo, _fp]
    if hasattr(L, "pt_history_denoise_feedback"):  # absent from older A/B builds of the library (tools/build_rev.sh)
        _hio, _dno, _hfo, _cam = C.POINTER(PtHistoryOptions), C.POINTER(PtDenoiseOptions), C.POINTER(PtHistoryFeedbackOptions), C.POINTER(PtCamera)
        _reproject_fb = [C.c_int, C.c_int, C.c_int, _cam, _fp, _fp, _u8p, C.c_int, _hio, _fp, _fp, _fp, _u8p, _fp, _fp, _fp]
        _fdn = [C.c_int, C.c_int, _fp, _fp, C.c_float, _fp, _fp, _fp, _fp, _dno, _hfo, _fp, _fp]
        L.pt_history_denoise_feedback.argtypes = [C.c_float, _dno, _hfo, _fp]
        L.pt_readback_history_feedback.argtypes = [_fp, _fp, _fp]
        L.pt_ctx_history_denoise_feedback.argtypes = [C.c_void_p, C.c_float, _dno, _hfo, _fp]
        L.pt_ctx_history_denoise_feedback_device.argtypes = [C.c_void_p, C.c_float, _dno, _hfo, C.POINTER(C.c_void_p)]
        L.pt_ctx_readback_history_feedback.argtypes = [C.c_void_p, _fp, _fp, _fp]
        L.pt_history_reproject_feedback_host.argtypes = _reproject_fb
        L.pt_stage_history_reproject_feedback.argtypes = _reproject_fb
        L.pt_history_denoise_feedback_host.argtypes = _fdn + [_fp, _u8p]
        L.pt_stage_history_denoise_feedback.argtypes = _fdn
    if hasattr(L, "pt_history_noise"):  # absent from older A/B builds of the library (tools/build_rev.sh)
        _hnz = [C.c_int, _fp, C.c_int, C.c_int64, C.c_float, _fp, _fp, _fp, _dp]
        _huntil = [C.c_int, C.c_int, C.c_int, C.c_float, _ip, _fp, _fp]
        L.pt_history_noise.argtypes = [C.c_float, C.c_uint32, _dp]
        L.pt_readback_history_noise.argtypes = [_fp]
        L.pt_history_render_until.argtypes = _huntil
        L.pt_ctx_history_noise.argtypes = [C.c_void_p, C.c_float, C.c_uint32, _dp]
        L.pt_ctx_readback_history_noise.argtypes = [C.c_void_p, _fp]
        L.pt_ctx_history_render_until.argtypes = [C.c_void_p] + _huntil
        L.pt_history_noise_host.argtypes = _hnz
        L.pt_stage_history_noise.argtypes = _hnz
    if hasattr(L, "pt_history_round_threshold"):  # absent from older A/B builds of the library (tools/build_rev.sh)
        _i64p, _dno = C.POINTER(C.c_int64), C.POINTER(PtDenoiseOptions)
        _hthreshold = [C.c_int, C.c_int, C.c_int, C.c_float, C.c_float, C.c_int, _ip, _i64p, _ip]
        _hnza = [C.c_int, _fp, _ip, _fp, _fp, _fp, _fp]
        _hselect = [C.c_int, C.c_int, _fp, _ip, _fp, _fp, C.c_float, C.c_int, _ip, _ip, _ip]
        _hcapture = [C.c_int, _fp, _fp, _fp, _ip, _fp, _fp, _fp, _fp]
        _hdna = [C.c_int, C.c_int, _fp, _fp, _fp, _ip, _fp, _fp, _dno]
        L.pt_history_noise_adaptive.argtypes = [_dp]
        L.pt_readback_history_noise_samples.argtypes = [_fp]
        L.pt_history_round_threshold.argtypes = [C.c_int, C.c_int, C.c_float, C.c_float, _ip, _ip]
        L.pt_history_render_threshold.argtypes = _hthreshold
        L.pt_history_resolve_adaptive.argtypes = [_fp]
        L.pt_history_capture_adaptive.argtypes = []
        L.pt_history_denoise_adaptive.argtypes = [_dno, _fp]
        L.pt_ctx_history_noise_adaptive.argtypes = [C.c_void_p, _dp]
        L.pt_ctx_readback_history_noise_samples.argtypes = [C.c_void_p, _fp]
        L.pt_ctx_history_round_threshold.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_float, C.c_float, _ip, _ip]
        L.pt_ctx_history_render_threshold.argtypes = [C.c_void_p] + _hthreshold
        L.pt_ctx_history_resolve_adaptive.argtypes = [C.c_void_p, _fp]
        L.pt_ctx_history_resolve_adaptive_device.argtypes = [C.c_void_p, C.POINTER(C.c_void_p)]
        L.pt_ctx_history_capture_adaptive.argtypes = [C.c_void_p]
        L.pt_ctx_history_denoise_adaptive.argtypes = [C.c_void_p, _dno, _fp]
        L.pt_ctx_history_denoise_adaptive_device.argtypes = [C.c_void_p, _dno, C.POINTER(C.c_void_p)]
        L.pt_history_noise_adaptive_host.argtypes = _hnza + [_fp, _dp]
        L.pt_stage_history_noise_adaptive.argtypes = _hnza + [_dp]
        L.pt_history_select_threshold_blend_host.argtypes = _hselect
        L.pt_stage_history_select_threshold_blend.argtypes = _hselect
        L.pt_history_blend_adaptive_host.argtypes = [C.c_int, _fp, _ip, _fp, _fp]
        L.pt_history_capture_adaptive_host.argtypes = _hcapture
        L.pt_stage_history_capture_adaptive.argtypes = _hcapture + [_fp]
        L.pt_history_denoise_adaptive_host.argtypes = _hdna + [_fp]
        L.pt_stage_history_denoise_adaptive.argtypes = _hdna + [_fp]
        L.pt_history_denoise_adaptive_variance_host.argtypes = _hdna + [_fp, _fp]
    if hasattr(L, "pt_group_history_round"):  # absent from older A/B builds of the library (tools/build_rev.sh)
        _hio, _hro, _dno = C.POINTER(PtHistoryOptions), C.POINTER(PtHistoryRoundOptions), C.POINTER(PtDenoiseOptions)
        L.pt_history_round_list.argtypes = [C.c_int, C.c_int, _ip, C.c_int, C.c_int]
        L.pt_ctx_history_round_list.argtypes = [C.c_void_p, C.c_int, C.c_int, _ip, C.c_int, C.c_int]
        L.pt_ctx_history_round_list_device.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int]
        L.pt_group_clear.argtypes = [C.c_void_p]
        L.pt_group_history_capture_ex.argtypes = [C.c_void_p, C.c_float, C.c_uint32]
        L.pt_group_history_reproject_ex.argtypes = [C.c_void_p, _hio, C.c_uint32]
        L.pt_group_history_resolve.argtypes = [C.c_void_p, C.c_float, _fp]
        L.pt_group_history_denoise_ex.argtypes = [C.c_void_p, C.c_float, _dno, C.c_uint32, _fp]
        L.pt_group_history_round.argtypes = [C.c_void_p, C.c_int, C.c_int, _hro, _ip, _ip]
        L.pt_group_history_drop.argtypes = [C.c_void_p]
        L.pt_group_readback_history.argtypes = [C.c_void_p, _fp, _fp]
        L.pt_group_readback_history_variance.argtypes = [C.c_void_p, _fp, _fp]
        L.pt_group_readback_history_extra.argtypes = [C.c_void_p, _fp]
        L.pt_group_device_bytes.argtypes = [C.c_void_p]
        L.pt_group_device_bytes.restype = C.c_int64
    _lib = L
    return L


def _check(rc: int) -> None:
    if rc != 0:
        raise PtError(lib().pt_last_error().decode(errors="replace"))


def _f(a: np.ndarray):
    assert a.dtype == np.float32 and a.flags.c_contiguous
    return a.ctypes.data_as(_fp)


def _i(a: np.ndarray):
    assert a.dtype == np.int32 and a.flags.c_contiguous
    return a.ctypes.data_as(_ip)


class Scene:
    """Host scene: `new Scene(file)` + main.cpp's initial camera state (include/pt_amd.h: pt_scene_load)."""

    def __init__(self, path: str, res: Optional[Tuple[int, int]] = None):
        self._h = C.c_void_p()
        w, h = res if res else (0, 0)
        _check(lib().pt_scene_load(os.fsencode(path), int(w), int(h), C.byref(self._h)))
        self.desc = PtSceneDesc()
        _check(lib().pt_scene_desc(self._h, C.byref(self.desc)))

    def __del__(self):
        h = getattr(self, "_h", None)
        if h is not None and h.value and _lib is not None:
            _lib.pt_scene_free(h)
            self._h = C.c_void_p()

    @property
    def resolution(self) -> Tuple[int, int]:
        return self.desc.camera.resolution[0], self.desc.camera.resolution[1]

    @property
    def trace_depth(self) -> int:
        return self.desc.trace_depth

    @trace_depth.setter
    def trace_depth(self, d: int) -> None:
        self.desc.trace_depth = int(d)

    @property
    def iterations(self) -> int:
        return lib().pt_scene_iterations(self._h)

    @property
    def image_name(self) -> str:
        return lib().pt_scene_image_name(self._h).decode()

    @property
    def camera(self) -> PtCamera:
        """A copy of the scene's camera as it stands (pt_scene_camera): what Renderer.set_camera takes."""
        cam = PtCamera()
        _check(lib().pt_scene_camera(self._h, C.byref(cam)))
        return cam

    def orbit(self, dphi: float, dtheta: float, dzoom: float) -> PtCamera:
        """A mouse drag of the reference's viewer (pt_scene_orbit); `desc.camera` follows.  Returns the new camera."""
        _check(lib().pt_scene_orbit(self._h, C.c_float(dphi), C.c_float(dtheta), C.c_float(dzoom)))
        cam = self.camera
        self.desc.camera = cam
        return cam

    @property
    def orbit_state(self) -> Tuple[float, float, float]:
        """(phi, theta, zoom) of main.cpp:63-71 as float32 values."""
        v = [C.c_float(0) for _ in range(3)]
        _check(lib().pt_scene_orbit_state(self._h, *(C.byref(x) for x in v)))
        return tuple(float(x.value) for x in v)

    def geoms(self):
        return [self.desc.geoms[i] for i in range(self.desc.num_geoms)]

    def geom_trs(self, geom: int) -> np.ndarray:
        """The TRANS / ROTAT / SCALE of the OBJECT geom `geom` came from, float32 [9] (pt_scene_geom_trs)."""
        trs = np.empty(9, np.float32)
        _check(lib().pt_scene_geom_trs(self._h, int(geom), _f(trs)))
        return trs

    def set_geom_trs(self, geom: int, trs: Sequence[float]) -> None:
        """Moves an object as the loader would have placed it (pt_scene_set_geom_trs); `desc` follows.  Renderer.set_geoms(scene)
        hands the moved geoms to a live renderer."""
        t = np.ascontiguousarray(trs, np.float32).reshape(-1)
        if t.size != 9:
            raise PtError(f"set_geom_trs: {t.size} values, 9 expected")
        _check(lib().pt_scene_set_geom_trs(self._h, int(geom), _f(t)))
        _check(lib().pt_scene_desc(self._h, C.byref(self.desc)))

    def materials(self):
        return [self.desc.materials[i] for i in range(self.desc.num_materials)]

    def material(self, m: int) -> PtMaterial:
        """Material `m` as the scene holds it, a copy (pt_scene_material)."""
        out = PtMaterial()
        _check(lib().pt_scene_material(self._h, int(m), C.byref(out)))
        return out

    def set_material(self, m: int, material: PtMaterial) -> None:
        """A new material in the place of material `m` (pt_scene_set_material); `desc` follows.  Renderer.set_materials(scene) hands
        the edited materials to a live renderer."""
        _check(lib().pt_scene_set_material(self._h, int(m), C.byref(material)))
        _check(lib().pt_scene_desc(self._h, C.byref(self.desc)))

    def grid(self, forced: bool = False):
        """The uniform grid of the cost model's resolution over the reference's leaf boxes, without the camera (pt_build_grid):
        (info, cell_start, records), or None when the scene is no grid candidate.  A renderer builds its grids the same way
        over its traversal boxes (tightened sphere leaves), so they need not equal this one byte for byte."""
        info = PtGridInfo()
        rc = lib().pt_build_grid(self.desc.geoms, self.desc.num_geoms, int(forced), C.byref(info), None, None)
        if rc < 0:
            raise PtError(lib().pt_last_error().decode(errors="replace"))
        if rc == 0:
            return None
        start = (C.c_uint32 * (info.num_cells + 1))()
        recs = (PtGridRecord * info.num_records)()
        lib().pt_build_grid(self.desc.geoms, self.desc.num_geoms, int(forced), C.byref(info), start, recs)
        return info, np.frombuffer(start, np.uint32).copy(), recs

    def traversal_boxes(self):
        """(boxes [num_geoms, 6], tightened count): the leaf boxes the traversal structures of a LARGE scene test
        (pt_traversal_boxes; sphere leaves tightened to the ellipsoid's box for ray origins in the scene or at the camera)."""
        boxes = np.zeros((self.desc.num_geoms, 6), np.float32)
        cam = np.asarray(list(self.desc.camera.position), np.float32)
        rc = lib().pt_traversal_boxes(self.desc.geoms, self.desc.num_geoms, _f(cam), _f(boxes))
        if rc < 0:
            raise PtError(lib().pt_last_error().decode(errors="replace"))
        return boxes, rc

    def bvh(self):
        n = lib().pt_build_bvh(self.desc.geoms, self.desc.num_geoms, None, 0)
        arr = (PtBVHNode * n)()
        lib().pt_build_bvh(self.desc.geoms, self.desc.num_geoms, arr, n)
        return arr


def selfcheck_ieee(kind: int, first: int, count: int, seed: int = 0, arith: str = "exact") -> int:
    """Mismatches between the guarded IEEE sqrt / reciprocal / quotient sequences and the compiler's expansions on the GPU
    (pt_selfcheck_ieee)."""
    n = C.c_uint64(0)
    _check(lib().pt_selfcheck_ieee(ARITH[arith], kind, first, count, seed, C.byref(n)))
    return int(n.value)


FAST_MATH_KINDS = ("rcp", "sqrt", "rsq", "sin_rev", "cos_rev", "sin_lobe", "cos_lobe", "sin_rev_ulp", "cos_rev_ulp")


def selfcheck_fast_math(kind, first: int, count: int, arith: str = "fast") -> float:
    """The largest error of one of a mode's scalar primitives against double precision on the GPU over `count` operands from `first`
    (pt_selfcheck_fast_math; kind: a name of FAST_MATH_KINDS or its number): ulp for rcp / sqrt / rsq / *_ulp, absolute otherwise."""
    k = FAST_MATH_KINDS.index(kind) if isinstance(kind, str) else int(kind)
    e = C.c_double(0.0)
    _check(lib().pt_selfcheck_fast_math(ARITH[arith], k, int(first), int(count), C.byref(e)))
    return float(e.value)


def selfcheck_camera_math(kind: int, count: int, seed: int = 0) -> int:
    """Operand sets on which a function of csrc/pt_camera_tables.h gives other bits on the GPU than on the host
    (pt_selfcheck_camera_math: kind 0 sqrt, 1 a / b, 2 nextafterf of (float)double, 3 center_half_box, 4 sphere_tight_box, 5 cell_range)."""
    n = C.c_uint64(0)
    _check(lib().pt_selfcheck_camera_math(int(kind), int(count), int(seed), C.byref(n)))
    return int(n.value)


def camera_tables_host(scene: "Scene", cam: PtCamera, debug_flags: int = 0, center_half: bool = False):
    """The host rebuild of the camera-dependent scene tables against a fresh build (pt_camera_tables_host, no GPU):
    (grid resolution at `cam` or (0, 0, 0), tightened leaves at `cam`, bit mask of the tables that differ; it must be 0)."""
    res = (C.c_int32 * 3)()
    tight, differing = C.c_int32(-1), C.c_int32(-1)
    _check(lib().pt_camera_tables_host(C.byref(scene.desc), C.byref(cam), int(debug_flags), int(bool(center_half)), res,
                                       C.byref(tight), C.byref(differing)))
    return tuple(res), int(tight.value), int(differing.value)


def camera_grid(nodes: np.ndarray, geom_types: np.ndarray, root_min, root_max, res, center_half: bool = False, coord_mag: float = 0.0,
                device: bool = False, caps: Optional[Tuple[int, int]] = None):
    """The grid of the camera-dependent tables over caller-supplied nodes (a TABLE_NODE array): pt_camera_grid_host, or with `device`
    pt_stage_camera_grid (the kernels of csrc/pt_camera_tables.hip; needs the default renderer).  Returns (PtCameraGridResult, start,
    items, items_b): uint32 words, the records as [refs, 8] words, None where the status is not 0 (and items_b without center_half).
    caps: the capacities (words, records) to allocate; None asks the function for the sizes first."""
    fn = lib().pt_stage_camera_grid if device else lib().pt_camera_grid_host
    assert nodes.dtype == TABLE_NODE and nodes.flags.c_contiguous
    types = np.ascontiguousarray(geom_types, np.int32)
    lo, hi = np.ascontiguousarray(root_min, np.float32), np.ascontiguousarray(root_max, np.float32)
    r = np.ascontiguousarray(res, np.int32)
    out = PtCameraGridResult()

    def call(start, items, items_b, words, records):
        ptr = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
        _check(fn(nodes.ctypes.data_as(C.c_void_p), int(nodes.size), _i(types), int(types.size), _f(lo), _f(hi), float(coord_mag), _i(r),
                  int(bool(center_half)), C.byref(out), ptr(start), words, ptr(items), ptr(items_b), records))

    if caps is None:
        call(None, None, None, 0, 0)
        if out.status != 0:
            return out, None, None, None
        caps = (int(out.num_cells) + 1 + 2 * int(out.guard), int(out.refs))
    start, items = np.zeros(max(caps[0], 1), np.uint32), np.zeros((max(caps[1], 1), 8), np.uint32)
    items_b = np.zeros_like(items) if center_half else None
    call(start, items, items_b, start.size, items.shape[0])
    if out.status != 0:
        return out, None, None, None
    words, refs = int(out.num_cells) + 1 + 2 * int(out.guard), int(out.refs)
    return out, start[:words], items[:refs], (items_b[:refs] if center_half else None)


def build_transform(trs: Sequence[float]):
    t = np.asarray(trs, np.float32).copy()
    m, i, it = (np.zeros(16, np.float32) for _ in range(3))
    lib().pt_build_transform(_f(t), _f(m), _f(i), _f(it))
    return m, i, it


def make_options(device: int = 0, pixel_begin: int = 0, pixel_count: int = 0, iters_per_batch: int = 0,
                 num_queues: int = 0, blocks_per_cu: int = 0, time_kernels: bool = False, legacy_traversal: bool = False,
                 debug_flags: int = 0, unfused_primary: bool = False, unfused_bounces: bool = False,
                 stripe_pixels: int = 0, stripe_stride: int = 0, arith="exact", aa_jitter: bool = False,
                 lds_table_kb: int = 0, primary_pieces: int = 0, paths_pieces: int = 0, paths_min_piece: int = 0, primary_share: int = 0,
                 convergence: int = 0) -> PtOptions:
    opt = PtOptions()
    opt.device = device
    opt.pixel_begin = pixel_begin
    opt.pixel_count = pixel_count
    opt.iters_per_batch = iters_per_batch
    opt.num_queues = num_queues
    opt.blocks_per_cu = blocks_per_cu
    opt.time_kernels = 1 if time_kernels else 0
    opt.legacy_traversal = 1 if legacy_traversal else 0
    opt.debug_flags = int(debug_flags)
    opt.unfused_primary = 1 if unfused_primary else 0
    opt.unfused_bounces = 1 if unfused_bounces else 0
    opt.stripe_pixels = int(stripe_pixels)
    opt.stripe_stride = int(stripe_stride)
    opt.arith = ARITH[arith] if isinstance(arith, str) else int(arith)
    opt.aa_jitter = 1 if aa_jitter else 0
    opt.convergence = int(convergence)  # 0 off, N > 0 reference frame captured at iteration N, -1 supplied (set_reference)
    opt.lds_table_kb = int(lds_table_kb)
    # PT_PRIMARY_PIECES (include/pt_amd.h): primary_share (0 automatic, 1 a trace per iteration, up to 64) rides in bits 16-22
    pp = int(primary_pieces)  # negative: passed on as it is (pt_init clamps it to one piece)
    opt.primary_pieces = pp if pp < 0 else min(pp, 0x7fff) | max(0, min(int(primary_share), 64)) << 16
    opt.paths_pieces = int(paths_pieces)
    opt.paths_min_piece = int(paths_min_piece)
    return opt


def split_features(planes: np.ndarray) -> dict:
    """The feature SUM planes [PT_FEATURE_PLANES, n, 4] (pt_readback_features) by name: normal [n, 3], depth [n] (sum of t),
    albedo [n, 3], hits [n], position [n, 3], object_id [n] int32 (1 + geom index of the last iteration, 0 = miss)."""
    p = planes.reshape(FEATURE_PLANES, -1, 4)
    return dict(normal=np.ascontiguousarray(p[0, :, :3]), depth=np.ascontiguousarray(p[0, :, 3]),
                albedo=np.ascontiguousarray(p[1, :, :3]), hits=np.ascontiguousarray(p[1, :, 3]),
                position=np.ascontiguousarray(p[2, :, :3]), object_id=np.ascontiguousarray(p[2, :, 3]).view(np.int32))


def denoise_options(levels: int = 0, sigma_color: float = 0.0, sigma_normal: float = 0.0, sigma_position: float = 0.0,
                    keep_albedo: bool = False) -> PtDenoiseOptions:
    """PtDenoiseOptions; 0 = the default of a field, a negative sigma switches its term off."""
    return PtDenoiseOptions(int(levels), float(sigma_color), float(sigma_normal), float(sigma_position), 1 if keep_albedo else 0)


def _denoise_arrays(rgb_sum, planes, w: int, rows: int, noise_planes=None, counts=None):
    """The flat, checked arrays of a filter call, those of the guided forms only where given, and the output: (s, p[, z][, c], out)."""
    s = np.ascontiguousarray(rgb_sum, np.float32).reshape(-1)
    p = np.ascontiguousarray(planes, np.float32).reshape(-1)
    if s.size != 3 * w * rows or p.size != 4 * FEATURE_PLANES * w * rows:
        raise PtError(f"denoise: {s.size} image and {p.size} plane floats for a frame of {w}x{rows}")
    arrays = [s, p]
    if noise_planes is not None:
        arrays.append(np.ascontiguousarray(noise_planes, np.float32).reshape(-1))
        if arrays[-1].size != 4 * NOISE_PLANES * w * rows:
            raise PtError(f"denoise_guided: {arrays[-1].size} noise plane floats for a frame of {w}x{rows}")
    if counts is not None:
        arrays.append(np.ascontiguousarray(counts, np.int32).reshape(-1))
        if arrays[-1].size != 2 * w * rows:
            raise PtError(f"denoise_adaptive: {arrays[-1].size} counts for a frame of {w}x{rows}")
    return (*arrays, np.empty((w * rows, 3), np.float32))


def _filter(fn, out: np.ndarray, *args, **opts) -> np.ndarray:
    """fn(*args, the options, out) -> out: what a denoise* wrapper does once it has its arrays."""
    opt = denoise_options(**opts)
    _check(fn(*args, C.byref(opt), _f(out)))
    return out


def denoise_host(rgb_sum: np.ndarray, planes: np.ndarray, w: int, rows: int, samples: float, **opts) -> np.ndarray:
    """The edge-avoiding filter on the host (pt_denoise_host; no GPU): SUM image [w*rows, 3] and feature SUM planes
    [PT_FEATURE_PLANES, w*rows, 4] in, averaged radiance [w*rows, 3] out.  The device result equals it bit for bit."""
    s, p, out = _denoise_arrays(rgb_sum, planes, w, rows)
    return _filter(lib().pt_denoise_host, out, int(w), int(rows), _f(s), _f(p), C.c_float(samples), **opts)


HISTORY_KEPT_PLANES = 3  # PT_HISTORY_KEPT_PLANES


def history_options(cap: float = 0.0, min_normal_dot: float = 0.0, plane_tol: float = 0.0, keep_view_dependent: bool = False) -> PtHistoryOptions:
    """PtHistoryOptions; 0 = the default of a field, a negative min_normal_dot / plane_tol switches its test off."""
    return PtHistoryOptions(float(cap), float(min_normal_dot), float(plane_tol), 1 if keep_view_dependent else 0)


def reject_geoms(scene: "Scene") -> np.ndarray:
    """reject_geom of pt_history_reproject for a scene: uint8 [num_geoms], 1 where the geom's material reflects."""
    geoms, mats = scene.geoms(), scene.materials()
    return np.array([1 if mats[g.materialid].hasReflective > 0 else 0 for g in geoms], np.uint8)


def history_capture_host(rgb_sum: np.ndarray, planes: np.ndarray, samples: float, current: Optional[np.ndarray] = None) -> np.ndarray:
    """pt_history_capture on the host (no GPU): SUM image [n, 3], feature SUM planes [PT_FEATURE_PLANES, n, 4] and the current plane
    [n, 4] (None: absent) in, the kept planes [PT_HISTORY_KEPT_PLANES, n, 4] out."""
    s = np.ascontiguousarray(rgb_sum, np.float32).reshape(-1)
    p = np.ascontiguousarray(planes, np.float32).reshape(-1)
    n = s.size // 3
    c = None if current is None else np.ascontiguousarray(current, np.float32).reshape(-1)
    if s.size != 3 * n or p.size != 4 * FEATURE_PLANES * n or (c is not None and c.size != 4 * n):
        raise PtError(f"history_capture_host: {s.size} image, {p.size} plane floats")
    out = np.empty((HISTORY_KEPT_PLANES, n, 4), np.float32)
    _check(lib().pt_history_capture_host(n, _f(s), _f(p), None if c is None else _f(c), C.c_float(samples), _f(out)))
    return out


def _history_reproject(call, kept_cam: PtCamera, kept: np.ndarray, planes: np.ndarray, reject: np.ndarray, w: int, rows: int, row0: int, **opts):
    k = np.ascontiguousarray(kept, np.float32).reshape(-1)
    p = np.ascontiguousarray(planes, np.float32).reshape(-1)
    r = np.ascontiguousarray(reject, np.uint8).reshape(-1)
    if k.size != 4 * HISTORY_KEPT_PLANES * w * rows or p.size != 4 * FEATURE_PLANES * w * rows:
        raise PtError(f"history_reproject: {k.size} kept and {p.size} plane floats for a tile of {w}x{rows}")
    out = np.empty((w * rows, 4), np.float32)
    opt = history_options(**opts)
    _check(call(int(w), int(rows), int(row0), C.byref(kept_cam), _f(k), _f(p), r.ctypes.data_as(C.POINTER(C.c_uint8)) if r.size else None, int(r.size),
                C.byref(opt), _f(out)))
    return out


def history_reproject_host(kept_cam: PtCamera, kept: np.ndarray, planes: np.ndarray, reject: np.ndarray, w: int, rows: int, row0: int = 0, **opts) -> np.ndarray:
    """pt_history_reproject on the host (no GPU): the kept camera and planes [PT_HISTORY_KEPT_PLANES, w*rows, 4], the CURRENT view's
    feature SUM planes and reject_geom (uint8 [num_geoms]) in, the current plane [w*rows, 4] out; options: history_options."""
    return _history_reproject(lib().pt_history_reproject_host, kept_cam, kept, planes, reject, w, rows, row0, **opts)


def stage_history_reproject(kept_cam: PtCamera, kept: np.ndarray, planes: np.ndarray, reject: np.ndarray, w: int, rows: int, row0: int = 0, **opts) -> np.ndarray:
    """history_reproject_host's arrays through the production kernel (pt_stage_history_reproject; a renderer must be live)."""
    return _history_reproject(lib().pt_stage_history_reproject, kept_cam, kept, planes, reject, w, rows, row0, **opts)


def history_blend_host(rgb_sum: np.ndarray, samples: float, current: Optional[np.ndarray] = None) -> np.ndarray:
    """pt_history_resolve's blend on the host (no GPU): SUM image [n, 3] and the current plane [n, 4] (None: absent) in, averaged
    radiance [n, 3] out."""
    s = np.ascontiguousarray(rgb_sum, np.float32).reshape(-1)
    n = s.size // 3
    c = None if current is None else np.ascontiguousarray(current, np.float32).reshape(-1)
    if s.size != 3 * n or (c is not None and c.size != 4 * n):
        raise PtError(f"history_blend_host: {s.size} image floats")
    out = np.empty((n, 3), np.float32)
    _check(lib().pt_history_blend_host(n, _f(s), C.c_float(samples), None if c is None else _f(c), _f(out)))
    return out


HISTORY_VARIANCE = 1  # PT_HISTORY_VARIANCE


def history_capture_variance_host(noise_planes: np.ndarray, groups: int, iters: int, samples: float, current: Optional[np.ndarray] = None,
                                  current_var: Optional[np.ndarray] = None) -> np.ndarray:
    """The variance side of pt_history_capture_ex on the host (no GPU): the fold's planes [PT_NOISE_PLANES, n, 4] with their counters
    M, T, and the planes C, VC [n, 4] (None: absent) in, VK [n, 4] out.  K is history_capture_host's."""
    z = np.ascontiguousarray(noise_planes, np.float32).reshape(-1)
    n = z.size // (4 * NOISE_PLANES)
    c = None if current is None else np.ascontiguousarray(current, np.float32).reshape(-1)
    v = None if current_var is None else np.ascontiguousarray(current_var, np.float32).reshape(-1)
    if z.size != 4 * NOISE_PLANES * n or any(a is not None and a.size != 4 * n for a in (c, v)):
        raise PtError(f"history_capture_variance_host: {z.size} noise plane floats")
    out = np.empty((n, 4), np.float32)
    _check(lib().pt_history_capture_variance_host(n, _f(z), int(groups), int(iters), C.c_float(samples), None if c is None else _f(c),
                                                  None if v is None else _f(v), _f(out)))
    return out


def _history_reproject_variance(call, kept_cam: PtCamera, kept, planes, reject, kept_var, w: int, rows: int, row0: int, **opts):
    k = np.ascontiguousarray(kept, np.float32).reshape(-1)
    p = np.ascontiguousarray(planes, np.float32).reshape(-1)
    r = np.ascontiguousarray(reject, np.uint8).reshape(-1)
    vk = np.ascontiguousarray(kept_var, np.float32).reshape(-1)
    if k.size != 4 * HISTORY_KEPT_PLANES * w * rows or p.size != 4 * FEATURE_PLANES * w * rows or vk.size != 4 * w * rows:
        raise PtError(f"history_reproject_variance: {k.size} kept, {p.size} plane and {vk.size} variance floats for a tile of {w}x{rows}")
    out, vout = np.empty((w * rows, 4), np.float32), np.empty((w * rows, 4), np.float32)
    opt = history_options(**opts)
    _check(call(int(w), int(rows), int(row0), C.byref(kept_cam), _f(k), _f(p), r.ctypes.data_as(C.POINTER(C.c_uint8)) if r.size else None, int(r.size),
                C.byref(opt), _f(vk), _f(out), _f(vout)))
    return out, vout


def history_reproject_variance_host(kept_cam: PtCamera, kept, planes, reject, kept_var, w: int, rows: int, row0: int = 0, **opts):
    """pt_history_reproject_ex with PT_HISTORY_VARIANCE on the host (no GPU): history_reproject_host's arrays and VK [w*rows, 4] in,
    (C, VC), [w*rows, 4] each, out."""
    return _history_reproject_variance(lib().pt_history_reproject_variance_host, kept_cam, kept, planes, reject, kept_var, w, rows, row0, **opts)


def stage_history_reproject_variance(kept_cam: PtCamera, kept, planes, reject, kept_var, w: int, rows: int, row0: int = 0, **opts):
    """history_reproject_variance_host's arrays through the production kernel (pt_stage_history_reproject_variance; a renderer must be live)."""
    return _history_reproject_variance(lib().pt_stage_history_reproject_variance, kept_cam, kept, planes, reject, kept_var, w, rows, row0, **opts)


def _history_denoise(call, rgb_sum, planes, noise_planes, w: int, rows: int, groups: int, iters: int, samples: float, current, current_var, **opts):
    s, p, z, out = _denoise_arrays(rgb_sum, planes, w, rows, noise_planes)
    c = None if current is None else np.ascontiguousarray(current, np.float32).reshape(-1)
    v = None if current_var is None else np.ascontiguousarray(current_var, np.float32).reshape(-1)
    if any(a is not None and a.size != 4 * w * rows for a in (c, v)):
        raise PtError(f"history_denoise: the current plane or its variance is not [{w * rows}, 4]")
    return _filter(call, out, int(w), int(rows), _f(s), _f(p), _f(z), int(groups), int(iters), C.c_float(samples), None if c is None else _f(c),
                   None if v is None else _f(v), **opts)


def history_denoise_host(rgb_sum, planes, noise_planes, w: int, rows: int, groups: int, iters: int, samples: float, current=None, current_var=None,
                         **opts) -> np.ndarray:
    """pt_history_denoise on the host (no GPU): denoise_guided_host's arrays, samples, and the planes C, VC [w*rows, 4] (None: absent)."""
    return _history_denoise(lib().pt_history_denoise_host, rgb_sum, planes, noise_planes, w, rows, groups, iters, samples, current, current_var, **opts)


def stage_history_denoise(rgb_sum, planes, noise_planes, w: int, rows: int, groups: int, iters: int, samples: float, current=None, current_var=None,
                          **opts) -> np.ndarray:
    """history_denoise_host's arguments through the filter's kernels (pt_stage_history_denoise; a renderer must be live)."""
    return _history_denoise(lib().pt_stage_history_denoise, rgb_sum, planes, noise_planes, w, rows, groups, iters, samples, current, current_var, **opts)


def _history_noise(call, noise_planes, groups: int, iters: int, samples: float, current, current_var):
    z = np.ascontiguousarray(noise_planes, np.float32).reshape(-1)
    n = z.size // (4 * NOISE_PLANES)
    c = None if current is None else np.ascontiguousarray(current, np.float32).reshape(-1)
    v = None if current_var is None else np.ascontiguousarray(current_var, np.float32).reshape(-1)
    if z.size != 4 * NOISE_PLANES * n or any(a is not None and a.size != 4 * n for a in (c, v)):
        raise PtError(f"history_noise: {z.size} noise plane floats")
    w, sse = np.empty(n, np.float32), C.c_double(-1.0)
    _check(call(n, _f(z), int(groups), int(iters), C.c_float(samples), None if c is None else _f(c), None if v is None else _f(v), _f(w), C.byref(sse)))
    return w, float(sse.value)


def history_noise_host(noise_planes: np.ndarray, groups: int, iters: int, samples: float, current: Optional[np.ndarray] = None,
                       current_var: Optional[np.ndarray] = None):
    """pt_history_noise on the host (no GPU): the fold's planes [PT_NOISE_PLANES, n, 4] with their counters M, T, and the planes C, VC
    [n, 4] (None: absent) in; (W float32 [n], SSE_blend added in pixel order) out."""
    return _history_noise(lib().pt_history_noise_host, noise_planes, groups, iters, samples, current, current_var)


def stage_history_noise(noise_planes: np.ndarray, groups: int, iters: int, samples: float, current: Optional[np.ndarray] = None,
                        current_var: Optional[np.ndarray] = None):
    """history_noise_host's arguments through the production kernels (pt_stage_history_noise; a renderer must be live): (W, the
    device's SSE_blend)."""
    return _history_noise(lib().pt_stage_history_noise, noise_planes, groups, iters, samples, current, current_var)


# ---- threshold rounds over the blend: the history steps with per-pixel counts (include/pt_amd.h: pt_history_round_threshold) ----
def _blend_arrays(who: str, n: int, counts, current, current_var):
    """counts int32 [n, 2] flat, and C, VC [n, 4] as ctypes arguments (None: absent)."""
    c = np.ascontiguousarray(counts, np.int32).reshape(-1)
    cur = None if current is None else np.ascontiguousarray(current, np.float32).reshape(-1)
    var = None if current_var is None else np.ascontiguousarray(current_var, np.float32).reshape(-1)
    if c.size != 2 * n or any(a is not None and a.size != 4 * n for a in (cur, var)):
        raise PtError(f"{who}: {c.size} counts, or a current plane or variance that is not [{n}, 4]")
    return c, cur, var, None if cur is None else _f(cur), None if var is None else _f(var)


def _history_noise_adaptive(call, host: bool, noise_planes, counts, current, current_var):
    z = np.ascontiguousarray(noise_planes, np.float32).reshape(-1)
    n = z.size // (4 * NOISE_PLANES)
    if z.size != 4 * NOISE_PLANES * n:
        raise PtError(f"history_noise_adaptive: {z.size} noise plane floats")
    c, cur, var, pc, pv = _blend_arrays("history_noise_adaptive", n, counts, current, current_var)
    w, ne, vb, sse = np.empty(n, np.float32), np.empty(n, np.float32), np.empty((n, 4), np.float32), C.c_double(-1.0)
    if host:
        _check(call(n, _f(z), _i(c), pc, pv, _f(w), _f(ne), _f(vb), C.byref(sse)))
        return w, ne, vb, float(sse.value)
    _check(call(n, _f(z), _i(c), pc, pv, _f(w), _f(ne), C.byref(sse)))
    return w, ne, float(sse.value)


def history_noise_adaptive_host(noise_planes, counts, current=None, current_var=None):
    """Pass A of a threshold round over the blend on the host (pt_history_noise_adaptive_host; no GPU): the fold's planes
    [PT_NOISE_PLANES, n, 4], counts int32 [n, 2] (T_p, M_p) and the planes C, VC [n, 4] (None: absent) in; (W [n], NE [n], the
    per-channel vb [n, 4], SSE_blend added in pixel order) out."""
    return _history_noise_adaptive(lib().pt_history_noise_adaptive_host, True, noise_planes, counts, current, current_var)


def stage_history_noise_adaptive(noise_planes, counts, current=None, current_var=None):
    """history_noise_adaptive_host's arguments through the production kernels (pt_stage_history_noise_adaptive; a renderer must be
    live): (W, NE, the device's SSE_blend)."""
    return _history_noise_adaptive(lib().pt_stage_history_noise_adaptive, False, noise_planes, counts, current, current_var)


def _select_threshold_blend(call, noise_planes, counts, w: int, rows: int, threshold: float, cap: int, current, current_var):
    z, c, out = _select_arrays(noise_planes, counts, w, rows, cap)
    _, cur, var, pc, pv = _blend_arrays("history_select_threshold_blend", int(w) * int(rows), counts, current, current_var)
    above, m = C.c_int32(-1), C.c_int32(-1)
    _check(call(int(w), int(rows), _f(z), _i(c), pc, pv, C.c_float(threshold), int(cap), _i(out), C.byref(above), C.byref(m)))
    if not 0 <= m.value <= int(cap):
        raise PtError(f"history_select_threshold_blend: a list of {m.value} (cap {cap})")
    return out, int(above.value), int(m.value)


def history_select_threshold_blend_host(noise_planes, counts, w: int, rows: int, threshold: float, cap: int, current=None, current_var=None):
    """The selection of a threshold round over the blend on the host (pt_history_select_threshold_blend_host; no GPU):
    adaptive_select_threshold_host's arguments and C, VC -> (the list's first m entries, above, m)."""
    out, above, m = _select_threshold_blend(lib().pt_history_select_threshold_blend_host, noise_planes, counts, w, rows, threshold, cap, current, current_var)
    return out[:m].copy(), above, m


def stage_history_select_threshold_blend(noise_planes, counts, w: int, rows: int, threshold: float, cap: int, current=None, current_var=None):
    """The same through passes A and B and the round's selection launches (pt_stage_history_select_threshold_blend; needs a Renderer);
    the entries behind the list's length must still be -1."""
    out, above, m = _select_threshold_blend(lib().pt_stage_history_select_threshold_blend, noise_planes, counts, w, rows, threshold, cap, current, current_var)
    if (out[m:] != -1).any():
        raise PtError(f"history_select_threshold_blend: a list of {m} (cap {cap}) with entries written behind it")
    return out[:m].copy(), above, m


def history_blend_adaptive_host(rgb_sum, counts, current=None) -> np.ndarray:
    """pt_history_resolve_adaptive's blend on the host (no GPU): SUM image [n, 3], counts int32 [n, 2] and C [n, 4] (None: absent)
    in, averaged radiance [n, 3] out."""
    s = np.ascontiguousarray(rgb_sum, np.float32).reshape(-1)
    n = s.size // 3
    c, cur, _, pc, _ = _blend_arrays("history_blend_adaptive_host", n, counts, current, None)
    out = np.empty((n, 3), np.float32)
    _check(lib().pt_history_blend_adaptive_host(n, _f(s), _i(c), pc, _f(out)))
    return out


def _history_capture_adaptive(call, stage: bool, rgb_sum, planes, noise_planes, counts, current, current_var):
    s = np.ascontiguousarray(rgb_sum, np.float32).reshape(-1)
    p = np.ascontiguousarray(planes, np.float32).reshape(-1)
    z = np.ascontiguousarray(noise_planes, np.float32).reshape(-1)
    n = s.size // 3
    if s.size != 3 * n or p.size != 4 * FEATURE_PLANES * n or z.size != 4 * NOISE_PLANES * n:
        raise PtError(f"history_capture_adaptive: {s.size} image, {p.size} plane and {z.size} noise plane floats")
    c, cur, var, pc, pv = _blend_arrays("history_capture_adaptive", n, counts, current, current_var)
    kept, kvar = np.empty((HISTORY_KEPT_PLANES, n, 4), np.float32), np.empty((n, 4), np.float32)
    if not stage:
        _check(call(n, _f(s), _f(p), _f(z), _i(c), pc, pv, _f(kept), _f(kvar)))
        return kept, kvar
    avg = np.empty((n, 3), np.float32)
    _check(call(n, _f(s), _f(p), _f(z), _i(c), pc, pv, _f(kept), _f(kvar), _f(avg)))
    return kept, kvar, avg


def history_capture_adaptive_host(rgb_sum, planes, noise_planes, counts, current=None, current_var=None):
    """pt_history_capture_adaptive on the host (no GPU): SUM image [n, 3], feature SUM planes, the fold's planes, counts int32 [n, 2]
    and C, VC (None: absent) in; (K [PT_HISTORY_KEPT_PLANES, n, 4], VK [n, 4]) out."""
    return _history_capture_adaptive(lib().pt_history_capture_adaptive_host, False, rgb_sum, planes, noise_planes, counts, current, current_var)


def stage_history_capture_adaptive(rgb_sum, planes, noise_planes, counts, current=None, current_var=None):
    """The same through the capture's and the blend's kernels (pt_stage_history_capture_adaptive; needs a Renderer): (K, VK, the blend [n, 3])."""
    return _history_capture_adaptive(lib().pt_stage_history_capture_adaptive, True, rgb_sum, planes, noise_planes, counts, current, current_var)


def _history_denoise_adaptive(call, rgb_sum, planes, noise_planes, counts, w: int, rows: int, current, current_var, **opts):
    s, p, z, c, out = _denoise_arrays(rgb_sum, planes, w, rows, noise_planes, counts)
    _, cur, var, pc, pv = _blend_arrays("history_denoise_adaptive", int(w) * int(rows), counts, current, current_var)
    return _filter(call, out, int(w), int(rows), _f(s), _f(p), _f(z), _i(c), pc, pv, **opts)


def history_denoise_adaptive_host(rgb_sum, planes, noise_planes, counts, w: int, rows: int, current=None, current_var=None, **opts) -> np.ndarray:
    """pt_history_denoise_adaptive on the host (no GPU): denoise_adaptive_host's arrays and the planes C, VC [w*rows, 4] (None: absent)."""
    return _history_denoise_adaptive(lib().pt_history_denoise_adaptive_host, rgb_sum, planes, noise_planes, counts, w, rows, current, current_var, **opts)


def stage_history_denoise_adaptive(rgb_sum, planes, noise_planes, counts, w: int, rows: int, current=None, current_var=None, **opts) -> np.ndarray:
    """history_denoise_adaptive_host's arguments through the filter's kernels (pt_stage_history_denoise_adaptive; needs a Renderer)."""
    return _history_denoise_adaptive(lib().pt_stage_history_denoise_adaptive, rgb_sum, planes, noise_planes, counts, w, rows, current, current_var, **opts)


def history_denoise_adaptive_variance_host(rgb_sum, planes, noise_planes, counts, w: int, rows: int, current=None, current_var=None, **opts):
    """The two variances that filter's levels start from (pt_history_denoise_adaptive_variance_host): (var_raw, var_0), [w*rows] each."""
    s, p, z, c, _ = _denoise_arrays(rgb_sum, planes, w, rows, noise_planes, counts)
    _, cur, var, pc, pv = _blend_arrays("history_denoise_adaptive", int(w) * int(rows), counts, current, current_var)
    raw, pre = np.empty(w * rows, np.float32), np.empty(w * rows, np.float32)
    opt = denoise_options(**opts)
    _check(lib().pt_history_denoise_adaptive_variance_host(int(w), int(rows), _f(s), _f(p), _f(z), _i(c), pc, pv, C.byref(opt), _f(raw), _f(pre)))
    return raw, pre


HISTORY_MOMENTS = 2  # PT_HISTORY_MOMENTS
HISTORY_MOMENTS_R_MAX = np.float32(0.3)  # PT_HISTORY_MOMENTS_R_MAX


def history_capture_moments_host(rgb_sum: np.ndarray, samples: float, current: Optional[np.ndarray] = None,
                                 current_var: Optional[np.ndarray] = None) -> np.ndarray:
    """The moments side of pt_history_capture_ex on the host (no GPU): the SUM image [n, 3] and the planes C, VC [n, 4] (None: absent)
    in, VK = {m2b.xyz, rb} [n, 4] out.  K is history_capture_host's."""
    s = np.ascontiguousarray(rgb_sum, np.float32).reshape(-1)
    n = s.size // 3
    c = None if current is None else np.ascontiguousarray(current, np.float32).reshape(-1)
    v = None if current_var is None else np.ascontiguousarray(current_var, np.float32).reshape(-1)
    if s.size != 3 * n or any(a is not None and a.size != 4 * n for a in (c, v)):
        raise PtError(f"history_capture_moments_host: {s.size} image floats")
    out = np.empty((n, 4), np.float32)
    _check(lib().pt_history_capture_moments_host(n, _f(s), C.c_float(samples), None if c is None else _f(c), None if v is None else _f(v), _f(out)))
    return out


def history_reproject_moments_host(kept_cam: PtCamera, kept, planes, reject, kept_var, w: int, rows: int, row0: int = 0, **opts):
    """pt_history_reproject_ex with PT_HISTORY_MOMENTS on the host (no GPU): history_reproject_host's arrays and VK [w*rows, 4] in,
    (C, VC), [w*rows, 4] each, out."""
    return _history_reproject_variance(lib().pt_history_reproject_moments_host, kept_cam, kept, planes, reject, kept_var, w, rows, row0, **opts)


def stage_history_reproject_moments(kept_cam: PtCamera, kept, planes, reject, kept_var, w: int, rows: int, row0: int = 0, **opts):
    """history_reproject_moments_host's arrays through the production kernel (pt_stage_history_reproject_moments; a renderer must be live)."""
    return _history_reproject_variance(lib().pt_stage_history_reproject_moments, kept_cam, kept, planes, reject, kept_var, w, rows, row0, **opts)


HISTORY_MOTION = 4  # PT_HISTORY_MOTION
HISTORY_MOTION_ROW = 24  # floats per geom of the motion table: D (3 x 4), Nm (3 x 3), 3 zeros


def _geom_array(geoms):
    """A ctypes array of PtGeom from a Scene, a ctypes array or a sequence of PtGeom; (array, count)."""
    if isinstance(geoms, Scene):
        return geoms.desc.geoms, geoms.desc.num_geoms
    seq = list(geoms)
    return (PtGeom * max(len(seq), 1))(*seq), len(seq)


def _material_array(materials):
    """A ctypes array of PtMaterial from a Scene, a ctypes array or a sequence of PtMaterial; (array, count)."""
    if isinstance(materials, Scene):
        return materials.desc.materials, materials.desc.num_materials
    seq = list(materials)
    return (PtMaterial * max(len(seq), 1))(*seq), len(seq)


def history_motion_host(kept, cur):
    """The motion table of PT_HISTORY_MOTION (pt_history_motion_host, no GPU): the kept and the current geoms (Scene, or sequences of
    PtGeom) in, (table float32 [n, 24], kind uint8 [n]) out: 0 still, 1 moved, 2 carries nothing."""
    ka, kn = _geom_array(kept)
    ca, cn = _geom_array(cur)
    if kn != cn or kn < 1:
        raise PtError(f"history_motion_host: {kn} kept and {cn} current geoms")
    table, kind = np.empty((kn, HISTORY_MOTION_ROW), np.float32), np.empty(kn, np.uint8)
    _check(lib().pt_history_motion_host(ka, ca, kn, _f(table), kind.ctypes.data_as(C.POINTER(C.c_uint8))))
    return table, kind


def _history_reproject_motion(call, kept_cam: PtCamera, kept, planes, reject, table, kind, w: int, rows: int, row0: int, flags: int, kept_var, **opts):
    k = np.ascontiguousarray(kept, np.float32).reshape(-1)
    p = np.ascontiguousarray(planes, np.float32).reshape(-1)
    r = np.ascontiguousarray(reject, np.uint8).reshape(-1)
    t = np.ascontiguousarray(table, np.float32).reshape(-1)
    kd = np.ascontiguousarray(kind, np.uint8).reshape(-1)
    vk = None if kept_var is None else np.ascontiguousarray(kept_var, np.float32).reshape(-1)
    if k.size != 4 * HISTORY_KEPT_PLANES * w * rows or p.size != 4 * FEATURE_PLANES * w * rows or (vk is not None and vk.size != 4 * w * rows):
        raise PtError(f"history_reproject_motion: {k.size} kept and {p.size} plane floats for a tile of {w}x{rows}")
    if t.size != HISTORY_MOTION_ROW * kd.size or kd.size != r.size:
        raise PtError(f"history_reproject_motion: {t.size} table floats and {kd.size} kinds for {r.size} geoms")
    out = np.empty((w * rows, 4), np.float32)
    vout = None if vk is None else np.empty((w * rows, 4), np.float32)
    opt = history_options(**opts)
    u8 = C.POINTER(C.c_uint8)
    _check(call(int(w), int(rows), int(row0), C.byref(kept_cam), _f(k), _f(p), r.ctypes.data_as(u8), int(r.size), C.byref(opt), None if vk is None else _f(vk),
                _f(t), kd.ctypes.data_as(u8), int(flags), _f(out), None if vout is None else _f(vout)))
    return out if vk is None else (out, vout)


def history_reproject_motion_host(kept_cam: PtCamera, kept, planes, reject, table, kind, w: int, rows: int, row0: int = 0, flags: int = HISTORY_MOTION,
                                  kept_var=None, **opts):
    """pt_history_reproject_ex with PT_HISTORY_MOTION on the host (no GPU): history_reproject_host's arrays, the motion table and the
    kinds (history_motion_host) in; C [w*rows, 4] out, or (C, VC) with HISTORY_VARIANCE or HISTORY_MOMENTS in `flags` and VK in kept_var."""
    return _history_reproject_motion(lib().pt_history_reproject_motion_host, kept_cam, kept, planes, reject, table, kind, w, rows, row0, flags, kept_var, **opts)


def stage_history_reproject_motion(kept_cam: PtCamera, kept, planes, reject, table, kind, w: int, rows: int, row0: int = 0, flags: int = HISTORY_MOTION,
                                   kept_var=None, **opts):
    """history_reproject_motion_host's arrays through the production kernel (pt_stage_history_reproject_motion; a renderer must be live)."""
    return _history_reproject_motion(lib().pt_stage_history_reproject_motion, kept_cam, kept, planes, reject, table, kind, w, rows, row0, flags, kept_var, **opts)


HISTORY_MATERIALS = 32  # PT_HISTORY_MATERIALS
HISTORY_RECOLOR_ROW = 4  # floats per geom of the recolour table


def history_recolor_host(kept, cur, geoms):
    """The recolour table of PT_HISTORY_MATERIALS (pt_history_recolor_host; no GPU): the kept and the current materials and the geoms
    (Scenes or sequences) in, (table float32 [n, 4], kind uint8 [n]) out, n the geoms: 0 unchanged, 1 recoloured, 2 carries nothing."""
    ka, kn = _material_array(kept)
    ca, cn = _material_array(cur)
    ga, gn = _geom_array(geoms)
    if kn != cn or kn < 1 or gn < 1:
        raise PtError(f"history_recolor_host: {kn} kept and {cn} current materials, {gn} geoms")
    table, kind = np.empty((gn, HISTORY_RECOLOR_ROW), np.float32), np.empty(gn, np.uint8)
    _check(lib().pt_history_recolor_host(ka, ca, kn, ga, gn, _f(table), kind.ctypes.data_as(C.POINTER(C.c_uint8))))
    return table, kind


def _history_reproject_materials(call, kept_cam: PtCamera, kept, planes, reject, recolor, rkind, w: int, rows: int, row0: int, flags: int, kept_var, table, kind, **opts):
    k = np.ascontiguousarray(kept, np.float32).reshape(-1)
    p = np.ascontiguousarray(planes, np.float32).reshape(-1)
    r = np.ascontiguousarray(reject, np.uint8).reshape(-1)
    rt = np.ascontiguousarray(recolor, np.float32).reshape(-1)
    rk = np.ascontiguousarray(rkind, np.uint8).reshape(-1)
    t = None if table is None else np.ascontiguousarray(table, np.float32).reshape(-1)
    kd = None if kind is None else np.ascontiguousarray(kind, np.uint8).reshape(-1)
    vk = None if kept_var is None else np.ascontiguousarray(kept_var, np.float32).reshape(-1)
    if k.size != 4 * HISTORY_KEPT_PLANES * w * rows or p.size != 4 * FEATURE_PLANES * w * rows or (vk is not None and vk.size != 4 * w * rows):
        raise PtError(f"history_reproject_materials: {k.size} kept and {p.size} plane floats for a tile of {w}x{rows}")
    if rt.size != HISTORY_RECOLOR_ROW * rk.size or rk.size != r.size or (t is not None and (kd is None or t.size != HISTORY_MOTION_ROW * r.size or kd.size != r.size)):
        raise PtError(f"history_reproject_materials: {rt.size} table floats and {rk.size} kinds for {r.size} geoms")
    out = np.empty((w * rows, 4), np.float32)
    vout = None if vk is None else np.empty((w * rows, 4), np.float32)
    opt = history_options(**opts)
    u8 = C.POINTER(C.c_uint8)
    _check(call(int(w), int(rows), int(row0), C.byref(kept_cam), _f(k), _f(p), r.ctypes.data_as(u8), int(r.size), C.byref(opt), None if vk is None else _f(vk),
                None if t is None else _f(t), None if kd is None else kd.ctypes.data_as(u8), _f(rt), rk.ctypes.data_as(u8), int(flags), _f(out),
                None if vout is None else _f(vout)))
    return out if vk is None else (out, vout)


def history_reproject_materials_host(kept_cam: PtCamera, kept, planes, reject, recolor, rkind, w: int, rows: int, row0: int = 0, flags: int = HISTORY_MATERIALS,
                                     kept_var=None, table=None, kind=None, **opts):
    """pt_history_reproject_ex with PT_HISTORY_MATERIALS on the host (no GPU): history_reproject_host's arrays, the recolour table and
    its kinds (history_recolor_host) in, with HISTORY_MOTION in `flags` also the motion table and kinds; C [w*rows, 4] out, or (C, VC)
    with HISTORY_VARIANCE or HISTORY_MOMENTS in `flags` and VK in kept_var."""
    return _history_reproject_materials(lib().pt_history_reproject_materials_host, kept_cam, kept, planes, reject, recolor, rkind, w, rows, row0, flags, kept_var,
                                        table, kind, **opts)


def stage_history_reproject_materials(kept_cam: PtCamera, kept, planes, reject, recolor, rkind, w: int, rows: int, row0: int = 0, flags: int = HISTORY_MATERIALS,
                                      kept_var=None, table=None, kind=None, **opts):
    """history_reproject_materials_host's arrays through the production kernel (pt_stage_history_reproject_materials; a renderer must be live)."""
    return _history_reproject_materials(lib().pt_stage_history_reproject_materials, kept_cam, kept, planes, reject, recolor, rkind, w, rows, row0, flags, kept_var,
                                        table, kind, **opts)


def _history_planes(current, current_var, w: int, rows: int):
    c = None if current is None else np.ascontiguousarray(current, np.float32).reshape(-1)
    v = None if current_var is None else np.ascontiguousarray(current_var, np.float32).reshape(-1)
    if any(a is not None and a.size != 4 * w * rows for a in (c, v)):
        raise PtError(f"history_denoise_moments: the current plane or its moments are not [{w * rows}, 4]")
    return c, v


def history_denoise_moments_host(rgb_sum, planes, w: int, rows: int, samples: float, current=None, current_var=None, stats: Optional[dict] = None,
                                 **opts) -> np.ndarray:
    """pt_history_denoise_ex with PT_HISTORY_MOMENTS on the host (no GPU): denoise_host's arrays, samples, and the planes C, VC
    [w*rows, 4] (None: absent).  stats (a dict) receives var_raw (after the spatial step) and mark (bool)."""
    s, p, out = _denoise_arrays(rgb_sum, planes, w, rows)
    c, v = _history_planes(current, current_var, w, rows)
    var_raw = np.empty(w * rows, np.float32) if stats is not None else None
    mark = np.empty(w * rows, np.uint8) if stats is not None else None
    opt = denoise_options(**opts)
    _check(lib().pt_history_denoise_moments_host(int(w), int(rows), _f(s), _f(p), C.c_float(samples), None if c is None else _f(c), None if v is None else _f(v),
                                                 C.byref(opt), _f(out), None if var_raw is None else _f(var_raw),
                                                 None if mark is None else mark.ctypes.data_as(C.POINTER(C.c_uint8))))
    if stats is not None:
        stats.update(var_raw=var_raw, mark=mark.astype(bool))
    return out


def stage_history_denoise_moments(rgb_sum, planes, w: int, rows: int, samples: float, current=None, current_var=None, **opts) -> np.ndarray:
    """history_denoise_moments_host's arguments through the filter's kernels (pt_stage_history_denoise_moments; a renderer must be live)."""
    s, p, out = _denoise_arrays(rgb_sum, planes, w, rows)
    c, v = _history_planes(current, current_var, w, rows)
    return _filter(lib().pt_stage_history_denoise_moments, out, int(w), int(rows), _f(s), _f(p), C.c_float(samples), None if c is None else _f(c),
                   None if v is None else _f(v), **opts)


# ---- the feedback: the filtered image fed back into the history (include/pt_amd.h: pt_history_denoise_feedback) ----
HISTORY_FEEDBACK = 16  # PT_HISTORY_FEEDBACK


def history_feedback_options(level: int = 0, variance: Optional[int] = None) -> PtHistoryFeedbackOptions:
    """PtHistoryFeedbackOptions from a level (0 = the default) and a variance RULE: 0 or 1, None = the default; the field's own
    encoding (0 = the default, -1 = rule 0) stays in here.  Any other number is passed on as it is, for the library to refuse."""
    return PtHistoryFeedbackOptions(int(level), 0 if variance is None else -1 if variance == 0 else int(variance))


def _history_reproject_feedback(call, kept_cam: PtCamera, kept, planes, reject, kept_var, kept_fb, w: int, rows: int, row0: int, table, kind, **opts):
    n = w * rows
    k = np.ascontiguousarray(kept, np.float32).reshape(-1)
    p = np.ascontiguousarray(planes, np.float32).reshape(-1)
    r = np.ascontiguousarray(reject, np.uint8).reshape(-1)
    vk = np.ascontiguousarray(kept_var, np.float32).reshape(-1)
    fk = np.ascontiguousarray(kept_fb, np.float32).reshape(-1)
    t = None if table is None else np.ascontiguousarray(table, np.float32).reshape(-1)
    kd = None if kind is None else np.ascontiguousarray(kind, np.uint8).reshape(-1)
    if k.size != 4 * HISTORY_KEPT_PLANES * n or p.size != 4 * FEATURE_PLANES * n or vk.size != 4 * n or fk.size != 4 * n:
        raise PtError(f"history_reproject_feedback: {k.size} kept, {p.size} plane, {vk.size} moment and {fk.size} feedback floats for a tile of {w}x{rows}")
    if t is not None and (kd is None or t.size != HISTORY_MOTION_ROW * kd.size or kd.size != r.size):
        raise PtError(f"history_reproject_feedback: {t.size} table floats for {r.size} geoms")
    out, vout, fout = (np.empty((n, 4), np.float32) for _ in range(3))
    opt = history_options(**opts)
    u8 = C.POINTER(C.c_uint8)
    _check(call(int(w), int(rows), int(row0), C.byref(kept_cam), _f(k), _f(p), r.ctypes.data_as(u8), int(r.size), C.byref(opt), _f(vk), _f(fk),
                None if t is None else _f(t), None if kd is None else kd.ctypes.data_as(u8), _f(out), _f(vout), _f(fout)))
    return out, vout, fout


def history_reproject_feedback_host(kept_cam: PtCamera, kept, planes, reject, kept_var, kept_fb, w: int, rows: int, row0: int = 0, table=None, kind=None,
                                    **opts):
    """pt_history_reproject_ex with PT_HISTORY_MOMENTS | PT_HISTORY_FEEDBACK on the host (no GPU): history_reproject_moments_host's
    arrays and FK [w*rows, 4] in, (C, VC, FC) out; table and kind (history_motion_host): the lookup with PT_HISTORY_MOTION as well."""
    return _history_reproject_feedback(lib().pt_history_reproject_feedback_host, kept_cam, kept, planes, reject, kept_var, kept_fb, w, rows, row0, table, kind,
                                       **opts)


def stage_history_reproject_feedback(kept_cam: PtCamera, kept, planes, reject, kept_var, kept_fb, w: int, rows: int, row0: int = 0, table=None, kind=None,
                                     **opts):
    """history_reproject_feedback_host's arrays through the production kernel (pt_stage_history_reproject_feedback; a renderer must be live)."""
    return _history_reproject_feedback(lib().pt_stage_history_reproject_feedback, kept_cam, kept, planes, reject, kept_var, kept_fb, w, rows, row0, table,
                                       kind, **opts)


def _history_denoise_feedback(call, host: bool, rgb_sum, planes, w: int, rows: int, samples: float, extra, current, current_var, current_fb, level: int,
                              variance: Optional[int], stats, **opts):
    s, p, out = _denoise_arrays(rgb_sum, planes, w, rows)
    c, v = _history_planes(current, current_var, w, rows)
    f, _ = _history_planes(current_fb, None, w, rows)
    e = None if extra is None else _extra(extra, w * rows)
    tap = np.empty((w * rows, 4), np.float32)
    opt, fb = denoise_options(**opts), history_feedback_options(level, variance)
    args = [int(w), int(rows), _f(s), _f(p), C.c_float(samples), None if e is None else _f(e), None if c is None else _f(c), None if v is None else _f(v),
            None if f is None else _f(f), C.byref(opt), C.byref(fb), _f(out), _f(tap)]
    if host:
        var_raw = np.empty(w * rows, np.float32) if stats is not None else None
        mark = np.empty(w * rows, np.uint8) if stats is not None else None
        args += [None if var_raw is None else _f(var_raw), None if mark is None else mark.ctypes.data_as(C.POINTER(C.c_uint8))]
    _check(call(*args))
    if host and stats is not None:
        stats.update(var_raw=var_raw, mark=mark.astype(bool))
    return out, tap


def history_denoise_feedback_host(rgb_sum, planes, w: int, rows: int, samples: float, extra=None, current=None, current_var=None, current_fb=None,
                                  level: int = 0, variance: Optional[int] = None, stats: Optional[dict] = None, **opts):
    """pt_history_denoise_feedback on the host (no GPU): history_denoise_moments_host's arrays, the extra plane E [w*rows] (None:
    absent) and FC [w*rows, 4] beside C and VC (None: absent) in; (the filtered image [w*rows, 3], the tap plane P [w*rows, 4]) out.
    stats (a dict) receives var_raw (after the spatial step) and mark (bool)."""
    return _history_denoise_feedback(lib().pt_history_denoise_feedback_host, True, rgb_sum, planes, w, rows, samples, extra, current, current_var, current_fb,
                                     level, variance, stats, **opts)


def stage_history_denoise_feedback(rgb_sum, planes, w: int, rows: int, samples: float, extra=None, current=None, current_var=None, current_fb=None,
                                   level: int = 0, variance: Optional[int] = None, **opts):
    """history_denoise_feedback_host's arguments through the filter's kernels (pt_stage_history_denoise_feedback; a renderer must be live)."""
    return _history_denoise_feedback(lib().pt_stage_history_denoise_feedback, False, rgb_sum, planes, w, rows, samples, extra, current, current_var,
                                     current_fb, level, variance, None, **opts)


# ---- the history probes: kept samples rendered again after a move (include/pt_amd.h: pt_history_probe_keep) ----
def history_probe_options(radius: int = 0, gain: float = 0.0) -> PtHistoryProbeOptions:
    """PtHistoryProbeOptions; 0 = the default of a field, radius -1 = 0."""
    return PtHistoryProbeOptions(int(radius), float(gain))


def history_probe_list_host(w: int, rows: int, phase: int) -> np.ndarray:
    """The tile pixels of the probes of a w x rows tile at `phase`, int32 [P], ascending (pt_history_probe_list_host; no GPU)."""
    count = C.c_int32(-1)
    _check(lib().pt_history_probe_list_host(int(w), int(rows), int(phase), None, C.byref(count)))
    lst = np.full(count.value, -1, np.int32)
    _check(lib().pt_history_probe_list_host(int(w), int(rows), int(phase), _i(lst) if lst.size else None, C.byref(count)))
    return lst


def _probe_moved(moved):
    m = np.ascontiguousarray(moved, np.uint8).reshape(-1)
    return m, (m.ctypes.data_as(C.POINTER(C.c_uint8)) if m.size else None)


def history_probe_keep_host(rgb_sum, planes, w: int, rows: int, phase: int) -> np.ndarray:
    """PK of pt_history_probe_keep on the host (no GPU): the SUM image [n, 3] and the feature SUM planes in, float32 [P, 4] out."""
    s = np.ascontiguousarray(rgb_sum, np.float32).reshape(-1)
    p = np.ascontiguousarray(planes, np.float32).reshape(-1)
    n = w * rows
    if s.size != 3 * n or p.size != 4 * FEATURE_PLANES * n:
        raise PtError(f"history_probe_keep: {s.size} image and {p.size} plane floats for a tile of {w}x{rows}")
    kept = np.zeros((history_probe_list_host(w, rows, phase).size, 4), np.float32)
    _check(lib().pt_history_probe_keep_host(int(w), int(rows), int(phase), _f(s), _f(p), _f(kept) if kept.size else None))
    return kept


def history_probe_gradient_host(kept, group_sum, planes, w: int, rows: int, phase: int, moved=()):
    """The probes' gradient on the host (pt_history_probe_gradient_host; no GPU): PK [P, 4], the replayed sums [P, 3], the feature
    SUM planes and moved_geom in; (L float32 [P], changed, skipped) out."""
    k = np.ascontiguousarray(kept, np.float32).reshape(-1)
    b = np.ascontiguousarray(group_sum, np.float32).reshape(-1)
    p = np.ascontiguousarray(planes, np.float32).reshape(-1)
    P = history_probe_list_host(w, rows, phase).size
    if k.size != 4 * P or b.size != 3 * P or p.size != 4 * FEATURE_PLANES * w * rows:
        raise PtError(f"history_probe_gradient: {k.size} kept, {b.size} group and {p.size} plane floats for {P} probes of {w}x{rows}")
    m, mp = _probe_moved(moved)
    lam = np.zeros(P, np.float32)
    changed, skipped = C.c_int32(-1), C.c_int32(-1)
    _check(lib().pt_history_probe_gradient_host(int(w), int(rows), int(phase), _f(k) if P else None, _f(b) if P else None, _f(p), mp, int(m.size),
                                                _f(lam) if P else None, C.byref(changed), C.byref(skipped)))
    return lam, int(changed.value), int(skipped.value)


def history_probe_apply_host(current, lam, planes, w: int, rows: int, phase: int, moved=(), radius: int = 0, gain: float = 0.0) -> np.ndarray:
    """The probes' apply on the host (pt_history_probe_apply_host; no GPU): a copy of the current plane [n, 4] with C.w shortened."""
    c = np.array(current, np.float32).reshape(-1)
    l = np.ascontiguousarray(lam, np.float32).reshape(-1)
    p = np.ascontiguousarray(planes, np.float32).reshape(-1)
    n = w * rows
    if c.size != 4 * n or p.size != 4 * FEATURE_PLANES * n or l.size != history_probe_list_host(w, rows, phase).size:
        raise PtError(f"history_probe_apply: {c.size} current, {l.size} lam and {p.size} plane floats for a tile of {w}x{rows}")
    m, mp = _probe_moved(moved)
    opt = history_probe_options(radius, gain)
    _check(lib().pt_history_probe_apply_host(int(w), int(rows), int(phase), _f(l) if l.size else None, _f(p), mp, int(m.size), C.byref(opt), _f(c)))
    return c.reshape(-1, 4)


# ---- the history round: extra samples for the pixels whose history is short (include/pt_amd.h: pt_history_round) ----
HISTORY_ROUND_MIN_HISTORY = np.float32(4.0)  # PT_HISTORY_ROUND_MIN_HISTORY


def history_round_options(min_history: float = 0.0, max_fraction: float = 0.0) -> PtHistoryRoundOptions:
    """PtHistoryRoundOptions; 0 = the default of a field."""
    return PtHistoryRoundOptions(float(min_history), float(max_fraction))


def emitter_geoms(scene: "Scene") -> np.ndarray:
    """emitter_geom of pt_history_round for a scene: uint8 [num_geoms], 1 where the geom's material emits."""
    geoms, mats = scene.geoms(), scene.materials()
    return np.array([1 if mats[g.materialid].emittance > 0 else 0 for g in geoms], np.uint8)


def history_list_capacity(max_fraction: float, n: int) -> int:
    """cap of pt_history_round: clamp(ceil((double)(float)max_fraction * n), 1, n); 0 = the default 1."""
    f = float(np.float32(max_fraction)) or 1.0
    return int(min(n, max(1, math.ceil(f * n))))


def _history_select(call, planes, w: int, rows: int, current, emitter, min_history: float, max_fraction: float):
    n = w * rows
    p = np.ascontiguousarray(planes, np.float32).reshape(-1)
    c = None if current is None else np.ascontiguousarray(current, np.float32).reshape(-1)
    e = np.ascontiguousarray(emitter, np.uint8).reshape(-1)
    if p.size != 4 * FEATURE_PLANES * n or (c is not None and c.size != 4 * n):
        raise PtError(f"history_select: {p.size} plane floats for a tile of {w}x{rows}")
    opt = history_round_options(min_history, max_fraction)
    cap = history_list_capacity(max_fraction, n) if 0 <= max_fraction <= 1 and math.isfinite(max_fraction) else 1  # (a refused option: the call says so)
    lst = np.full(cap, -1, np.int32)
    fresh, m = C.c_int32(-1), C.c_int32(-1)
    _check(call(int(w), int(rows), _f(p), None if c is None else _f(c), e.ctypes.data_as(C.POINTER(C.c_uint8)) if e.size else None, int(e.size), C.byref(opt),
                _i(lst), C.byref(fresh), C.byref(m)))
    return lst, int(fresh.value), int(m.value)


def history_select_host(planes, w: int, rows: int, current=None, emitter=(), min_history: float = 0.0, max_fraction: float = 0.0):
    """The history round's key and selection on the host (pt_history_select_host; no GPU): the feature SUM planes
    [PT_FEATURE_PLANES, w*rows, 4], the current plane [w*rows, 4] (None: absent) and emitter_geom in; (list [cap] int32 with the first
    m entries written, fresh, m) out."""
    return _history_select(lib().pt_history_select_host, planes, w, rows, current, emitter, min_history, max_fraction)


def stage_history_select(planes, w: int, rows: int, current=None, emitter=(), min_history: float = 0.0, max_fraction: float = 0.0):
    """history_select_host's arguments through the device kernels (pt_stage_history_select; a renderer must be live); the entries
    behind m are -1."""
    return _history_select(lib().pt_stage_history_select, planes, w, rows, current, emitter, min_history, max_fraction)


def _history_merge(call, rgb_sum, extra, lst, group_sum, group_iters: int):
    s = np.array(rgb_sum, np.float32).reshape(-1)
    e = np.array(extra, np.float32).reshape(-1)
    l = np.ascontiguousarray(lst, np.int32).reshape(-1)
    b = np.ascontiguousarray(group_sum, np.float32).reshape(-1)
    if s.size != 3 * e.size or b.size != 3 * l.size:
        raise PtError(f"history_merge: {s.size} image, {e.size} extra, {b.size} group floats for a list of {l.size}")
    _check(call(int(e.size), _f(s), _f(e), _i(l), int(l.size), _f(b), int(group_iters)))
    return s.reshape(-1, 3), e


def history_merge_host(rgb_sum, extra, lst, group_sum, group_iters: int):
    """The history round's merge on the host (pt_history_merge_host; no GPU): copies of the SUM image [n, 3] and the extra plane [n]
    with the group sum [m, 3] of group_iters iterations joined at the listed pixels: (rgb_sum, extra)."""
    return _history_merge(lib().pt_history_merge_host, rgb_sum, extra, lst, group_sum, group_iters)


def stage_history_merge(rgb_sum, extra, lst, group_sum, group_iters: int):
    """history_merge_host's arguments through the device kernel (pt_stage_history_merge; a renderer must be live)."""
    return _history_merge(lib().pt_stage_history_merge, rgb_sum, extra, lst, group_sum, group_iters)


def _extra(extra, n: int) -> np.ndarray:
    e = np.ascontiguousarray(extra, np.float32).reshape(-1)
    if e.size != n:
        raise PtError(f"history: {e.size} extra floats for {n} pixels")
    return e


def history_blend_counted_host(rgb_sum, samples: float, extra, current=None) -> np.ndarray:
    """history_blend_host with the extra plane [n]: every pixel's samples are samples + extra[p] (pt_history_blend_counted_host)."""
    s = np.ascontiguousarray(rgb_sum, np.float32).reshape(-1)
    n = s.size // 3
    c = None if current is None else np.ascontiguousarray(current, np.float32).reshape(-1)
    if s.size != 3 * n or (c is not None and c.size != 4 * n):
        raise PtError(f"history_blend_counted_host: {s.size} image floats")
    out = np.empty((n, 3), np.float32)
    _check(lib().pt_history_blend_counted_host(n, _f(s), C.c_float(samples), _f(_extra(extra, n)), None if c is None else _f(c), _f(out)))
    return out


def history_capture_counted_host(rgb_sum, planes, samples: float, extra, current=None) -> np.ndarray:
    """history_capture_host with the extra plane [n] (pt_history_capture_counted_host)."""
    s = np.ascontiguousarray(rgb_sum, np.float32).reshape(-1)
    p = np.ascontiguousarray(planes, np.float32).reshape(-1)
    n = s.size // 3
    c = None if current is None else np.ascontiguousarray(current, np.float32).reshape(-1)
    if s.size != 3 * n or p.size != 4 * FEATURE_PLANES * n or (c is not None and c.size != 4 * n):
        raise PtError(f"history_capture_counted_host: {s.size} image, {p.size} plane floats")
    out = np.empty((HISTORY_KEPT_PLANES, n, 4), np.float32)
    _check(lib().pt_history_capture_counted_host(n, _f(s), _f(p), None if c is None else _f(c), C.c_float(samples), _f(_extra(extra, n)), _f(out)))
    return out


def history_capture_moments_counted_host(rgb_sum, samples: float, extra, current=None, current_var=None) -> np.ndarray:
    """history_capture_moments_host with the extra plane [n] (pt_history_capture_moments_counted_host)."""
    s = np.ascontiguousarray(rgb_sum, np.float32).reshape(-1)
    n = s.size // 3
    c = None if current is None else np.ascontiguousarray(current, np.float32).reshape(-1)
    v = None if current_var is None else np.ascontiguousarray(current_var, np.float32).reshape(-1)
    if s.size != 3 * n or any(a is not None and a.size != 4 * n for a in (c, v)):
        raise PtError(f"history_capture_moments_counted_host: {s.size} image floats")
    out = np.empty((n, 4), np.float32)
    _check(lib().pt_history_capture_moments_counted_host(n, _f(s), C.c_float(samples), _f(_extra(extra, n)), None if c is None else _f(c),
                                                         None if v is None else _f(v), _f(out)))
    return out


def history_denoise_moments_counted_host(rgb_sum, planes, w: int, rows: int, samples: float, extra, current=None, current_var=None,
                                         stats: Optional[dict] = None, **opts) -> np.ndarray:
    """history_denoise_moments_host with the extra plane [w*rows] (pt_history_denoise_moments_counted_host)."""
    s, p, out = _denoise_arrays(rgb_sum, planes, w, rows)
    c, v = _history_planes(current, current_var, w, rows)
    var_raw = np.empty(w * rows, np.float32) if stats is not None else None
    mark = np.empty(w * rows, np.uint8) if stats is not None else None
    opt = denoise_options(**opts)
    _check(lib().pt_history_denoise_moments_counted_host(int(w), int(rows), _f(s), _f(p), C.c_float(samples), _f(_extra(extra, w * rows)),
                                                         None if c is None else _f(c), None if v is None else _f(v), C.byref(opt), _f(out),
                                                         None if var_raw is None else _f(var_raw),
                                                         None if mark is None else mark.ctypes.data_as(C.POINTER(C.c_uint8))))
    if stats is not None:
        stats.update(var_raw=var_raw, mark=mark.astype(bool))
    return out


def split_noise(planes: np.ndarray) -> dict:
    """The noise planes [PT_NOISE_PLANES, n, 4] (pt_readback_noise) by name: prev [n, 3] (the SUM image at the last fold),
    q [n, 3] (sum over the groups of B^2 / n), variance [n] (w: estimated variance of the averaged radiance, channels added)."""
    p = planes.reshape(NOISE_PLANES, -1, 4)
    return dict(prev=np.ascontiguousarray(p[0, :, :3]), q=np.ascontiguousarray(p[1, :, :3]), variance=np.ascontiguousarray(p[0, :, 3]))


def noise_fold_host(rgb_sum: np.ndarray, planes: np.ndarray, group_iters: int, groups_after: int, iters_after: int) -> float:
    """One fold of the noise estimate on the host (pt_noise_fold_host; no GPU): SUM image [n, 3], planes float32
    [PT_NOISE_PLANES, n, 4] updated IN PLACE; returns SSE_est (-1 while groups_after < 2).  The device's planes equal it bit for bit."""
    s = np.ascontiguousarray(rgb_sum, np.float32).reshape(-1)
    if planes.dtype != np.float32 or not planes.flags.c_contiguous or planes.size != 4 * NOISE_PLANES * (s.size // 3) or s.size % 3:
        raise PtError(f"noise_fold_host: {s.size} image floats and {planes.size} plane floats (contiguous float32 [{NOISE_PLANES}, n, 4])")
    sse = C.c_double(-1.0)
    _check(lib().pt_noise_fold_host(s.size // 3, _f(s), _f(planes), int(group_iters), int(groups_after), int(iters_after), C.byref(sse)))
    return float(sse.value)


def join_noise(noise: dict) -> np.ndarray:
    """split_noise's dict (Renderer.readback_noise) back into the planes [PT_NOISE_PLANES, n, 4] the guided filter reads."""
    n = noise["variance"].shape[0]
    planes = np.zeros((NOISE_PLANES, n, 4), np.float32)
    planes[0, :, :3], planes[0, :, 3], planes[1, :, :3] = noise["prev"], noise["variance"], noise["q"]
    return planes


def denoise_guided_host(rgb_sum: np.ndarray, planes: np.ndarray, noise_planes: np.ndarray, w: int, rows: int, groups: int, iters: int,
                        **opts) -> np.ndarray:
    """The variance-guided filter on the host (pt_denoise_guided_host; no GPU): denoise_host's arrays, the noise planes
    [PT_NOISE_PLANES, w*rows, 4] and the counters M, T of the folds that made them.  The device result equals it bit for bit."""
    s, p, z, out = _denoise_arrays(rgb_sum, planes, w, rows, noise_planes)
    return _filter(lib().pt_denoise_guided_host, out, int(w), int(rows), _f(s), _f(p), _f(z), int(groups), int(iters), **opts)


def denoise_guided_variance_host(rgb_sum: np.ndarray, planes: np.ndarray, noise_planes: np.ndarray, w: int, rows: int, groups: int, iters: int,
                                 **opts):
    """The two variances the guided filter's levels start from (pt_denoise_guided_variance_host): (var_raw, var_0), [w*rows] each."""
    s, p, z, _ = _denoise_arrays(rgb_sum, planes, w, rows, noise_planes)
    raw, pre = np.empty(w * rows, np.float32), np.empty(w * rows, np.float32)
    opt = denoise_options(**opts)
    _check(lib().pt_denoise_guided_variance_host(int(w), int(rows), _f(s), _f(p), _f(z), int(groups), int(iters), C.byref(opt), _f(raw), _f(pre)))
    return raw, pre


def denoise_adaptive_host(rgb_sum: np.ndarray, planes: np.ndarray, noise_planes: np.ndarray, counts: np.ndarray, w: int, rows: int,
                          **opts) -> np.ndarray:
    """The variance-guided filter with per-pixel counts on the host (pt_denoise_adaptive_host; no GPU): denoise_guided_host's arrays
    and counts int32 [w*rows, 2] (T_p, M_p; Renderer.readback_adaptive).  The device result equals it bit for bit."""
    s, p, z, c, out = _denoise_arrays(rgb_sum, planes, w, rows, noise_planes, counts)
    return _filter(lib().pt_denoise_adaptive_host, out, int(w), int(rows), _f(s), _f(p), _f(z), _i(c), **opts)


def denoise_adaptive_variance_host(rgb_sum: np.ndarray, planes: np.ndarray, noise_planes: np.ndarray, counts: np.ndarray, w: int, rows: int,
                                   **opts):
    """The two variances the adaptive filter's levels start from (pt_denoise_adaptive_variance_host): (var_raw, var_0), [w*rows] each."""
    s, p, z, c, _ = _denoise_arrays(rgb_sum, planes, w, rows, noise_planes, counts)
    raw, pre = np.empty(w * rows, np.float32), np.empty(w * rows, np.float32)
    opt = denoise_options(**opts)
    _check(lib().pt_denoise_adaptive_variance_host(int(w), int(rows), _f(s), _f(p), _f(z), _i(c), C.byref(opt), _f(raw), _f(pre)))
    return raw, pre


def _select_arrays(noise_planes: np.ndarray, counts: np.ndarray, w: int, rows: int, m: int):
    z = np.ascontiguousarray(noise_planes, np.float32).reshape(-1)
    c = np.ascontiguousarray(counts, np.int32).reshape(-1)
    n = int(w) * int(rows)
    if z.size != NOISE_PLANES * n * 4 or c.size != 2 * n:
        raise PtError(f"adaptive_select: {z.size} noise plane floats and {c.size} counts for a tile of {w}x{rows}")
    if not 1 <= int(m) <= n:
        raise PtError(f"adaptive_select: a list of {m} out of {n} pixels")
    return z, c, np.full(int(m), -1, np.int32)


def adaptive_select_host(noise_planes: np.ndarray, counts: np.ndarray, w: int, rows: int, m: int) -> np.ndarray:
    """The selection of an adaptive round on the host (pt_adaptive_select_host; no GPU): noise planes [PT_NOISE_PLANES, n, 4], counts
    int32 [n, 2] (T_p, M_p) of a tile of w x rows -> the m tile indices with the largest key, ascending (int32 [m])."""
    z, c, out = _select_arrays(noise_planes, counts, w, rows, m)
    _check(lib().pt_adaptive_select_host(int(w), int(rows), _f(z), _i(c), int(m), _i(out)))
    return out


def stage_adaptive_select(noise_planes: np.ndarray, counts: np.ndarray, w: int, rows: int, m: int) -> np.ndarray:
    """adaptive_select_host's arguments through the selection's kernels (pt_stage_adaptive_select; needs a Renderer)."""
    z, c, out = _select_arrays(noise_planes, counts, w, rows, m)
    _check(lib().pt_stage_adaptive_select(int(w), int(rows), _f(z), _i(c), int(m), _i(out)))
    return out


def adaptive_merge_host(rgb_sum: np.ndarray, planes: np.ndarray, counts: np.ndarray, pixel_list: np.ndarray, group_sum: np.ndarray,
                        group_iters: int) -> float:
    """The merge of an adaptive round on the host (pt_adaptive_merge_host; no GPU): SUM image float32 [n, 3], planes float32
    [PT_NOISE_PLANES, n, 4] and counts int32 [n, 2], all contiguous and updated IN PLACE, from the group sums [m, 3] of the listed
    pixels.  Returns SSE_est, the estimates of all pixels added in pixel order."""
    lst = np.ascontiguousarray(pixel_list, np.int32).reshape(-1)
    sw = np.ascontiguousarray(group_sum, np.float32).reshape(-1)
    n = rgb_sum.size // 3
    for a, dt, size in ((rgb_sum, np.float32, 3 * n), (planes, np.float32, NOISE_PLANES * n * 4), (counts, np.int32, 2 * n)):
        if a.dtype != dt or not a.flags.c_contiguous or a.size != size:
            raise PtError(f"adaptive_merge_host: contiguous float32 [n, 3], float32 [{NOISE_PLANES}, n, 4] and int32 [n, 2] wanted")
    if sw.size != 3 * lst.size:
        raise PtError(f"adaptive_merge_host: {sw.size} group sum floats for a list of {lst.size}")
    sse = C.c_double(-1.0)
    _check(lib().pt_adaptive_merge_host(n, _f(rgb_sum.reshape(-1)), _f(planes.reshape(-1)), _i(counts.reshape(-1)), _i(lst), lst.size, _f(sw),
                                        int(group_iters), C.byref(sse)))
    return float(sse.value)


def stage_render_list(pixel_list: np.ndarray, iter_first: int, iter_count: int) -> np.ndarray:
    """The worker context of an adaptive round alone (pt_stage_render_list; needs a Renderer): the group sum float32 [m, 3] of the
    iterations for the listed tile pixels (distinct, any order)."""
    lst = np.ascontiguousarray(pixel_list, np.int32).reshape(-1)
    out = np.empty((lst.size, 3), np.float32)
    _check(lib().pt_stage_render_list(_i(lst), lst.size, int(iter_first), int(iter_count), _f(out)))
    return out


def stage_render_list_capacity(pixel_list: np.ndarray, capacity: int, iter_first: int, iter_count: int) -> np.ndarray:
    """stage_render_list on a worker planned for `capacity` >= len(pixel_list) pixels (pt_stage_render_list_capacity): the worker is
    kept across calls while the capacity is equal."""
    lst = np.ascontiguousarray(pixel_list, np.int32).reshape(-1)
    out = np.empty((lst.size, 3), np.float32)
    _check(lib().pt_stage_render_list_capacity(_i(lst), lst.size, int(capacity), int(iter_first), int(iter_count), _f(out)))
    return out


def _select_threshold(call, noise_planes, counts, w: int, rows: int, threshold: float, cap: int):
    z, c, out = _select_arrays(noise_planes, counts, w, rows, cap)
    above, m = C.c_int32(-1), C.c_int32(-1)
    _check(call(int(w), int(rows), _f(z), _i(c), C.c_float(threshold), int(cap), _i(out), C.byref(above), C.byref(m)))
    if not 0 <= m.value <= int(cap) or (out[m.value:] != -1).any():
        raise PtError(f"adaptive_select_threshold: a list of {m.value} (cap {cap}) with entries written behind it")
    return out[:m.value].copy(), int(above.value), int(m.value)


def adaptive_select_threshold_host(noise_planes: np.ndarray, counts: np.ndarray, w: int, rows: int, threshold: float, cap: int):
    """The selection by threshold on the host (pt_adaptive_select_threshold_host; no GPU): adaptive_select_host's arrays -> (the list
    int32 [m] in ascending tile index, above = pixels whose key exceeds threshold^2, m = min(above, cap))."""
    return _select_threshold(lib().pt_adaptive_select_threshold_host, noise_planes, counts, w, rows, threshold, cap)


def stage_adaptive_select_threshold(noise_planes: np.ndarray, counts: np.ndarray, w: int, rows: int, threshold: float, cap: int):
    """adaptive_select_threshold_host's arguments through the selection's kernels (pt_stage_adaptive_select_threshold; needs a Renderer)."""
    return _select_threshold(lib().pt_stage_adaptive_select_threshold, noise_planes, counts, w, rows, threshold, cap)


def _group_partition(call, pixel_list, w: int, h: int, n: int):
    lst = np.ascontiguousarray(pixel_list, np.int32).reshape(-1)
    parts = np.full(max(lst.size, 1), -1, np.int32)
    counts = np.full(max(int(n), 1), -1, np.int32)
    _check(call(int(w), int(h), int(n), _i(lst), lst.size, _i(parts), _i(counts)))
    ends = np.cumsum(counts)
    return [parts[e - c:e].copy() for c, e in zip(counts, ends)], counts


def group_partition_host(pixel_list: np.ndarray, w: int, h: int, n: int):
    """A frame's pixel list (ascending frame indices of a frame w x h) cut for the n contexts of a group (pt_group_partition_host; no
    GPU): ([part 0, ..., part n-1] as int32 tile indices, their lengths int32 [n])."""
    return _group_partition(lib().pt_group_partition_host, pixel_list, w, h, n)


def stage_group_partition(pixel_list: np.ndarray, w: int, h: int, n: int):
    """group_partition_host's arguments through the partition's kernels (pt_stage_group_partition; needs a Renderer)."""
    return _group_partition(lib().pt_stage_group_partition, pixel_list, w, h, n)


def _noise(call, *handle) -> dict:
    sse, groups, iters = C.c_double(-1.0), C.c_int32(0), C.c_int32(0)
    _check(call(*handle, C.byref(sse), C.byref(groups), C.byref(iters)))
    return dict(sse=float(sse.value), groups=int(groups.value), iterations=int(iters.value))


def _render_until(call, handle, iter_first, max_iters, group_iters, target_db):
    done, psnr = C.c_int32(0), C.c_float(-1.0)
    _check(call(*handle, int(iter_first), int(max_iters), int(group_iters), C.c_float(target_db), C.byref(done), C.byref(psnr)))
    return int(done.value), float(psnr.value)


class Renderer:
    """pathtraceInit / pathtrace / pathtraceFree over the C ABI (the default instance, like the reference's
    file-scope renderer state).  `arith`: "exact" (bit-identical to the oracle), "fma" or "fast" (PT_ARITH_*)."""

    def __init__(self, scene: Scene, device: int = 0, pixel_begin: int = 0, pixel_count: int = 0, **kw):
        opt = make_options(device=device, pixel_begin=pixel_begin, pixel_count=pixel_count, **kw)
        self.scene = scene
        w, h = scene.resolution
        self.n = pixel_count if pixel_count > 0 else w * h - pixel_begin
        self.pixel_begin = pixel_begin
        _check(lib().pt_init(C.byref(scene.desc), C.byref(opt)))
        self._live = True

    def render(self, iter_first: int, iter_count: int) -> None:
        _check(lib().pt_render(int(iter_first), int(iter_count)))

    def sync(self) -> None:
        _check(lib().pt_sync())

    def readback(self) -> np.ndarray:
        """Running SUM image of the tile, float32 [n, 3]."""
        out = np.empty((self.n, 3), np.float32)
        _check(lib().pt_readback(_f(out)))
        return out

    def readback_device(self, dev_ptr: int) -> None:
        _check(lib().pt_readback_device(C.c_void_p(dev_ptr)))

    def save_u8(self, samples: float) -> np.ndarray:
        """saveImage()'s bytes computed on the device: uint8 [rows, W, 3], x mirrored (whole-row tiles only)."""
        w, _ = self.scene.resolution
        out = np.empty((self.n // w, w, 3), np.uint8)
        _check(lib().pt_save_u8(C.c_float(samples), out.ctypes.data_as(C.POINTER(C.c_uint8))))
        return out

    def preview(self, iterations: int) -> np.ndarray:
        out = np.empty((self.n, 4), np.uint8)
        _check(lib().pt_preview_rgba8(int(iterations), out.ctypes.data_as(C.POINTER(C.c_uint8))))
        return out

    def stats(self) -> PtStats:
        st = PtStats()
        _check(lib().pt_get_stats(C.byref(st)))
        return st

    def reset_stats(self) -> None:
        _check(lib().pt_reset_stats())

    def clear(self) -> None:
        """Restart the accumulation (SUM image and statistics zeroed) on the same, already touched buffers."""
        _check(lib().pt_clear())

    def set_camera(self, cam: PtCamera, device_tables: bool = False) -> None:
        """Move the camera of the live renderer (pt_set_camera): from here on it gives what a renderer freshly created with
        `cam` gives, without the teardown, the allocations and the traversal probe of a new one.  device_tables: the
        camera-dependent tables are rebuilt on the device (pt_set_camera_ex, PT_SET_CAMERA_DEVICE_TABLES), the same bytes."""
        if device_tables:
            _check(lib().pt_set_camera_ex(C.byref(cam), PT_SET_CAMERA_DEVICE_TABLES))
        else:
            _check(lib().pt_set_camera(C.byref(cam)))

    def set_camera_times(self) -> PtSetCameraTimes:
        """Tables / re-arm / total milliseconds of the last move, and which build made its tables (pt_get_set_camera_times)."""
        t = PtSetCameraTimes()
        _check(lib().pt_get_set_camera_times(C.byref(t)))
        return t

    def set_geoms(self, geoms) -> None:
        """New transforms for the objects of the live renderer (pt_set_geoms): a Scene (after Scene.set_geom_trs) or a sequence of
        PtGeom.  From here on the renderer gives what one freshly created with these geoms gives; the camera stays."""
        arr, n = _geom_array(geoms)
        _check(lib().pt_set_geoms(arr, n))

    def set_materials(self, materials) -> None:
        """New materials for the live renderer (pt_set_materials): a Scene (after Scene.set_material) or a sequence of PtMaterial.
        From here on the renderer gives what one freshly created with these materials gives; camera and geoms stay."""
        arr, n = _material_array(materials)
        _check(lib().pt_set_materials(arr, n))

    def set_materials_times(self) -> PtSetMaterialsTimes:
        """Upload / re-arm / total milliseconds of the last set_materials (pt_get_set_materials_times)."""
        t = PtSetMaterialsTimes()
        _check(lib().pt_get_set_materials_times(C.byref(t)))
        return t

    def set_geoms_times(self) -> PtSetGeomsTimes:
        """Build / upload / re-arm / total milliseconds of the last set_geoms (pt_get_set_geoms_times)."""
        t = PtSetGeomsTimes()
        _check(lib().pt_get_set_geoms_times(C.byref(t)))
        return t

    @staticmethod
    def read_tables() -> dict:
        """The camera-dependent tables as they lie on the device, bytes by name (TABLE_NAMES; pt_stage_read_tables); b"" = absent."""
        out = {}
        for which, name in enumerate(TABLE_NAMES):
            n = C.c_uint64(0)
            _check(lib().pt_stage_read_tables(which, None, 0, C.byref(n)))
            buf = (C.c_uint8 * max(int(n.value), 1))()
            _check(lib().pt_stage_read_tables(which, buf, int(n.value), C.byref(n)))
            out[name] = bytes(buf)[:int(n.value)]
        return out

    def setup_times(self) -> PtSetupTimes:
        t = PtSetupTimes()
        _check(lib().pt_get_setup_times(C.byref(t)))
        return t

    # ---- first-hit feature buffers (include/pt_amd.h: pt_render_features) ----
    def render_features(self, iter_first: int, iter_count: int) -> None:
        """Adds what the camera rays of iterations iter_first .. iter_first + iter_count - 1 see to the feature SUM buffers."""
        _check(lib().pt_render_features(int(iter_first), int(iter_count)))

    def readback_features(self) -> dict:
        """The feature SUM buffers of the tile by name (split_features)."""
        out = np.empty((FEATURE_PLANES, self.n, 4), np.float32)
        _check(lib().pt_readback_features(_f(out)))
        return split_features(out)

    def readback_feature_planes(self) -> np.ndarray:
        """The feature SUM buffers of the tile as they lie, float32 [PT_FEATURE_PLANES, n, 4] (what the *_host functions take)."""
        out = np.empty((FEATURE_PLANES, self.n, 4), np.float32)
        _check(lib().pt_readback_features(_f(out)))
        return out

    # ---- reprojected sample history (include/pt_amd.h: pt_history_capture) ----
    def history_capture(self, samples: float) -> None:
        """Keeps the blend of the image (`samples` iterations) with the current history, and the first-hit surface, for the next view."""
        _check(lib().pt_history_capture(C.c_float(samples)))

    def history_reproject(self, **opts) -> None:
        """Resamples the kept history to the current camera from the current feature sums (options: history_options)."""
        opt = history_options(**opts)
        _check(lib().pt_history_reproject(C.byref(opt)))

    def history_resolve(self, samples: float) -> np.ndarray:
        """The image blended with the reprojected history: averaged radiance of the tile, float32 [n, 3]."""
        out = np.empty((self.n, 3), np.float32)
        _check(lib().pt_history_resolve(C.c_float(samples), _f(out)))
        return out

    def readback_history(self):
        """(kept planes [PT_HISTORY_KEPT_PLANES, n, 4], current plane [n, 4]; zeros while it is absent)."""
        kept = np.empty((HISTORY_KEPT_PLANES, self.n, 4), np.float32)
        cur = np.empty((self.n, 4), np.float32)
        _check(lib().pt_readback_history(_f(kept), _f(cur)))
        return kept, cur

    def history_drop(self) -> None:
        _check(lib().pt_history_drop())

    def history_capture_ex(self, samples: float, flags: int = HISTORY_VARIANCE) -> None:
        """history_capture, with PT_HISTORY_VARIANCE also keeping the variance of the blend (pt_history_capture_ex)."""
        _check(lib().pt_history_capture_ex(C.c_float(samples), int(flags)))

    def history_reproject_ex(self, flags: int = HISTORY_VARIANCE, **opts) -> None:
        """history_reproject, with PT_HISTORY_VARIANCE also resampling the kept variance (pt_history_reproject_ex); HISTORY_MOTION, alone
        or beside one of the two kinds, follows the objects that set_geoms moved since the capture."""
        opt = history_options(**opts)
        _check(lib().pt_history_reproject_ex(C.byref(opt), int(flags)))

    def history_denoise(self, samples: float, **opts) -> np.ndarray:
        """The blend of history_resolve filtered by the variance-guided filter with the blend's variance (pt_history_denoise;
        options: denoise_options): float32 [n, 3]."""
        return _filter(lib().pt_history_denoise, np.empty((self.n, 3), np.float32), C.c_float(samples), **opts)

    def history_denoise_ex(self, samples: float, flags: int = HISTORY_MOMENTS, **opts) -> np.ndarray:
        """The blend filtered with the variance the history's moments give (pt_history_denoise_ex with PT_HISTORY_MOMENTS: no folds,
        1 spp per view is enough); flags == 0 is history_denoise."""
        opt = denoise_options(**opts)
        out = np.empty((self.n, 3), np.float32)
        _check(lib().pt_history_denoise_ex(C.c_float(samples), C.byref(opt), int(flags), _f(out)))
        return out

    def history_denoise_feedback(self, samples: float, level: int = 0, variance: Optional[int] = None, **opts) -> np.ndarray:
        """The blend of the new samples with the FILTERED history, filtered like history_denoise_ex's (pt_history_denoise_feedback);
        the output of filter level `level` becomes the pending plane that history_capture_ex with HISTORY_FEEDBACK promotes."""
        opt, fb = denoise_options(**opts), history_feedback_options(level, variance)
        out = np.empty((self.n, 3), np.float32)
        _check(lib().pt_history_denoise_feedback(C.c_float(samples), C.byref(opt), C.byref(fb), _f(out)))
        return out

    def readback_history_feedback(self):
        """(FK, FC, P), float32 [n, 4] each; zeros while absent."""
        fk, fc, pend = (np.empty((self.n, 4), np.float32) for _ in range(3))
        _check(lib().pt_readback_history_feedback(_f(fk), _f(fc), _f(pend)))
        return fk, fc, pend

    def history_round(self, iter_first: int, group_iters: int, min_history: float = 0, max_fraction: float = 0):
        """A group of further iterations for the pixels whose carried history weighs less than min_history samples, the shortest
        max_fraction of the tile at the most (pt_history_round; synchronises once): (fresh pixels, pixels rendered)."""
        opt = history_round_options(min_history, max_fraction)
        fresh, selected = C.c_int32(-1), C.c_int32(-1)
        _check(lib().pt_history_round(int(iter_first), int(group_iters), C.byref(opt), C.byref(fresh), C.byref(selected)))
        return int(fresh.value), int(selected.value)

    def history_round_list(self, iter_first: int, group_iters: int, pixel_list: np.ndarray, capacity: int) -> None:
        """history_round without key and selection, over the caller's list (pt_history_round_list): distinct tile indices in ascending
        order, at most `capacity`, on the worker kept for `capacity` pixels; any tile, striped ones included.  Asynchronous."""
        lst = np.ascontiguousarray(pixel_list, np.int32).reshape(-1)
        self._round_list = lst  # (the upload is queued on the renderer's stream)
        _check(lib().pt_history_round_list(int(iter_first), int(group_iters), _i(lst), lst.size, int(capacity)))

    def history_probe_keep(self, iter_first: int, iter_count: int, phase: int = 0) -> None:
        """Keeps every third pixel of every third row of the image — iterations iter_first .. iter_first + iter_count - 1, all it holds —
        as probes for the next view (pt_history_probe_keep; asynchronous)."""
        _check(lib().pt_history_probe_keep(int(iter_first), int(iter_count), int(phase)))

    def history_probe_check(self, radius: int = 0, gain: float = 0.0):
        """Renders the kept probes again in the world as it is now and shortens the carried history C.w around those that differ
        (pt_history_probe_check; synchronises once): (probes, changed, skipped)."""
        opt = history_probe_options(radius, gain)
        probes, changed, skipped = C.c_int32(-1), C.c_int32(-1), C.c_int32(-1)
        _check(lib().pt_history_probe_check(C.byref(opt), C.byref(probes), C.byref(changed), C.byref(skipped)))
        return int(probes.value), int(changed.value), int(skipped.value)

    def readback_history_probe(self):
        """(PK float32 [P, 4], L float32 [P]; zeros before a check) of the kept probes; P = 0 when nothing is kept."""
        count = C.c_int32(-1)
        _check(lib().pt_readback_history_probe(None, None, C.byref(count)))
        kept, lam = np.zeros((count.value, 4), np.float32), np.zeros(count.value, np.float32)
        if count.value:
            _check(lib().pt_readback_history_probe(_f(kept), _f(lam), C.byref(count)))
        return kept, lam

    def readback_history_extra(self) -> np.ndarray:
        """The extra plane E, float32 [n]: the samples a pixel holds beyond the uniform ones; zeros while absent."""
        out = np.empty(self.n, np.float32)
        _check(lib().pt_readback_history_extra(_f(out)))
        return out

    def readback_history_variance(self):
        """(VK, VC), float32 [n, 4] each; zeros while absent."""
        vk, vc = np.empty((self.n, 4), np.float32), np.empty((self.n, 4), np.float32)
        _check(lib().pt_readback_history_variance(_f(vk), _f(vc)))
        return vk, vc

    def history_noise(self, samples: float, flags: int = HISTORY_VARIANCE) -> float:
        """SSE_blend: the variance of the blend of the image with the reprojected history, summed over the tile (pt_history_noise;
        synchronises); psnr_from_sse(sse, n) is the estimated PSNR of the blend."""
        sse = C.c_double(-1.0)
        _check(lib().pt_history_noise(C.c_float(samples), int(flags), C.byref(sse)))
        return float(sse.value)

    def readback_history_noise(self) -> np.ndarray:
        """The plane W of the last history_noise / history_render_until, float32 [n]."""
        out = np.empty(self.n, np.float32)
        _check(lib().pt_readback_history_noise(_f(out)))
        return out

    def history_render_until(self, iter_first: int, max_iters: int, target_db: float, group_iters: int = 0):
        """render_until judging the blend with the history (pt_history_render_until): (iterations rendered, the blend's last estimated
        PSNR in dB or -1, the view's own at the same fold or -1)."""
        done, psnr, view = C.c_int32(0), C.c_float(-1.0), C.c_float(-1.0)
        _check(lib().pt_history_render_until(int(iter_first), int(max_iters), int(group_iters), C.c_float(target_db), C.byref(done), C.byref(psnr),
                                             C.byref(view)))
        return int(done.value), float(psnr.value), float(view.value)

    # ---- threshold rounds over the blend (include/pt_amd.h: pt_history_round_threshold) ----
    def history_noise_adaptive(self) -> float:
        """history_noise with the sample counts of every pixel, valid in the adaptive state too (pt_history_noise_adaptive; synchronises):
        SSE_blend.  readback_history_noise returns W, readback_history_noise_samples NE."""
        sse = C.c_double(-1.0)
        _check(lib().pt_history_noise_adaptive(C.byref(sse)))
        return float(sse.value)

    def readback_history_noise_samples(self) -> np.ndarray:
        """The plane NE beside W: the blend's effective sample count Tf_p + Th per pixel, float32 [n]."""
        out = np.empty(self.n, np.float32)
        _check(lib().pt_readback_history_noise_samples(_f(out)))
        return out

    def history_round_threshold(self, iter_first: int, group_iters: int, threshold: float, max_fraction: float = 1.0):
        """adaptive_round_threshold keyed by the variance of the blend with the reprojected history (pt_history_round_threshold):
        (pixels above, pixels rendered)."""
        above, selected = C.c_int32(-1), C.c_int32(-1)
        _check(lib().pt_history_round_threshold(int(iter_first), int(group_iters), C.c_float(threshold), C.c_float(max_fraction), C.byref(above),
                                                C.byref(selected)))
        return int(above.value), int(selected.value)

    def history_render_threshold(self, iter_first: int, max_iters: int, threshold: float, max_fraction: float = 0.25, group_iters: int = 0,
                                 min_pixels: int = 0):
        """render_threshold over those rounds (pt_history_render_threshold): (iteration numbers used, pixel-samples rendered, pixels
        above at the last count or -1)."""
        done, samples, above = C.c_int32(0), C.c_int64(0), C.c_int32(-1)
        _check(lib().pt_history_render_threshold(int(iter_first), int(max_iters), int(group_iters), C.c_float(threshold), C.c_float(max_fraction),
                                                 int(min_pixels), C.byref(done), C.byref(samples), C.byref(above)))
        return int(done.value), int(samples.value), int(above.value)

    def history_resolve_adaptive(self) -> np.ndarray:
        """history_resolve with every pixel's own sample count (pt_history_resolve_adaptive): float32 [n, 3]."""
        out = np.empty((self.n, 3), np.float32)
        _check(lib().pt_history_resolve_adaptive(_f(out)))
        return out

    def history_capture_adaptive(self) -> None:
        """history_capture_ex(HISTORY_VARIANCE) with every pixel's own counts (pt_history_capture_adaptive)."""
        _check(lib().pt_history_capture_adaptive())

    def history_denoise_adaptive(self, **opts) -> np.ndarray:
        """history_denoise with every pixel's own counts (pt_history_denoise_adaptive): float32 [n, 3]."""
        return _filter(lib().pt_history_denoise_adaptive, np.empty((self.n, 3), np.float32), **opts)

    def denoise(self, samples: float, **opts) -> np.ndarray:
        """The image filtered by the edge-avoiding filter over the feature buffers (pt_denoise; options: denoise_options):
        averaged radiance of the tile, float32 [n, 3].  The tile is whole contiguous rows; a feature pass must have run."""
        return _filter(lib().pt_denoise, np.empty((self.n, 3), np.float32), C.c_float(samples), **opts)

    def denoise_guided(self, **opts) -> np.ndarray:
        """The image filtered by the variance-guided form of the filter (pt_denoise_guided): as denoise, the colour term following
        the noise estimate.  At least two groups must have been folded and nothing rendered since the last fold."""
        return _filter(lib().pt_denoise_guided, np.empty((self.n, 3), np.float32), **opts)

    def denoise_adaptive(self, **opts) -> np.ndarray:
        """The image filtered by the variance-guided filter with per-pixel sample counts (pt_denoise_adaptive): denoise_guided for
        the adaptive state, valid in the uniform state too.  Same preconditions as denoise_guided."""
        return _filter(lib().pt_denoise_adaptive, np.empty((self.n, 3), np.float32), **opts)

    # ---- noise estimate from batch sums (include/pt_amd.h: pt_noise_fold) ----
    def noise_fold(self) -> None:
        """Folds the iterations rendered since the last fold into the noise estimate as one group (asynchronous)."""
        _check(lib().pt_noise_fold())

    def noise(self) -> dict:
        """sse (SSE_est of the last fold, -1 before two groups), groups, iterations folded so far; psnr_from_sse(sse, n) is
        the estimated PSNR of the tile."""
        return _noise(lib().pt_get_noise)

    def readback_noise(self) -> dict:
        """The noise planes of the tile by name (split_noise): prev, q, variance."""
        out = np.empty((NOISE_PLANES, self.n, 4), np.float32)
        _check(lib().pt_readback_noise(_f(out)))
        return split_noise(out)

    def render_until(self, iter_first: int, max_iters: int, target_db: float, group_iters: int = 0):
        """Renders groups of group_iters iterations (0 = a batch) until the estimated PSNR is above target_db or max_iters
        are done (pt_render_until): (iterations rendered, last estimated PSNR in dB or -1)."""
        return _render_until(lib().pt_render_until, (), iter_first, max_iters, group_iters, target_db)

    # ---- adaptive sampling (include/pt_amd.h: pt_adaptive_round) ----
    def adaptive_round(self, iter_first: int, group_iters: int, fraction: float) -> None:
        """One round: the noisiest `fraction` of the pixels get iterations iter_first .. iter_first + group_iters - 1 (asynchronous)."""
        _check(lib().pt_adaptive_round(int(iter_first), int(group_iters), C.c_float(fraction)))

    def render_adaptive(self, iter_first: int, max_iters: int, target_db: float, fraction: float, group_iters: int = 0):
        """render_until with rounds (pt_render_adaptive): (iteration numbers used, pixel-samples rendered, last estimated PSNR or -1)."""
        done, samples, psnr = C.c_int32(0), C.c_int64(0), C.c_float(-1.0)
        _check(lib().pt_render_adaptive(int(iter_first), int(max_iters), int(group_iters), C.c_float(fraction), C.c_float(target_db), C.byref(done),
                                        C.byref(samples), C.byref(psnr)))
        return int(done.value), int(samples.value), float(psnr.value)

    def adaptive_round_threshold(self, iter_first: int, group_iters: int, threshold: float, max_fraction: float = 1.0):
        """One round over the pixels whose estimated standard error exceeds `threshold`, the noisiest max_fraction of the tile at the
        most (pt_adaptive_round_threshold; synchronises once): (pixels above, pixels rendered)."""
        above, selected = C.c_int32(-1), C.c_int32(-1)
        _check(lib().pt_adaptive_round_threshold(int(iter_first), int(group_iters), C.c_float(threshold), C.c_float(max_fraction), C.byref(above),
                                                 C.byref(selected)))
        return int(above.value), int(selected.value)

    def render_threshold(self, iter_first: int, max_iters: int, threshold: float, max_fraction: float = 0.25, group_iters: int = 0,
                         min_pixels: int = 0):
        """Uniform groups until two are folded, then threshold rounds until at most min_pixels pixels are above or max_iters iteration
        numbers are used (pt_render_threshold): (iteration numbers used, pixel-samples rendered, pixels above at the last count or -1)."""
        done, samples, above = C.c_int32(0), C.c_int64(0), C.c_int32(-1)
        _check(lib().pt_render_threshold(int(iter_first), int(max_iters), int(group_iters), C.c_float(threshold), C.c_float(max_fraction), int(min_pixels),
                                         C.byref(done), C.byref(samples), C.byref(above)))
        return int(done.value), int(samples.value), int(above.value)

    def adaptive_round_list(self, iter_first: int, group_iters: int, pixel_list: np.ndarray, capacity: int) -> None:
        """One round over the caller's list (pt_adaptive_round_list): distinct tile indices in ascending order, at most `capacity`, on
        the worker kept for `capacity` pixels; any tile, striped ones included.  Asynchronous."""
        lst = np.ascontiguousarray(pixel_list, np.int32).reshape(-1)
        self._round_list = lst  # (the upload is queued on the renderer's stream)
        _check(lib().pt_adaptive_round_list(int(iter_first), int(group_iters), _i(lst), lst.size, int(capacity)))

    def readback_adaptive(self) -> np.ndarray:
        """The per-pixel counts int32 [n, 2]: iterations T_p, groups M_p."""
        out = np.empty((self.n, 2), np.int32)
        _check(lib().pt_readback_adaptive(_i(out)))
        return out

    def resolve(self) -> np.ndarray:
        """Averaged radiance float32 [n, 3]: the SUM image over every pixel's own iterations (pt_resolve)."""
        out = np.empty((self.n, 3), np.float32)
        _check(lib().pt_resolve(_f(out)))
        return out

    # ---- convergence metric (make_options(convergence=...)) ----
    def set_reference(self, rgb_avg: np.ndarray) -> None:
        """The reference frame of convergence=-1: averaged radiance of the tile, float32 [n, 3]."""
        a = np.ascontiguousarray(rgb_avg, np.float32).reshape(-1)
        if a.size != 3 * self.n:
            raise PtError(f"set_reference: {a.size} floats for a tile of {self.n} pixels")
        _check(lib().pt_set_reference(_f(a)))

    def convergence(self, first: int, count: int) -> np.ndarray:
        """Sum of squared errors of iterations first .. first + count - 1 against the reference frame, float64 [count];
        -1 where there is none.  psnr_from_sse(sse, pixels) gives the reference's PSNR."""
        out = np.empty(max(int(count), 0), np.float64)
        _check(lib().pt_get_convergence(int(first), out.size, out.ctypes.data_as(C.POINTER(C.c_double))))
        return out

    def iterations_to_clean(self, threshold_db: float = 35.0) -> int:
        it = C.c_int32(-1)
        _check(lib().pt_iterations_to_clean(C.c_float(threshold_db), C.byref(it)))
        return int(it.value)

    def free(self) -> None:
        if self._live:
            self._live = False
            _check(lib().pt_free())

    # ---- stage-level entry points (parity tests) ----
    @staticmethod
    def stage_generate(pix_begin: int, n: int):
        o = np.zeros((3, n), np.float32)
        d = np.zeros((3, n), np.float32)
        _check(lib().pt_stage_generate(pix_begin, n, _f(o), _f(d)))
        return o, d

    @staticmethod
    def stage_intersect(o: np.ndarray, d: np.ndarray):
        n = o.shape[1]
        o = np.ascontiguousarray(o, np.float32)
        d = np.ascontiguousarray(d, np.float32)
        t = np.zeros(n, np.float32)
        nrm = np.zeros((3, n), np.float32)
        mat = np.zeros(n, np.int32)
        pt = np.zeros((3, n), np.float32)
        _check(lib().pt_stage_intersect(n, _f(o), _f(d), _f(t), _f(nrm), _i(mat), _f(pt)))
        return dict(t=t, nrm=nrm, mat=mat, pt=pt)

    @staticmethod
    def stage_intersect_grid(o: np.ndarray, d: np.ndarray, primary_form: bool = False):
        """stage_intersect's records through the uniform-grid walk of the fused kernels (pt_stage_intersect_grid): as depth 0
        walks (primary_form) or as the bounce kernel does.  The renderer must walk a grid (stats().grid_cells > 0)."""
        n = o.shape[1]
        o = np.ascontiguousarray(o, np.float32)
        d = np.ascontiguousarray(d, np.float32)
        t = np.zeros(n, np.float32)
        nrm = np.zeros((3, n), np.float32)
        mat = np.zeros(n, np.int32)
        pt = np.zeros((3, n), np.float32)
        _check(lib().pt_stage_intersect_grid(n, _f(o), _f(d), 1 if primary_form else 0, _f(t), _f(nrm), _i(mat), _f(pt)))
        return dict(t=t, nrm=nrm, mat=mat, pt=pt)

    @staticmethod
    def grid_info():
        """(PtGridInfo, longest cell list) of the grid the renderer walks (pt_stage_grid_info)."""
        info, longest = PtGridInfo(), C.c_int32(0)
        _check(lib().pt_stage_grid_info(C.byref(info), C.byref(longest)))
        return info, int(longest.value)

    @staticmethod
    def stage_save_u8(rgb_sum: np.ndarray, w: int, h: int, samples: float) -> np.ndarray:
        a = np.ascontiguousarray(rgb_sum, np.float32)
        out = np.empty((h, w, 3), np.uint8)
        _check(lib().pt_stage_save_u8(w, h, C.c_float(samples), _f(a), out.ctypes.data_as(C.POINTER(C.c_uint8))))
        return out

    @staticmethod
    def stage_denoise(rgb_sum: np.ndarray, planes: np.ndarray, w: int, rows: int, samples: float, **opts) -> np.ndarray:
        """denoise_host's arguments through the filter kernels (pt_stage_denoise)."""
        s, p, out = _denoise_arrays(rgb_sum, planes, w, rows)
        return _filter(lib().pt_stage_denoise, out, int(w), int(rows), _f(s), _f(p), C.c_float(samples), **opts)

    @staticmethod
    def stage_denoise_guided(rgb_sum: np.ndarray, planes: np.ndarray, noise_planes: np.ndarray, w: int, rows: int, groups: int, iters: int,
                             **opts) -> np.ndarray:
        """denoise_guided_host's arguments through the guided filter's kernels (pt_stage_denoise_guided)."""
        s, p, z, out = _denoise_arrays(rgb_sum, planes, w, rows, noise_planes)
        return _filter(lib().pt_stage_denoise_guided, out, int(w), int(rows), _f(s), _f(p), _f(z), int(groups), int(iters), **opts)

    @staticmethod
    def stage_denoise_adaptive(rgb_sum: np.ndarray, planes: np.ndarray, noise_planes: np.ndarray, counts: np.ndarray, w: int, rows: int,
                               **opts) -> np.ndarray:
        """denoise_adaptive_host's arguments through the adaptive filter's kernels (pt_stage_denoise_adaptive)."""
        s, p, z, c, out = _denoise_arrays(rgb_sum, planes, w, rows, noise_planes, counts)
        return _filter(lib().pt_stage_denoise_adaptive, out, int(w), int(rows), _f(s), _f(p), _f(z), _i(c), **opts)

    @staticmethod
    def stage_shade(depth: int, it, pixel, hit: dict, o, d, color):
        n = o.shape[1]
        o, d, color = (np.ascontiguousarray(a, np.float32).copy() for a in (o, d, color))
        alive = np.zeros(n, np.int32)
        _check(lib().pt_stage_shade(n, depth, _i(np.ascontiguousarray(it, np.int32)),
                                    _i(np.ascontiguousarray(pixel, np.int32)), _f(hit["t"]), _f(hit["nrm"]),
                                    _i(hit["mat"]), _f(hit["pt"]), _f(o), _f(d), _f(color), _i(alive)))
        return o, d, color, alive


def pt_free() -> None:
    _check(lib().pt_free())


TRANSPORT = {"auto": 0, "rccl": 1, "copy": 2}  # PT_GROUP_TRANSPORT_* (include/pt_amd.h)


class Group:
    """pt_group_*: one process driving several GPUs, row-interleaved tiles, one exchange at write-out (RCCL; peer /
    device copies when `devices` names a device more than once — several contexts on one GPU — or on request)."""

    def __init__(self, scene: Scene, devices: Sequence[int], transport: str = "auto", **kw):
        self.scene = scene
        self._h = C.c_void_p()
        dev = np.asarray(list(devices), np.int32)
        opt = make_options(**kw)
        _check(lib().pt_group_create_ex(C.byref(scene.desc), C.byref(opt), _i(dev), len(dev), TRANSPORT[transport],
                                        C.byref(self._h)))

    @property
    def transport(self) -> str:
        t = lib().pt_group_transport(self._h)
        return {v: k for k, v in TRANSPORT.items()}[t]

    def render(self, iter_first: int, iter_count: int) -> None:
        _check(lib().pt_group_render(self._h, int(iter_first), int(iter_count)))

    def set_camera(self, cam: PtCamera, device_tables: bool = False) -> None:
        """Renderer.set_camera on every context (pt_group_set_camera, pt_group_set_camera_ex); a refusal leaves every context as it was."""
        if device_tables:
            _check(lib().pt_group_set_camera_ex(self._h, C.byref(cam), PT_SET_CAMERA_DEVICE_TABLES))
        else:
            _check(lib().pt_group_set_camera(self._h, C.byref(cam)))

    def set_materials(self, materials) -> None:
        """Renderer.set_materials on every context (pt_group_set_materials); a refusal leaves every context as it was."""
        arr, n = _material_array(materials)
        _check(lib().pt_group_set_materials(self._h, arr, n))

    def set_geoms(self, geoms) -> None:
        """Renderer.set_geoms on every context (pt_group_set_geoms); a refusal leaves every context as it was."""
        arr, n = _geom_array(geoms)
        _check(lib().pt_group_set_geoms(self._h, arr, n))

    def gather(self) -> np.ndarray:
        w, h = self.scene.resolution
        out = np.empty((w * h, 3), np.float32)
        _check(lib().pt_group_gather(self._h, _f(out)))
        return out

    def render_features(self, iter_first: int, iter_count: int) -> None:
        _check(lib().pt_group_render_features(self._h, int(iter_first), int(iter_count)))

    def gather_features(self) -> dict:
        """The feature SUM buffers of the whole frame by name (split_features), raw orientation."""
        w, h = self.scene.resolution
        out = np.empty((FEATURE_PLANES, w * h, 4), np.float32)
        _check(lib().pt_group_gather_features(self._h, _f(out)))
        return split_features(out)

    def denoise(self, samples: float, **opts) -> np.ndarray:
        """Renderer.denoise of the whole frame (pt_group_denoise): float32 [W*H, 3], raw orientation."""
        w, h = self.scene.resolution
        return _filter(lib().pt_group_denoise, np.empty((w * h, 3), np.float32), self._h, C.c_float(samples), **opts)

    def denoise_guided(self, **opts) -> np.ndarray:
        """Renderer.denoise_guided of the whole frame (pt_group_denoise_guided): float32 [W*H, 3], raw orientation."""
        w, h = self.scene.resolution
        return _filter(lib().pt_group_denoise_guided, np.empty((w * h, 3), np.float32), self._h, **opts)

    def noise_fold(self) -> None:
        """Renderer.noise_fold on every context (pt_group_noise_fold)."""
        _check(lib().pt_group_noise_fold(self._h))

    def noise(self) -> dict:
        """Renderer.noise of the whole frame: the contexts' SSE_est added in context order (pt_group_get_noise)."""
        return _noise(lib().pt_group_get_noise, self._h)

    def render_until(self, iter_first: int, max_iters: int, target_db: float, group_iters: int = 0):
        """Renderer.render_until of the whole frame (pt_group_render_until); the PSNR is taken over W*H pixels."""
        return _render_until(lib().pt_group_render_until, (self._h,), iter_first, max_iters, group_iters, target_db)

    # ---- adaptive sampling by threshold across the group (include/pt_amd.h: pt_group_adaptive_round_threshold) ----
    def adaptive_round_threshold(self, iter_first: int, group_iters: int, threshold: float, max_fraction: float = 1.0):
        """Renderer.adaptive_round_threshold of the whole frame (pt_group_adaptive_round_threshold): (pixels above, pixels rendered)."""
        above, selected = C.c_int32(-1), C.c_int32(-1)
        _check(lib().pt_group_adaptive_round_threshold(self._h, int(iter_first), int(group_iters), C.c_float(threshold), C.c_float(max_fraction),
                                                       C.byref(above), C.byref(selected)))
        return int(above.value), int(selected.value)

    def render_threshold(self, iter_first: int, max_iters: int, threshold: float, max_fraction: float = 0.25, group_iters: int = 0,
                         min_pixels: int = 0):
        """Renderer.render_threshold of the whole frame (pt_group_render_threshold); group_iters 0 = the first context's batch."""
        done, samples, above = C.c_int32(0), C.c_int64(0), C.c_int32(-1)
        _check(lib().pt_group_render_threshold(self._h, int(iter_first), int(max_iters), int(group_iters), C.c_float(threshold), C.c_float(max_fraction),
                                               int(min_pixels), C.byref(done), C.byref(samples), C.byref(above)))
        return int(done.value), int(samples.value), int(above.value)

    def gather_adaptive(self) -> np.ndarray:
        """The per-pixel counts of the whole frame int32 [W*H, 2] (pt_group_gather_adaptive), raw orientation."""
        w, h = self.scene.resolution
        out = np.empty((w * h, 2), np.int32)
        _check(lib().pt_group_gather_adaptive(self._h, _i(out)))
        return out

    def resolve(self) -> np.ndarray:
        """Renderer.resolve of the whole frame (pt_group_resolve): float32 [W*H, 3], raw orientation."""
        w, h = self.scene.resolution
        out = np.empty((w * h, 3), np.float32)
        _check(lib().pt_group_resolve(self._h, _f(out)))
        return out

    def denoise_adaptive(self, **opts) -> np.ndarray:
        """Renderer.denoise_adaptive of the whole frame (pt_group_denoise_adaptive): float32 [W*H, 3], raw orientation."""
        w, h = self.scene.resolution
        return _filter(lib().pt_group_denoise_adaptive, np.empty((w * h, 3), np.float32), self._h, **opts)

    # ---- the reprojected history of the whole frame (include/pt_amd.h: "history in groups") ----
    def clear(self) -> None:
        """Renderer.clear on every context (pt_group_clear); the history's current planes become absent."""
        _check(lib().pt_group_clear(self._h))

    def history_capture_ex(self, samples: float, flags: int = HISTORY_MOMENTS) -> None:
        """Renderer.history_capture_ex of the whole frame (pt_group_history_capture_ex): flags 0 or HISTORY_MOMENTS."""
        _check(lib().pt_group_history_capture_ex(self._h, C.c_float(samples), int(flags)))

    def history_capture(self, samples: float) -> None:
        self.history_capture_ex(samples, 0)

    def history_reproject_ex(self, flags: int = HISTORY_MOMENTS, **opts) -> None:
        """Renderer.history_reproject_ex of the whole frame (pt_group_history_reproject_ex): 0 or HISTORY_MOMENTS, each alone or with
        HISTORY_MOTION."""
        opt = history_options(**opts)
        _check(lib().pt_group_history_reproject_ex(self._h, C.byref(opt), int(flags)))

    def history_reproject(self, **opts) -> None:
        self.history_reproject_ex(0, **opts)

    def history_resolve(self, samples: float) -> np.ndarray:
        """Renderer.history_resolve of the whole frame (pt_group_history_resolve): float32 [W*H, 3], raw orientation."""
        w, h = self.scene.resolution
        out = np.empty((w * h, 3), np.float32)
        _check(lib().pt_group_history_resolve(self._h, C.c_float(samples), _f(out)))
        return out

    def history_denoise_ex(self, samples: float, flags: int = HISTORY_MOMENTS, **opts) -> np.ndarray:
        """Renderer.history_denoise_ex of the whole frame (pt_group_history_denoise_ex; HISTORY_MOMENTS only): float32 [W*H, 3]."""
        w, h = self.scene.resolution
        opt = denoise_options(**opts)
        out = np.empty((w * h, 3), np.float32)
        _check(lib().pt_group_history_denoise_ex(self._h, C.c_float(samples), C.byref(opt), int(flags), _f(out)))
        return out

    def history_round(self, iter_first: int, group_iters: int, min_history: float = 0, max_fraction: float = 0):
        """Renderer.history_round of the whole frame (pt_group_history_round): (fresh pixels, pixels rendered)."""
        opt = history_round_options(min_history, max_fraction)
        fresh, selected = C.c_int32(-1), C.c_int32(-1)
        _check(lib().pt_group_history_round(self._h, int(iter_first), int(group_iters), C.byref(opt), C.byref(fresh), C.byref(selected)))
        return int(fresh.value), int(selected.value)

    def history_drop(self) -> None:
        _check(lib().pt_group_history_drop(self._h))

    def readback_history(self):
        """(kept planes [PT_HISTORY_KEPT_PLANES, W*H, 4], current plane [W*H, 4]; zeros while it is absent) of the frame."""
        w, h = self.scene.resolution
        kept = np.empty((HISTORY_KEPT_PLANES, w * h, 4), np.float32)
        cur = np.empty((w * h, 4), np.float32)
        _check(lib().pt_group_readback_history(self._h, _f(kept), _f(cur)))
        return kept, cur

    def readback_history_variance(self):
        """(VK, VC) of the frame, float32 [W*H, 4] each; zeros while absent."""
        w, h = self.scene.resolution
        vk, vc = np.empty((w * h, 4), np.float32), np.empty((w * h, 4), np.float32)
        _check(lib().pt_group_readback_history_variance(self._h, _f(vk), _f(vc)))
        return vk, vc

    def readback_history_extra(self) -> np.ndarray:
        """The extra plane E of the frame, float32 [W*H]; zeros while absent."""
        w, h = self.scene.resolution
        out = np.empty(w * h, np.float32)
        _check(lib().pt_group_readback_history_extra(self._h, _f(out)))
        return out

    def device_bytes(self) -> int:
        """Bytes of the group's own device buffers (pt_group_device_bytes); the contexts': stats(i).device_bytes."""
        return int(lib().pt_group_device_bytes(self._h))

    def context(self, i: int) -> int:
        """The handle of context i for the pt_ctx_* functions (pt_group_context)."""
        return lib().pt_group_context(self._h, int(i))

    def gather_u8(self, samples: float) -> np.ndarray:
        w, h = self.scene.resolution
        out = np.empty((h, w, 3), np.uint8)
        _check(lib().pt_group_gather_u8(self._h, C.c_float(samples), out.ctypes.data_as(C.POINTER(C.c_uint8))))
        return out

    def preview(self, iterations: int) -> np.ndarray:
        """Progressive preview of the running average (sendImageToPBO on every device + one exchange): uint8 [H*W, 4]."""
        w, h = self.scene.resolution
        out = np.empty((w * h, 4), np.uint8)
        _check(lib().pt_group_preview_rgba8(self._h, int(iterations), out.ctypes.data_as(C.POINTER(C.c_uint8))))
        return out

    def stats(self, i: int = 0) -> PtStats:
        st = PtStats()
        _check(lib().pt_ctx_get_stats(lib().pt_group_context(self._h, i), C.byref(st)))
        return st

    def set_reference(self, rgb_avg: np.ndarray) -> None:
        """The reference frame of convergence=-1 for the whole frame: averaged radiance, float32 [W*H, 3], raw orientation."""
        w, h = self.scene.resolution
        a = np.ascontiguousarray(rgb_avg, np.float32).reshape(-1)
        if a.size != 3 * w * h:
            raise PtError(f"set_reference: {a.size} floats for a frame of {w}x{h}")
        _check(lib().pt_group_set_reference(self._h, _f(a)))

    def convergence(self, first: int, count: int) -> np.ndarray:
        """SSE of the whole frame per iteration (the contexts' sums added in context order); -1 where there is none."""
        out = np.empty(max(int(count), 0), np.float64)
        _check(lib().pt_group_get_convergence(self._h, int(first), out.size, out.ctypes.data_as(C.POINTER(C.c_double))))
        return out

    def iterations_to_clean(self, threshold_db: float = 35.0) -> int:
        it = C.c_int32(-1)
        _check(lib().pt_group_iterations_to_clean(self._h, C.c_float(threshold_db), C.byref(it)))
        return int(it.value)

    def free(self) -> None:
        if self._h:
            lib().pt_group_destroy(self._h)
            self._h = C.c_void_p()


def write_png_rgb8(path: str, rgb8: np.ndarray) -> None:
    a = np.ascontiguousarray(rgb8, np.uint8)
    h, w = a.shape[0], a.shape[1]
    if lib().pt_write_png_rgb8(os.fsencode(path), a.ctypes.data_as(C.POINTER(C.c_uint8)), w, h) != 0:
        raise PtError(f"cannot write {path}")


def output_basename(name: str, samples: int) -> str:
    buf = C.create_string_buffer(512)
    lib().pt_output_basename(name.encode(), int(samples), buf, 512)
    return buf.value.decode()


def save_png(path: str, rgb_sum: np.ndarray, w: int, h: int, samples: float) -> None:
    a = np.ascontiguousarray(rgb_sum, np.float32)
    if lib().pt_save_png(os.fsencode(path), _f(a), w, h, C.c_float(samples)) != 0:
        raise PtError(f"cannot write {path}")


def save_hdr(path: str, rgb_sum: np.ndarray, w: int, h: int, samples: float) -> None:
    """image::saveHDR's Radiance file (x mirrored, sum / samples), byte for byte the reference writer's."""
    a = np.ascontiguousarray(rgb_sum, np.float32)
    if lib().pt_save_hdr(os.fsencode(path), _f(a), w, h, C.c_float(samples)) != 0:
        raise PtError(f"cannot write {path}")


def save_pfm(path: str, rgb_sum: np.ndarray, w: int, h: int, samples: float) -> None:
    a = np.ascontiguousarray(rgb_sum, np.float32)
    if lib().pt_save_pfm(os.fsencode(path), _f(a), w, h, C.c_float(samples)) != 0:
        raise PtError(f"cannot write {path}")


def load_pfm(path: str, samples: float = 1.0) -> np.ndarray:
    """The inverse of save_pfm: float32 [h, w, 3], raw orientation, file contents times `samples`."""
    w, h = C.c_int32(0), C.c_int32(0)
    if lib().pt_load_pfm(os.fsencode(path), None, 0, C.byref(w), C.byref(h), C.c_float(samples)) != 0:
        raise PtError(f"cannot read {path}")
    out = np.empty((h.value, w.value, 3), np.float32)
    if lib().pt_load_pfm(os.fsencode(path), _f(out), w.value * h.value, C.byref(w), C.byref(h), C.c_float(samples)) != 0:
        raise PtError(f"cannot read {path}")
    return out


def psnr_from_sse(sse: float, pixels: int) -> float:
    """computePSNR's last lines (pt_psnr_from_sse): FLT_MAX where the reference prints "Inf"."""
    return float(lib().pt_psnr_from_sse(C.c_double(sse), C.c_int64(pixels)))
