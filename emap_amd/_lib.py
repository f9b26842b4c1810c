"""ctypes binding of libemap_hip.so: the four headers under include/, each through its own table and pair of views (HEADERS), and the
fifth and the sixth, include/emap_score_hip.h and include/emap_field_hip.h, through records of the same form beside them (SCORE_HEADER,
FIELD_HEADER).

The library is built in-tree by ``__graft_entry__.build()`` (``emap_amd/csrc/build.sh``).
There is no CPU fallback: if the library is missing, or a call is made without a GPU, the error is
raised to the caller.
"""
from __future__ import annotations

import ctypes as C
import os
import types

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("EMAP_HIP_LIB") or os.path.join(_HERE, "lib", "libemap_hip.so")   # env override: A/B builds

PREC_BF16 = 0
PREC_BF16X3 = 1
PREC_F16 = 2
PREC_F16X3 = 3
PREC_F16X3M = 4    # f16x3 with MX-fp6 cross terms in the forward sweep of the value+gradient pass too (include/emap_hip.h)
PREC_F16X3E = 5    # f16x3 with f16 cross terms in both sweeps of the value+gradient pass (no MX fp6): the wider-margin mode
PRECISIONS = {"bf16": PREC_BF16, "bf16x3": PREC_BF16X3, "f16": PREC_F16, "f16x3": PREC_F16X3, "f16x3m": PREC_F16X3M, "f16x3e": PREC_F16X3E}
UDF_TYPES = {"abs": 0, "square": 1, "sdf": 2}
MAX_LIN = 12
MAX_TRAIN_IMAGES = 1024      # EMAP_MAX_TRAIN_IMAGES: the longest list DeviceRaySampler.set_train_images takes
MAX_SAMPLES_PER_RAY = 1024   # EMAP_MAX_SAMPLES_PER_RAY: S = n_samples + up_sample_steps * (n_importance // up_sample_steps)
ABI_VERSION = 12   # ABI 12 removed emap_set_value_tile_mode (the 32x32 value kernel)

# EmapRenderParams.render_mode (ABI 11): use_unbias_render / use_norm_grad_for_cosine of the reference renderer
RENDER_UNBIASED = 0
RENDER_UNBIASED_NORMCOS = 1
RENDER_PLAIN = 2

# the record of emap_train_monitor (EMAP_MON_* of include/emap_hip.h): float64 fields at fixed indices - the first MON_ROW of them are the
# per-step fields (one ring row), the rest the running ones
MON_NAMES = ("iter_step", "loss", "edge_loss", "eikonal_loss", "eikonal_ns_loss", "psnr", "variance", "beta", "gamma", "udf_min", "udf_mean",
             "weight_sum", "lr_geo", "lr", "cos_anneal_ratio", "flip_saturation",
             "steps", "window_n", "window_sum", "loss_avg", "windows", "nonfinite_steps", "first_nonfinite_iter")
MON_ROW = 16
MON_FIELDS = len(MON_NAMES)
MON = {k: i for i, k in enumerate(MON_NAMES)}

F_NAN_SAMPLES = 1
F_NAN_GRADERR = 2
F_MLP_NONFINITE = 4


class NetConfig(C.Structure):
    _fields_ = [("d_hidden", C.c_int32), ("n_lin", C.c_int32), ("skip_l", C.c_int32), ("multires", C.c_int32),
                ("d_out", C.c_int32), ("udf_type", C.c_int32), ("scale", C.c_float)]


class CompositeOut(C.Structure):
    _fields_ = [(k, C.c_void_p) for k in (
        "weights", "alpha", "mid_z", "dists", "inside_sphere", "gradient_mag", "gradients_flip", "edge", "depth",
        "weight_sum", "normals", "scalars")]


class RenderParams(C.Structure):
    _fields_ = [("n_rays", C.c_int32), ("n_samples", C.c_int32), ("n_importance", C.c_int32),
                ("up_sample_steps", C.c_int32), ("inv_s", C.c_float), ("beta", C.c_float), ("gamma", C.c_float),
                ("cos_anneal_ratio", C.c_float), ("has_cos_anneal", C.c_int32), ("flip_saturation", C.c_float),
                ("near_surface", C.c_float), ("sparse_scale", C.c_float), ("background", C.c_float),
                ("has_background", C.c_int32), ("variance_dev", C.c_void_p), ("beta_dev", C.c_void_p),
                ("gamma_dev", C.c_void_p), ("beta_min", C.c_float), ("render_mode", C.c_int32)]


class CompositeGrads(C.Structure):
    _fields_ = [("d_edge", C.c_void_p), ("d_depth", C.c_void_p), ("d_gradient_error", C.c_void_p),
                ("d_gradient_error_near_surface", C.c_void_p), ("scalars", C.c_void_p), ("d_variance", C.c_void_p),
                ("d_beta", C.c_void_p), ("d_gamma", C.c_void_p), ("grad_scale", C.c_float), ("accumulate", C.c_int32),
                ("zero_tail", C.c_void_p), ("n_zero_tail", C.c_int64)]


class ParamGrads(C.Structure):
    _fields_ = [("g_host", C.POINTER(C.c_void_p)), ("v_host", C.POINTER(C.c_void_p)), ("dg_host", C.POINTER(C.c_void_p)),
                ("dv_host", C.POINTER(C.c_void_p)), ("db_host", C.POINTER(C.c_void_p)), ("weight_norm", C.c_int32),
                ("accumulate", C.c_int32), ("grad_scale", C.c_float), ("reserved", C.c_int32)]


class RayDataset(C.Structure):
    _fields_ = [("edges", C.c_void_p), ("pixel_order", C.c_void_p), ("n_edge", C.c_void_p), ("density", C.c_void_p),
                ("kinv", C.c_void_p), ("pose", C.c_void_p), ("image_perm", C.c_void_p), ("n_images", C.c_int32), ("H", C.c_int32),
                ("W", C.c_int32), ("reserved", C.c_int32)]


class RayBatch(C.Structure):
    _fields_ = [(k, C.c_void_p) for k in ("rays_o", "rays_v", "edge", "depth_scale", "ndc_uv", "p_cam", "pixels", "img_idx", "t_rand")]


# every symbol include/emap_hip.h declares: name -> (restype, argtypes).  _RC marks an int that is a return code (0 = success): those
# symbols, and only those, also appear in the checked view api()
_P = C.c_void_p
_RC = "rc"
SYMBOLS = {
    "emap_abi_version": (C.c_int, []),
    "emap_last_error": (C.c_char_p, []),
    "emap_set_grad_mode": (C.c_int, [C.c_int]),
    "emap_set_fused_sampling": (C.c_int, [C.c_int]),
    "emap_set_fused_composite": (C.c_int, [C.c_int]),
    "emap_packed_bytes": (_RC, [C.POINTER(NetConfig), C.c_int, C.POINTER(C.c_size_t)]),
    "emap_pack_weights": (_RC, [C.POINTER(NetConfig), C.POINTER(_P), C.POINTER(_P), C.POINTER(_P), _P, C.c_int, _P]),
    "emap_udf_fwd": (_RC, [C.POINTER(NetConfig), _P, C.c_int, _P, C.c_int64, _P, _P]),
    "emap_udf_scratch_bytes": (_RC, [C.POINTER(NetConfig), C.c_int, C.c_int64, C.POINTER(C.c_size_t)]),
    "emap_udf_fwd_grad": (_RC, [C.POINTER(NetConfig), _P, C.c_int, _P, C.c_int64, _P, _P, _P, C.c_size_t, _P]),
    "emap_embed": (_RC, [_P, C.c_int64, C.c_int, _P, _P]),
    "emap_null_direction": (_RC, [_P, C.c_int64, C.c_int, _P, _P]),
    "emap_lattice_points": (_RC, [C.c_int, C.c_int64, C.c_int64, _P, _P]),
    "emap_compact_workspace_bytes": (_RC, [C.c_int64, C.POINTER(C.c_size_t)]),
    "emap_compact_append": (_RC, [_P, _P, C.c_int64, C.c_int64, C.c_float, C.c_int, _P, _P, _P, C.c_int64, _P, _P, C.c_size_t, _P]),
    "emap_jitter_points": (_RC, [_P, _P, C.c_int64, C.c_int, C.c_float, _P, _P]),
    "emap_shift_points": (_RC, [_P, _P, _P, C.c_int64, _P, _P]),
    "emap_nn_workspace_bytes": (_RC, [C.c_int64, C.POINTER(C.c_size_t)]),
    "emap_nearest_neighbors": (_RC, [_P, C.c_int64, _P, C.c_int64, C.c_int, _P, _P, _P, C.c_size_t, _P]),
    "emap_dist_stats": (_RC, [_P, C.c_int64, C.POINTER(C.c_float), C.c_int, _P, _P]),
    "emap_edge_sample_counts": (_RC, [_P, C.c_int, _P, C.c_int, C.c_double, C.c_int, _P, _P, _P]),
    "emap_edge_sample_fill": (_RC, [_P, C.c_int, _P, C.c_int, _P, _P, _P, _P, C.c_int64, _P]),
    "emap_edge_sample_fill_tangents": (_RC, [_P, C.c_int, _P, C.c_int, _P, _P, _P, _P, _P, C.c_int64, _P]),
    "emap_sample_pdf": (_RC, [_P, _P, C.c_int, C.c_int, C.c_int, _P, _P, _P, _P]),
    "emap_sample_pdf_u": (_RC, [_P, _P, _P, C.c_int, C.c_int, C.c_int, _P, _P, _P, _P]),
    "emap_upsample_step": (_RC, [_P, _P, _P, _P, C.c_int, C.c_int, C.c_int, _P, C.c_float, C.c_float, C.c_float,
                                     _P, _P, _P, _P]),
    "emap_upsample_step_plain": (_RC, [_P, _P, _P, _P, C.c_int, C.c_int, C.c_int, _P, C.c_float, C.c_float, _P, _P, _P, _P]),
    "emap_merge_sorted": (_RC, [_P, _P, _P, _P, C.c_int, C.c_int, C.c_int, _P, _P, _P, _P]),
    "emap_composite_fwd": (_RC, [_P, _P, _P, _P, _P, _P, C.c_int, C.c_int, _P, C.c_float, C.c_float, C.c_float,
                                     C.c_float, C.c_int, C.c_float, C.c_float, C.c_float, C.c_float, C.c_int,
                                     C.POINTER(CompositeOut), _P, _P, _P]),
    "emap_composite_fwd_p": (_RC, [_P, _P, _P, _P, _P, _P, C.c_int, C.c_int, _P, C.POINTER(RenderParams),
                                       C.POINTER(CompositeOut), _P, _P, _P]),
    "emap_render_workspace_bytes": (_RC, [C.POINTER(NetConfig), C.c_int, C.POINTER(RenderParams), C.POINTER(C.c_size_t)]),
    "emap_render_fwd": (_RC, [C.POINTER(NetConfig), _P, C.c_int, C.POINTER(RenderParams), _P, _P, _P, _P, _P, _P,
                                  _P, _P, _P, C.POINTER(CompositeOut), _P, C.c_size_t, _P, _P]),
    "emap_composite_bwd": (_RC, [_P, _P, _P, _P, _P, _P, C.c_int, C.c_int, _P, C.POINTER(RenderParams),
                                     C.POINTER(CompositeGrads), _P, _P, _P, _P]),
    "emap_udf_vjp_workspace_bytes": (_RC, [C.POINTER(NetConfig), C.c_int, C.c_int64, C.POINTER(C.c_size_t)]),
    "emap_udf_vjp": (_RC, [C.POINTER(NetConfig), _P, C.c_int, _P, C.c_int64, _P, _P, C.POINTER(ParamGrads), _P, C.c_size_t,
                               _P, _P]),
    "emap_render_bwd_workspace_bytes": (_RC, [C.POINTER(NetConfig), C.c_int, C.POINTER(RenderParams), C.POINTER(C.c_size_t)]),
    "emap_render_bwd": (_RC, [C.POINTER(NetConfig), _P, C.c_int, C.POINTER(RenderParams), _P, _P, _P, _P, _P, _P, _P,
                                  C.POINTER(CompositeGrads), C.POINTER(ParamGrads), _P, C.c_size_t, _P, _P]),
    "emap_render_bwd_absmax_offset": (_RC, [C.POINTER(NetConfig), C.c_int, C.POINTER(RenderParams), C.POINTER(C.c_size_t)]),
    "emap_render_bwd_staged": (_RC, [C.POINTER(NetConfig), _P, C.c_int, C.POINTER(RenderParams), _P, _P, _P, _P, _P, _P, _P,
                                         C.POINTER(CompositeGrads), C.POINTER(ParamGrads), _P, C.c_size_t, _P, _P, C.c_int]),
    "emap_sample_rays": (_RC, [C.POINTER(RayDataset), C.c_int, C.c_int, C.c_int, C.c_uint64, C.c_uint64, _P, _P, C.POINTER(RayBatch), _P]),
    "emap_check_train_images": (_RC, [C.POINTER(C.c_int32), C.c_int, C.c_int]),
    "emap_sample_rays_train": (_RC, [C.POINTER(RayDataset), _P, C.c_int, _P, _P, C.c_int, C.c_int, C.c_uint64, _P, _P, C.POINTER(RayBatch), _P]),
    "emap_gen_rays_count": (_RC, [C.POINTER(RayDataset), C.c_int, C.POINTER(C.c_int64), C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "emap_gen_rays_at": (_RC, [C.POINTER(RayDataset), C.c_int, C.c_int, C.c_int64, C.c_int64, _P, _P, _P, _P]),
    "emap_train_stats": (_RC, [_P, _P, _P, C.c_int, C.c_float, _P, _P, _P]),
    "emap_train_loss": (_RC, [_P, C.c_float, C.c_float, C.c_float, _P, _P]),
    "emap_adam_step": (_RC, [_P, _P, _P, _P, _P, C.c_int64, C.c_int64, C.c_float, C.c_float, C.c_double, C.c_double, C.c_float, _P]),
    "emap_adam_step_masked": (_RC, [_P, _P, _P, _P, _P, C.c_int64, C.c_int64, C.c_float, C.c_float, C.c_double, C.c_double, C.c_float, _P, _P, _P]),
    "emap_train_schedule": (_RC, [_P, C.c_int64, C.c_double, C.c_double, C.c_double, C.c_double, C.c_double, C.c_double, C.c_int, C.c_int64,
                                      C.c_double, _P, _P]),
    "emap_render_fwd_sched": (_RC, [C.POINTER(NetConfig), _P, C.c_int, C.POINTER(RenderParams), _P, _P, _P, _P, _P, _P,
                                        _P, _P, _P, C.POINTER(CompositeOut), _P, C.c_size_t, _P, _P, _P]),
    "emap_render_bwd_staged_sched": (_RC, [C.POINTER(NetConfig), _P, C.c_int, C.POINTER(RenderParams), _P, _P, _P, _P, _P, _P, _P,
                                               C.POINTER(CompositeGrads), C.POINTER(ParamGrads), _P, C.c_size_t, _P, _P, C.c_int, _P]),
    "emap_adam_step_masked_sched": (_RC, [_P, _P, _P, _P, _P, C.c_int64, C.c_int64, _P, C.c_double, C.c_double, C.c_float, _P, _P, _P]),
    "emap_train_monitor_workspace_bytes": (_RC, [C.c_int, C.POINTER(C.c_size_t)]),
    "emap_train_monitor": (_RC, [_P, _P, C.c_int, C.c_int, _P, _P, _P, _P, C.c_float, C.c_float, C.c_float, C.c_int64, C.c_int, C.c_int,
                                     _P, _P, _P, _P, C.c_size_t, _P]),
    "emap_ar_local_bytes": (_RC, [C.c_int64, C.POINTER(C.c_size_t)]),
    "emap_ar_alloc": (_RC, [C.c_size_t, C.POINTER(C.c_void_p), _P]),
    "emap_ar_open": (_RC, [_P, C.POINTER(C.c_void_p)]),
    "emap_ar_close": (_RC, [_P]),
    "emap_ar_free": (_RC, [_P]),
    "emap_ar_allreduce_sum": (_RC, [_P, C.c_int64, C.c_int, C.c_int, C.POINTER(C.c_void_p), C.c_size_t, _P]),
    "emap_ar_error": (_RC, [_P, C.POINTER(C.c_int)]),
    "emap_ar_set_timeout_ms": (_RC, [C.c_int64]),
    "emap_profile_enable": (_RC, [C.c_int]),
    "emap_profile_read": (_RC, [C.POINTER(C.c_float), C.POINTER(C.c_int)]),
    "emap_profile_read_kernel": (_RC, [C.c_int, C.POINTER(C.c_float), C.POINTER(C.c_int)]),
    "emap_profile_read_clock": (_RC, [C.c_int, C.POINTER(C.c_float)]),
    "emap_linspace_host": (None, [C.c_float, C.c_float, C.c_int, C.POINTER(C.c_float)]),
}

# every symbol include/emap_eval_hip.h declares, in the same form: the second header of the same library (HEADERS, below)
EVAL_ABI_VERSION = 1
EVAL_POINTS_DTYPES = {torch.float64: 0, torch.float32: 1}                       # EMAP_EVAL_POINTS_*
EVAL_MAPS_DTYPES = {torch.uint8: 0, torch.float32: 1, torch.float64: 2}         # EMAP_EVAL_MAPS_*
EVAL_SYMBOLS = {
    "emap_eval_abi_version": (C.c_int, []),
    "emap_point_visibility": (_RC, [_P, C.c_int, C.c_int64, _P, _P, _P, _P, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_double, C.c_int,
                                    _P, _P, _P]),
}

# every symbol include/emap_fit_hip.h declares: the third header
FIT_ABI_VERSION = 1
FIT_MAX_POLYLINE_POINTS = 1024     # EMAP_FIT_MAX_POLYLINE_POINTS
FIT_MAX_LINES = 16                 # EMAP_FIT_MAX_LINES
FIT_LINK_LDS_POINTS = 1 << 20      # EMAP_FIT_LINK_LDS_POINTS
FIT_SYMBOLS = {
    "emap_fit_abi_version": (C.c_int, []),
    "emap_fit_link": (_RC, [_P, C.c_int, _P, _P, _P, C.c_int, C.c_int, C.c_int, C.c_double, C.c_double, C.c_double, C.c_int, C.c_int, _P, _P, _P,
                            _P, _P]),
    "emap_fit_lines": (_RC, [_P, _P, C.c_int, C.c_double, C.c_int, C.c_int, _P, _P, _P, _P]),
    "emap_fit_beziers": (_RC, [_P, _P, C.c_int, _P, _P, _P]),
    "emap_fit_merge_lines": (_RC, [_P, C.c_int, _P, _P, C.c_double, C.c_double, _P, _P, _P, C.c_size_t, _P]),
    "emap_fit_merge_endpoints": (_RC, [_P, C.c_int, C.c_double, _P, _P, _P, C.c_size_t, _P]),
}

# every symbol include/emap_raster_hip.h declares: the fourth header
RASTER_ABI_VERSION = 1
RASTER_MAX_CURVE_SEGMENTS = 256    # EMAP_RASTER_MAX_CURVE_SEGMENTS
RASTER_MAX_SEGMENTS = 1 << 20      # EMAP_RASTER_MAX_SEGMENTS
RASTER_MAX_HALF_WIDTH = 64.0       # EMAP_RASTER_MAX_HALF_WIDTH
RASTER_MAX_FRAMES = 65535          # EMAP_RASTER_MAX_FRAMES
RASTER_MAX_DIM = 65536             # EMAP_RASTER_MAX_DIM
RASTER_ROW_BYTES = 64              # EMAP_RASTER_ROW_BYTES
RASTER_SYMBOLS = {
    "emap_raster_abi_version": (C.c_int, []),
    "emap_raster_workspace_bytes": (_RC, [C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_size_t)]),
    "emap_raster_edges": (_RC, [_P, C.c_int, _P, C.c_int, C.c_int, _P, _P, _P, _P, C.c_int, C.c_int, C.c_int, C.c_double, C.c_double, _P, _P, _P,
                                C.c_size_t, _P]),
}

# the four headers of the one library, each with its own table, version and pair of views: all that _view() and tests/test_headers_cpu.py
# know of them.  `constants`: the #defines this module mirrors, name -> Python value
HEADERS = {
    "main": dict(header="emap_hip.h", symbols=SYMBOLS, version_fn="emap_abi_version", version=ABI_VERSION, mismatch="libemap_hip.so ABI version mismatch",
                 constants={**{"EMAP_PREC_" + k.upper(): v for k, v in PRECISIONS.items()}, **{"EMAP_UDF_" + k.upper(): v for k, v in UDF_TYPES.items()},
                            "EMAP_MAX_LIN": MAX_LIN, "EMAP_MAX_TRAIN_IMAGES": MAX_TRAIN_IMAGES, "EMAP_MAX_SAMPLES_PER_RAY": MAX_SAMPLES_PER_RAY,
                            "EMAP_RENDER_UNBIASED": RENDER_UNBIASED, "EMAP_RENDER_UNBIASED_NORMCOS": RENDER_UNBIASED_NORMCOS, "EMAP_RENDER_PLAIN": RENDER_PLAIN,
                            "EMAP_F_NAN_SAMPLES": F_NAN_SAMPLES, "EMAP_F_NAN_GRADERR": F_NAN_GRADERR, "EMAP_F_MLP_NONFINITE": F_MLP_NONFINITE}),
    "eval": dict(header="emap_eval_hip.h", symbols=EVAL_SYMBOLS, version_fn="emap_eval_abi_version", version=EVAL_ABI_VERSION,
                 mismatch="libemap_hip.so evaluation ABI version mismatch (include/emap_eval_hip.h)",
                 constants={"EMAP_EVAL_POINTS_F64": EVAL_POINTS_DTYPES[torch.float64], "EMAP_EVAL_POINTS_F32": EVAL_POINTS_DTYPES[torch.float32],
                            **{"EMAP_EVAL_MAPS_" + k: EVAL_MAPS_DTYPES[t] for k, t in (("U8", torch.uint8), ("F32", torch.float32), ("F64", torch.float64))}}),
    "fit": dict(header="emap_fit_hip.h", symbols=FIT_SYMBOLS, version_fn="emap_fit_abi_version", version=FIT_ABI_VERSION,
                mismatch="libemap_hip.so fitting ABI version mismatch (include/emap_fit_hip.h)",
                constants={"EMAP_FIT_MAX_POLYLINE_POINTS": FIT_MAX_POLYLINE_POINTS, "EMAP_FIT_MAX_LINES": FIT_MAX_LINES, "EMAP_FIT_LINK_LDS_POINTS": FIT_LINK_LDS_POINTS}),
    "raster": dict(header="emap_raster_hip.h", symbols=RASTER_SYMBOLS, version_fn="emap_raster_abi_version", version=RASTER_ABI_VERSION,
                   mismatch="libemap_hip.so rasteriser ABI version mismatch (include/emap_raster_hip.h)",
                   constants={"EMAP_RASTER_MAX_CURVE_SEGMENTS": RASTER_MAX_CURVE_SEGMENTS, "EMAP_RASTER_MAX_SEGMENTS": RASTER_MAX_SEGMENTS,
                              "EMAP_RASTER_MAX_HALF_WIDTH": RASTER_MAX_HALF_WIDTH, "EMAP_RASTER_MAX_FRAMES": RASTER_MAX_FRAMES,
                              "EMAP_RASTER_MAX_DIM": RASTER_MAX_DIM, "EMAP_RASTER_ROW_BYTES": RASTER_ROW_BYTES}),
}

# every symbol include/emap_score_hip.h declares: the fifth header.  Its record has the fields of a HEADERS entry and sits beside that
# registry, not in it: _view() finds it under SCORE_KEY
SCORE_ABI_VERSION = 1
SCORE_MAX_DIM = 32768              # EMAP_SCORE_MAX_DIM
SCORE_MAX_FRAMES = 65535           # EMAP_SCORE_MAX_FRAMES
SCORE_MAX_THRESHOLDS = 8           # EMAP_SCORE_MAX_THRESHOLDS
SCORE_NONE = 2147483647            # EMAP_SCORE_NONE
SCORE_MAPS_DTYPES = {torch.uint8: 0, torch.float32: 1}      # EMAP_SCORE_MAPS_*
SCORE_WORKSPACE_PIXEL_BYTES = 2    # EMAP_SCORE_WORKSPACE_PIXEL_BYTES
SCORE_SYMBOLS = {
    "emap_score_abi_version": (C.c_int, []),
    "emap_score_workspace_bytes": (_RC, [C.c_int, C.c_int, C.c_int, C.POINTER(C.c_size_t)]),
    "emap_score_distance_maps": (_RC, [_P, C.c_int, C.c_double, C.c_int, C.c_int, C.c_int, _P, _P, C.c_size_t, _P]),
    "emap_score_stats": (_RC, [_P, C.c_int, C.c_double, _P, _P, C.c_int, C.POINTER(C.c_double), C.c_int, C.c_int, C.c_int, C.c_int, _P, _P, _P, _P]),
}
SCORE_KEY = "score"
SCORE_HEADER = dict(header="emap_score_hip.h", symbols=SCORE_SYMBOLS, version_fn="emap_score_abi_version", version=SCORE_ABI_VERSION,
                    mismatch="libemap_hip.so scoring ABI version mismatch (include/emap_score_hip.h)",
                    constants={"EMAP_SCORE_MAX_DIM": SCORE_MAX_DIM, "EMAP_SCORE_MAX_FRAMES": SCORE_MAX_FRAMES,
                               "EMAP_SCORE_MAX_THRESHOLDS": SCORE_MAX_THRESHOLDS, "EMAP_SCORE_NONE": SCORE_NONE,
                               "EMAP_SCORE_MAPS_U8": SCORE_MAPS_DTYPES[torch.uint8], "EMAP_SCORE_MAPS_F32": SCORE_MAPS_DTYPES[torch.float32],
                               "EMAP_SCORE_WORKSPACE_PIXEL_BYTES": SCORE_WORKSPACE_PIXEL_BYTES})
# every symbol include/emap_field_hip.h declares: the sixth header, a record of the same form
FIELD_ABI_VERSION = 1
FIELD_MAX_CURVE_SEGMENTS = 256     # EMAP_FIELD_MAX_CURVE_SEGMENTS
FIELD_MAX_SEGMENTS = 1 << 20       # EMAP_FIELD_MAX_SEGMENTS
FIELD_MAX_POINTS = 2147483647      # EMAP_FIELD_MAX_POINTS
FIELD_MAX_THRESHOLDS = 8           # EMAP_FIELD_MAX_THRESHOLDS
FIELD_POINTS_DTYPES = {torch.float64: 0, torch.float32: 1}      # EMAP_FIELD_POINTS_*
FIELD_SYMBOLS = {
    "emap_field_abi_version": (C.c_int, []),
    "emap_field_expand_edges": (_RC, [_P, C.c_int, _P, C.c_int, C.c_int, _P, _P, _P]),
    "emap_field_workspace_bytes": (_RC, [C.c_int64, C.c_int, C.c_int, C.POINTER(C.c_size_t)]),
    "emap_field_point_distances": (_RC, [_P, C.c_int, C.c_int64, _P, C.c_int, C.c_int, _P, _P, _P, _P, C.c_size_t, _P]),
    "emap_field_stats": (_RC, [_P, _P, C.c_int, C.POINTER(C.c_double), C.c_int, C.c_int64, _P, _P, _P, _P]),
}
FIELD_KEY = "field"
FIELD_HEADER = dict(header="emap_field_hip.h", symbols=FIELD_SYMBOLS, version_fn="emap_field_abi_version", version=FIELD_ABI_VERSION,
                    mismatch="libemap_hip.so distance-field ABI version mismatch (include/emap_field_hip.h)",
                    constants={"EMAP_FIELD_MAX_CURVE_SEGMENTS": FIELD_MAX_CURVE_SEGMENTS, "EMAP_FIELD_MAX_SEGMENTS": FIELD_MAX_SEGMENTS,
                               "EMAP_FIELD_MAX_POINTS": FIELD_MAX_POINTS, "EMAP_FIELD_MAX_THRESHOLDS": FIELD_MAX_THRESHOLDS,
                               "EMAP_FIELD_POINTS_F64": FIELD_POINTS_DTYPES[torch.float64], "EMAP_FIELD_POINTS_F32": FIELD_POINTS_DTYPES[torch.float32]})
_MORE_HEADERS = {SCORE_KEY: SCORE_HEADER, FIELD_KEY: FIELD_HEADER}      # records _view() knows beside HEADERS

_lib = None         # the loaded library; setting it to None makes the next call load it again (__graft_entry__.verify_library)
_views = {}         # header key -> (the library its symbols were bound on, its checked view)


class EmapLibraryError(RuntimeError):
    pass


class _Ptr:
    """argtype of the void* parameters of the checked view: None, an int, a c_void_p, a ctypes array, or anything with .data_ptr()
    (a tensor).  Only the address is taken: device, dtype and layout are the call site's business (require_cuda, f32c)."""

    @classmethod
    def from_param(cls, v):
        dp = getattr(v, "data_ptr", None)
        return C.c_void_p.from_param(v) if dp is None else C.c_void_p(dp())


def _errcheck(rc, fn, args):
    if rc != 0:
        check(rc, fn.__name__[5:])
    return rc


def _load():
    if not os.path.exists(LIB_PATH):
        raise EmapLibraryError(f"{LIB_PATH} not found: the HIP extension is not built. Run `python -c 'import __graft_entry__ as g; g.build()'` "
                               "(or emap_amd/csrc/build.sh). emap_amd has no CPU fallback.")
    try:
        return C.CDLL(LIB_PATH)
    except OSError as e:  # pragma: no cover
        raise EmapLibraryError(f"cannot load {LIB_PATH}: {e}") from e


def _bind(l, symbols):
    """Give every symbol of the table its restype / argtypes on the loaded library `l`; -> the checked view of the rc-returning ones."""
    a = types.SimpleNamespace()
    for name, (res, args) in symbols.items():
        try:
            fn = getattr(l, name)
        except AttributeError as e:
            raise EmapLibraryError(f"{LIB_PATH} does not export {name}") from e
        fn.restype = C.c_int if res is _RC else res
        fn.argtypes = args
        if res is _RC:
            ck = l[name]            # indexing makes a function object of its own; the attribute above is the cached raw one
            ck.restype, ck.argtypes, ck.errcheck = C.c_int, [_Ptr if t is _P else t for t in args], _errcheck
            setattr(a, name[5:], ck)
    return a


def _view(key):
    """(raw, checked) views of the header HEADERS[key] (or the record beside it): the library with the header's symbols bound, and one entry per rc-returning symbol.
    The main header's first use loads the library; a header is bound and its version checked on first use, and again after a reload."""
    global _lib
    l = _view("main")[0] if key != "main" else _lib if _lib is not None else _load()
    if key not in _views or _views[key][0] is not l:
        h = HEADERS[key] if key in HEADERS else _MORE_HEADERS[key]
        a = _bind(l, h["symbols"])
        if getattr(l, h["version_fn"])() != h["version"]:
            raise EmapLibraryError(h["mismatch"])
        _lib, _views[key] = l, (l, a)
    return _views[key]


def lib():
    """Load (once) and return the bound library: raw ctypes functions that return the rc.  Raises EmapLibraryError if it is not built."""
    return _view("main")[0]


def api():
    """The checked view of lib(): one entry per rc-returning symbol, named without ``emap_`` (``api().render_fwd``).  A call raises
    what check() raises when the rc is not 0; void* parameters take tensors (_Ptr) and struct parameters take the struct itself.
    Package code calls the library through this view; lib() is for code that looks at return codes."""
    return _view("main")[1]


def eval_lib():         # lib() with the symbols of include/emap_eval_hip.h bound as well (EVAL_SYMBOLS): the raw view of the second header
    return _view("eval")[0]


def eval_api():         # the checked view of eval_lib(): one entry per rc-returning symbol of EVAL_SYMBOLS, named without emap_; as api()
    return _view("eval")[1]


def fit_lib():         # lib() with the symbols of include/emap_fit_hip.h bound as well (FIT_SYMBOLS): the raw view of the third header
    return _view("fit")[0]


def fit_api():         # the checked view of fit_lib(): one entry per rc-returning symbol of FIT_SYMBOLS, named without emap_; as api()
    return _view("fit")[1]


def raster_lib():         # lib() with the symbols of include/emap_raster_hip.h bound as well (RASTER_SYMBOLS): the raw view of the fourth header
    return _view("raster")[0]


def raster_api():         # the checked view of raster_lib(): one entry per rc-returning symbol of RASTER_SYMBOLS, named without emap_; as api()
    return _view("raster")[1]


def score_lib():         # lib() with the symbols of include/emap_score_hip.h bound as well (SCORE_SYMBOLS): the raw view of the fifth header
    return _view(SCORE_KEY)[0]


def score_api():         # the checked view of score_lib(): one entry per rc-returning symbol of SCORE_SYMBOLS, named without emap_; as api()
    return _view(SCORE_KEY)[1]


def field_lib():         # lib() with the symbols of include/emap_field_hip.h bound as well (FIELD_SYMBOLS): the raw view of the sixth header
    return _view(FIELD_KEY)[0]


def field_api():         # the checked view of field_lib(): one entry per rc-returning symbol of FIELD_SYMBOLS, named without emap_; as api()
    return _view(FIELD_KEY)[1]


def size_of(query: str, *args) -> int:
    """The value of a size or offset query - a checked symbol whose last parameter is a size_t*: size_of("packed_bytes", cfg, prec)."""
    n = C.c_size_t()
    getattr(api(), query)(*args, n)
    return n.value


def check(rc: int, what: str = ""):
    if rc != 0:
        msg = lib().emap_last_error().decode("utf-8", "replace")
        raise RuntimeError(f"libemap_hip {what} failed (rc={rc}): {msg}")


def require_cuda(t: torch.Tensor, name: str):
    if not t.is_cuda:
        raise RuntimeError(
            f"emap_amd: `{name}` is on {t.device}; the HIP path needs tensors on an MI355X (cuda) device. "
            "There is no CPU fallback.")


def ptr(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def stream_ptr(device=None):
    """Current stream of `device` (default: the current device).  Callers that take tensors from an explicit device wrap the
    C call in ``torch.cuda.device(t.device)`` and pass ``t.device`` here, so kernels land on the tensor's device and stream."""
    return C.c_void_p(torch.cuda.current_stream(device).cuda_stream)


def on_device(t: torch.Tensor):
    """Context manager: make t's device current for the C call (kernel launches and the per-function LDS attribute are per device)."""
    return torch.cuda.device(t.device)


def f32c(t: torch.Tensor) -> torch.Tensor:
    """fp32 contiguous view/copy (the kernels' only layout)."""
    if t.dtype != torch.float32:
        t = t.float()
    return t.contiguous()
