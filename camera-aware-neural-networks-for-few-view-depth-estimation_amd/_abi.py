"""ctypes binding of include/cad/cad.h (libcad_hip.so, built in-tree for gfx950).

This is the ONLY way the Python host reaches device code: there is no CPU fallback.  If the shared
library is missing the import fails loudly (run `make -C <package dir>` or __graft_entry__.build()).
"""
from __future__ import annotations

import ctypes as C
import os
import re

PKG_DIR = os.path.dirname(os.path.abspath(__file__))
# CAD_LIB selects an A/B variant build (make VARIANT=... -> libcad_hip_<variant>.so) for tuning runs
LIB_PATH = os.path.join(PKG_DIR, os.environ.get("CAD_LIB", "libcad_hip.so"))
HEADER = os.path.join(os.path.dirname(PKG_DIR), "include", "cad", "cad.h")

P = C.c_void_p
F = C.c_float
I = C.c_int
I64 = C.c_int64
FP = C.POINTER(C.c_float)
I64P = C.POINTER(C.c_int64)
DP = C.POINTER(C.c_double)


class UnetDesc(C.Structure):
    _fields_ = [("in_channels", I), ("init_features", I), ("max_depth", F), ("max_batch", I),
                ("height", I), ("width", I)]


class ResUnetDesc(C.Structure):
    _fields_ = [("in_channels", I), ("max_batch", I), ("height", I), ("width", I), ("max_depth", F)]


class GeoNetDesc(C.Structure):
    _fields_ = [("variant", I), ("in_channels", I), ("init_features", I), ("camera_dim", I), ("max_depth", F),
                ("use_pcl", I), ("use_attention", I), ("max_batch", I), ("height", I), ("width", I)]


class AdamOpts(C.Structure):
    _fields_ = [("lr", F), ("beta1", F), ("beta2", F), ("eps", F), ("weight_decay", F)]


OPTIM_RULES = {"adam": 0, "adamw": 1, "sgd": 2}   # CAD_OPTIM_*


class OptimOpts(C.Structure):
    """cad_optim_opts (cad.h)."""
    _fields_ = [("rule", I), ("lr", F), ("beta1", F), ("beta2", F), ("eps", F), ("weight_decay", F), ("momentum", F),
                ("ema_decay", F)]


class LrOpts(C.Structure):
    """cad_lr_opts (cad.h)."""
    _fields_ = [("lr", F), ("scheduler", C.c_char_p), ("step_size", I), ("gamma", F), ("warmup_epochs", I),
                ("lr_min", F)]


class CommStats(C.Structure):
    """cad_comm_stats (cad.h): exchange accounting of the overlapped backward all-reduce."""
    _fields_ = [("calls", I64), ("timed_calls", I64), ("buckets", I64), ("bytes", I64), ("exposed_ms", C.c_double),
                ("span_ms", C.c_double)]


class ArchiveEntry(C.Structure):
    """cad_archive_entry (cad.h): one tensor / empty submodule of a torch::save archive."""
    _fields_ = [("name", C.c_char_p), ("kind", I), ("dtype", I), ("ndim", I), ("shape", C.c_int64 * 8),
                ("data", C.c_void_p)]


class EvalConfig(C.Structure):
    """cad_eval_config (cad.h): DepthMetrics::compute's depth range and prediction clamp."""
    _fields_ = [("min_depth", F), ("max_depth", F), ("clamp_pred", I)]


EVAL_KEYS = ("abs_rel", "sq_rel", "rmse", "rmse_log", "mae", "log10", "delta_1.25", "delta_1.25^2", "delta_1.25^3",
             "num_valid_pixels", "mean_pred_depth", "mean_gt_depth")


EVAL_ALIGN = {"none": 0, "median": 1, "log_mean": 2, "scale_shift": 3}   # cad_eval_align


def eval_align_mode(align) -> int:
    """cad_eval_align value of a mode name; ValueError for anything else (no device call)."""
    if not isinstance(align, str) or align not in EVAL_ALIGN:
        raise ValueError(f"align must be one of {tuple(EVAL_ALIGN)}, not {align!r}")
    return EVAL_ALIGN[align]


class EvalSummary(C.Structure):
    """cad_eval_summary (cad.h)."""
    _fields_ = [("count", I64)] + [(k, F * 12) for k in ("mean", "std", "median", "min", "max", "pooled")]


GEOM_SUMS = 8      # CAD_GEOM_SUMS
GEOM_KEYS = ["normal_mean", "normal_median", "normal_rmse", "normal_11.25", "normal_22.5", "normal_30",
             "num_normal_pixels", "point_mae", "point_rmse"]   # cad.h's CAD_GEOM_METRICS order


class GeomSummary(C.Structure):
    """cad_geom_summary (cad.h)."""
    _fields_ = [("count", I64), ("count_normal", I64), ("count_point", I64)] + \
               [(k, F * 9) for k in ("mean", "std", "median", "min", "max", "pooled")]


STRATA_MAX_BINS = 16                    # CAD_STRATA_MAX_BINS
STRATA_AXES = {"depth": 0, "angle": 1}  # CAD_STRATA_DEPTH / CAD_STRATA_ANGLE


class StrataConfig(C.Structure):
    """cad_strata_config (cad.h): the depth cuts in metres and the angle cuts in degrees; 0 cuts: axis off."""
    _fields_ = [("n_depth_cuts", I), ("depth_cuts", F * (STRATA_MAX_BINS - 1)), ("n_angle_cuts", I),
                ("angle_cuts_deg", F * (STRATA_MAX_BINS - 1))]


def strata_config(depth_bins=None, angle_bins=None) -> "StrataConfig":
    """cad_strata_config of two cut lists (None or empty: that axis is off).  Only what the fixed-size struct
    cannot hold is refused here (ValueError naming the count); every other rule is the library's."""
    cfg = StrataConfig()
    for name, cuts, n_field, field in (("depth_bins", depth_bins, "n_depth_cuts", "depth_cuts"),
                                       ("angle_bins", angle_bins, "n_angle_cuts", "angle_cuts_deg")):
        cuts = [] if cuts is None else [float(c) for c in cuts]
        if len(cuts) > STRATA_MAX_BINS - 1:
            raise ValueError(f"{name}: {len(cuts)} cuts given, at most {STRATA_MAX_BINS - 1} ({STRATA_MAX_BINS} bins)")
        setattr(cfg, n_field, len(cuts))
        for j, c in enumerate(cuts):
            getattr(cfg, field)[j] = c
    return cfg


def strata_axis(axis) -> int:
    if axis not in STRATA_AXES:
        raise ValueError(f"axis must be one of {tuple(STRATA_AXES)}, not {axis!r}")
    return STRATA_AXES[axis]


class View(C.Structure):
    """cad_view (cad.h, "virtual cameras"): a change of intrinsics and a rotation about the camera centre."""
    _fields_ = [("zoom_x", F), ("zoom_y", F), ("shift_x", F), ("shift_y", F), ("yaw_deg", F), ("pitch_deg", F),
                ("roll_deg", F)]

    def __repr__(self):
        return "View(" + ", ".join(f"{k}={getattr(self, k):g}" for k, _ in self._fields_) + ")"

    def as_dict(self) -> dict:
        return {k: float(getattr(self, k)) for k, _ in self._fields_}


VIEW_AXES = ("zoom", "zoom_x", "zoom_y", "shift_x", "shift_y", "yaw", "pitch", "roll")   # build/evaluate --camera-sweep


def view(zoom=None, zoom_x=1.0, zoom_y=1.0, shift_x=0.0, shift_y=0.0, yaw=0.0, pitch=0.0, roll=0.0) -> "View":
    """A cad_view: zoom sets both zoom fields; angles in degrees.  What the library refuses (a non-finite field,
    a non-positive zoom, an angle of magnitude >= 80 degrees) raises ValueError with its message; no device call."""
    if zoom is not None:
        zoom_x = zoom_y = zoom
    v = View(*(float(x) for x in (zoom_x, zoom_y, shift_x, shift_y, yaw, pitch, roll)))
    lib = load()
    if lib.cad_view_check(C.byref(v)) != 0:
        raise ValueError(lib.cad_last_error().decode(errors="replace"))
    return v


def view_label(axis, value) -> str:
    """'zoom:1.5': the label build/evaluate gives the view of one --camera-sweep value (%.7g of the fp32 number)."""
    return f"{axis}:{C.c_float(float(value)).value:.7g}"


def sweep_views(camera_sweep) -> list:
    """{"zoom": [0.7, 1.5], "yaw": [-7, 7]} -> [(label, View)], one view per value with every other field neutral,
    in the mapping's order.  ValueError for an unknown axis, an empty list or a refused value; no device call."""
    out = []
    for axis, values in dict(camera_sweep).items():
        if axis not in VIEW_AXES:
            raise ValueError(f"camera_sweep axis must be one of {VIEW_AXES}, not {axis!r}")
        values = [values] if isinstance(values, (int, float)) else list(values)
        if not values:
            raise ValueError(f"camera_sweep axis {axis!r}: no values")
        for val in values:
            out.append((view_label(axis, val), view(**{axis: val})))
    return out


def view_rotation(v: "View"):
    """cad_view_rotation (host only): the view's R = Rz(roll) Rx(pitch) Ry(yaw), (3, 3) float32, P' = R P."""
    import numpy as np
    R = np.zeros((3, 3), np.float32)
    check(load().cad_view_rotation(C.byref(v), R.ctypes.data_as(FP)), "cad_view_rotation")
    return R


COLORMAPS = {"gray": 0, "jet": 1, "hot": 2}   # CAD_CMAP_*; 3 = CAD_CMAP_CUSTOM (cad_exporter_set_lut)
CMAP_CUSTOM = 3


class RenderOpts(C.Structure):
    """cad_render_opts (cad.h)."""
    _fields_ = [("colormap", I), ("fixed_range", I), ("lo", F), ("hi", F), ("invalid", C.c_uint8 * 3),
                ("row_stride", I64), ("col_offset", I64), ("image_stride", I64), ("units_per_metre", F)]


class HistSegment(C.Structure):
    """cad_hist_segment (cad.h): element i of base[offset : offset + count] counts iff r = i % period < keep
    (and, with an inner rule, r % inner_period < inner_keep)."""
    _fields_ = [("offset", I64), ("count", I64), ("period", I64), ("keep", I64), ("inner_period", I64), ("inner_keep", I64)]


HIST_BINS = 1548    # CAD_HIST_BINS
HIST_STATS = ("num", "min", "max", "sum", "sum_squares", "nonfinite")   # a row of cad_hist_read

# name: (restype, argtypes)
SIGNATURES = {
    "cad_abi_version": (I, []),
    "cad_last_error": (C.c_char_p, []),
    "cad_device_count": (I, [C.POINTER(I)]),
    "cad_set_device": (I, [I]),
    "cad_stream_synchronize": (I, [P]),
    "cad_malloc": (I, [I, I64, C.POINTER(P)]),
    "cad_free": (None, [P]),
    "cad_memcpy": (I, [P, P, I64, I, P]),
    "cad_adam_state": (I, [P, C.POINTER(P), C.POINTER(P)]),
    "cad_adam_set_step_count": (I, [P, I64]),
    "cad_set_gemm_engine": (I, [I]),
    "cad_set_alias_check": (I, [I]),
    "cad_alias_views_overlap": (I, [P, I64, I64, I64, I64, I, P, I64, I64, I64, I64, I]),
    "cad_get_gemm_engine": (I, []),
    "cad_unet_create": (I, [C.POINTER(UnetDesc), I, C.POINTER(P)]),
    "cad_resunet_create": (I, [C.POINTER(ResUnetDesc), I, C.POINTER(P)]),
    "cad_resunet_destroy": (None, [P]),
    "cad_resunet_count_parameters": (I64, [P]),
    "cad_resunet_num_tensors": (I, [P, I]),
    "cad_resunet_tensor_info": (I, [P, I, I, C.POINTER(C.c_char_p), C.POINTER(I), I64P]),
    "cad_resunet_set_tensor": (I, [P, I, I, FP, I64]),
    "cad_resunet_get_tensor": (I, [P, I, I, FP, I64]),
    "cad_resunet_get_grad": (I, [P, I, FP, I64]),
    "cad_resunet_train": (I, [P, I]),
    "cad_resunet_set_fp8": (I, [P, I]),
    "cad_resunet_fp8_units": (I, [P]),
    "cad_resunet_flat": (I, [P, C.POINTER(P), C.POINTER(P), I64P]),
    "cad_resunet_forward": (I, [P, P, P, I, P]),
    "cad_resunet_backward": (I, [P, P, P]),
    "cad_resunet_num_stages": (I, [P]),
    "cad_resunet_debug_buffer": (I64, [P, C.c_char_p, FP, I64]),
    "cad_resunet_grad_layout": (I, [C.POINTER(I), I64P, I64P, I64P]),
    "cad_resunet_stage_grad_range": (I, [P, I, I64P, I64P]),
    "cad_resunet_backward_stage": (I, [P, I, P, P]),
    "cad_resunet_backward_allreduce": (I, [P, P, P, I64, P]),
    "cad_resunet_clip_grad_norm": (I, [P, F, F, P]),
    "cad_resunet_last_grad_norm": (I, [P, FP, P]),
    "cad_resunet_adam_step": (I, [P, F, F, F, F, F, P]),
    "cad_geonet_create": (I, [C.POINTER(GeoNetDesc), I, C.POINTER(P)]),
    "cad_geonet_destroy": (None, [P]),
    "cad_geonet_count_parameters": (I64, [P]),
    "cad_geonet_num_tensors": (I, [P, I]),
    "cad_geonet_tensor_info": (I, [P, I, I, C.POINTER(C.c_char_p), C.POINTER(I), I64P]),
    "cad_geonet_set_tensor": (I, [P, I, I, FP, I64]),
    "cad_geonet_get_tensor": (I, [P, I, I, FP, I64]),
    "cad_geonet_get_grad": (I, [P, I, FP, I64]),
    "cad_geonet_train": (I, [P, I]),
    "cad_geonet_flat": (I, [P, C.POINTER(P), C.POINTER(P), I64P]),
    "cad_geonet_forward": (I, [P, P, P, P, P, I, P]),
    "cad_geonet_backward": (I, [P, P, P]),
    "cad_geonet_num_stages": (I, [P]),
    "cad_geonet_grad_layout": (I, [C.POINTER(GeoNetDesc), C.POINTER(I), I64P, I64P, I64P]),
    "cad_geonet_stage_grad_range": (I, [P, I, I64P, I64P]),
    "cad_geonet_backward_stage": (I, [P, I, P, P]),
    "cad_geonet_backward_allreduce": (I, [P, P, P, I64, P]),
    "cad_geonet_clip_grad_norm": (I, [P, F, F, P]),
    "cad_geonet_last_grad_norm": (I, [P, FP, P]),
    "cad_geonet_adam_step": (I, [P, F, F, F, F, F, P]),
    "cad_geonet_num_batches_tracked": (I64, [P, I]),
    "cad_geonet_debug_buffer": (I64, [P, C.c_char_p, FP, I64]),
    "cad_op_cbam": (I, [P, P, P, I, I, I, I, P, P, P, P]),
    "cad_op_pcl": (I, [P, P, P, P, I, I, I, I, P, P, P, P, P]),
    "cad_op_cbam_head": (I, [P, I, P, P, P, P, P, F, P, I, I, I, I, I, P, P, P, P, P, P, FP, P]),
    "cad_unet_create_model": (I, [C.POINTER(UnetDesc), I, I, C.POINTER(P)]),
    "cad_unet_model": (I, [P]),
    "cad_unet_forward_cam": (I, [P, P, P, P, I, P]),
    "cad_camera_from_K": (I, [P, I, P, P]),
    "cad_unet_destroy": (None, [P]),
    "cad_unet_count_parameters": (I64, [P]),
    "cad_unet_num_params": (I, [P]),
    "cad_unet_num_buffers": (I, [P]),
    "cad_unet_tensor_info": (I, [P, I, I, C.POINTER(C.c_char_p), C.POINTER(I), I64P]),
    "cad_unet_set_tensor": (I, [P, I, I, FP, I64]),
    "cad_unet_get_tensor": (I, [P, I, I, FP, I64]),
    "cad_unet_get_grad": (I, [P, I, FP, I64]),
    "cad_unet_train": (I, [P, I]),
    "cad_unet_set_fused_eval": (I, [P, I]),
    "cad_unet_get_fused_eval": (I, [P]),
    "cad_unet_fused_eval_convs": (I, [P, C.POINTER(I), C.POINTER(I)]),
    "cad_unet_flat": (I, [P, C.POINTER(P), C.POINTER(P), I64P]),
    "cad_unet_use_external_slabs": (I, [P, P, P]),
    "cad_unet_forward": (I, [P, P, P, I, P]),
    "cad_unet_backward": (I, [P, P, P]),
    "cad_unet_num_stages": (I, [P]),
    "cad_unet_backward_stage": (I, [P, I, P, P]),
    "cad_unet_stage_grad_range": (I, [P, I, I64P, I64P]),
    "cad_clip_grad_norm": (I, [P, F, F, P]),
    "cad_unet_last_grad_norm": (I, [P, FP, P]),
    "cad_adam_create": (I, [P, C.POINTER(AdamOpts), C.POINTER(P)]),
    "cad_adam_destroy": (None, [P]),
    "cad_adam_step": (I, [P, P]),
    "cad_adam_set_lr": (I, [P, F]),
    "cad_adam_step_count": (I64, [P]),
    "cad_optim_create": (I, [P, C.POINTER(OptimOpts), C.POINTER(P)]),
    "cad_optim_destroy": (None, [P]),
    "cad_optim_step": (I, [P, P]),
    "cad_optim_set_lr": (I, [P, F]),
    "cad_optim_lr": (F, [P]),
    "cad_optim_rule": (I, [P]),
    "cad_optim_step_count": (I64, [P]),
    "cad_optim_set_step_count": (I, [P, I64]),
    "cad_optim_state": (I, [P, C.POINTER(P), C.POINTER(P), C.POINTER(P)]),
    "cad_optim_attach_ema": (I, [P, F, P]),
    "cad_optim_ema_swap": (I, [P, P]),
    "cad_optim_swapped": (I, [P]),
    "cad_geonet_optim_step": (I, [P, C.POINTER(OptimOpts), P]),
    "cad_lr_at": (I, [C.POINTER(LrOpts), I, I, FP]),
    "cad_loss_create": (I, [F, F, F, F, I, I, I, I, C.POINTER(P)]),
    "cad_loss_destroy": (None, [P]),
    "cad_loss_forward_backward": (I, [P, P, P, P, P, I, P, P, P]),
    "cad_loss_get_components": (I, [P, FP, P]),
    "cad_depth_metrics": (I, [P, P, I, I, I, FP, P]),
    "cad_event_create": (I, [C.POINTER(P)]),
    "cad_event_destroy": (None, [P]),
    "cad_event_record": (I, [P, P]),
    "cad_event_elapsed_ms": (I, [P, P, FP]),
    "cad_evaluator_create": (I, [I64, I, I, I, C.POINTER(EvalConfig), I, C.POINTER(P)]),
    "cad_evaluator_destroy": (None, [P]),
    "cad_evaluator_reset": (I, [P]),
    "cad_evaluator_update": (I, [P, P, P, P, I, P]),
    "cad_evaluator_count": (I64, [P]),
    "cad_evaluator_sums": (I, [P, C.POINTER(C.c_double), P]),
    "cad_evaluator_metrics": (I, [P, FP, C.POINTER(EvalSummary)]),
    "cad_eval_finish": (I, [C.POINTER(C.c_double), I64, FP, C.POINTER(EvalSummary)]),
    "cad_evaluator_set_strata": (I, [P, C.POINTER(StrataConfig)]),
    "cad_evaluator_update_k": (I, [P, P, P, P, P, I, P]),
    "cad_evaluator_strata_bins": (I, [P, I]),
    "cad_evaluator_strata_sums": (I, [P, I, C.POINTER(C.c_double), P]),
    "cad_strata_angle_thresholds": (I, [FP, I, FP]),
    "cad_eval_strata_finish": (I, [C.POINTER(C.c_double), I64, I, FP, C.POINTER(EvalSummary)]),
    "cad_evaluator_set_geometry": (I, [P, I]),
    "cad_evaluator_get_geometry": (I, [P]),
    "cad_evaluator_geom_sums": (I, [P, C.POINTER(C.c_double), P]),
    "cad_evaluator_geom_medians": (I, [P, FP, P]),
    "cad_eval_geom_finish": (I, [C.POINTER(C.c_double), FP, C.POINTER(C.c_double), I64, FP, C.POINTER(GeomSummary)]),
    "cad_depth_normals": (I, [P, P, P, I, I, I, F, F, P, P, P]),
    "cad_evaluator_set_alignment": (I, [P, I]),
    "cad_evaluator_get_alignment": (I, [P]),
    "cad_evaluator_alignment": (I, [P, FP, P]),
    "cad_evaluator_aligned": (I, [P, C.POINTER(C.c_uint8), P]),
    "cad_valid_medians": (I, [P, P, P, I, I, I, F, F, P, P]),
    "cad_eval_solve_alignment": (I, [I, C.POINTER(C.c_double), FP, FP]),
    "cad_ray_directions": (I, [P, I, I, I, P, P]),
    "cad_view_check": (I, [C.POINTER(View)]),
    "cad_view_rotation": (I, [C.POINTER(View), FP]),
    "cad_view_resolve": (I, [C.POINTER(View), P, I, I, I, P, P, P]),
    "cad_camera_view": (I, [P, P, P, P, P, P, I, I, I, P, P, P, P]),
    "cad_unet_debug_buffer": (I64, [P, C.c_char_p, FP, I64]),
    "cad_profile_enable": (I, [I]),
    "cad_profile_reset": (I, []),
    "cad_profile_only": (I, [C.c_char_p]),
    "cad_profile_report": (I, [C.c_char_p, I]),
    "cad_op_conv3x3_fwd": (I, [P, I64, I, I, P, I, P, I64, I, I, I, I, P]),
    "cad_op_conv3x3_dgrad": (I, [P, I, P, I, P, I64, I, I, I, P]),
    "cad_op_conv3x3_wgrad": (I, [P, I, P, I64, I, I, P, I, I, I, P]),
    "cad_op_conv3x3_wgrad_bf16": (I, [P, I64, I, P, I64, I, I, P, I, I, I, P]),
    "cad_op_conv3x3_fwd_bf16": (I, [P, I64, I, I, P, I, P, I64, I, I, I, I, I, I, P]),
    "cad_op_conv3x3_dgrad_bf16": (I, [P, I64, I, P, I, P, I64, I, I, I, I, P]),
    "cad_op_conv3x3_fwd_act": (I, [P, I64, I, I, P, I, P, P, P, P, P, I64, I, I, I, I, I, P]),
    "cad_op_conv3x3_fwd_act_bf16": (I, [P, I64, I, I, P, I, P, P, P, P, P, I64, I, I, I, I, I, P]),
    "cad_op_mx8_quantize": (I, [P, I, I64, I, I, I64, P, P, I64, I, P]),
    "cad_op_dense_x8": (I, [P, P, I64, I, P, P, I64, I, P, I64, P]),
    "cad_op_conv3x3_x8": (I, [P, P, I64, I, P, P, I64, I, P, I, I, I, P]),
    "cad_op_convT_fwd": (I, [P, I, P, P, I, P, I64, I, I, I, I, P]),
    "cad_op_convT_fwd_bf16": (I, [P, I64, I, I, P, P, I, P, I64, I, I, I, I, P]),
    "cad_op_convT_dgrad": (I, [P, I64, I, I, P, I, P, I, I, I, P]),
    "cad_op_convT_wgrad": (I, [P, I, P, I64, I, I, P, I, I, I, P]),
    "cad_op_maxpool_fwd": (I, [P, I64, I, I, I, I, P, P, P]),
    "cad_op_dense_fwd_bf16": (I, [P, I64, I, I, P, I64, I, I, P, I64, I, I, P, I64, P, P, P, I64, P]),
    "cad_op_dense_wgrad_bf16": (I, [P, I64, I, I, P, I64, I, I, P, I64, I64, I64, P]),
    "cad_op_im2col": (I, [P, I, I64, I, I, I, I, I, I, I, I, I, P, I, P]),
    "cad_op_col2im": (I, [P, I, I, I, I, I, I, I, I, I, P, I64, P]),
    "cad_op_maxpool3s2_fwd": (I, [P, I, I, I, I, P, P, P, P]),
    "cad_op_maxpool3s2_bwd": (I, [P, P, I, I, I, I, P, P, I64, P]),
    "cad_op_bn_add_relu": (I, [P, I, P, P, P, P, P, P, I64, I, I64, P, P, P, P, I64, P]),
    "cad_op_relu_mask": (I, [P, I64, I, P, I, I64, P, P]),
    "cad_op_mask_inplace": (I, [P, I64, I, P, I, I64, P]),
    "cad_op_add_strided": (I, [P, I64, P, I64, I, I, I, I, I, I, P]),
    "cad_op_copy_twin": (I, [P, I64, I, I, I, I, I, I, P, I64, I, P]),
    "cad_op_transpose_split": (I, [P, I64, I, I, P, P]),
    "cad_batcher_create": (I, [I, I, I, I, C.POINTER(P)]),
    "cad_batcher_destroy": (None, [P]),
    "cad_batcher_assemble": (I, [P, C.c_void_p, I, P, P, P, P]),
    "cad_aug_sampler_create": (I, [C.c_void_p, C.c_uint32, C.POINTER(P)]),
    "cad_aug_sampler_destroy": (None, [P]),
    "cad_aug_sampler_draw": (I, [P, I, I, C.c_void_p]),
    "cad_color_matrix": (I, [F, F, FP]),
    "cad_loss_forward_backward_masked": (I, [P, P, P, P, P, P, I, P, P, P]),
    "cad_comm_get_unique_id": (I, [C.c_void_p]),
    "cad_comm_create": (I, [C.c_void_p, I, I, I, C.POINTER(P)]),
    "cad_comm_destroy": (None, [P]),
    "cad_comm_rank": (I, [P]),
    "cad_comm_size": (I, [P]),
    "cad_comm_set_timing": (I, [P, I]),
    "cad_comm_stats_read": (I, [P, P]),
    "cad_comm_allreduce": (I, [P, P, I64, I, P]),
    "cad_comm_broadcast": (I, [P, P, I64, I, P]),
    "cad_comm_broadcast_params": (I, [P, P, I, P]),
    "cad_grad_allreduce": (I, [P, P, P]),
    "cad_unet_backward_allreduce": (I, [P, P, P, I64, P]),
    "cad_plan_grad_buckets": (I, [I64P, I64P, I, I64, I64P, I64P, C.POINTER(I)]),
    "cad_model_grad_layout": (I, [I, I, I, C.POINTER(I), I64P, I64P, I64P]),
    "cad_unet_save_torch": (I, [P, C.c_char_p]),
    "cad_unet_load_torch": (I, [P, C.c_char_p]),
    "cad_unet_num_batches_tracked": (I64, [P]),
    "cad_archive_write": (I, [C.c_char_p, C.POINTER(ArchiveEntry), I]),
    "cad_archive_open": (I, [C.c_char_p, C.POINTER(P)]),
    "cad_archive_close": (None, [P]),
    "cad_archive_count": (I, [P]),
    "cad_archive_find": (I, [P, C.c_char_p]),
    "cad_archive_info": (I, [P, I, C.POINTER(C.c_char_p), C.POINTER(I), C.POINTER(I), I64P]),
    "cad_archive_read": (I, [P, I, P, I64]),
    "cad_dataset_open": (I, [C.c_char_p, C.POINTER(C.c_char_p), I, C.POINTER(P)]),
    "cad_dataset_synthetic": (I, [I64, I, I, C.c_uint32, C.POINTER(P)]),
    "cad_jpeg_decode": (I, [P, I64, P, I64, C.POINTER(I), C.POINTER(I), C.POINTER(I)]),
    "cad_dataset_destroy": (None, [P]),
    "cad_dataset_size": (I64, [P]),
    "cad_dataset_image_dir": (C.c_char_p, [P, I64]),
    "cad_dataset_sensor": (C.c_char_p, [P, I64]),
    "cad_dataset_read": (I, [P, I64, P, I64, P, I64, P]),
    "cad_loader_create": (I, [P, I, I, I, P, C.c_uint32, I, I, I, C.POINTER(P)]),
    "cad_loader_destroy": (None, [P]),
    "cad_loader_start_epoch": (I, [P, I64P, I64]),
    "cad_loader_next": (I, [P, P, P, P, P]),
    "cad_colormap_lut": (I, [C.c_char_p, P]),
    "cad_exporter_create": (I, [I, I, I, I, C.POINTER(P)]),
    "cad_exporter_destroy": (None, [P]),
    "cad_exporter_set_lut": (I, [P, P]),
    "cad_exporter_range": (I, [P, P, P, P, I, P, P]),
    "cad_exporter_render": (I, [P, P, P, P, I, C.POINTER(RenderOpts), P, P, P]),
    "cad_exporter_image": (I, [P, P, I, C.POINTER(RenderOpts), P, P]),
    "cad_exporter_normals": (I, [P, P, P, P, I, C.POINTER(RenderOpts), P, P]),
    "cad_exporter_points": (I, [P, P, P, P, P, I, I, F, F, P, P, P]),
    "cad_hflip": (I, [P, P, I64, I, I, P]),
    "cad_flip_mean": (I, [P, P, P, I64, I, I, P]),
    "cad_png_encode": (I, [P, I, I, I, I, P, I64, I64P]),
    "cad_png_decode": (I, [P, I64, P, I64, C.POINTER(I), C.POINTER(I), C.POINTER(I), C.POINTER(I)]),
    "cad_ply_write": (I, [C.c_char_p, P, I64]),
    "cad_crc32c": (C.c_uint32, [P, I64]),
    "cad_crc32c_masked": (C.c_uint32, [P, I64]),
    "cad_tb_open": (I, [C.c_char_p, C.POINTER(P)]),
    "cad_tb_close": (None, [P]),
    "cad_tb_flush": (I, [P]),
    "cad_tb_path": (C.c_char_p, [P]),
    "cad_tb_hparams_path": (C.c_char_p, [P]),
    "cad_tb_scalar": (I, [P, C.c_char_p, F, I64]),
    "cad_tb_histogram": (I, [P, C.c_char_p, I64, DP, DP, DP, I]),
    "cad_tb_image": (I, [P, C.c_char_p, I64, I, I, I, P, I64]),
    "cad_tb_text": (I, [P, C.c_char_p, I64, C.c_char_p]),
    "cad_tb_custom_scalars": (I, [P, C.POINTER(C.c_char_p), C.POINTER(C.c_char_p), C.POINTER(C.c_char_p), I]),
    "cad_tb_hparams": (I, [P, C.POINTER(C.c_char_p), DP, I, C.POINTER(C.c_char_p), FP, I, C.c_char_p]),
    "cad_tb_default_bins": (I, [DP, I]),
    "cad_tb_trim_histogram": (I, [C.POINTER(C.c_uint32), I, DP, DP, DP, C.POINTER(I)]),
    "cad_hist_create": (I, [C.POINTER(HistSegment), I, I, C.POINTER(P)]),
    "cad_hist_destroy": (None, [P]),
    "cad_hist_num_segments": (I, [P]),
    "cad_hist_run": (I, [P, P, P]),
    "cad_hist_read": (I, [P, DP, C.POINTER(C.c_uint32)]),
    "cad_unet_histograms": (I, [P, I, P, C.POINTER(P)]),
    "cad_resunet_histograms": (I, [P, I, P, C.POINTER(P)]),
    "cad_geonet_histograms": (I, [P, I, P, C.POINTER(P)]),
}


class Sample(C.Structure):
    """cad_sample (cad.h): one decoded sample and its augmentation parameters."""
    _fields_ = [("rgb", P), ("depth", P), ("h0", I), ("w0", I), ("bgr", I), ("depth_scale", F),
                ("K", F * 9), ("aug", I), ("crop", I), ("crop_scale", F), ("crop_x", I), ("crop_y", I),
                ("flip", I), ("jitter", I), ("brightness", F), ("contrast", F), ("dh0", I), ("dw0", I),
                ("color", I), ("saturation", F), ("hue", F), ("gamma_on", I), ("gamma", F)]


class DecodedInfo(C.Structure):
    """cad_decoded_info (cad.h)."""
    _fields_ = [("h0", I), ("w0", I), ("dh0", I), ("dw0", I), ("depth_scale", F), ("K", F * 9)]


class AugConfig(C.Structure):
    """cad_aug_config = AugmentationConfig (sunrgbd_loader.h:30-42), defaults as there; the declared stages
    (saturation_delta, hue_delta, enable_random_gamma, gamma_min, gamma_max) default to 0 / off."""
    _fields_ = [("enable_random_crop", I), ("crop_scale_min", F), ("crop_scale_max", F),
                ("enable_horizontal_flip", I), ("horizontal_flip_prob", F), ("enable_color_jitter", I),
                ("brightness_delta", F), ("contrast_delta", F), ("saturation_delta", F), ("hue_delta", F),
                ("enable_random_gamma", I), ("gamma_min", F), ("gamma_max", F)]

    def __init__(self, **kw):
        d = dict(enable_random_crop=1, crop_scale_min=0.7, crop_scale_max=1.0, enable_horizontal_flip=1,
                 horizontal_flip_prob=0.5, enable_color_jitter=1, brightness_delta=0.2, contrast_delta=0.2)
        d.update(kw)
        super().__init__(**d)


class CadError(RuntimeError):
    pass


def header_functions(path: str = HEADER):
    """Every function name declared in include/cad/cad.h."""
    with open(path) as fh:
        text = fh.read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(cad_[A-Za-z0-9_]+)\s*\(", text)))


_lib = None


def load():
    """Load libcad_hip.so (fails loudly if it was not built)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError(f"libcad_hip.so not built at {LIB_PATH}: run `make -C {PKG_DIR}` "
                          "(or __graft_entry__.build()); there is no CPU fallback")
    lib = C.CDLL(LIB_PATH)
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name, None)
        if fn is None:
            if "CAD_LIB" in os.environ:   # an older A/B variant build (tools/ab_step.py): no such entry point
                continue
            raise AttributeError(f"{LIB_PATH} does not export {name} (stale build? run make)")
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib


def check(status: int, what: str = ""):
    if status != 0:
        msg = load().cad_last_error().decode(errors="replace")
        raise CadError(f"{what} failed (status {status}): {msg}")
