"""ctypes binding of libcalib_ba_hip.so (include/cba.h) and the Python host mirror of the reference's
``OptimizeJointly`` entry point.

The library is hand-written HIP for gfx950; there is no CPU fallback -- importing works anywhere, but
every compute call raises :class:`EngineError` when the shared object or a GPU is missing.
"""
from __future__ import annotations

import ctypes as C
import os
from dataclasses import dataclass
from typing import Callable, List, Optional, Sequence

import numpy as np

from .problem import CENTRAL_GENERIC, Camera, Problem, State

_HERE = os.path.dirname(os.path.abspath(__file__))
# CBA_HIP_LIB: another build of the same library (kernel A/B measurements against another checkout); default = the in-tree build
LIB_PATH = os.environ.get("CBA_HIP_LIB") or os.path.join(_HERE, "libcalib_ba_hip.so")


class EngineError(RuntimeError):
    pass


class CbaCamera(C.Structure):
    _fields_ = [("model_type", C.c_int32), ("width", C.c_int32), ("height", C.c_int32),
                ("calib_min_x", C.c_int32), ("calib_min_y", C.c_int32),
                ("calib_max_x", C.c_int32), ("calib_max_y", C.c_int32),
                ("grid_w", C.c_int32), ("grid_h", C.c_int32)]


ALLREDUCE_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_int64, C.c_void_p)
COLLECTIVE_FN = C.CFUNCTYPE(C.c_int, C.c_int32, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p)   # cba_collective_fn
COLL_ALLREDUCE_SUM, COLL_REDUCE_SCATTER_SUM, COLL_ALLGATHER = 0, 1, 2


class CbaSolverOptions(C.Structure):
    """cba_solver_options: scheduling options of the reduced solve (all zero = defaults)."""
    _fields_ = [("factor_tail_rows", C.c_int32), ("back_substitution", C.c_int32), ("elimination", C.c_int32), ("grid_strips", C.c_int32),
                ("grid_single_tile_tasks", C.c_int32)]


ELIMINATION_AUTO, ELIMINATION_POSE_FIRST, ELIMINATION_GRID_FIRST = 0, 1, 2


DEFAULT_FACTOR_TAIL_ROWS = 8192      # what factor_tail_rows = 0 selects on one GPU (include/cba.h; 6144 / 4096 in the distributed solve with 2-3 / >= 4 ranks)


class CbaConfig(C.Structure):
    _fields_ = [("n_cameras", C.c_int32), ("cameras", C.POINTER(CbaCamera)),
                ("n_images", C.c_int32), ("n_points", C.c_int32),
                ("numerical_diff_delta", C.c_double),
                ("localize_only", C.c_int32), ("eliminate_points", C.c_int32), ("device", C.c_int32),
                ("allreduce", ALLREDUCE_FN), ("allreduce_user", C.c_void_p),
                ("n_images_global", C.c_int32),
                ("reduce_buffer", C.c_void_p), ("reduce_buffer_doubles", C.c_int64),
                ("deterministic", C.c_int32), ("distributed_solve", C.c_int32), ("rank", C.c_int32), ("world_size", C.c_int32),
                ("collective", COLLECTIVE_FN), ("collective_user", C.c_void_p), ("solver", CbaSolverOptions)]


class CbaFitReport(C.Structure):
    _fields_ = [("initial_cost", C.c_double), ("final_cost", C.c_double), ("lambda_", C.c_double),
                ("iterations_performed", C.c_int32), ("lm_attempts", C.c_int32), ("t_pass", C.c_double), ("t_solve", C.c_double)]


class CbaParametricCamera(C.Structure):
    _fields_ = [("width", C.c_int32), ("height", C.c_int32), ("use_equidistant_projection", C.c_int32), ("reserved", C.c_int32),
                ("parameters", C.c_double * 12)]


class CbaParametricFitOptions(C.Structure):
    _fields_ = [("subsample_step", C.c_int32), ("max_iteration_count", C.c_int32), ("max_lm_attempts", C.c_int32),
                ("allow_rotation", C.c_int32), ("n_deltas", C.c_int32), ("reserved", C.c_int32), ("deltas", C.c_double * 8)]


class CbaCompareOptions(C.Structure):
    _fields_ = [("rotation", C.c_double * 9), ("border_x", C.c_int32), ("border_y", C.c_int32),
                ("max_visualization_extent", C.c_double), ("max_visualization_extent_pixels", C.c_double),
                ("initial_estimate", C.c_int32), ("straggler_threshold", C.c_int32)]


COMPARE_ARRAYS = (("base_directions", 3, np.float64), ("fitted_directions", 3, np.float64), ("errors", 3, np.float64),
                  ("reprojection_errors", 2, np.float64), ("flags", 0, np.uint8))
COMPARE_IMAGES = (("error_magnitudes", 0), ("error_direction_angles", 3), ("error_directions", 3), ("reprojection_magnitudes", 0),
                  ("reprojections", 3))


class CbaCompareOutputs(C.Structure):
    _fields_ = [(name, C.c_void_p) for name, _, _ in COMPARE_ARRAYS] + [(name, C.c_void_p) for name, _ in COMPARE_IMAGES]


class CbaCompareStats(C.Structure):
    _fields_ = [("n_base_ok", C.c_int64), ("n_both_ok", C.c_int64), ("n_projected", C.c_int64), ("n_second_launch", C.c_int64),
                ("max_error_component", C.c_double), ("max_error_norm", C.c_double),
                ("reprojection_error_sum", C.c_double), ("reprojection_error_max", C.c_double),
                ("reprojection_error_median", C.c_double), ("has_median", C.c_int32)]


INITIAL_ESTIMATE_CENTER, INITIAL_ESTIMATE_PIXEL = 0, 1


class CbaUndistortOptions(C.Structure):
    _fields_ = [("width", C.c_int32), ("height", C.c_int32), ("fx", C.c_double), ("fy", C.c_double), ("cx", C.c_double), ("cy", C.c_double),
                ("rotation", C.c_double * 9), ("initial_estimate", C.c_int32), ("straggler_threshold", C.c_int32)]


class CbaLocalizationOptions(C.Structure):
    _fields_ = [("n_trials", C.c_int64), ("first_trial", C.c_int64), ("seed", C.c_uint64), ("min_distance", C.c_double),
                ("max_distance", C.c_double), ("point_count", C.c_int32), ("max_candidates", C.c_int32), ("max_iterations", C.c_int32),
                ("reserved", C.c_int32)]


# (name, trailing shape with P = the point count, dtype) of cba_localization_outputs, in its order
LOCALIZATION_ARRAYS = (("errors", (), np.float32), ("rotation_angles", (), np.float64), ("poses", (7,), np.float64),
                       ("iterations", (), np.int32), ("flags", (), np.uint8), ("candidates_used", (), np.int32),
                       ("pixels", ("P", 2), np.float32), ("distances", ("P",), np.float32), ("points", ("P", 3), np.float64),
                       ("bearings", ("P", 3), np.float64))
LOCALIZATION_SAMPLES = ("pixels", "distances", "points", "bearings")


class CbaLocalizationOutputs(C.Structure):
    _fields_ = [(name, C.c_void_p) for name, _, _ in LOCALIZATION_ARRAYS]


class CbaLocalizationStats(C.Structure):
    _fields_ = [("n_trials", C.c_int64), ("n_valid", C.c_int64), ("n_converged", C.c_int64), ("mean_error", C.c_float),
                ("median_error", C.c_float), ("max_error", C.c_float), ("reserved", C.c_float), ("median_rotation_angle", C.c_double)]


LOCALIZATION_DEFAULTS = dict(n_trials=10000, point_count=15, min_distance=1.5, max_distance=2.5, max_iterations=50)


class CbaLocalizeImagesOptions(C.Structure):
    _fields_ = [("seed", C.c_uint64), ("threshold", C.c_double), ("bearing_mode", C.c_int32), ("n_hypotheses", C.c_int32),
                ("min_calibrated_match_count", C.c_int32), ("min_inliers", C.c_int32), ("refine_set", C.c_int32),
                ("max_iterations", C.c_int32)]


class CbaLocalizeImagesInput(C.Structure):
    _fields_ = [("n_slots", C.c_int64), ("n_features", C.c_int64), ("n_models", C.c_int32), ("reserved", C.c_int32),
                ("models", C.POINTER(C.c_void_p)), ("slot_id", C.c_void_p), ("slot_model", C.c_void_p), ("feature_start", C.c_void_p),
                ("pixels", C.c_void_p), ("points", C.c_void_p), ("candidate", C.c_void_p), ("start_poses", C.c_void_p)]


# (name, per "slot" / "feature", trailing shape with H = the hypothesis count, dtype) of cba_localize_images_outputs, in its order
LOCALIZE_IMAGES_ARRAYS = (("image_tr_global", "slot", (7,), np.float64), ("flags", "slot", (), np.uint8),
                          ("match_count", "slot", (), np.int32), ("list_length", "slot", (), np.int32),
                          ("best_hypothesis", "slot", (), np.int32), ("best_inliers", "slot", (), np.int32),
                          ("inliers_after_refinement", "slot", (), np.int32), ("iterations", "slot", (), np.int32),
                          ("final_cost", "slot", (), np.float64), ("bearings", "feature", (3,), np.float64),
                          ("valid", "feature", (), np.uint8), ("list", "feature", (), np.int32), ("samples", "slot", ("H", 4), np.int32),
                          ("hypothesis_poses", "slot", (12,), np.float64))
LOCALIZE_IMAGES_DEBUG = ("bearings", "valid", "list", "samples", "hypothesis_poses")
LOCALIZE_IMAGES_DEFAULTS = dict(n_hypotheses=16, min_calibrated_match_count=7, min_inliers=4, max_iterations=50)
LOCALIZED, LOCALIZE_STOP_RULE_MET, LOCALIZE_NONCENTRAL = 2, 4, 8      # bits of the flags (bit 0: more than 3 features)


class CbaLocalizeImagesOutputs(C.Structure):
    _fields_ = [(name, C.c_void_p) for name, _, _, _ in LOCALIZE_IMAGES_ARRAYS]


class CbaReport(C.Structure):
    _fields_ = [("initial_cost", C.c_double), ("final_cost", C.c_double), ("lambda_", C.c_double),
                ("accepted", C.c_int32), ("lm_attempts", C.c_int32),
                ("n_residuals_valid", C.c_int64), ("n_jacobians_dropped", C.c_int64),
                ("t_jac", C.c_double), ("t_solve", C.c_double), ("t_cost", C.c_double),
                ("t_accumulate", C.c_double), ("t_gemm", C.c_double), ("t_factor", C.c_double)]


# Prototype of every function include/cba.h declares: name -> (restype, argtypes).  load() applies the table once; the tests check
# it against the header and that the library exports every name.
_I, _I32, _I64, _F64, _VP = C.c_int, C.c_int32, C.c_int64, C.c_double, C.c_void_p
_D, _U8, _I32P, _I64P, _F32P = C.POINTER(C.c_double), C.POINTER(C.c_uint8), C.POINTER(C.c_int32), C.POINTER(C.c_int64), C.POINTER(C.c_float)
_CAM, _PCAM, _CFG = C.POINTER(CbaCamera), C.POINTER(CbaParametricCamera), C.POINTER(CbaConfig)
PROTOTYPES = {
    "cba_prepare_device": (_I, [_I32]),
    "cba_last_error": (C.c_char_p, []),
    "cba_version": (C.c_char_p, []),
    "cba_create": (_I, [_CFG, C.POINTER(_VP)]),
    "cba_destroy": (None, [_VP]),
    "cba_set_observations": (_I, [_VP, _I64, _F32P, _I32P, _I32P, _I32P, _D]),
    "cba_set_state": (_I, [_VP, _D, _D, _D, C.POINTER(_D)]),
    "cba_get_state": (_I, [_VP, _D, _D, _D, C.POINTER(_D)]),
    "cba_get_last_projection": (_I, [_VP, _D]),
    "cba_step": (_I, [_VP, _F64, _I32, _F64, C.POINTER(CbaReport)]),
    "cba_cost": (_I, [_VP, _D, _I64P, _D]),
    "cba_fd_redo_overflow": (_I64, [_VP]),
    "cba_debug_fd_redo_counts": (_I, [_VP, _I64P]),
    "cba_project": (_I, [_CAM, _D, _I64, _D, _D, _D, _U8, _I32]),
    "cba_unproject": (_I, [_CAM, _D, _I64, _D, _D, _D, _U8, _I32]),
    "cba_model_create": (_I, [_CAM, _D, _I32, C.POINTER(_VP)]),
    "cba_model_destroy": (None, [_VP]),
    "cba_model_set_grid": (_I, [_VP, _D]),
    "cba_model_project": (_I, [_VP, _I64, _D, _D, _D, _U8]),
    "cba_model_unproject": (_I, [_VP, _I64, _D, _D, _D, _U8]),
    "cba_model_direction_image": (_I, [_VP, _U8, _D, _U8]),
    "cba_render_nearest_feature_image": (_I, [_I32, _I32, _I64, _I32P, _F32P, _I32, _U8, _F32P]),
    "cba_model_center_point": (_I, [_VP, _D, _I64P]),
    "cba_model_line_offsets": (_I, [_VP, _D, _D, _U8, _D]),
    "cba_model_compare": (_I, [_VP, _VP, C.POINTER(CbaCompareOptions), C.POINTER(CbaCompareOutputs), C.POINTER(CbaCompareStats)]),
    "cba_model_direction_moments": (_I, [_VP, _VP, _I32, _I32, _D, _I64P]),
    "cba_model_localization_accuracy": (_I, [_VP, _VP, C.POINTER(CbaLocalizationOptions), C.POINTER(CbaLocalizationOutputs),
                                             C.POINTER(CbaLocalizationStats)]),
    "cba_model_localize_images": (_I, [C.POINTER(CbaLocalizeImagesInput), C.POINTER(CbaLocalizeImagesOptions), C.POINTER(CbaLocalizeImagesOutputs)]),
    "cba_schur_solve": (_I, [_I32, _I32, _I32, _D, _D, _D, _D, _D, _D, _I32]),
    "cba_schur_solve_opt": (_I, [_I32, _I32, _I32, _D, _D, _D, _D, _D, _D, C.POINTER(CbaSolverOptions), _I32]),
    "cba_debug_reduced_system": (_I, [_I32, _I32, _I32, _D, _D, _D, _D, _D, _F64, _I32, _D, C.POINTER(C.c_uint64), _I32P, _I32]),
    "cba_fit_grid_to_directions": (_I, [_CAM, _D, _I64, _D, _D, _I32, C.POINTER(CbaFitReport), _I32]),
    "cba_parametric_project": (_I, [_PCAM, _I64, _D, _D, _U8, _I32]),
    "cba_parametric_unproject": (_I, [_PCAM, _I64, _D, _D, _U8, _I32]),
    "cba_parametric_fit_pass": (_I, [_PCAM, _D, _D, _I32, _I32, _I32, _F64, _I32, _D, _U8, _D, _D, _D, _D, _I32]),
    "cba_fit_parametric_to_dense_model": (_I, [_PCAM, _D, _I32, _I32, _VP, C.POINTER(CbaParametricFitOptions), _D, C.POINTER(CbaFitReport), _I32]),
    "cba_model_compare_parametric": (_I, [_VP, _PCAM, C.POINTER(CbaCompareOptions), C.POINTER(CbaCompareOutputs), C.POINTER(CbaCompareStats)]),
    "cba_debug_dump": (_I, [_VP, _I32, _VP, C.c_size_t]),
    "cba_set_straggler_threshold": (_I, [_VP, _I32]),
    "cba_set_fd_schedule": (_I, [_VP, _I32]),
    "cba_debug_accumulate": (_I, [_VP, _D]),
    "cba_debug_solve": (_I, [_VP, _F64]),
    "cba_debug_apply_update": (_I, [_VP, _D]),
    "cba_debug_gridfirst": (_I, [_VP, _F64, _I32, _I32, _I32, _VP, C.c_size_t]),
    "cba_gridfirst_plan_query": (_I64, [_CAM, _I32, _I32, _I32, _I32, _I32, _I32, _VP, _I64]),
    "cba_debug_time_direction_image": (_I, [_VP, _I32, _I32, _I32, _D]),
    "cba_elimination_order": (_I32, [_VP, _I32P]),
    "cba_total_dof": (_I32, [_VP]),
    "cba_dense_dof": (_I32, [_VP]),
    "cba_jacobian_record_doubles": (_I32, [_VP]),
    "cba_reduce_buffer_doubles": (_I64, [_CFG]),
    "cba_kernel_stats": (_I, [_VP, _I32, _D, _D, _D, _I32P]),
}
EXPORTED_SYMBOLS = list(PROTOTYPES)
# The same table for include/cba_undistort.h (tests/test_undistort_header.py checks it against that header)
UNDISTORT_PROTOTYPES = {
    "cba_model_undistortion_map": (_I, [_VP, C.POINTER(CbaUndistortOptions), _D, _U8, _F32P, _I64P]),
    "cba_remap_create": (_I, [_VP, C.POINTER(CbaUndistortOptions), C.POINTER(_VP)]),
    "cba_remap_create_from_map": (_I, [_I32, _I32, _F32P, _I32, C.POINTER(_VP)]),
    "cba_remap_destroy": (None, [_VP]),
    "cba_remap_get_map": (_I, [_VP, _F32P]),
    "cba_remap_apply": (_I, [_VP, _I32, _I32, _I32, _I32, _VP, _VP, C.c_uint8]),
    "cba_remap_apply_device": (_I, [_VP, _I32, _I32, _I32, _I32, _VP, _VP, C.c_uint8, _VP]),
}


class CbaStereoOptions(C.Structure):
    _fields_ = [("context_radius", C.c_int32), ("iterations", C.c_int32), ("min_depth", C.c_float), ("max_depth", C.c_float),
                ("max_normal_2d_length", C.c_float), ("cost_threshold", C.c_float), ("angle_threshold", C.c_float),
                ("lr_consistency_factor_threshold", C.c_float), ("seed", C.c_uint64)]


# The same table for include/cba_stereo.h (tests/test_stereo_cases.py checks it against that header)
_I8P, _SOPT = C.POINTER(C.c_int8), C.POINTER(CbaStereoOptions)
# The same table for include/cba_diagnostics.h
DIAGNOSTICS_PROTOTYPES = {
    "cba_debug_straggler_stats": (_I, [_VP, _I64P]),
    "cba_debug_gridfirst_tile_list_query": (_I64, [_I32, _I32, _I32, C.POINTER(C.c_uint64), _I32, _I32, _I32P, _I64]),
    "cba_debug_gridfirst_tile_list": (_I64, [_VP, _I32P, _I64, _I32P]),
    "cba_debug_hdd_clear_list_query": (_I64, [_CFG, _I32P, _I64, _I64P]),
    "cba_debug_hdd_clear_list": (_I64, [_VP, _I32P, _I64, _I64P]),
    "cba_debug_set_hdd_full_clear": (_I, [_VP, _I32]),
}
STEREO_PROTOTYPES = {
    "cba_stereo_create": (_I, [_I32, _I32, _I32, _I32, _F32P, C.c_float, C.c_float, C.c_float, C.c_float, _I32, _I32, _F32P, _F32P, _I32,
                               C.POINTER(_VP)]),
    "cba_stereo_destroy": (None, [_VP]),
    "cba_stereo_set_images": (_I, [_VP, _U8, _U8]),
    "cba_stereo_set_pose": (_I, [_VP, _F32P]),
    "cba_stereo_match": (_I, [_VP, _SOPT]),
    "cba_stereo_get_state": (_I, [_VP, _F32P, _I8P, _F32P]),
    "cba_stereo_set_state": (_I, [_VP, _F32P, _I8P, _F32P]),
    "cba_stereo_run_stage": (_I, [_VP, _SOPT, _I32, _I32]),
    "cba_stereo_cost": (_I, [_VP, _SOPT, _F32P, _I8P, _F32P]),
    "cba_stereo_filter": (_I, [_VP, _SOPT, _F32P, _F32P]),
}
STEREO_INIT, STEREO_MUTATION, STEREO_PROPAGATION, STEREO_REFINEMENT = 0, 1, 2, 3


class CbaStereoPostOptions(C.Structure):
    _fields_ = [("bilateral_sigma_xy", C.c_float), ("bilateral_radius_factor", C.c_float), ("bilateral_sigma_inv_depth", C.c_float),
                ("hole_filling_iterations", C.c_int32), ("min_component_size", C.c_int32), ("similar_depth_ratio", C.c_float)]


# The same table for include/cba_stereo_post.h (tests/test_stereo_post_cases.py checks it against that header)
_SPOPT = C.POINTER(CbaStereoPostOptions)
STEREO_POST_PROTOTYPES = {
    "cba_stereo_post_stage": (_I, [_VP, _SOPT, _SPOPT, _I32, _F32P, _F32P, _F32P, _F32P]),
    "cba_stereo_finish": (_I, [_VP, _SOPT, _SPOPT, _F32P, _F32P]),
}
STEREO_POST_MEDIAN, STEREO_POST_BILATERAL, STEREO_POST_FILL_HOLES, STEREO_POST_COMPONENTS = 0, 1, 2, 3
STEREO_POST_MAX_RADIUS = 32

# The same table for include/cba_point_cloud.h (tests/test_point_cloud_cases.py checks it against that header)
POINT_CLOUD_PROTOTYPES = {
    "cba_cloud_pair_create": (_I, [_I32, _I32, _I32, _F32P, _F32P, _F32P, _I64, _U8, _F32P, _I64, _U8, _I32, C.POINTER(_VP)]),
    "cba_cloud_pair_create_from_depth": (_I, [_I32, _I32, _I32, _F32P, _F32P, _U8, _F32P, _F32P, _U8, _I32, C.POINTER(_VP)]),
    "cba_cloud_pair_destroy": (None, [_VP]),
    "cba_cloud_pair_counts": (_I, [_VP, _I64P]),
    "cba_cloud_pair_moments": (_I, [_VP, _D]),
    "cba_cloud_pair_align": (_I, [_VP, _F32P, _F32P, _F32P, _D, _F32P]),
    "cba_cloud_pair_get_clouds": (_I, [_VP, _F32P, _U8, _F32P, _U8]),
}

DUMP_COST_VECTOR, DUMP_PIXELS, DUMP_FLAGS, DUMP_JACOBIANS = 1, 2, 3, 4
DUMP_BLOCK_DIAG_H, DUMP_BLOCK_DIAG_B, DUMP_OFF_DIAG_H, DUMP_DENSE_H, DUMP_DENSE_B, DUMP_X = 5, 6, 7, 8, 9, 10
DUMP_TEST_COST_VECTOR = 11
DUMP_CELLS, DUMP_POSE_SLOT = 12, 13
# items of cba_debug_gridfirst
GF_TOUCHED, GF_ACT, GF_KMASK, GF_ROWMASK, GF_F, GF_XF, GF_DIMS, GF_FORM_TILES, GF_BORDER = range(9)
GF_DIM_NAMES = ("act_words", "n_act_tiles", "kmask_words", "kmask_tiles", "mask_words", "nbf", "s0_c0", "s0_c1", "n_form_tiles", "nbg", "ntc",
                "strips_in_place")

_lib: Optional[C.CDLL] = None


def load() -> C.CDLL:
    """Loads libcalib_ba_hip.so; fails loudly if it has not been built (no fallback path exists)."""
    global _lib
    if _lib is not None:
        return _lib
    # torch bundles its own copy of the HIP runtime (same SONAME libamdhip64.so.7).  Importing it first
    # makes the dynamic loader resolve our NEEDED entry to that copy, so that device pointers and
    # streams are shared by one runtime when torch.distributed does the all-reduce.
    # four concurrent engine streams + RCCL's own: ask the runtime for more than its default of four
    # hardware queues (only effective if HIP has not been initialised yet)
    os.environ.setdefault("GPU_MAX_HW_QUEUES", "8")
    try:
        import torch  # noqa: F401
    except Exception:
        pass
    if not os.path.exists(LIB_PATH):
        raise EngineError(f"{LIB_PATH} is missing -- run `python -c 'import __graft_entry__ as g; g.build()'`; "
                          "the engine has no CPU fallback")
    L = C.CDLL(LIB_PATH)
    for name, (restype, argtypes) in {**PROTOTYPES, **UNDISTORT_PROTOTYPES, **STEREO_PROTOTYPES, **STEREO_POST_PROTOTYPES,
                                      **POINT_CLOUD_PROTOTYPES, **DIAGNOSTICS_PROTOTYPES}.items():
        fn = getattr(L, name, None)
        if fn is None and name in DIAGNOSTICS_PROTOTYPES and os.environ.get("CBA_HIP_LIB"):
            continue      # an older build under CBA_HIP_LIB may lack a diagnostic: calling it raises AttributeError
        if fn is None:
            raise AttributeError(f"{LIB_PATH} does not export {name}")
        fn.restype, fn.argtypes = restype, argtypes
    _lib = L
    return L


def gridfirst_plan(cameras: Sequence[Camera], n_images: int, n_points: int, strips: int = 0, single_tile_tasks: bool = False) -> dict:
    """cba_gridfirst_plan_query: the static plan of the grid-first elimination order (host only, no device).

    Keys: the header fields (G, Gf, n_rp, n_border, n_fact, n_pad, nbg, nbf, ntc, n_tasks0, mask_words, half_bandwidth, strips0),
    f_of_grid (G,), chains (n, 4), tasks (n, 4: kind | intervals << 8, r, c, first interval), ivals (n, 2), rowmask (nbf, words),
    flops (3,), gperm (list per camera), shared (the buffer of shared blocks that image sharding all-reduces per step: doubles, section
    offsets off_rp_grid / off_rig / off_pp / off_b, G, band_ref_col = reference dense column of every band position; the layout of
    distributed.GridFirstSharedLayout)."""
    L = load()
    cams = (CbaCamera * len(cameras))(*[_cam_struct(c) for c in cameras])

    def q(what, dtype):
        n = L.cba_gridfirst_plan_query(cams, len(cameras), n_images, n_points, strips, int(single_tile_tasks), what, None, 0)
        if n < 0:
            _check(int(n), "cba_gridfirst_plan_query")
        out = np.zeros(int(n) // np.dtype(dtype).itemsize, dtype=dtype)
        if n:
            L.cba_gridfirst_plan_query(cams, len(cameras), n_images, n_points, strips, int(single_tile_tasks), what, out.ctypes.data_as(C.c_void_p), int(n))
        return out

    h = q(0, np.int32)
    names = ["G", "Gf", "n_rp", "n_border", "n_fact", "n_pad", "nbg", "nbf", "ntc", "n_chains", "n_tasks", "n_tasks0", "n_ivals",
             "mask_words", "half_bandwidth", "strips0"]
    plan = {k: int(v) for k, v in zip(names, h)}
    plan["f_of_grid"] = q(1, np.int32)
    plan["chains"] = q(2, np.int32).reshape(-1, 4)
    plan["tasks"] = q(3, np.int32).reshape(-1, 4)
    plan["ivals"] = q(4, np.int32).reshape(-1, 2)
    plan["rowmask"] = q(5, np.uint64).reshape(plan["nbf"], plan["mask_words"])
    plan["flops"] = q(6, np.float64)
    plan["gperm"] = [q(16 + c, np.int32) for c in range(len(cameras))]
    sh = q(7, np.int64)
    plan["shared"] = {k: int(v) for k, v in zip(["doubles", "off_rp_grid", "off_rig", "off_pp", "off_b", "G"], sh)}
    plan["shared"]["band_ref_col"] = q(8, np.int32)
    return plan


def gridfirst_tile_list_query(mode: int, masks: np.ndarray, n_slabs: int, allow_parts: bool) -> np.ndarray:
    """cba_debug_gridfirst_tile_list_query: the tile list of the border update that the library builds from `masks` (nt, words) uint64
    (host only, no device) -- mode 0: K-slab masks, mode 1: block-row activity words.  Returns the entries (n, 4): tm, tn, s0, s1."""
    L = load()
    m = np.ascontiguousarray(masks, dtype=np.uint64)
    assert m.ndim == 2
    mp = m.ctypes.data_as(C.POINTER(C.c_uint64))
    n = int(L.cba_debug_gridfirst_tile_list_query(int(mode), m.shape[0], m.shape[1], mp, int(n_slabs), int(bool(allow_parts)), None, 0))
    if n < 0:
        _check(n, "cba_debug_gridfirst_tile_list_query")
    out = np.zeros((n, 4), dtype=np.int32)
    if n:
        got = int(L.cba_debug_gridfirst_tile_list_query(int(mode), m.shape[0], m.shape[1], mp, int(n_slabs), int(bool(allow_parts)),
                                                        out.ctypes.data_as(_I32P), n))
        assert got == n
    return out


HDD_CLEAR_INFO = ("n_pad", "dense_dof", "entries", "selective")


def _hdd_clear_list(call, what: str):
    info = (C.c_int64 * 4)()
    n = int(call(None, 0, info))
    if n < 0:
        _check(n, what)
    out = np.zeros((n, 3), dtype=np.int32)
    if n:
        assert int(call(out.ctypes.data_as(_I32P), n, info)) == n
    return out, {k: int(v) for k, v in zip(HDD_CLEAR_INFO, info)}


def hdd_clear_list_query(problem: Problem, elimination: int = 0, grid_strips: int = 0):
    """cba_debug_hdd_clear_list_query: (segments (n, 3): row, first column, length; info) -- the row segments of H_dd that a Jacobian
    pass of the problem an Engine would create can write (host only, no device).  info: n_pad (row stride of H_dd), dense_dof,
    entries (covered by the list), selective (1 = the pass clears the list, 0 = the whole of H_dd)."""
    L = load()
    cams = (CbaCamera * problem.n_cameras)(*[_cam_struct(c) for c in problem.cameras])
    cfg = CbaConfig(problem.n_cameras, cams, problem.n_images, problem.n_points, problem.fd_delta,
                    int(problem.localize_only), int(problem.eliminate_points), 0, ALLREDUCE_FN(0), None, 0, None, 0, 0,
                    0, 0, 1, COLLECTIVE_FN(0), None, CbaSolverOptions(0, 0, int(elimination), int(grid_strips), 0))
    return _hdd_clear_list(lambda seg, cap, info: L.cba_debug_hdd_clear_list_query(C.byref(cfg), seg, cap, info),
                           "cba_debug_hdd_clear_list_query")


def prepare(device: int = 0) -> None:
    """Creates the engine's HIP streams for `device` now (cba_prepare_device).  Call it before the process launches
    its first GPU kernel: streams created that early run the dominant GEMM ~15 % faster than streams created later
    (measured on MI355X / ROCm 7.2 in round 2).  Optional -- cba_create does it on demand."""
    _check(load().cba_prepare_device(int(device)), "cba_prepare_device")


def _check(rc: int, what: str) -> None:
    if rc != 0:
        msg = load().cba_last_error()
        raise EngineError(f"{what} failed with code {rc}: {msg.decode() if msg else ''}")


def _dp(a: np.ndarray):
    assert a.dtype == np.float64 and a.flags.c_contiguous
    return a.ctypes.data_as(C.POINTER(C.c_double))


def _cam_struct(cam: Camera) -> CbaCamera:
    return CbaCamera(cam.model_type, cam.width, cam.height, cam.calib_min_x, cam.calib_min_y,
                     cam.calib_max_x, cam.calib_max_y, cam.grid_w, cam.grid_h)


@dataclass
class StepReport:
    """OptimizationReport (libvis lm_optimizer.h:55-77) + the values OptimizeJointly returns by pointer."""
    initial_cost: float
    final_cost: float
    final_lambda: float
    accepted: bool
    lm_attempts: int
    n_residuals_valid: int
    n_jacobians_dropped: int
    t_jac: float
    t_solve: float
    t_cost: float
    t_accumulate: float
    t_gemm: float
    t_factor: float


class Engine:
    """Device-resident BA problem (cba_problem)."""

    def __init__(self, problem: Problem, device: int = 0, allreduce: Optional[Callable[[int, int], int]] = None,
                 n_images_global: int = 0, reduce_buffer_ptr: int = 0, reduce_buffer_doubles: int = 0,
                 last_projection: Optional[np.ndarray] = None, deterministic: bool = False,
                 allreduce_native: Optional[tuple] = None, distributed_solve: bool = False, rank: int = 0, world_size: int = 1,
                 collective: Optional[Callable[[int, int, int, int], int]] = None, collective_native: Optional[tuple] = None,
                 factor_tail_rows: int = 0, back_substitution_panels: bool = False, elimination: int = 0, grid_strips: int = 0,
                 grid_single_tile_tasks: bool = False):
        self.L = load()
        self.problem = problem
        self._cams = (CbaCamera * problem.n_cameras)(*[_cam_struct(c) for c in problem.cameras])
        self._cb = None
        if allreduce is not None:
            def _cb(ptr, count, user, _f=allreduce):
                try:
                    return int(_f(int(ptr), int(count)) or 0)
                except Exception:  # never let an exception cross the C boundary
                    import traceback
                    traceback.print_exc()
                    return 1
            self._cb = ALLREDUCE_FN(_cb)
        cb, user = (self._cb if self._cb is not None else ALLREDUCE_FN(0)), None
        if allreduce_native is not None:     # (C function pointer, user pointer), e.g. distributed.NativeRccl.fn / .user
            cb, user = C.cast(allreduce_native[0], ALLREDUCE_FN), allreduce_native[1]
        # collective(op, send_ptr, recv_ptr, count) -> 0: reduce-scatter / all-gather of the distributed solve (cba_collective_fn)
        self._ccb = None
        if collective is not None:
            def _ccb(op, send, recv, count, user, _f=collective):
                try:
                    return int(_f(int(op), int(send or 0), int(recv or 0), int(count)) or 0)
                except Exception:
                    import traceback
                    traceback.print_exc()
                    return 1
            self._ccb = COLLECTIVE_FN(_ccb)
        ccb, cuser = (self._ccb if self._ccb is not None else COLLECTIVE_FN(0)), None
        if collective_native is not None:
            ccb, cuser = C.cast(collective_native[0], COLLECTIVE_FN), collective_native[1]
        cfg = CbaConfig(problem.n_cameras, self._cams, problem.n_images, problem.n_points, problem.fd_delta,
                        int(problem.localize_only), int(problem.eliminate_points), device,
                        cb, user, n_images_global,
                        reduce_buffer_ptr or None, reduce_buffer_doubles, int(deterministic), int(distributed_solve), int(rank), int(world_size),
                        ccb, cuser, CbaSolverOptions(int(factor_tail_rows), int(bool(back_substitution_panels)), int(elimination), int(grid_strips), int(bool(grid_single_tile_tasks))))
        self._cfg = cfg
        self._h = C.c_void_p()
        _check(self.L.cba_create(C.byref(cfg), C.byref(self._h)), "cba_create")
        self.set_observations(problem, last_projection)

    def set_observations(self, problem: Problem, last_projection: Optional[np.ndarray] = None) -> None:
        """cba_set_observations: replaces the observations (same cameras, imagesets and points); last_projection = warm starts or None."""
        _check(self.L.cba_set_observations(
            self._h, problem.n_obs, problem.obs_xy.ctypes.data_as(C.POINTER(C.c_float)),
            problem.obs_point.ctypes.data_as(C.POINTER(C.c_int32)),
            problem.obs_image.ctypes.data_as(C.POINTER(C.c_int32)),
            problem.obs_camera.ctypes.data_as(C.POINTER(C.c_int32)),
            None if last_projection is None else _dp(np.ascontiguousarray(last_projection, dtype=np.float64).reshape(-1, 2))),
            "cba_set_observations")
        self.problem = problem

    @staticmethod
    def reduce_buffer_doubles(problem: Problem, distributed_solve: bool = False, world_size: int = 1) -> int:
        cams = (CbaCamera * problem.n_cameras)(*[_cam_struct(c) for c in problem.cameras])
        cfg = CbaConfig(problem.n_cameras, cams, problem.n_images, problem.n_points, problem.fd_delta,
                        int(problem.localize_only), int(problem.eliminate_points), 0, ALLREDUCE_FN(0), None, 0, None, 0, 0,
                        int(distributed_solve), 0, int(world_size), COLLECTIVE_FN(0), None, CbaSolverOptions(0, 0, 0, 0, 0))
        return int(load().cba_reduce_buffer_doubles(C.byref(cfg)))

    def close(self) -> None:
        if getattr(self, "_h", None) is not None and self._h:
            self.L.cba_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # -- state ---------------------------------------------------------------------------------
    def set_state(self, st: State) -> None:
        grids = (C.POINTER(C.c_double) * len(st.grids))(*[_dp(g) for g in st.grids])
        _check(self.L.cba_set_state(self._h, _dp(st.rig_tr_global), _dp(st.camera_tr_rig), _dp(st.points), grids),
               "cba_set_state")

    def get_state(self, like: State) -> State:
        out = like.copy()
        grids = (C.POINTER(C.c_double) * len(out.grids))(*[_dp(g) for g in out.grids])
        _check(self.L.cba_get_state(self._h, _dp(out.rig_tr_global), _dp(out.camera_tr_rig), _dp(out.points), grids),
               "cba_get_state")
        return out

    def get_last_projection(self) -> np.ndarray:
        out = np.zeros((self.problem.n_obs, 2))
        _check(self.L.cba_get_last_projection(self._h, _dp(out)), "cba_get_last_projection")
        return out

    # -- optimisation ----------------------------------------------------------------------------
    def step(self, init_lambda: float = -1.0, max_lm_attempts: int = 50, init_lambda_factor: float = 0.00001) -> StepReport:
        r = CbaReport()
        _check(self.L.cba_step(self._h, init_lambda, max_lm_attempts, init_lambda_factor, C.byref(r)), "cba_step")
        return StepReport(r.initial_cost, r.final_cost, r.lambda_, bool(r.accepted), r.lm_attempts,
                          r.n_residuals_valid, r.n_jacobians_dropped, r.t_jac, r.t_solve, r.t_cost,
                          r.t_accumulate, r.t_gemm, r.t_factor)

    def cost(self, want_vector: bool = False):
        cost = C.c_double(0)
        nv = C.c_int64(0)
        vec = np.zeros(self.problem.n_obs) if want_vector else None
        _check(self.L.cba_cost(self._h, C.byref(cost), C.byref(nv), _dp(vec) if vec is not None else None), "cba_cost")
        return (cost.value, nv.value, vec) if want_vector else (cost.value, nv.value)

    def kernel_stats(self, which: int):
        s, f, b = C.c_double(0), C.c_double(0), C.c_double(0)
        n = C.c_int32(0)
        _check(self.L.cba_kernel_stats(self._h, which, C.byref(s), C.byref(f), C.byref(b), C.byref(n)), "cba_kernel_stats")
        return dict(seconds=s.value, flops=f.value, bytes=b.value, launches=n.value)

    def elimination_order(self) -> dict:
        """cba_elimination_order: which order this problem uses (cba_solver_options.elimination resolved) and its sizes."""
        out = (C.c_int32 * 4)()
        order = int(self.L.cba_elimination_order(self._h, out))
        return dict(order={1: "pose-first", 2: "grid-first"}.get(order, "?"), strips=int(out[0]), dense_rows=int(out[1]), grid_rows=int(out[2]), chains=int(out[3]))

    # -- parity / debug ----------------------------------------------------------------------------
    def set_fd_schedule(self, schedule: int) -> None:
        """cba_set_fd_schedule: -1 = automatic (default), 0 = pooled finite-difference tasks, 1 = one task per lane with the lanes
        ordered by predicted iteration count, 2 = one task per lane in consecutive order (bit-identical to 1; A/B runs and tests)."""
        _check(self.L.cba_set_fd_schedule(self._h, int(schedule)), "cba_set_fd_schedule")

    def set_straggler_threshold(self, outer_iterations: int) -> None:
        """cba_set_straggler_threshold: outer projection iterations before an observation goes to the straggler kernel."""
        _check(self.L.cba_set_straggler_threshold(self._h, int(outer_iterations)), "cba_set_straggler_threshold")

    def fd_redo_overflow(self) -> int:
        """cba_fd_redo_overflow: finite-difference tasks of the last Jacobian pass that found the follow-up list full (expected 0)."""
        return int(self.L.cba_fd_redo_overflow(self._h))

    def fd_redo_counts(self):
        """cba_debug_fd_redo_counts: (main list, side-stream list, overflow) of the last Jacobian pass."""
        out = (C.c_int64 * 3)()
        _check(self.L.cba_debug_fd_redo_counts(self._h, out), "cba_debug_fd_redo_counts")
        return int(out[0]), int(out[1]), int(out[2])

    def straggler_stats(self) -> dict:
        """cba_debug_straggler_stats: counters of the base projection's straggler kernel in the last pass over the observations."""
        out = (C.c_int64 * 5)()
        _check(self.L.cba_debug_straggler_stats(self._h, out), "cba_debug_straggler_stats")
        return dict(zip(("predicted", "listed", "period_1", "period_2_or_more", "full_budget"), (int(v) for v in out)))

    def gridfirst_tile_list(self):
        """cba_debug_gridfirst_tile_list: (entries (n, 4): tm, tn, s0, s1, info) of the problem's current host tile list of the border
        update; info: valid, age (solves since cba_set_observations built the list), dirty (rebuilt since the last upload), n_slabs."""
        info = (C.c_int32 * 4)()
        n = int(self.L.cba_debug_gridfirst_tile_list(self._h, None, 0, info))
        if n < 0:
            _check(n, "cba_debug_gridfirst_tile_list")
        out = np.zeros((n, 4), dtype=np.int32)
        if n:
            assert int(self.L.cba_debug_gridfirst_tile_list(self._h, out.ctypes.data_as(_I32P), n, info)) == n
        return out, dict(valid=int(info[0]), age=int(info[1]), dirty=int(info[2]), n_slabs=int(info[3]))

    def hdd_clear_list(self):
        """cba_debug_hdd_clear_list: (segments (n, 3), info) of this problem, as hdd_clear_list_query; info["selective"] is 0 as well
        while set_hdd_full_clear(True) holds."""
        return _hdd_clear_list(lambda seg, cap, info: self.L.cba_debug_hdd_clear_list(self._h, seg, cap, info), "cba_debug_hdd_clear_list")

    def set_hdd_full_clear(self, on: bool) -> None:
        """cba_debug_set_hdd_full_clear: every later Jacobian pass clears the whole of H_dd (A/B runs and tests); same results."""
        _check(self.L.cba_debug_set_hdd_full_clear(self._h, int(bool(on))), "cba_debug_set_hdd_full_clear")

    def debug_accumulate(self) -> float:
        cost = C.c_double(0)
        _check(self.L.cba_debug_accumulate(self._h, C.byref(cost)), "cba_debug_accumulate")
        return cost.value

    def debug_solve(self, lam: float) -> np.ndarray:
        _check(self.L.cba_debug_solve(self._h, lam), "cba_debug_solve")
        return self.dump(DUMP_X)

    def debug_apply_update(self, x: np.ndarray) -> None:
        x = np.ascontiguousarray(x, dtype=np.float64)
        assert x.size == self.problem.total_dof
        _check(self.L.cba_debug_apply_update(self._h, _dp(x)), "cba_debug_apply_update")

    def dump(self, what: int) -> np.ndarray:
        p = self.problem
        n, bs, nb, dd = p.n_obs, p.block_size, p.n_blocks, p.dense_dof
        rec = self.L.cba_jacobian_record_doubles(self._h)
        shapes = {
            DUMP_COST_VECTOR: ((n,), np.float64), DUMP_TEST_COST_VECTOR: ((n,), np.float64),
            DUMP_PIXELS: ((n, 2), np.float64), DUMP_FLAGS: ((n,), np.uint8),
            DUMP_JACOBIANS: ((n, rec), np.float64),
            DUMP_BLOCK_DIAG_H: ((nb, bs, bs), np.float64), DUMP_BLOCK_DIAG_B: ((nb * bs,), np.float64),
            DUMP_OFF_DIAG_H: ((nb * bs, dd), np.float64), DUMP_DENSE_H: ((dd, dd), np.float64),
            DUMP_DENSE_B: ((dd,), np.float64), DUMP_X: ((p.total_dof,), np.float64),
            DUMP_CELLS: ((n, 2), np.int32), DUMP_POSE_SLOT: ((p.n_images,), np.int32),
        }
        shape, dt = shapes[what]
        out = np.zeros(shape, dtype=dt)
        _check(self.L.cba_debug_dump(self._h, what, out.ctypes.data_as(C.c_void_p), out.nbytes), "cba_debug_dump")
        return out

    def gridfirst_dims(self) -> dict:
        """cba_debug_gridfirst(CBA_GF_DIMS): the sizes of the grid-first system's masks and tile lists (GF_DIM_NAMES)."""
        out = np.zeros(len(GF_DIM_NAMES), dtype=np.int32)
        _check(self.L.cba_debug_gridfirst(self._h, 0.0, -1, 0, GF_DIMS, out.ctypes.data_as(C.c_void_p), out.nbytes), "cba_debug_gridfirst")
        return {k: int(v) for k, v in zip(GF_DIM_NAMES, out)}

    def debug_gridfirst(self, lam: float, stage: int, what: int, poison: bool = False) -> np.ndarray:
        """cba_debug_gridfirst: after debug_accumulate(), the launches of a grid-first solve for `lam` up to and including `stage`
        (0 forming kernel, 1 block-sparse launch of the grid rows, 2 border update, 3 border factorisation, 4 back substitution and
        scatter; -1 none) on the problem's own buffers, then item `what` (GF_*).  poison: the grid x border tiles whose activity bit
        is off hold quiet NaNs while the stages run."""
        d = self.gridfirst_dims()
        n_pad, nbg = 64 * d["ntc"], d["nbg"]
        shapes = {
            GF_TOUCHED: ((d["n_act_tiles"], d["act_words"]), np.uint64), GF_ACT: ((d["n_act_tiles"], d["act_words"]), np.uint64),
            GF_KMASK: ((d["kmask_tiles"], d["kmask_words"]), np.uint64), GF_ROWMASK: ((d["nbf"], d["mask_words"]), np.uint64),
            GF_F: ((n_pad, n_pad), np.float64), GF_XF: ((64 * d["nbf"],), np.float64), GF_DIMS: ((len(GF_DIM_NAMES),), np.int32),
            GF_FORM_TILES: ((d["n_form_tiles"], 2), np.int32), GF_BORDER: ((n_pad - 64 * nbg, n_pad - 64 * nbg), np.float64),
        }
        shape, dt = shapes[what]
        out = np.zeros(shape, dtype=dt)
        _check(self.L.cba_debug_gridfirst(self._h, float(lam), int(stage), int(bool(poison)), int(what), out.ctypes.data_as(C.c_void_p), out.nbytes),
               "cba_debug_gridfirst")
        return out


class DeviceModel:
    """Device-resident camera model (cba_model): the grid is uploaded once, scratch buffers are kept between calls."""

    def __init__(self, cam: Camera, grid: np.ndarray, device: int = 0):
        self.L = load()
        self.cam = cam
        g = np.ascontiguousarray(grid, dtype=np.float64)
        cs = _cam_struct(cam)
        self._h = C.c_void_p()
        _check(self.L.cba_model_create(C.byref(cs), _dp(g), device, C.byref(self._h)), "cba_model_create")

    def close(self):
        if getattr(self, "_h", None):
            self.L.cba_model_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_grid(self, grid: np.ndarray) -> None:
        g = np.ascontiguousarray(grid, dtype=np.float64)
        _check(self.L.cba_model_set_grid(self._h, _dp(g)), "cba_model_set_grid")

    def project(self, local_points: np.ndarray, init: Optional[np.ndarray] = None):
        pts = np.ascontiguousarray(local_points, dtype=np.float64).reshape(-1, 3)
        n = pts.shape[0]
        px = np.zeros((n, 2)); ok = np.zeros(n, dtype=np.uint8)
        ini = None if init is None else np.ascontiguousarray(init, dtype=np.float64).reshape(-1, 2)
        _check(self.L.cba_model_project(self._h, n, _dp(pts), _dp(ini) if ini is not None else None, _dp(px),
                                        ok.ctypes.data_as(C.POINTER(C.c_uint8))), "cba_model_project")
        return px, ok.astype(bool)

    def unproject(self, pixels: np.ndarray, with_jacobian: bool = False):
        px = np.ascontiguousarray(pixels, dtype=np.float64).reshape(-1, 2)
        n = px.shape[0]
        lines = np.zeros((n, 6)); ok = np.zeros(n, dtype=np.uint8)
        jac = np.zeros((n, 6, 2)) if with_jacobian else None
        _check(self.L.cba_model_unproject(self._h, n, _dp(px), _dp(lines), _dp(jac) if jac is not None else None,
                                          ok.ctypes.data_as(C.POINTER(C.c_uint8))), "cba_model_unproject")
        return (lines, jac, ok.astype(bool)) if with_jacobian else (lines, ok.astype(bool))

    # -- calibration report images ---------------------------------------------------------------
    def direction_image(self, want_directions: bool = False, want_ok: bool = False):
        """cba_model_direction_image: rgb (H, W, 3) uint8 [, directions (H, W, 3) with NaN where Unproject fails] [, ok (H, W) bool]."""
        H, W = self.cam.height, self.cam.width
        rgb = np.zeros((H, W, 3), dtype=np.uint8)
        dirs = np.zeros((H, W, 3)) if want_directions else None
        ok = np.zeros((H, W), dtype=np.uint8) if want_ok else None
        u8p = C.POINTER(C.c_uint8)
        _check(self.L.cba_model_direction_image(self._h, rgb.ctypes.data_as(u8p), _dp(dirs) if dirs is not None else None,
                                                ok.ctypes.data_as(u8p) if ok is not None else None), "cba_model_direction_image")
        out = (rgb,) + ((dirs,) if want_directions else ()) + ((ok.astype(bool),) if want_ok else ())
        return out if len(out) > 1 else rgb

    def time_direction_image(self, use_stage: bool = True, with_directions: bool = False, launches: int = 20) -> float:
        """cba_debug_time_direction_image: seconds per launch of k_direction_image (kernel only)."""
        sec = C.c_double(0)
        _check(self.L.cba_debug_time_direction_image(self._h, int(use_stage), int(with_directions), int(launches), C.byref(sec)),
               "cba_debug_time_direction_image")
        return float(sec.value)

    def center_point(self):
        """cba_model_center_point (non-central model): (centre (3,), number of lines)."""
        center = np.zeros(3)
        n = C.c_int64(0)
        _check(self.L.cba_model_center_point(self._h, _dp(center), C.byref(n)), "cba_model_center_point")
        return center, int(n.value)

    def line_offsets(self, center: np.ndarray):
        """cba_model_line_offsets (non-central model): (offsets (H, W, 3), rgb (H, W, 3) uint8, max_extent)."""
        H, W = self.cam.height, self.cam.width
        c = np.ascontiguousarray(center, dtype=np.float64).reshape(3)
        off = np.zeros((H, W, 3)); rgb = np.zeros((H, W, 3), dtype=np.uint8)
        ext = C.c_double(0)
        _check(self.L.cba_model_line_offsets(self._h, _dp(c), _dp(off), rgb.ctypes.data_as(C.POINTER(C.c_uint8)), C.byref(ext)),
               "cba_model_line_offsets")
        return off, rgb, float(ext.value)

    # -- comparison of two calibrations ------------------------------------------------------------
    def compare(self, fitted: "DeviceModel", rotation: Optional[np.ndarray] = None, border=(0, 0), max_visualization_extent: float = -1.0,
                max_visualization_extent_pixels: float = -1.0, initial_estimate: int = INITIAL_ESTIMATE_CENTER,
                straggler_threshold: int = 0, want_arrays: bool = True, want_images: bool = True) -> dict:
        """cba_model_compare with this model as the base: the per-pixel arrays ((H, W[, k]) of the fitted model's image), the five
        images and the statistics, in one dict.  reprojection_error_median is None when nothing projected."""
        return self._compare(fitted.cam.width, fitted.cam.height, rotation, border, max_visualization_extent, max_visualization_extent_pixels,
                             initial_estimate, straggler_threshold, want_arrays, want_images,
                             lambda o, out, st: _check(self.L.cba_model_compare(self._h, fitted._h, o, out, st), "cba_model_compare"))

    def compare_parametric(self, fitted, rotation: Optional[np.ndarray] = None, border=(0, 0), max_visualization_extent: float = -1.0,
                           max_visualization_extent_pixels: float = -1.0, want_arrays: bool = True, want_images: bool = True) -> dict:
        """cba_model_compare_parametric with this model as the base and a ``parametric.ThinPrismFisheye`` as the fitted model: the
        dict of ``compare`` (n_second_launch is 0: the fitted model projects in closed form)."""
        cs = fitted.struct()
        return self._compare(int(fitted.width), int(fitted.height), rotation, border, max_visualization_extent, max_visualization_extent_pixels,
                             INITIAL_ESTIMATE_CENTER, 0, want_arrays, want_images,
                             lambda o, out, st: _check(self.L.cba_model_compare_parametric(self._h, C.byref(cs), o, out, st),
                                                       "cba_model_compare_parametric"))

    def _compare(self, W, H, rotation, border, max_visualization_extent, max_visualization_extent_pixels, initial_estimate,
                 straggler_threshold, want_arrays, want_images, call) -> dict:
        o = CbaCompareOptions()
        o.rotation[:] = list(np.asarray(np.eye(3) if rotation is None else rotation, dtype=np.float64).reshape(9))
        o.border_x, o.border_y = int(border[0]), int(border[1])
        o.max_visualization_extent, o.max_visualization_extent_pixels = float(max_visualization_extent), float(max_visualization_extent_pixels)
        o.initial_estimate, o.straggler_threshold = int(initial_estimate), int(straggler_threshold)
        out, res = CbaCompareOutputs(), {}
        if want_arrays:
            for name, k, dt in COMPARE_ARRAYS:
                res[name] = np.zeros((H, W, k) if k else (H, W), dtype=dt)
                setattr(out, name, res[name].ctypes.data)
        if want_images:
            for name, k in COMPARE_IMAGES:
                res[name] = np.zeros((H, W, k) if k else (H, W), dtype=np.uint8)
                setattr(out, name, res[name].ctypes.data)
        st = CbaCompareStats()
        call(C.byref(o), C.byref(out), C.byref(st))
        for name, _ in CbaCompareStats._fields_:
            res[name] = getattr(st, name)
        res["reprojection_error_median"] = st.reprojection_error_median if st.has_median else None
        del res["has_median"]
        return res

    def direction_moments(self, fitted: "DeviceModel", border=(0, 0)):
        """cba_model_direction_moments with this model as the base: (M (3, 3) = sum f a^T, number of pixels summed)."""
        M = np.zeros((3, 3))
        n = C.c_int64(0)
        _check(self.L.cba_model_direction_moments(self._h, fitted._h, int(border[0]), int(border[1]), _dp(M), C.byref(n)),
               "cba_model_direction_moments")
        return M, int(n.value)

    # -- undistortion ------------------------------------------------------------------------------
    def undistortion_map(self, pinhole: "Pinhole", rotation: Optional[np.ndarray] = None, initial_estimate: int = INITIAL_ESTIMATE_CENTER,
                         straggler_threshold: int = 0, want_source_pixels: bool = True, want_ok: bool = True, want_map: bool = True) -> dict:
        """cba_model_undistortion_map: source_pixels (H, W, 2) fp64 (pixel-corner convention, NaN where the projection fails), ok (H, W)
        bool, map_xy (H, W, 2) float32 (pixel-centre convention), n_second_launch; H, W = the pinhole image."""
        o = undistort_options(pinhole, rotation, initial_estimate, straggler_threshold)
        H, W = int(pinhole.height), int(pinhole.width)
        shape = (max(H, 0), max(W, 0))
        px = np.zeros(shape + (2,)) if want_source_pixels else None
        ok = np.zeros(shape, dtype=np.uint8) if want_ok else None
        mp = np.zeros(shape + (2,), dtype=np.float32) if want_map else None
        n2 = C.c_int64(0)
        _check(self.L.cba_model_undistortion_map(self._h, C.byref(o), _dp(px) if px is not None else None,
                                                 ok.ctypes.data_as(_U8) if ok is not None else None,
                                                 mp.ctypes.data_as(_F32P) if mp is not None else None, C.byref(n2)), "cba_model_undistortion_map")
        res = dict(n_second_launch=int(n2.value))
        if px is not None:
            res["source_pixels"] = px
        if ok is not None:
            res["ok"] = ok.astype(bool)
        if mp is not None:
            res["map_xy"] = mp
        return res

    def localization_accuracy(self, compared: "DeviceModel", n_trials: int = 0, first_trial: int = 0, point_count: int = 0,
                              min_distance: float = 0.0, max_distance: float = 0.0, seed: int = 0, max_candidates: int = 0,
                              max_iterations: int = 0, want_trials: bool = True, want_samples: bool = False) -> dict:
        """cba_model_localization_accuracy with this model as the ground truth (0 = an option's default): the statistics, with
        want_trials the per-trial arrays and with want_samples the pixels, distances, points and bearings of every trial."""
        T = int(n_trials) or LOCALIZATION_DEFAULTS["n_trials"]
        P = int(point_count) or LOCALIZATION_DEFAULTS["point_count"]
        o = CbaLocalizationOptions()
        o.n_trials, o.first_trial, o.seed = int(n_trials), int(first_trial), int(seed) & 0xFFFFFFFFFFFFFFFF
        o.min_distance, o.max_distance = float(min_distance), float(max_distance)
        o.point_count, o.max_candidates, o.max_iterations = int(point_count), int(max_candidates), int(max_iterations)
        out, res = CbaLocalizationOutputs(), {}
        if T > 0 and 0 < P <= 1024:          # (anything else is the library's to reject)
            for name, tail, dt in LOCALIZATION_ARRAYS:
                if want_samples if name in LOCALIZATION_SAMPLES else want_trials:
                    res[name] = np.zeros((T,) + tuple(P if d == "P" else d for d in tail), dtype=dt)
                    setattr(out, name, res[name].ctypes.data)
        st = CbaLocalizationStats()
        _check(self.L.cba_model_localization_accuracy(self._h, compared._h, C.byref(o), C.byref(out), C.byref(st)),
               "cba_model_localization_accuracy")
        for name, _ in CbaLocalizationStats._fields_:
            if name != "reserved":
                res[name] = getattr(st, name)
        return res


    # -- localization of a dataset's images ----------------------------------------------------------
    @staticmethod
    def localize_images(models, slot_id, slot_model, feature_start, pixels, points, candidate, seed: int = 0, threshold: float = 0.0,
                        bearing_mode: int = 0, n_hypotheses: int = 0, min_calibrated_match_count: int = 0, min_inliers: int = 0,
                        refine_set: int = 0, max_iterations: int = 0, want_debug: bool = False, start_poses=None) -> dict:
        """cba_model_localize_images over the slots of `models` (DeviceModel objects on one device; 0 = an option's default): the
        per-slot arrays, with want_debug also the bearings and valid bytes of stage A, the correspondence lists, the sample table and
        the best hypotheses' poses."""
        L = load()
        ids = np.ascontiguousarray(slot_id, dtype=np.uint64).reshape(-1)
        sm = np.ascontiguousarray(slot_model, dtype=np.int32).reshape(-1)
        fs = np.ascontiguousarray(feature_start, dtype=np.int32).reshape(-1)
        px = np.ascontiguousarray(pixels, dtype=np.float32).reshape(-1, 2)
        pts = np.ascontiguousarray(points, dtype=np.float64).reshape(-1, 3)
        cand = np.ascontiguousarray(candidate, dtype=np.uint8).reshape(-1)
        S, F = ids.shape[0], px.shape[0]
        if not (sm.shape[0] == S and fs.shape[0] == S + 1 and pts.shape[0] == F and cand.shape[0] == F):
            raise ValueError("localize_images: array lengths do not agree")
        handles = (C.c_void_p * max(1, len(models)))(*[m._h for m in models])
        inp = CbaLocalizeImagesInput()
        inp.n_slots, inp.n_features, inp.n_models = S, F, len(models)
        inp.models = C.cast(handles, C.POINTER(C.c_void_p))
        inp.slot_id, inp.slot_model, inp.feature_start = ids.ctypes.data, sm.ctypes.data, fs.ctypes.data
        inp.pixels, inp.points, inp.candidate = px.ctypes.data, pts.ctypes.data, cand.ctypes.data
        sp = None
        if start_poses is not None:
            sp = np.ascontiguousarray(start_poses, dtype=np.float64).reshape(S, 12)
            inp.start_poses = sp.ctypes.data
        o = CbaLocalizeImagesOptions()
        o.seed, o.threshold, o.bearing_mode, o.n_hypotheses = int(seed) & 0xFFFFFFFFFFFFFFFF, float(threshold), int(bearing_mode), int(n_hypotheses)
        o.min_calibrated_match_count, o.min_inliers, o.refine_set, o.max_iterations = (int(min_calibrated_match_count), int(min_inliers),
                                                                                      int(refine_set), int(max_iterations))
        H = int(n_hypotheses) or LOCALIZE_IMAGES_DEFAULTS["n_hypotheses"]
        out, res = CbaLocalizeImagesOutputs(), {}
        if 0 < H <= 256:                     # (anything else is the library's to reject)
            for name, per, tail, dt in LOCALIZE_IMAGES_ARRAYS:
                if want_debug or name not in LOCALIZE_IMAGES_DEBUG:
                    res[name] = np.zeros((S if per == "slot" else F,) + tuple(H if d == "H" else d for d in tail), dtype=dt)
                    setattr(out, name, res[name].ctypes.data)
        _check(L.cba_model_localize_images(C.byref(inp), C.byref(o), C.byref(out)), "cba_model_localize_images")
        return res


class Pinhole:
    """The target of an undistortion: image size and fx, fy, cx, cy in the "pixel corner" convention."""

    def __init__(self, width: int, height: int, fx: float, fy: float, cx: float, cy: float):
        self.width, self.height = int(width), int(height)
        self.fx, self.fy, self.cx, self.cy = float(fx), float(fy), float(cx), float(cy)

    def __repr__(self):
        return f"Pinhole({self.width}, {self.height}, {self.fx!r}, {self.fy!r}, {self.cx!r}, {self.cy!r})"


def undistort_options(pinhole: Pinhole, rotation: Optional[np.ndarray] = None, initial_estimate: int = INITIAL_ESTIMATE_CENTER,
                      straggler_threshold: int = 0) -> CbaUndistortOptions:
    o = CbaUndistortOptions()
    o.width, o.height = int(pinhole.width), int(pinhole.height)
    o.fx, o.fy, o.cx, o.cy = float(pinhole.fx), float(pinhole.fy), float(pinhole.cx), float(pinhole.cy)
    o.rotation[:] = list(np.asarray(np.eye(3) if rotation is None else rotation, dtype=np.float64).reshape(9))
    o.initial_estimate, o.straggler_threshold = int(initial_estimate), int(straggler_threshold)
    return o


class Remap:
    """cba_remap: a device-resident float map (H, W, 2; pixel-centre convention, NaN = no source) and the bilinear remap of uint8
    images through it.  Build it from a model (``Remap.from_model``: the map never leaves the device) or from an explicit map."""

    def __init__(self, map_xy: np.ndarray, device: int = 0):
        self.L = load()
        m = np.ascontiguousarray(map_xy, dtype=np.float32)
        if m.ndim != 3 or m.shape[2] != 2:
            raise ValueError("Remap: the map is (H, W, 2)")
        self.height, self.width = int(m.shape[0]), int(m.shape[1])
        self._h = C.c_void_p()
        _check(self.L.cba_remap_create_from_map(self.width, self.height, m.ctypes.data_as(_F32P), int(device), C.byref(self._h)),
               "cba_remap_create_from_map")

    @classmethod
    def from_model(cls, model: "DeviceModel", pinhole: Pinhole, rotation: Optional[np.ndarray] = None,
                   initial_estimate: int = INITIAL_ESTIMATE_CENTER, straggler_threshold: int = 0) -> "Remap":
        self = cls.__new__(cls)
        self.L = load()
        self.height, self.width = int(pinhole.height), int(pinhole.width)
        self._h = C.c_void_p()
        o = undistort_options(pinhole, rotation, initial_estimate, straggler_threshold)
        _check(self.L.cba_remap_create(model._h, C.byref(o), C.byref(self._h)), "cba_remap_create")
        return self

    def close(self):
        if getattr(self, "_h", None):
            self.L.cba_remap_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def get_map(self) -> np.ndarray:
        out = np.zeros((self.height, self.width, 2), dtype=np.float32)
        _check(self.L.cba_remap_get_map(self._h, out.ctypes.data_as(_F32P)), "cba_remap_get_map")
        return out

    @staticmethod
    def _layout(shape):
        """(n, src_h, src_w, channels, batched) of an (H, W), (H, W, 3), (N, H, W, 1) or (N, H, W, 3) image array"""
        if len(shape) == 2:
            return 1, shape[0], shape[1], 1, False
        if len(shape) == 3 and shape[2] == 3:
            return 1, shape[0], shape[1], 3, False
        if len(shape) == 4:
            return shape[0], shape[1], shape[2], shape[3], True
        raise ValueError("images: (H, W), (H, W, 3) or a batch (N, H, W, C)")

    def _out_shape(self, n, ch, batched, squeeze):
        shape = (self.height, self.width) if squeeze else (self.height, self.width, ch)
        return (n,) + shape if batched else shape

    def apply(self, images, fill: int = 0):
        """A numpy uint8 array goes through cba_remap_apply and comes back as one; a torch uint8 tensor on the handle's device goes
        through cba_remap_apply_device on torch's current stream and comes back as a tensor (no host copy, no synchronisation)."""
        if isinstance(images, np.ndarray):
            src = np.ascontiguousarray(images)
            if src.dtype != np.uint8:
                raise ValueError("images: uint8")
            n, sh, sw, ch, batched = self._layout(src.shape)
            dst = np.zeros(self._out_shape(n, ch, batched, src.ndim == 2), dtype=np.uint8)
            _check(self.L.cba_remap_apply(self._h, n, sw, sh, ch, src.ctypes.data, dst.ctypes.data, int(fill)), "cba_remap_apply")
            return dst
        import torch
        if not isinstance(images, torch.Tensor) or images.dtype != torch.uint8 or not images.is_cuda:
            raise ValueError("images: a numpy uint8 array or a torch uint8 tensor on the GPU")
        src = images.contiguous()
        n, sh, sw, ch, batched = self._layout(tuple(src.shape))
        dst = torch.empty(self._out_shape(n, ch, batched, src.dim() == 2), dtype=torch.uint8, device=src.device)
        stream = torch.cuda.current_stream(src.device).cuda_stream
        _check(self.L.cba_remap_apply_device(self._h, n, sw, sh, ch, src.data_ptr(), dst.data_ptr(), int(fill), stream), "cba_remap_apply_device")
        return dst


def stereo_options(context_radius: int = 10, iterations: int = 50, min_depth: float = 0.3, max_depth: float = 20.0,
                   max_normal_2d_length: float = 1.0, cost_threshold: float = 1.0, angle_threshold: float = 1.3,
                   lr_consistency_factor_threshold: float = 1.025, seed: int = 0) -> CbaStereoOptions:
    """cba_stereo_options; the defaults are the reference tool's settings and its matcher's defaults."""
    return CbaStereoOptions(int(context_radius), int(iterations), float(min_depth), float(max_depth), float(max_normal_2d_length),
                            float(cost_threshold), float(angle_threshold), float(lr_consistency_factor_threshold), int(seed) & (2 ** 64 - 1))


def stereo_post_options(bilateral_sigma_xy: float = 1.5, bilateral_radius_factor: float = 2.0, bilateral_sigma_inv_depth: float = 0.005,
                        hole_filling_iterations: int = 3, min_component_size: int = 50, similar_depth_ratio: float = 1.005) -> CbaStereoPostOptions:
    """cba_stereo_post_options (include/cba_stereo_post.h; a 0 selects the member's default, -1 no hole filling / every component kept);
    the defaults are the reference matcher's and its tool's."""
    return CbaStereoPostOptions(float(bilateral_sigma_xy), float(bilateral_radius_factor), float(bilateral_sigma_inv_depth),
                                int(hole_filling_iterations), int(min_component_size), float(similar_depth_ratio))


class StereoHandle:
    """cba_stereo (include/cba_stereo.h): one matching direction on the device.  unprojection (H, W, 2) and projection (PH, PW, 2)
    float32, grid = (fx, fy, cx, cy) of the projection lookup's pinhole, stereo_tr_reference 12 floats (row-major 3 x 4)."""

    def __init__(self, unprojection: np.ndarray, stereo_size, projection: np.ndarray, grid, stereo_tr_reference: np.ndarray, device: int = 0):
        self.L = load()
        u = np.ascontiguousarray(unprojection, dtype=np.float32)
        p = np.ascontiguousarray(projection, dtype=np.float32)
        if u.ndim != 3 or u.shape[2] != 2 or p.ndim != 3 or p.shape[2] != 2:
            raise ValueError("StereoHandle: the lookups are (H, W, 2)")
        self.height, self.width = int(u.shape[0]), int(u.shape[1])
        self.stereo_width, self.stereo_height = int(stereo_size[0]), int(stereo_size[1])
        m = np.ascontiguousarray(stereo_tr_reference, dtype=np.float32).reshape(12)
        self._h = C.c_void_p()
        _check(self.L.cba_stereo_create(self.width, self.height, self.stereo_width, self.stereo_height, u.ctypes.data_as(_F32P),
                                        float(grid[0]), float(grid[1]), float(grid[2]), float(grid[3]), int(p.shape[1]), int(p.shape[0]),
                                        p.ctypes.data_as(_F32P), m.ctypes.data_as(_F32P), int(device), C.byref(self._h)), "cba_stereo_create")

    def close(self):
        if getattr(self, "_h", None):
            self.L.cba_stereo_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_images(self, reference_image: np.ndarray, stereo_image: np.ndarray) -> None:
        a, b = np.ascontiguousarray(reference_image, dtype=np.uint8), np.ascontiguousarray(stereo_image, dtype=np.uint8)
        if a.shape != (self.height, self.width) or b.shape != (self.stereo_height, self.stereo_width):
            raise ValueError("StereoHandle.set_images: 8-bit one-channel images of the two cameras' sizes")
        _check(self.L.cba_stereo_set_images(self._h, a.ctypes.data_as(_U8), b.ctypes.data_as(_U8)), "cba_stereo_set_images")

    def set_pose(self, stereo_tr_reference: np.ndarray) -> None:
        m = np.ascontiguousarray(stereo_tr_reference, dtype=np.float32).reshape(12)
        _check(self.L.cba_stereo_set_pose(self._h, m.ctypes.data_as(_F32P)), "cba_stereo_set_pose")

    def match(self, options: CbaStereoOptions) -> None:
        _check(self.L.cba_stereo_match(self._h, C.byref(options)), "cba_stereo_match")

    def run_stage(self, options: CbaStereoOptions, stage: int, pass_index: int) -> None:
        _check(self.L.cba_stereo_run_stage(self._h, C.byref(options), int(stage), int(pass_index)), "cba_stereo_run_stage")

    def get_state(self):
        """(inv_depth (H, W) float32, normal (H, W, 2) int8, cost (H, W) float32)"""
        d = np.zeros((self.height, self.width), dtype=np.float32)
        n = np.zeros((self.height, self.width, 2), dtype=np.int8)
        c = np.zeros((self.height, self.width), dtype=np.float32)
        _check(self.L.cba_stereo_get_state(self._h, d.ctypes.data_as(_F32P), n.ctypes.data_as(_I8P), c.ctypes.data_as(_F32P)), "cba_stereo_get_state")
        return d, n, c

    def _state_arrays(self, inv_depth, normal, cost=None):
        d = np.ascontiguousarray(inv_depth, dtype=np.float32)
        n = np.ascontiguousarray(normal, dtype=np.int8)
        c = None if cost is None else np.ascontiguousarray(cost, dtype=np.float32)
        if d.shape != (self.height, self.width) or n.shape != (self.height, self.width, 2) or (c is not None and c.shape != d.shape):
            raise ValueError("StereoHandle: a state is inv_depth (H, W), normal (H, W, 2), cost (H, W)")
        return d, n, c

    def set_state(self, inv_depth, normal, cost) -> None:
        d, n, c = self._state_arrays(inv_depth, normal, cost)
        _check(self.L.cba_stereo_set_state(self._h, d.ctypes.data_as(_F32P), n.ctypes.data_as(_I8P), c.ctypes.data_as(_F32P)), "cba_stereo_set_state")

    def cost(self, options: CbaStereoOptions, inv_depth, normal) -> np.ndarray:
        d, n, _ = self._state_arrays(inv_depth, normal)
        out = np.zeros((self.height, self.width), dtype=np.float32)
        _check(self.L.cba_stereo_cost(self._h, C.byref(options), d.ctypes.data_as(_F32P), n.ctypes.data_as(_I8P), out.ctypes.data_as(_F32P)),
               "cba_stereo_cost")
        return out

    def filter(self, options: CbaStereoOptions, other_inv_depth: Optional[np.ndarray] = None) -> np.ndarray:
        other = None
        if other_inv_depth is not None:
            other = np.ascontiguousarray(other_inv_depth, dtype=np.float32)
            if other.shape != (self.stereo_height, self.stereo_width):
                raise ValueError("StereoHandle.filter: the other direction's map has the stereo image's size")
        out = np.zeros((self.height, self.width), dtype=np.float32)
        _check(self.L.cba_stereo_filter(self._h, C.byref(options), other.ctypes.data_as(_F32P) if other is not None else None,
                                        out.ctypes.data_as(_F32P)), "cba_stereo_filter")
        return out

    def _other_map(self, other_inv_depth, who: str):
        if other_inv_depth is None:
            return None
        other = np.ascontiguousarray(other_inv_depth, dtype=np.float32)
        if other.shape != (self.stereo_height, self.stereo_width):
            raise ValueError(f"StereoHandle.{who}: the other direction's map has the stereo image's size")
        return other

    def post_stage(self, options: CbaStereoOptions, post_options: CbaStereoPostOptions, stage: int, inv_depth, cost=None):
        """cba_stereo_post_stage: one post-processing stage on a given map; the state is not touched.  Returns the map, and for the
        median (which needs `cost`) the pair (map, cost)."""
        d = np.ascontiguousarray(inv_depth, dtype=np.float32)
        c = None if cost is None else np.ascontiguousarray(cost, dtype=np.float32)
        if d.shape != (self.height, self.width) or (c is not None and c.shape != d.shape):
            raise ValueError("StereoHandle.post_stage: maps of the reference image's size")
        out = np.zeros_like(d)
        cost_out = None if c is None else np.zeros_like(d)
        _check(self.L.cba_stereo_post_stage(self._h, C.byref(options), C.byref(post_options), int(stage), d.ctypes.data_as(_F32P),
                                            c.ctypes.data_as(_F32P) if c is not None else None, out.ctypes.data_as(_F32P),
                                            cost_out.ctypes.data_as(_F32P) if c is not None else None), "cba_stereo_post_stage")
        return out if c is None else (out, cost_out)

    def finish(self, options: CbaStereoOptions, post_options: CbaStereoPostOptions, other_inv_depth: Optional[np.ndarray] = None) -> np.ndarray:
        """cba_stereo_finish: median of the state, filter, bilateral, hole filling, components, all on the device."""
        other = self._other_map(other_inv_depth, "finish")
        out = np.zeros((self.height, self.width), dtype=np.float32)
        _check(self.L.cba_stereo_finish(self._h, C.byref(options), C.byref(post_options),
                                        other.ctypes.data_as(_F32P) if other is not None else None, out.ctypes.data_as(_F32P)), "cba_stereo_finish")
        return out


def _u8_or_none(a):
    return None if a is None else a.ctypes.data_as(_U8)


class CloudPair:
    """cba_cloud_pair (include/cba_point_cloud.h): the common pixels of two depth maps of one image and their two clouds on the
    device.  Build one with ``from_clouds`` (the files' path) or ``from_depth`` (two in-memory stereo results)."""

    def __init__(self, handle, width: int, height: int):
        self.L = load()
        self._h, self.width, self.height = handle, int(width), int(height)

    @classmethod
    def from_clouds(cls, depth_target, depth_source, context_radius: int, xyz_target, grey_target, xyz_source, grey_source, device: int = 0):
        """Depth maps (H, W) float32, positions (n, 3) float32, grey (n,) uint8 or None."""
        L = load()
        dt, ds = np.ascontiguousarray(depth_target, dtype=np.float32), np.ascontiguousarray(depth_source, dtype=np.float32)
        if dt.ndim != 2 or ds.shape != dt.shape:
            raise ValueError("CloudPair: two depth maps (H, W) of the same size")
        xt, xs = (np.ascontiguousarray(a, dtype=np.float32).reshape(-1, 3) for a in (xyz_target, xyz_source))
        gt, gs = (None if g is None else np.ascontiguousarray(g, dtype=np.uint8).reshape(-1) for g in (grey_target, grey_source))
        if (gt is not None and gt.size != xt.shape[0]) or (gs is not None and gs.size != xs.shape[0]):
            raise ValueError("CloudPair: one grey value per point")
        h = C.c_void_p()
        _check(L.cba_cloud_pair_create(dt.shape[1], dt.shape[0], int(context_radius), dt.ctypes.data_as(_F32P), ds.ctypes.data_as(_F32P),
                                       xt.ctypes.data_as(_F32P), xt.shape[0], _u8_or_none(gt), xs.ctypes.data_as(_F32P), xs.shape[0],
                                       _u8_or_none(gs), int(device), C.byref(h)), "cba_cloud_pair_create")
        return cls(h, dt.shape[1], dt.shape[0])

    @classmethod
    def from_depth(cls, inv_depth_target, unprojection_target, image_target, inv_depth_source, unprojection_source, image_source,
                   context_radius: int, device: int = 0):
        """Inverse-depth maps (H, W) float32, un-projection lookups (H, W, 2) float32, grey images (H, W) uint8 or None."""
        L = load()
        mt, ms = np.ascontiguousarray(inv_depth_target, dtype=np.float32), np.ascontiguousarray(inv_depth_source, dtype=np.float32)
        ut, us = np.ascontiguousarray(unprojection_target, dtype=np.float32), np.ascontiguousarray(unprojection_source, dtype=np.float32)
        if mt.ndim != 2 or ms.shape != mt.shape or ut.shape != mt.shape + (2,) or us.shape != ut.shape:
            raise ValueError("CloudPair: maps (H, W) and lookups (H, W, 2) of the same size")
        it, is_ = (None if g is None else np.ascontiguousarray(g, dtype=np.uint8) for g in (image_target, image_source))
        if (it is not None and it.shape != mt.shape) or (is_ is not None and is_.shape != mt.shape):
            raise ValueError("CloudPair: grey images of the maps' size")
        h = C.c_void_p()
        _check(L.cba_cloud_pair_create_from_depth(mt.shape[1], mt.shape[0], int(context_radius), mt.ctypes.data_as(_F32P),
                                                  ut.ctypes.data_as(_F32P), _u8_or_none(it), ms.ctypes.data_as(_F32P),
                                                  us.ctypes.data_as(_F32P), _u8_or_none(is_), int(device), C.byref(h)),
               "cba_cloud_pair_create_from_depth")
        return cls(h, mt.shape[1], mt.shape[0])

    def close(self):
        if getattr(self, "_h", None):
            self.L.cba_cloud_pair_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def counts(self):
        """(valid inner pixels of the target, of the source, common pixels)"""
        out = np.zeros(3, dtype=np.int64)
        _check(self.L.cba_cloud_pair_counts(self._h, out.ctypes.data_as(_I64P)), "cba_cloud_pair_counts")
        return int(out[0]), int(out[1]), int(out[2])

    def moments(self) -> np.ndarray:
        """17 doubles: n, mean of the source, mean of the target, covariance (target x source, row-major), variance of the source."""
        out = np.zeros(17)
        _check(self.L.cba_cloud_pair_moments(self._h, _dp(out)), "cba_cloud_pair_moments")
        return out

    def align(self, A, t):
        """(distance image (H, W) float32, stats (n, sum d, sum d^2), max distance as a float32 scalar)"""
        A32, t32 = np.ascontiguousarray(A, dtype=np.float32).reshape(9), np.ascontiguousarray(t, dtype=np.float32).reshape(3)
        image = np.zeros((self.height, self.width), dtype=np.float32)
        stats, largest = np.zeros(3), np.zeros(1, dtype=np.float32)
        _check(self.L.cba_cloud_pair_align(self._h, A32.ctypes.data_as(_F32P), t32.ctypes.data_as(_F32P), image.ctypes.data_as(_F32P),
                                           _dp(stats), largest.ctypes.data_as(_F32P)), "cba_cloud_pair_align")
        return image, stats, largest[0]

    def clouds(self):
        """(target positions (n, 3), target grey (n,), source positions after the last align (n, 3), source grey (n,))"""
        n = self.counts()[2]
        xt, xs = np.zeros((n, 3), dtype=np.float32), np.zeros((n, 3), dtype=np.float32)
        gt, gs = np.zeros(n, dtype=np.uint8), np.zeros(n, dtype=np.uint8)
        _check(self.L.cba_cloud_pair_get_clouds(self._h, xt.ctypes.data_as(_F32P), gt.ctypes.data_as(_U8), xs.ctypes.data_as(_F32P),
                                                gs.ctypes.data_as(_U8)), "cba_cloud_pair_get_clouds")
        return xt, gt, xs, gs


def render_nearest_feature_image(width: int, height: int, site_xy_quarter_px: np.ndarray, site_rgb: np.ndarray, device: int = 0,
                                 want_accum: bool = False):
    """cba_render_nearest_feature_image: rgb (H, W, 3) uint8 [, the float image (H, W, 3) float32]."""
    L = load()
    xy = np.ascontiguousarray(site_xy_quarter_px, dtype=np.int32).reshape(-1, 2)
    col = np.ascontiguousarray(site_rgb, dtype=np.float32).reshape(-1, 3)
    assert xy.shape[0] == col.shape[0]
    rgb = np.zeros((height, width, 3), dtype=np.uint8)
    acc = np.zeros((height, width, 3), dtype=np.float32) if want_accum else None
    _check(L.cba_render_nearest_feature_image(int(width), int(height), xy.shape[0], xy.ctypes.data_as(C.POINTER(C.c_int32)),
                                              col.ctypes.data_as(C.POINTER(C.c_float)), int(device),
                                              rgb.ctypes.data_as(C.POINTER(C.c_uint8)),
                                              acc.ctypes.data_as(C.POINTER(C.c_float)) if acc is not None else None),
           "cba_render_nearest_feature_image")
    return (rgb, acc) if want_accum else rgb


# ---- stateless model-level API (CameraModel::Project / Unproject) -----------------------------------
def project(cam: Camera, grid: np.ndarray, local_points: np.ndarray, init: Optional[np.ndarray] = None, device: int = 0):
    L = load()
    g = np.ascontiguousarray(grid, dtype=np.float64)
    pts = np.ascontiguousarray(local_points, dtype=np.float64).reshape(-1, 3)
    n = pts.shape[0]
    px = np.zeros((n, 2))
    ok = np.zeros(n, dtype=np.uint8)
    ini = None if init is None else np.ascontiguousarray(init, dtype=np.float64).reshape(-1, 2)
    cs = _cam_struct(cam)
    _check(L.cba_project(C.byref(cs), _dp(g), n, _dp(pts), _dp(ini) if ini is not None else None, _dp(px),
                         ok.ctypes.data_as(C.POINTER(C.c_uint8)), device), "cba_project")
    return px, ok.astype(bool)


def unproject(cam: Camera, grid: np.ndarray, pixels: np.ndarray, with_jacobian: bool = False, device: int = 0):
    L = load()
    g = np.ascontiguousarray(grid, dtype=np.float64)
    px = np.ascontiguousarray(pixels, dtype=np.float64).reshape(-1, 2)
    n = px.shape[0]
    lines = np.zeros((n, 6))
    jac = np.zeros((n, 6, 2)) if with_jacobian else None
    ok = np.zeros(n, dtype=np.uint8)
    cs = _cam_struct(cam)
    _check(L.cba_unproject(C.byref(cs), _dp(g), n, _dp(px), _dp(lines), _dp(jac) if jac is not None else None,
                           ok.ctypes.data_as(C.POINTER(C.c_uint8)), device), "cba_unproject")
    return (lines, jac, ok.astype(bool)) if with_jacobian else (lines, ok.astype(bool))


def schur_solve(block_diag_H: np.ndarray, off_diag_H: np.ndarray, dense_H: np.ndarray, block_diag_b: np.ndarray,
                dense_b: np.ndarray, device: int = 0, factor_tail_rows: int = 0, back_substitution_panels: bool = False) -> np.ndarray:
    """LMOptimizer::SolveWithSchurComplementDenseOffDiag on host arrays (reference layout); the two keyword options are
    cba_solver_options (scheduling only)."""
    L = load()
    bD = np.ascontiguousarray(block_diag_H, dtype=np.float64)
    nb, bs = bD.shape[0], bD.shape[1]
    oH = np.ascontiguousarray(off_diag_H, dtype=np.float64)
    dH = np.ascontiguousarray(dense_H, dtype=np.float64)
    bb = np.ascontiguousarray(block_diag_b, dtype=np.float64)
    db = np.ascontiguousarray(dense_b, dtype=np.float64)
    dd = dH.shape[0]
    x = np.zeros(nb * bs + dd)
    if factor_tail_rows or back_substitution_panels:
        opt = CbaSolverOptions(int(factor_tail_rows), int(bool(back_substitution_panels)), 0, 0, 0)
        _check(L.cba_schur_solve_opt(bs, nb, dd, _dp(bD), _dp(oH), _dp(dH), _dp(bb), _dp(db), _dp(x), C.byref(opt), device), "cba_schur_solve_opt")
    else:
        _check(L.cba_schur_solve(bs, nb, dd, _dp(bD), _dp(oH), _dp(dH), _dp(bb), _dp(db), _dp(x), device), "cba_schur_solve")
    return x


def reduced_system(block_diag_H: np.ndarray, off_diag_H: np.ndarray, dense_H: np.ndarray, block_diag_b: np.ndarray,
                   dense_b: np.ndarray, lam: float, mode: int, device: int = 0):
    """cba_debug_reduced_system: the pose-first reduced system of these arrays, unfactored, formed by the engine's own launches.
    mode 0 dense product, 1 block-sparse, 2 block-sparse with the chunk order.  Returns (S (n_pad, n_pad), upper triangle valid, last
    column = right-hand side; mask (n_pad / 128, mask_words) uint64; dims = (n_pad, Kpad, mask_words, n_chunks))."""
    L = load()
    bD = np.ascontiguousarray(block_diag_H, dtype=np.float64)
    nb, bs = bD.shape[0], bD.shape[1]
    oH = np.ascontiguousarray(off_diag_H, dtype=np.float64)
    dH = np.ascontiguousarray(dense_H, dtype=np.float64)
    bb = np.ascontiguousarray(block_diag_b, dtype=np.float64)
    db = np.ascontiguousarray(dense_b, dtype=np.float64)
    dd = dH.shape[0]
    assert oH.shape == (nb * bs, dd) and dH.shape == (dd, dd) and bb.size == nb * bs and db.size == dd
    dims = np.zeros(4, dtype=np.int32)
    ip = dims.ctypes.data_as(C.POINTER(C.c_int32))
    _check(L.cba_debug_reduced_system(bs, nb, dd, None, None, None, None, None, float(lam), int(mode), None, None, ip, device),
           "cba_debug_reduced_system")
    n_pad, words = int(dims[0]), int(dims[2])
    S = np.zeros((n_pad, n_pad))
    mask = np.zeros((n_pad // 128, words), dtype=np.uint64)
    _check(L.cba_debug_reduced_system(bs, nb, dd, _dp(bD), _dp(oH), _dp(dH), _dp(bb), _dp(db), float(lam), int(mode), _dp(S),
                                      mask.ctypes.data_as(C.POINTER(C.c_uint64)), ip, device), "cba_debug_reduced_system")
    return S, mask, tuple(int(v) for v in dims)


# ---- host mirror of the reference entry point ---------------------------------------------------------
def fit_grid_to_directions(cam: Camera, grid: np.ndarray, grid_points: np.ndarray, directions: np.ndarray,
                           max_iteration_count: int, device: int = 0):
    """cba_fit_grid_to_directions (CentralGenericModel::FitToPixelDirectionsImpl).  Returns (new grid (G,3), report dict)."""
    L = load()
    g = np.ascontiguousarray(grid, dtype=np.float64).reshape(-1, 3).copy()
    gp = np.ascontiguousarray(grid_points, dtype=np.float64).reshape(-1, 2)
    d = np.ascontiguousarray(directions, dtype=np.float64).reshape(-1, 3)
    assert gp.shape[0] == d.shape[0] and g.shape[0] == cam.grid_points
    cs = _cam_struct(cam)
    rep = CbaFitReport()
    _check(L.cba_fit_grid_to_directions(C.byref(cs), _dp(g), gp.shape[0], _dp(gp) if gp.size else None,
                                        _dp(d) if d.size else None, max_iteration_count, C.byref(rep), device),
           "cba_fit_grid_to_directions")
    return g, dict(initial_cost=rep.initial_cost, final_cost=rep.final_cost, final_lambda=rep.lambda_,
                   iterations=rep.iterations_performed, lm_attempts=rep.lm_attempts, t_pass=rep.t_pass, t_solve=rep.t_solve)


def optimize_jointly(problem: Problem, state: State, max_iteration_count: int, init_lambda: float = -1.0,
                     device: int = 0, engine: Optional[Engine] = None, print_progress: bool = False):
    """Python mirror of ``vis::OptimizeJointly`` (APP/bundle_adjustment/joint_optimization.h:53-70).

    ``problem`` carries numerical_diff_delta / localize_only / eliminate_points; regularization_weight
    must be 0 as in the reference (the branch is disabled there, joint_optimization.cc:299-305).
    Returns (final_cost, final_lambda, performed_an_iteration, new_state, reports).
    """
    own = engine is None
    eng = engine or Engine(problem, device)
    try:
        eng.set_state(state)
        final_cost = -1.0
        final_lambda = init_lambda
        performed = False
        reports: List[StepReport] = []
        for it in range(max_iteration_count):   # joint_optimization.cc:906-940
            rep = eng.step(init_lambda)
            reports.append(rep)
            final_cost = rep.final_cost
            init_lambda = final_lambda = rep.final_lambda
            if print_progress:
                print(f"LMOptimizer: [{it}] cost {rep.initial_cost:.9g} -> {rep.final_cost:.9g}, lambda {rep.final_lambda:.3g}, "
                      f"attempts {rep.lm_attempts}")
            if not rep.accepted:
                break
            performed = True
        return final_cost, final_lambda, performed, eng.get_state(state), reports
    finally:
        if own:
            eng.close()


def run_bundle_adjustment(engine: Engine, state: State, max_iteration_count: int = 100,
                          cost_reduction_threshold: float = 1e-4, print_progress: bool = False):
    """Outer convergence loop of the reference's ``RunBundleAdjustment`` (APP/calibration.cc:187-304):
    repeated ``OptimizeJointly(max_iteration_count=1)`` carrying lambda, stop when no update was
    performed or ``cost >= last_cost - threshold`` (:298).  The state stays device-resident between
    iterations (the reference rebuilds everything per call).  Gauge beautification
    (ChooseNiceCameraOrientation, :248-254) and state saving are outside the hot path and not done here.
    Returns (final_cost, iterations, reports)."""
    engine.set_state(state)
    lam = -1.0
    last_cost = float("inf")
    reports: List[StepReport] = []
    for it in range(max_iteration_count):
        rep = engine.step(lam)
        reports.append(rep)
        lam = rep.final_lambda
        if print_progress:
            print(f"[{it}] cost {rep.final_cost:.9g} lambda {lam:.3g} attempts {rep.lm_attempts}")
        if not rep.accepted:
            break
        if rep.final_cost >= last_cost - cost_reduction_threshold:
            break
        last_cost = rep.final_cost
    return reports[-1].final_cost, len(reports), reports
