"""ctypes binding of include/erp_match.h (the C ABI of lib/liberp_match.so).

This is exactly the binding a Python user of the reference path would add (see
INTEGRATION.md).  There is no CPU fallback: if the HIP library is missing or no device is
visible, every entry point raises.
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

from . import _build

P = C.c_void_p

ERP_OK = 0
ERP_INVALID_ARG = 1
ERP_TOO_FEW_POINTS = 2
ERP_NO_VALID_HYPOTHESIS = 3
ERP_HIP_ERROR = 4
ERP_NO_DEVICE = 5
ERP_OUT_OF_MEMORY = 6
ERP_INTERNAL = 7
STATUS_NAMES = {0: "ok", 1: "invalid argument", 2: "too few points",
                3: "no valid rotation hypothesis", 4: "HIP error", 5: "no HIP device",
                6: "out of device memory", 7: "internal consistency check failed"}


class DMatch(C.Structure):
    _fields_ = [("queryIdx", C.c_int32), ("trainIdx", C.c_int32), ("imgIdx", C.c_int32),
                ("distance", C.c_float)]


class Point2f(C.Structure):
    _fields_ = [("x", C.c_float), ("y", C.c_float)]


class RansacCfg(C.Structure):
    _fields_ = [("iters", C.c_int32), ("sampler", C.c_int32), ("sample_frac", C.c_double),
                ("trim_lo", C.c_double), ("trim_hi", C.c_double), ("valid_abs", C.c_double),
                ("seed", C.c_uint32), ("inlier_thr", C.c_float), ("offset", C.c_uint64)]


class Hypothesis(C.Structure):
    _fields_ = [("R1", C.c_float * 3), ("R2", C.c_float * 3), ("T", C.c_float * 3),
                ("R1_valid", C.c_int32), ("R2_valid", C.c_int32), ("inliers", C.c_int32),
                ("E", C.c_double * 9)]


class PairResult(C.Structure):
    _fields_ = [("R", C.c_float * 3), ("T", C.c_float * 3), ("status", C.c_int32),
                ("M", C.c_int32), ("K", C.c_int32), ("min_idx", C.c_int32),
                ("sample_n", C.c_int32), ("near_ties", C.c_int32), ("survivors", C.c_int32),
                ("binned_rows", C.c_int32), ("min_dist", C.c_double)]


class PairBatch(C.Structure):
    _fields_ = [("n_pairs", C.c_int32), ("dim", C.c_int32), ("max_nq", C.c_int32),
                ("max_nt", C.c_int32), ("desc_l", P), ("desc_r", P), ("kp_l", P), ("kp_r", P),
                ("off_l", P), ("off_r", P), ("width", P), ("height", P)]


class BatchOutputs(C.Structure):
    _fields_ = [("results", P), ("matches", P), ("key_left", P), ("key_right", P), ("hyps", P),
                ("samples", P), ("rvec", P), ("tvec", P), ("dist", P)]


class PolishRound(C.Structure):
    _fields_ = [("R", C.c_float * 3), ("T", C.c_float * 3), ("n_fit", C.c_int32),
                ("n_inliers", C.c_int32), ("which", C.c_int32), ("reserved", C.c_int32),
                ("E", C.c_double * 9)]


class PolishResult(C.Structure):
    _fields_ = [("R", C.c_float * 3), ("T", C.c_float * 3), ("status", C.c_int32),
                ("winner_iter", C.c_int32), ("winner_which", C.c_int32),
                ("rounds_done", C.c_int32), ("n_inliers", C.c_int32),
                ("n_inliers_winner", C.c_int32), ("E", C.c_double * 9)]


class PolishInputs(C.Structure):
    _fields_ = [("n_pairs", C.c_int32), ("iters", C.c_int32), ("key_stride", C.c_int64),
                ("key_left", P), ("key_right", P), ("width", P), ("height", P), ("results", P),
                ("hyps", P)]


class Winner(C.Structure):
    _fields_ = [("status", C.c_int32), ("iter", C.c_int32), ("which", C.c_int32),
                ("sample_n", C.c_int32), ("E", C.c_double * 9)]


class Support(C.Structure):
    _fields_ = [("status", C.c_int32), ("iter", C.c_int32), ("which", C.c_int32),
                ("inliers", C.c_int32), ("scored", C.c_int32), ("consensus_iter", C.c_int32),
                ("consensus_inliers", C.c_int32), ("row", C.c_int32)]


class SupportOutputs(C.Structure):
    _fields_ = [("support", P), ("winners", P), ("results", P), ("counts", P)]


class Pose(C.Structure):
    _fields_ = [("status", C.c_int32), ("which", C.c_int32), ("t_sign", C.c_int32),
                ("n_voters", C.c_int32), ("votes", C.c_int32 * 4), ("rot_agrees", C.c_int32),
                ("t_flipped", C.c_int32), ("R", C.c_float * 3), ("T", C.c_float * 3),
                ("Rm", C.c_double * 9), ("t", C.c_double * 3)]


class PoseInputs(C.Structure):
    _fields_ = [("n_pairs", C.c_int32), ("reserved", C.c_int32), ("key_stride", C.c_int64),
                ("key_left", P), ("key_right", P), ("width", P), ("height", P), ("results", P),
                ("e", P), ("e_stride", C.c_int64), ("src_status", P),
                ("src_status_stride", C.c_int64), ("mask", P)]


class GuidedCfg(C.Structure):
    _fields_ = [("thr", C.c_float), ("ratio", C.c_float), ("max_dist", C.c_float),
                ("unique", C.c_int32)]


class GuidedInputs(C.Structure):
    _fields_ = [("batch", PairBatch), ("results", P), ("e", P), ("e_stride", C.c_int64),
                ("src_status", P), ("src_status_stride", C.c_int64)]


class GuidedOutputs(C.Structure):
    _fields_ = [("count", P), ("matches", P), ("key_left", P), ("key_right", P), ("gated", P),
                ("results_out", P), ("winners_out", P)]


DMATCH_DTYPE = np.dtype([("queryIdx", "<i4"), ("trainIdx", "<i4"), ("imgIdx", "<i4"),
                         ("distance", "<f4")])
HYP_DTYPE = np.dtype([("R1", "<f4", 3), ("R2", "<f4", 3), ("T", "<f4", 3), ("R1_valid", "<i4"),
                      ("R2_valid", "<i4"), ("inliers", "<i4"), ("E", "<f8", 9)], align=True)
RESULT_DTYPE = np.dtype([("R", "<f4", 3), ("T", "<f4", 3), ("status", "<i4"), ("M", "<i4"),
                         ("K", "<i4"), ("min_idx", "<i4"), ("sample_n", "<i4"),
                         ("near_ties", "<i4"), ("survivors", "<i4"), ("binned_rows", "<i4"),
                         ("min_dist", "<f8")], align=True)
POLISH_ROUND_DTYPE = np.dtype([("R", "<f4", 3), ("T", "<f4", 3), ("n_fit", "<i4"),
                               ("n_inliers", "<i4"), ("which", "<i4"), ("reserved", "<i4"),
                               ("E", "<f8", 9)], align=True)
POLISH_DTYPE = np.dtype([("R", "<f4", 3), ("T", "<f4", 3), ("status", "<i4"),
                         ("winner_iter", "<i4"), ("winner_which", "<i4"), ("rounds_done", "<i4"),
                         ("n_inliers", "<i4"), ("n_inliers_winner", "<i4"), ("E", "<f8", 9)],
                        align=True)
WINNER_DTYPE = np.dtype([("status", "<i4"), ("iter", "<i4"), ("which", "<i4"), ("sample_n", "<i4"),
                         ("E", "<f8", 9)], align=True)
SUPPORT_DTYPE = np.dtype([("status", "<i4"), ("iter", "<i4"), ("which", "<i4"), ("inliers", "<i4"),
                          ("scored", "<i4"), ("consensus_iter", "<i4"),
                          ("consensus_inliers", "<i4"), ("row", "<i4")], align=True)
POSE_DTYPE = np.dtype([("status", "<i4"), ("which", "<i4"), ("t_sign", "<i4"), ("n_voters", "<i4"),
                       ("votes", "<i4", 4), ("rot_agrees", "<i4"), ("t_flipped", "<i4"),
                       ("R", "<f4", 3), ("T", "<f4", 3), ("Rm", "<f8", 9), ("t", "<f8", 3)],
                      align=True)
POLISH_MAX_ROUNDS = 8


def support_to_numpy(t) -> np.ndarray:
    """erp_support records (PairBatchRunner.run(..., want=("support",)) "support": a torch uint8
    tensor [P, 32], or a numpy array of those bytes) -> [P] of SUPPORT_DTYPE"""
    a = t.cpu().numpy() if hasattr(t, "cpu") else np.ascontiguousarray(t)
    return a.view(SUPPORT_DTYPE).reshape(-1)


assert POSE_DTYPE.itemsize == C.sizeof(Pose) == 160
assert C.sizeof(PoseInputs) == 96
assert C.sizeof(GuidedCfg) == 16 and C.sizeof(GuidedInputs) == 120 and \
    C.sizeof(GuidedOutputs) == 56
assert WINNER_DTYPE.itemsize == C.sizeof(Winner) == 88
assert SUPPORT_DTYPE.itemsize == C.sizeof(Support) == 32 and C.sizeof(SupportOutputs) == 32
assert DMATCH_DTYPE.itemsize == C.sizeof(DMatch) == 16
assert POLISH_ROUND_DTYPE.itemsize == C.sizeof(PolishRound) == 112
assert POLISH_DTYPE.itemsize == C.sizeof(PolishResult) == 120
assert C.sizeof(PolishInputs) == 64
assert HYP_DTYPE.itemsize == C.sizeof(Hypothesis) == 120
assert RESULT_DTYPE.itemsize == C.sizeof(PairResult) == 64
assert C.sizeof(RansacCfg) == 56

# every symbol include/erp_match.h declares (checked by tests/test_capi_symbols.py)
EXPORTED = ["erp_ctx_create", "erp_ctx_destroy", "erp_status_string", "erp_ransac_cfg_default",
            "erp_abi_version", "erp_ctx_reserve", "erp_match_knn2_ratio", "erp_match_two_image",
            "erp_eight_point_find_dev", "erp_eight_point_find", "erp_initial_guess",
            "erp_eight_point_estimation", "erp_pair_batch_run", "erp_ctx_set_profiling",
            "erp_stage_name", "erp_ctx_stage_times", "erp_eight_point_hypotheses_dev",
            "erp_consensus_dev", "erp_ctx_set_matcher", "erp_consensus_hyps_dev",
            "erp_crop_rotated_image_dev", "erp_spherical_bands_dev", "erp_rotate_keypoints_dev",
            "erp_unrotate_band_keypoints_dev", "erp_rotate_image_dev", "erp_rectify_dev",
            "erp_vertical_rotate_dev", "erp_eular2rot", "erp_rot2eular", "erp_rot_from_vec",
            "erp_inv3", "erp_rectify_matrices", "erp_consensus_hyps_shard_dev",
            "erp_consensus_hyps_finish_dev", "erp_surf_params_default",
            "erp_surf_detect_compute_dev", "erp_epipolar_draw_dev", "erp_draw_match_dev",
            "erp_random_shuffle_prefix", "erp_ctx_set_graphs", "erp_debug_check_pads", "erp_debug_lip_counters",
            "erp_debug_snapshot", "erp_ctx_set_option", "erp_ctx_get_option",
            "erp_debug_set_alloc_pad", "erp_pack_band_features_dev",
            "erp_image_pairs_features_dev", "erp_image_pairs_run",
            "erp_rand_stream_create", "erp_rand_stream_destroy", "erp_rand_stream_get",
            "erp_rand_stream_set", "erp_rand_stream_advance", "erp_rand_stream_process",
            "erp_ctx_set_rand_stream", "erp_ctx_get_rand_stream",
            "erp_rand_stream_shuffle_prefix", "erp_image_sweep_features_dev",
            "erp_image_sweep_run", "erp_match_error_dev", "erp_vertical_rotate_batch_dev",
            "erp_rectify_batch_dev", "erp_rectify_results_dev", "erp_rectify_matrices_results",
            "erp_polish_dev", "erp_eight_point_find_polished", "erp_pair_batch_run_winners",
            "erp_eight_point_find_winner_dev", "erp_eight_point_find_winner",
            "erp_polish_winners_dev", "erp_pose_select_dev", "erp_eight_point_find_posed",
            "erp_match_guided_dev", "erp_match_guided", "erp_pair_batch_run_support",
            "erp_eight_point_find_support_dev", "erp_eight_point_find_support",
            "erp_stereo_params_default", "erp_stereo_rows_dev",
            "erp_stereo_params_ex_default", "erp_stereo_rows_ex_dev"]
STAGES = ["knn2_filter", "knn2_merge", "bearings", "jump_prep", "sampler", "eigen",
          "valid_compact", "consensus_rows", "consensus_final", "consensus_bounds",
          "consensus_select", "windows", "gram", "knn2_candidates", "knn2_rescore",
          "consensus_refine", "knn2_exact", "sampler_gram", "inliers"]
# erp_ctx_option (include/erp_match.h): route options, results identical on every setting
OPTIONS = {"small_batch": 0, "sampler_lat": 1, "sampler_split": 2, "gram_tiles": 3,
           "zoom_levels": 4, "small_zoom": 5, "lip2": 6, "lipg": 7, "refine_hint": 8,
           "flat_refs": 9, "bound_ratio": 10, "debug_stages": 11, "debug_snap": 12,
           "sampler_tiers": 13, "vertical_shared": 14, "sampler_share": 15,
           "support_count": 16, "stereo_chunk_mb": 17}
MATCHER_MFMA_FILTER = 0  # erp_matcher_method
MATCHER_VALU_EXACT = 1


class SurfParams(C.Structure):
    _fields_ = [("hessian_threshold", C.c_double), ("n_octaves", C.c_int32),
                ("n_octave_layers", C.c_int32), ("extended", C.c_int32), ("upright", C.c_int32)]


class PackedPairs(C.Structure):
    _fields_ = [("desc_l", P), ("desc_r", P), ("kp_l", P), ("kp_r", P), ("off_l", P), ("off_r", P),
                ("width", P), ("height", P), ("band_counts", P), ("cap_l", C.c_int64),
                ("cap_r", C.c_int64)]


class ImageBatchInfo(C.Structure):
    _fields_ = [("need_kp", C.c_int32), ("max_nq", C.c_int32), ("max_nt", C.c_int32),
                ("groups", C.c_int32), ("fits", C.c_int32), ("reserved", C.c_int32),
                ("rows_l", C.c_int64), ("rows_r", C.c_int64)]


assert C.sizeof(PackedPairs) == 88 and C.sizeof(ImageBatchInfo) == 40


STEREO_INVALID = -32768  # ERP_STEREO_INVALID


class StereoParams(C.Structure):
    _fields_ = [("d_min", C.c_int32), ("n_disp", C.c_int32), ("p1", C.c_int32), ("p2", C.c_int32),
                ("lr_max", C.c_int32), ("wrap_rows", C.c_int32), ("channels", C.c_int32)]


class StereoParamsEx(C.Structure):  # erp_stereo_params_ex: rules 4b (n_paths) and 6b (uniqueness)
    _fields_ = [("base", StereoParams), ("n_paths", C.c_int32), ("uniqueness", C.c_int32),
                ("reserved", C.c_int32 * 2)]


assert C.sizeof(StereoParams) == 28 and C.sizeof(StereoParamsEx) == 44


class RectifyOutputs(C.Structure):
    _fields_ = [("left_rect", P), ("right_rect", P), ("left_vertical", P), ("right_vertical", P),
                ("done", P)]


KEYPOINT_DTYPE = np.dtype([("x", "<f4"), ("y", "<f4"), ("size", "<f4"), ("angle", "<f4"),
                           ("response", "<f4"), ("octave", "<i4"), ("class_id", "<i4")])
assert KEYPOINT_DTYPE.itemsize == 28


class ErpError(RuntimeError):
    def __init__(self, status: int, where: str):
        super().__init__(f"{where}: {STATUS_NAMES.get(status, status)} (erp_status {status})")
        self.status = status


_lib = None


def lib_path() -> str:
    # ERP_LIB_PATH: a development build elsewhere (A/B experiments); default: the in-tree library
    return os.environ.get("ERP_LIB_PATH") or _build.LIB_PATH


def load(build_if_missing: bool = False):
    """Load lib/liberp_match.so.  Raises if it is missing: there is no fallback path."""
    global _lib
    if _lib is not None:
        return _lib
    path = lib_path()
    if not os.path.exists(path):
        if build_if_missing:
            _build.build()
        else:
            raise RuntimeError(f"HIP library {path} is not built; run __graft_entry__.build() or "
                               "python -m erp_match_eightpoint_test_amd._build")
    L = C.CDLL(path)
    L.erp_ctx_create.argtypes = [C.c_int32, C.POINTER(P)]
    L.erp_ctx_destroy.argtypes = [P]
    L.erp_status_string.argtypes = [C.c_int]
    L.erp_status_string.restype = C.c_char_p
    L.erp_ransac_cfg_default.argtypes = [C.POINTER(RansacCfg)]
    L.erp_ransac_cfg_default.restype = None
    L.erp_abi_version.restype = C.c_int32
    L.erp_ctx_reserve.argtypes = [P, C.c_int32, C.c_int32, C.c_int32, C.c_int32]
    L.erp_match_knn2_ratio.argtypes = [P, P, C.c_int32, P, C.c_int32, C.c_int32, C.c_float, P, P, P]
    L.erp_match_two_image.argtypes = [P, P, C.c_int32, P, C.c_int32, C.c_int32, P, P]
    L.erp_eight_point_find_dev.argtypes = [P, C.c_int32, C.c_int32, P, P, C.c_int32,
                                           C.POINTER(RansacCfg), P, P, P]
    L.erp_eight_point_find.argtypes = [P, C.c_int32, C.c_int32, P, P, C.c_int32,
                                       C.POINTER(RansacCfg), P, P, P]
    L.erp_initial_guess.argtypes = [P, P, P, C.c_int32, C.POINTER(RansacCfg), P, P, P]
    L.erp_eight_point_estimation.argtypes = [P, P, P, C.c_int32, P]
    L.erp_pair_batch_run.argtypes = [P, C.POINTER(PairBatch), C.c_float, C.POINTER(RansacCfg),
                                     C.POINTER(BatchOutputs), P]
    L.erp_eight_point_hypotheses_dev.argtypes = [P, C.c_int32, C.c_int32, P, P, C.c_int32,
                                                 C.POINTER(RansacCfg), P, P]
    L.erp_consensus_dev.argtypes = [P, P, P, C.c_int32, C.c_double, C.c_double, P, P]
    L.erp_ctx_set_profiling.argtypes = [P, C.c_int32]
    L.erp_ctx_set_matcher.argtypes = [P, C.c_int32]
    L.erp_ctx_set_graphs.argtypes = [P, C.c_int32]
    L.erp_ctx_set_option.argtypes = [P, C.c_int32, C.c_int32]
    L.erp_ctx_get_option.argtypes = [P, C.c_int32, C.POINTER(C.c_int32)]
    L.erp_debug_set_alloc_pad.argtypes = [C.c_size_t]
    L.erp_debug_set_alloc_pad.restype = None
    L.erp_debug_check_pads.restype = C.c_int
    L.erp_debug_check_pads.argtypes = []
    L.erp_debug_lip_counters.restype = C.c_int
    L.erp_debug_lip_counters.argtypes = [C.c_void_p]
    L.erp_debug_snapshot.restype = C.c_longlong
    L.erp_debug_snapshot.argtypes = [P, C.c_void_p, C.c_size_t]
    L.erp_crop_rotated_image_dev.argtypes = [P, P, C.c_int32, C.c_int32, C.c_float, P, P]
    L.erp_spherical_bands_dev.argtypes = [P, P, C.c_int32, C.c_int32, C.c_int32, P, P]
    L.erp_rotate_keypoints_dev.argtypes = [P, P, C.c_int32, C.c_float, C.c_int32, C.c_int32, P]
    L.erp_unrotate_band_keypoints_dev.argtypes = [P, P, P, C.c_int32, C.c_int32, P]
    L.erp_rotate_image_dev.argtypes = [P, P, C.c_int32, C.c_int32, P, P, P]
    L.erp_rectify_dev.argtypes = [P, P, P, C.c_int32, C.c_int32, P, P, P, P, P]
    L.erp_vertical_rotate_dev.argtypes = [P, P, C.c_int32, C.c_int32, P, P]
    L.erp_eular2rot.argtypes = [P, P]
    L.erp_eular2rot.restype = None
    L.erp_rot2eular.argtypes = [P, P]
    L.erp_rot2eular.restype = None
    L.erp_rot_from_vec.argtypes = [P, P, P]
    L.erp_rot_from_vec.restype = None
    L.erp_inv3.argtypes = [P, P]
    L.erp_inv3.restype = C.c_int32
    L.erp_rectify_matrices.argtypes = [P, P, P, P]
    L.erp_vertical_rotate_batch_dev.argtypes = [P, P, C.c_int32, C.c_int32, C.c_int32, C.c_int32,
                                                P, P]
    L.erp_rectify_batch_dev.argtypes = [P, P, P, C.c_int32, C.c_int32, C.c_int32, P, P, P,
                                        C.c_int32, C.POINTER(RectifyOutputs), P]
    L.erp_rectify_results_dev.argtypes = [P, P, P, C.c_int32, C.c_int32, C.c_int32, P, C.c_int32,
                                          C.POINTER(RectifyOutputs), P]
    L.erp_rectify_matrices_results.argtypes = [P, C.c_int32, P, P, P]
    L.erp_consensus_hyps_shard_dev.argtypes = [P, C.c_int32, P, C.c_int32, C.POINTER(RansacCfg),
                                               C.c_int32, C.c_int32, P, P, P, P]
    L.erp_consensus_hyps_finish_dev.argtypes = [P, C.c_int32, P, C.c_int32, C.POINTER(RansacCfg),
                                                P, P, P, P, P]
    L.erp_surf_params_default.argtypes = [C.POINTER(SurfParams)]
    L.erp_surf_params_default.restype = None
    L.erp_surf_detect_compute_dev.argtypes = [P, P, C.c_int32, C.c_int32, C.c_int32, C.c_int32,
                                              C.POINTER(SurfParams), C.c_int32, P, P, P, P]
    L.erp_consensus_hyps_dev.argtypes = [P, C.c_int32, P, C.c_int32, C.POINTER(RansacCfg), P, P]
    L.erp_epipolar_draw_dev.argtypes = [P, P, P, C.c_int32, C.c_int32, C.c_int32, C.c_int32,
                                        C.c_int32, C.c_int32, C.c_uint32, C.c_uint64, P, P, P, P]
    L.erp_draw_match_dev.argtypes = [P, P, P, C.c_int32, C.c_int32, P, P, C.c_int32, P, P]
    L.erp_random_shuffle_prefix.argtypes = [C.c_uint32, C.c_uint64, C.c_int32, C.c_int32, P]
    L.erp_pack_band_features_dev.argtypes = [P, P, P, P, C.c_int32, C.c_int32, C.c_int32,
                                             C.c_int32, C.POINTER(PackedPairs), P]
    L.erp_image_pairs_features_dev.argtypes = [P, P, P, C.c_int32, C.c_int32, C.c_int32,
                                               C.POINTER(SurfParams), C.c_int32, C.c_int32,
                                               C.c_int32, C.POINTER(PackedPairs),
                                               C.POINTER(ImageBatchInfo), P]
    L.erp_image_pairs_run.argtypes = [P, P, P, C.c_int32, C.c_int32, C.c_int32,
                                      C.POINTER(SurfParams), C.c_int32, C.c_int32, C.c_int32,
                                      C.POINTER(PackedPairs), C.c_float, C.POINTER(RansacCfg),
                                      C.POINTER(BatchOutputs), C.POINTER(ImageBatchInfo), P]
    L.erp_image_sweep_features_dev.argtypes = [P, P, P, C.c_int32, P, C.c_int32, C.c_int32,
                                               C.POINTER(SurfParams), C.c_int32, C.c_int32,
                                               C.c_int32, C.POINTER(PackedPairs),
                                               C.POINTER(ImageBatchInfo), P]
    L.erp_image_sweep_run.argtypes = [P, P, P, C.c_int32, P, C.c_int32, C.c_int32,
                                      C.POINTER(SurfParams), C.c_int32, C.c_int32, C.c_int32,
                                      C.POINTER(PackedPairs), C.c_float, C.POINTER(RansacCfg),
                                      C.POINTER(BatchOutputs), P, C.POINTER(ImageBatchInfo), P]
    L.erp_match_error_dev.argtypes = [P, P, P, C.c_int64, P, C.c_int64, C.c_int32, P, C.c_int32,
                                      C.c_int32, P, P]
    L.erp_rand_stream_create.argtypes = [C.c_uint32, C.c_uint64, C.POINTER(P)]
    L.erp_rand_stream_destroy.argtypes = [P]
    L.erp_rand_stream_get.argtypes = [P, C.POINTER(C.c_uint32), C.POINTER(C.c_uint64)]
    L.erp_rand_stream_set.argtypes = [P, C.c_uint32, C.c_uint64]
    L.erp_rand_stream_advance.argtypes = [P, C.c_uint64]
    L.erp_rand_stream_process.argtypes = [C.c_int32, C.POINTER(P)]
    L.erp_ctx_set_rand_stream.argtypes = [P, P]
    L.erp_ctx_get_rand_stream.argtypes = [P, C.POINTER(P)]
    L.erp_rand_stream_shuffle_prefix.argtypes = [P, C.c_int32, C.c_int32, P]
    L.erp_polish_dev.argtypes = [P, C.POINTER(PolishInputs), C.c_double, C.c_float, C.c_int32, P,
                                 P, P, P]
    L.erp_eight_point_find_polished.argtypes = [P, C.c_int32, C.c_int32, P, P, C.c_int32,
                                                C.POINTER(RansacCfg), C.c_float, C.c_int32, P, P,
                                                P]
    L.erp_pair_batch_run_winners.argtypes = [P, C.POINTER(PairBatch), C.c_float,
                                             C.POINTER(RansacCfg), C.POINTER(BatchOutputs), P, P]
    L.erp_eight_point_find_winner_dev.argtypes = [P, C.c_int32, C.c_int32, P, P, C.c_int32,
                                                  C.POINTER(RansacCfg), P, P, P, P]
    L.erp_eight_point_find_winner.argtypes = [P, C.c_int32, C.c_int32, P, P, C.c_int32,
                                              C.POINTER(RansacCfg), P, P, P, P]
    L.erp_polish_winners_dev.argtypes = [P, C.POINTER(PolishInputs), P, C.c_double, C.c_float,
                                         C.c_int32, P, P, P, P]
    L.erp_pair_batch_run_support.argtypes = [P, C.POINTER(PairBatch), C.c_float,
                                             C.POINTER(RansacCfg), C.POINTER(BatchOutputs),
                                             C.c_float, C.POINTER(SupportOutputs), P]
    L.erp_eight_point_find_support_dev.argtypes = [P, C.c_int32, C.c_int32, P, P, C.c_int32,
                                                   C.POINTER(RansacCfg), P, P, C.c_float,
                                                   C.POINTER(SupportOutputs), P]
    L.erp_eight_point_find_support.argtypes = [P, C.c_int32, C.c_int32, P, P, C.c_int32,
                                               C.POINTER(RansacCfg), C.c_float, P, P, P, P, P, P,
                                               P]
    L.erp_pose_select_dev.argtypes = [P, C.POINTER(PoseInputs), C.c_float, C.c_double, P, P, P, P,
                                      P]
    L.erp_eight_point_find_posed.argtypes = [P, C.c_int32, C.c_int32, P, P, C.c_int32,
                                             C.POINTER(RansacCfg), C.c_float, C.c_int32,
                                             C.c_double, P, P, P, P, P, P]
    L.erp_match_guided_dev.argtypes = [P, C.POINTER(GuidedInputs), C.POINTER(GuidedCfg),
                                       C.POINTER(GuidedOutputs), P]
    L.erp_match_guided.argtypes = [P, P, C.c_int32, P, C.c_int32, P, P, C.c_int32, C.c_int32, P,
                                   C.POINTER(GuidedCfg), P, P]
    L.erp_stereo_params_default.argtypes = [C.POINTER(StereoParams)]
    L.erp_stereo_params_default.restype = None
    L.erp_stereo_rows_dev.argtypes = [P, P, P, C.c_int32, C.c_int32, C.c_int32,
                                      C.POINTER(StereoParams), P, P, P]
    L.erp_stereo_params_ex_default.argtypes = [C.POINTER(StereoParamsEx)]
    L.erp_stereo_params_ex_default.restype = None
    L.erp_stereo_rows_ex_dev.argtypes = [P, P, P, C.c_int32, C.c_int32, C.c_int32,
                                         C.POINTER(StereoParamsEx), P, P, P]
    L.erp_stage_name.argtypes = [C.c_int32]
    L.erp_stage_name.restype = C.c_char_p
    L.erp_ctx_stage_times.argtypes = [P, P, P]
    _lib = L
    return L


def default_cfg(**kw) -> RansacCfg:
    cfg = RansacCfg()
    load().erp_ransac_cfg_default(C.byref(cfg))
    for k, v in kw.items():
        setattr(cfg, k, v)
    return cfg


def check(status: int, where: str):
    if status != ERP_OK:
        raise ErpError(status, where)


class RandStream:
    """erp_rand_stream: the glibc rand() stream continued from call to call (include/erp_match.h
    "rand stream").  Host only until a GPU call uses it.  Attach it with
    Context.set_rand_stream or the ``stream=`` keyword of eight_point / epipolar_tool /
    PairBatchRunner; calls take it in call order."""

    def __init__(self, seed: int = 1, offset: int = 0, _handle=None):
        self.L = load()
        self.owned = _handle is None
        self.h = P() if self.owned else _handle
        if self.owned:
            check(self.L.erp_rand_stream_create(seed, offset, C.byref(self.h)),
                  "erp_rand_stream_create")

    def get(self) -> tuple:
        """(seed, draws consumed), after the stream's last device update"""
        seed, draws = C.c_uint32(), C.c_uint64()
        check(self.L.erp_rand_stream_get(self.h, C.byref(seed), C.byref(draws)),
              "erp_rand_stream_get")
        return int(seed.value), int(draws.value)

    @property
    def draws(self) -> int:
        return self.get()[1]

    def set(self, seed: int, offset: int):
        check(self.L.erp_rand_stream_set(self.h, seed, offset), "erp_rand_stream_set")

    def advance(self, n: int):
        """skip n draws (rand() calls made elsewhere, e.g. by FLANN)"""
        check(self.L.erp_rand_stream_advance(self.h, n), "erp_rand_stream_advance")

    def shuffle_prefix(self, m: int, n: int) -> np.ndarray:
        """the first n of std::random_shuffle(iota(m)) on the stream; consumes m - 1 draws"""
        out = np.zeros(max(n, 1), np.int32)
        check(self.L.erp_rand_stream_shuffle_prefix(self.h, m, n, out.ctypes.data_as(P)),
              "erp_rand_stream_shuffle_prefix")
        return out[:n]

    def close(self):
        if self.owned and self.h:
            self.L.erp_rand_stream_destroy(self.h)
        self.h = P()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def process_rand_stream(device: int = 0) -> RandStream:
    """the process-wide stream of a device, at (1, 0) in a fresh process (glibc's global rand()
    state); never destroyed"""
    h = P()
    check(load().erp_rand_stream_process(device, C.byref(h)), "erp_rand_stream_process")
    return RandStream(_handle=h)


def _check_tensors(where: str, pairs):
    """every (tensor, dtype) of pairs is a contiguous CUDA tensor of that dtype"""
    import torch
    for t, dt in pairs:
        if not isinstance(t, torch.Tensor) or t.dtype != dt or not t.is_cuda or \
                not t.is_contiguous():
            raise ValueError(f"{where}: inputs must be contiguous CUDA tensors of the C types")


def _stream_or_current(stream, dev):
    import torch
    return stream if stream is not None else torch.cuda.current_stream(dev).cuda_stream


def _alloc_outputs(shapes: dict, names, dev):
    """-> (out, ptr): the outputs ``names`` of shapes = {name: (shape, dtype)} as fresh tensors,
    and ptr(name) = its device address, None for an output that was not asked for"""
    import torch
    out = {k: torch.empty(shapes[k][0], dtype=shapes[k][1], device=dev) for k in names}
    return out, lambda k: out[k].data_ptr() if k in out else None


class Context:
    """erp_ctx: one per device/thread; owns the grow-only device scratch."""

    def __init__(self, device: int = 0):
        self.L = load()
        self.h = P()
        check(self.L.erp_ctx_create(device, C.byref(self.h)), "erp_ctx_create")
        self.device = device
        self.rand_stream = None

    def set_profiling(self, enable: bool = True):
        check(self.L.erp_ctx_set_profiling(self.h, 1 if enable else 0), "set_profiling")

    def set_graphs(self, enable: bool = True):
        """erp_ctx_set_graphs: replay erp_pair_batch_run's launch sequence as a HIP graph"""
        check(self.L.erp_ctx_set_graphs(self.h, 1 if enable else 0), "set_graphs")

    def set_matcher(self, method: int):
        """erp_ctx_set_matcher: MATCHER_MFMA_FILTER (default) or MATCHER_VALU_EXACT."""
        check(self.L.erp_ctx_set_matcher(self.h, int(method)), "set_matcher")

    def set_option(self, name: str, value: int):
        """erp_ctx_set_option: a route option by name (OPTIONS; include/erp_match.h documents
        each).  Every setting gives the same results; the defaults are the measured fastest."""
        check(self.L.erp_ctx_set_option(self.h, OPTIONS[name], int(value)), f"set_option({name})")

    def get_option(self, name: str) -> int:
        v = C.c_int32()
        check(self.L.erp_ctx_get_option(self.h, OPTIONS[name], C.byref(v)), f"get_option({name})")
        return int(v.value)

    def set_rand_stream(self, stream: "RandStream | None"):
        """erp_ctx_set_rand_stream: the consuming calls on this context draw from ``stream`` and
        advance it (None detaches: cfg.seed / cfg.offset again).  Keeps the stream alive."""
        check(self.L.erp_ctx_set_rand_stream(self.h, stream.h if stream is not None else None),
              "set_rand_stream")
        self.rand_stream = stream

    def polish(self, results, hyps, key_left, key_right, width, height, thr: float,
               rounds: int = 3, valid_abs: float = 1.57, want_rounds: bool = False,
               want_mask: bool = True, stream=None, winners=None) -> dict:
        """erp_polish_dev on torch CUDA tensors: results [P, 64] uint8, hyps [P, iters, 120]
        uint8, key_left / key_right [P, stride, 2] float32, width / height [P] int32 -> {"polish":
        uint8 [P, 120] (POLISH_DTYPE), "rounds": uint8 [P, rounds, 112] (want_rounds), "mask":
        uint8 [P, stride] (want_mask)}.  Asynchronous on ``stream`` (default: torch's current
        stream); valid_abs = the cfg.valid_abs of the call that wrote the records.
        ``hyps=None, winners=`` uint8 [P, 88] (WINNER_DTYPE, what erp_pair_batch_run_winners
        wrote): erp_polish_winners_dev, the same outputs without the hypothesis records."""
        import torch
        from_winners = hyps is None
        rec = winners if from_winners else hyps
        _check_tensors("polish", ((results, torch.uint8), (rec, torch.uint8),
                                  (key_left, torch.float32), (key_right, torch.float32),
                                  (width, torch.int32), (height, torch.int32)))
        n = results.shape[0]
        rec_ok = (rec.dim() == 2 and rec.shape[1] == WINNER_DTYPE.itemsize) if from_winners else \
            (rec.dim() == 3 and rec.shape[2] == HYP_DTYPE.itemsize)
        if results.dim() != 2 or results.shape[1] != RESULT_DTYPE.itemsize or not rec_ok or \
                rec.shape[0] != n or \
                key_left.shape != key_right.shape or key_left.dim() != 3 or \
                key_left.shape[0] != n or key_left.shape[2] != 2 or width.numel() != n or \
                height.numel() != n:
            raise ValueError("polish: results [P, 64], hyps [P, iters, 120] (or winners [P, 88]), "
                             "keys [P, stride, 2], width / height [P] expected")
        dev = results.device
        rounds = int(rounds)
        inp = PolishInputs(n, 0 if from_winners else hyps.shape[1], key_left.shape[1],
                           key_left.data_ptr(), key_right.data_ptr(), width.data_ptr(),
                           height.data_ptr(), results.data_ptr(),
                           None if from_winners else hyps.data_ptr())
        shapes = {"polish": ((n, POLISH_DTYPE.itemsize), torch.uint8),
                  "rounds": ((n, max(rounds, 0), POLISH_ROUND_DTYPE.itemsize), torch.uint8),
                  "mask": ((n, key_left.shape[1]), torch.uint8)}
        names = ["polish"] + ["rounds"] * bool(want_rounds) + ["mask"] * bool(want_mask)
        out, ptr = _alloc_outputs(shapes, names, dev)
        tail = (valid_abs, thr, rounds, ptr("polish"), ptr("rounds") if rounds > 0 else None,
                ptr("mask"), _stream_or_current(stream, dev))
        if from_winners:
            check(self.L.erp_polish_winners_dev(self.h, C.byref(inp), winners.data_ptr(), *tail),
                  "erp_polish_winners_dev")
        else:
            check(self.L.erp_polish_dev(self.h, C.byref(inp), *tail), "erp_polish_dev")
        return out

    def select_pose(self, results, key_left, key_right, width, height, source, e_offset: int,
                    status_offset: int | None = None, mask=None, thr: float = 0.0,
                    min_sin2: float = 0.0, want=("depth", "front", "results"),
                    stream=None) -> dict:
        """erp_pose_select_dev on torch CUDA tensors: results [P, 64] uint8, key_left / key_right
        [P, stride, 2] float32, width / height [P] int32, source = uint8 [P, record bytes] records
        that hold each pair's solved 9-vector at byte ``e_offset`` and (``status_offset``) its
        int32 status -- winner records (16, 0) or polish records (48, 24) --, mask uint8 [P,
        stride] or None -> {"pose": uint8 [P, 160] (POSE_DTYPE), "depth": float64 [P, stride, 2],
        "front": uint8 [P, stride], "results": uint8 [P, 64]} (the last three as ``want`` names
        them).  Asynchronous on ``stream`` (default: torch's current stream)."""
        import torch
        chk = [(results, torch.uint8), (source, torch.uint8), (key_left, torch.float32),
               (key_right, torch.float32), (width, torch.int32), (height, torch.int32)]
        if mask is not None:
            chk.append((mask, torch.uint8))
        _check_tensors("select_pose", chk)
        n = results.shape[0]
        if results.dim() != 2 or results.shape[1] != RESULT_DTYPE.itemsize or source.dim() != 2 or \
                source.shape[0] != n or e_offset < 0 or e_offset + 72 > source.shape[1] or \
                (status_offset is not None and not 0 <= status_offset <= source.shape[1] - 4) or \
                key_left.shape != key_right.shape or key_left.dim() != 3 or \
                key_left.shape[0] != n or key_left.shape[2] != 2 or width.numel() != n or \
                height.numel() != n or \
                (mask is not None and tuple(mask.shape) != tuple(key_left.shape[:2])):
            raise ValueError("select_pose: results [P, 64], source [P, bytes], keys [P, stride, 2], "
                             "width / height [P], mask [P, stride] expected")
        unknown = [k for k in want if k not in ("depth", "front", "results")]
        if unknown:
            raise ValueError(f"select_pose: unknown outputs {unknown}")
        dev = results.device
        stride, rec = key_left.shape[1], source.shape[1]
        inp = PoseInputs(n, 0, stride, key_left.data_ptr(), key_right.data_ptr(),
                         width.data_ptr(), height.data_ptr(), results.data_ptr(),
                         source.data_ptr() + e_offset, rec,
                         None if status_offset is None else source.data_ptr() + status_offset,
                         rec, None if mask is None else mask.data_ptr())
        shapes = {"pose": ((n, POSE_DTYPE.itemsize), torch.uint8),
                  "depth": ((n, stride, 2), torch.float64), "front": ((n, stride), torch.uint8),
                  "results": ((n, RESULT_DTYPE.itemsize), torch.uint8)}
        out, ptr = _alloc_outputs(shapes, ["pose", *want], dev)
        check(self.L.erp_pose_select_dev(self.h, C.byref(inp), thr, min_sin2, ptr("pose"),
                                         ptr("depth"), ptr("front"), ptr("results"),
                                         _stream_or_current(stream, dev)),
              "erp_pose_select_dev")
        return out

    GUIDED_WANT = ("matches", "key_left", "key_right", "gated", "results", "winners")

    def guided_match(self, desc_l, desc_r, kp_l, kp_r, off_l, off_r, width, height, max_nq: int,
                     max_nt: int, source, e_offset: int, status_offset: int | None = None,
                     results=None, thr: float = 0.003, ratio: float = 0.8, max_dist: float = 0.0,
                     unique: bool = True, want=GUIDED_WANT, stream=None) -> dict:
        """erp_match_guided_dev on torch CUDA tensors: the packed batch as PairBatchRunner.run
        takes it, source = uint8 [P, record bytes] records that hold each pair's solved 9-vector
        at byte ``e_offset`` and (``status_offset``) its int32 status -- winner records (16, 0)
        or polish records (48, 24) --, results uint8 [P, 64] or None (every pair counts as ok)
        -> {"count": int32 [P], "matches": int32 [P, max_nq, 4] (DMatch rows), "key_left" /
        "key_right": float32 [P, max_nq, 2], "gated": int64 [P], "results": uint8 [P, 64] (M
        replaced), "winners": uint8 [P, 88]} (all but count as ``want`` names them).
        Asynchronous on ``stream`` (default: torch's current stream)."""
        import torch
        chk = [(desc_l, torch.float32), (desc_r, torch.float32), (kp_l, torch.float32),
               (kp_r, torch.float32), (off_l, torch.int64), (off_r, torch.int64),
               (width, torch.int32), (height, torch.int32), (source, torch.uint8)]
        if results is not None:
            chk.append((results, torch.uint8))
        _check_tensors("guided_match", chk)
        n = off_l.shape[0] - 1
        if off_r.shape[0] != n + 1 or width.numel() != n or height.numel() != n or \
                source.dim() != 2 or source.shape[0] != n or e_offset < 0 or \
                e_offset + 72 > source.shape[1] or desc_l.dim() != 2 or desc_r.dim() != 2 or \
                (status_offset is not None and not 0 <= status_offset <= source.shape[1] - 4) or \
                (results is not None and tuple(results.shape) != (n, RESULT_DTYPE.itemsize)):
            raise ValueError("guided_match: off_l / off_r [P + 1], width / height [P], source "
                             "[P, bytes], results [P, 64] expected")
        unknown = [k for k in want if k not in self.GUIDED_WANT]
        if unknown or ("results" in want and results is None):
            raise ValueError(f"guided_match: unknown outputs {unknown}, or 'results' without "
                             "result records")
        dev, rec = desc_l.device, source.shape[1]
        inp = GuidedInputs(
            PairBatch(n, desc_l.shape[1], max_nq, max_nt, desc_l.data_ptr(), desc_r.data_ptr(),
                      kp_l.data_ptr(), kp_r.data_ptr(), off_l.data_ptr(), off_r.data_ptr(),
                      width.data_ptr(), height.data_ptr()),
            None if results is None else results.data_ptr(), source.data_ptr() + e_offset, rec,
            None if status_offset is None else source.data_ptr() + status_offset, rec)
        shapes = {"count": ((n,), torch.int32), "matches": ((n, max_nq, 4), torch.int32),
                  "key_left": ((n, max_nq, 2), torch.float32),
                  "key_right": ((n, max_nq, 2), torch.float32), "gated": ((n,), torch.int64),
                  "results": ((n, RESULT_DTYPE.itemsize), torch.uint8),
                  "winners": ((n, WINNER_DTYPE.itemsize), torch.uint8)}
        out, ptr = _alloc_outputs(shapes, ["count", *want], dev)
        o = GuidedOutputs(ptr("count"), ptr("matches"), ptr("key_left"), ptr("key_right"),
                          ptr("gated"), ptr("results"), ptr("winners"))
        cfg = GuidedCfg(thr, ratio, max_dist, 1 if unique else 0)
        check(self.L.erp_match_guided_dev(self.h, C.byref(inp), C.byref(cfg), C.byref(o),
                                          _stream_or_current(stream, dev)),
              "erp_match_guided_dev")
        return out

    def stage_times(self) -> dict:
        """{stage: (total_ms, launches)} since the last call (syncs on the recorded events)."""
        ms = np.zeros(len(STAGES), np.float64)
        n = np.zeros(len(STAGES), np.int64)
        check(self.L.erp_ctx_stage_times(self.h, ms.ctypes.data_as(P), n.ctypes.data_as(P)),
              "stage_times")
        return {s: (float(ms[i]), int(n[i])) for i, s in enumerate(STAGES)}

    def close(self):
        if self.h:
            self.L.erp_ctx_destroy(self.h)
            self.h = P()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
