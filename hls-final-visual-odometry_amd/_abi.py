from __future__ import annotations

import ctypes as C
import os
import subprocess

import numpy as np


HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("VISO_HIP_LIB") or os.path.join(HERE, "libviso_hip.so")  # override: experiment builds
CHECK_LIB_PATH = os.path.join(HERE, "libviso_hip_check.so")  # the -DVH_CHECK build (tests only)
NOSNAKE_LIB_PATH = os.path.join(HERE, "libviso_hip_nosnake.so")  # the -DVH_SNAKE=0 build: flow tiles over the plain bin order (tests only)
CSRC = os.path.join(HERE, "csrc")
INCLUDE = os.path.normpath(os.path.join(HERE, "..", "include"))


def source_sha256() -> str:
    """sha256 over what determines the code object: every source, header and the Makefile under csrc/ plus the public
    header (names and contents, sorted).  Build-independent -- the `.so` hashes differently on every rebuild -- so a
    profile (profiles/traffic_latest.json) can say which code it was taken on (bench.py: roofline.traffic)."""
    import hashlib
    h = hashlib.sha256()
    files = [os.path.join(CSRC, f) for f in sorted(os.listdir(CSRC))
             if f.endswith((".hip", ".h", ".hpp", ".cpp")) or f == "Makefile"]
    files.append(os.path.join(INCLUDE, "viso_hip.h"))
    for f in files:
        h.update(os.path.basename(f).encode() + b"\0")
        h.update(open(f, "rb").read())
        h.update(b"\0")
    return h.hexdigest()


VH_OK = 0
VH_ERR_INVALID_ARG, VH_ERR_NO_DEVICE, VH_ERR_HIP, VH_ERR_CAPACITY, VH_ERR_UNSUPPORTED, VH_ERR_STATE = -1, -2, -3, -4, -5, -6
SET_1P, SET_2P, SET_1C, SET_2C = 0, 1, 2, 3
METHOD_FLOW, METHOD_STEREO, METHOD_QUAD = 0, 1, 2
#: rule of the outlier vote (vh_vote_rule): the reference's flow vote under its literal 5 / stock libviso2's per-method rule
VOTE_REFERENCE, VOTE_STOCK = 0, 1


def _abi_table():
    """Every symbol include/viso_hip.h declares -> (restype, argtypes), as _lib() sets them; None: the symbol is called
    with ctypes' defaults (an int result, arguments converted as they come), and so is an argtypes of None."""
    vp, i32, i64, f32, f64 = C.c_void_p, C.c_int32, C.c_int64, C.c_float, C.c_double
    return {
        "vh_abi_version": None, "vh_device_count": None, "vh_error_string": (C.c_char_p, [i32]), "vh_last_error": (C.c_char_p, None),
        "vh_default_params": None,
        "vh_create": (i32, [vp, i32, vp]), "vh_create_ex": (i32, [vp, i32, i32, i32, vp]), "vh_destroy": (None, [vp]),
        "vh_set_intrinsics": (i32, [vp, f64, f64, f64, f64]), "vh_push_back": (i32, [vp, vp, vp, vp, i32]),
        "vh_push_back_device": (i32, [vp, vp, vp, vp, i32]),
        "vh_match_features": (i32, [vp, i32, vp]), "vh_remove_outliers": (i32, [vp]), "vh_remove_outliers_pm": (i32, [vp, i32, vp]),
        "vh_remove_outliers_device": (i32, [i32, i32, vp, i64, vp, i32, i32, f32, f32, vp, i32, vp, vp, vp]),
        "vh_bucket_features": (i32, [vp, i32, f32, f32]), "vh_get_matches": (i32, [vp, vp, i32, vp]), "vh_get_features": (i32, [vp, i32, vp, i32, vp]),
        "vh_synchronize": (i32, [vp]),
        "vh_set_stream": (i32, [vp, vp]), "vh_clear_stream": (i32, [vp]), "vh_stream_wait_images": (i32, [vp, vp]),
        "vh_host_alloc": (i32, [i32, C.c_size_t, vp]), "vh_host_free": (i32, [vp]),
        "vh_compute_features": (i32, [vp, i32, vp, vp, vp, i32, vp, vp, i32, vp, vp, vp]), "vh_filters": (i32, [i32, vp, i32, i32, vp, vp, vp, vp]),
        "vh_create_index": (i32, [vp, i32, vp, vp, i32, vp, vp]), "vh_match_all": (i32, [vp, i32, vp, vp, i32, vp, i32, i32, vp]),
        "vh_match_all_prior": (i32, [vp, i32, vp, vp, i32, vp, i32, i32, f64, f64, vp]),
        "vh_match": (i32, [vp, i32, vp, i32, vp, i32, vp, i32, vp, i32, vp, i32, vp, i32, vp]),
        "vh_group_create": (i32, [vp, i32, i32, i32, i32, vp]), "vh_group_destroy": (None, [vp]), "vh_group_streams": (i32, [vp]),
        "vh_group_device_bytes": (i64, [vp]), "vh_group_push_back_device": (i32, [vp, vp, vp, i64, vp, i32]),
        "vh_group_push_back": (i32, [vp, vp, vp, i64, vp, i32]), "vh_group_match_features": (i32, [vp, i32]),
        "vh_group_match_features_prior": (i32, [vp, i32, vp]), "vh_group_remove_outliers": (i32, [vp, i32]),
        "vh_group_get_matches": (i32, [vp, i32, vp, i32, vp]), "vh_group_get_matches_all": (i32, [vp, vp, i32, vp]),
        "vh_group_download_matches_async": (i32, [vp, vp, i32, vp]), "vh_group_wait_download": (i32, [vp]),
        "vh_group_get_features": (i32, [vp, i32, i32, vp, i32, vp]),
        "vh_group_get_counts": (i32, [vp, vp, vp]), "vh_group_synchronize": (i32, [vp]), "vh_group_set_stream": (i32, [vp, vp]),
        "vh_group_clear_stream": (i32, [vp]), "vh_group_stream_wait_images": (i32, [vp, vp]), "vh_group_profile_enable": (i32, [vp, i32]),
        "vh_group_profile_read": (i32, [vp, C.c_char_p, vp, vp]), "vh_group_profile_reset": (i32, [vp]), "vh_group_debug_fail_next_alloc": (i32, [vp]),
        "vh_debug_vote_stack_slots": (i32, [i32]),
        "vh_default_ego_params": None, "vh_estimate_motion_stereo": (i32, [vp, i32, i32, vp, vp, vp, vp, vp, vp, vp]),
        "vh_group_estimate_motion": (i32, [vp, vp, vp, vp, vp, vp]), "vh_group_search_stats": (i32, [vp, vp, vp]),
        "vh_default_mono_params": None, "vh_estimate_motion_mono": (i32, [vp, i32, i32, vp, vp, vp, vp, vp, vp, vp]),
        "vh_group_estimate_motion_mono": (i32, [vp, vp, vp, vp, vp, vp]),
        "vh_group_post_begin": (i32, [vp, i32]), "vh_group_post_finish": (i32, [vp, i32, i32, f32, f32, i32, vp, vp, vp, vp, vp, vp, i32, vp, vp]),
        "vh_group_post_finish_mono": (i32, [vp, i32, i32, f32, f32, i32, vp, vp, vp, vp, vp, vp, i32, vp, vp]),
        "vh_group_post_device_config": (i32, [vp, i32, i32, i32]), "vh_group_post_begin_device": (i32, [vp, i32, i32, f32, f32, vp, vp, vp, vp, i32]),
        "vh_group_post_finish_device": (i32, [vp, i32, vp, vp, vp, vp, i32, vp]),
        "vh_sequence_create": (i32, [vp, i32, i32, i32, i32, vp]), "vh_sequence_push_back_device": (i32, [vp, vp, vp, i64, vp, i32]),
        "vh_sequence_push_back": (i32, [vp, vp, vp, i64, vp, i32]), "vh_sequence_position": (i32, [vp, vp, vp]),
        "vh_refine_matches": (i32, [vp, i32, i32, vp, vp, vp, vp, vp, vp, i32, vp]),
        "vh_set_multi_stage_matching": (i32, [vp, i32]), "vh_group_set_multi_stage_matching": (i32, [vp, i32]),
        "vh_get_sparse_matches": (i32, [vp, vp, i32, vp]), "vh_group_get_sparse_matches": (i32, [vp, i32, vp, i32, vp]),
        "vh_prior_statistics": (i32, [vp, vp, i32, vp, i32, vp]),
        "vh_match_ranged": (i32, [vp, i32, vp, i32, vp, i32, vp, i32, vp, i32, vp, i32, vp, vp, i32, vp]),
        "vh_set_multi_stage_device": (i32, [vp, i32]), "vh_group_set_multi_stage_device": (i32, [vp, i32]),
        "vh_prior_statistics_device": (i32, [vp, i32, vp, i32, i32, vp, i64, vp, vp]),
        "vh_set_track_linking": (i32, [vp, i32]), "vh_group_set_track_linking": (i32, [vp, i32]), "vh_get_tracks": (i32, [vp, vp, i32, vp]),
        "vh_group_get_tracks": (i32, [vp, i32, vp, i32, vp]), "vh_group_get_tracks_all": (i32, [vp, vp, i32, vp]),
        "vh_group_tracks_device": (i32, [vp, vp, vp]), "vh_link_tracks": (i32, [i32, i32, vp, i64, vp, i32, vp, vp, vp]),
        "vh_track_carry_free": (None, [vp]), "vh_group_debug_fail_alloc_after": (i32, [vp, i32]),
        "vh_default_recon_params": (None, [vp]), "vh_reconstruct_tracks": (i32, [vp, i32, i32, vp, i32, vp, vp, vp, vp, vp, vp]),
        "vh_reconstruct_last_kernel_ms": (f64, []),
        "vh_sequence_set_reconstruction": (i32, [vp, vp, i32]), "vh_sequence_reconstruct": (i32, [vp, vp, vp, vp]),
        "vh_sequence_get_recon_tracks": (i32, [vp, vp, i32, vp]), "vh_reconstruct_lists": (i32, [vp, i32, i32, vp, i64, vp, i32, vp, vp, i32, vp]),
        "vh_group_set_reconstruction": (i32, [vp, vp, i32]), "vh_group_reconstruct": (i32, [vp, vp, vp, vp]),
        "vh_group_get_recon_tracks": (i32, [vp, i32, vp, i32, vp]), "vh_group_get_recon_counts": (i32, [vp, vp, vp]),
        "vh_group_debug_reconstruct_lists": (i32, [vp, i32, i32, i32, vp, i64, vp, i32, vp, vp, i32, vp]),
        "vh_motion_inliers": (i32, [vp, i32, i32, vp, vp, vp, vp, vp, vp, vp, vp]), "vh_group_motion_inliers": (i32, [vp, vp, vp, vp, vp]),
        "vh_match_inliers": (i32, [vp, vp, vp, i32, vp]), "vh_group_get_inlier_flags": (i32, [vp, i32, vp, i32, vp]),
        "vh_group_get_inlier_matches": (i32, [vp, i32, vp, vp, i32, vp]),
        "vh_group_get_inlier_matches_all": (i32, [vp, vp, vp, i32, vp]), "vh_get_inlier_matches": (i32, [vp, vp, vp, i32, vp]),
        "vh_group_inliers_device": (i32, [vp, vp, vp, vp, vp]),
        "vh_estimate_motion_mono_model": (i32, [vp, i32, i32, vp, vp, vp, vp, vp, vp, vp, vp]),
        "vh_group_estimate_motion_mono_model": (i32, [vp, vp, vp, vp, vp, vp, vp]),
        "vh_motion_inliers_mono": (i32, [vp, i32, i32, vp, vp, vp, vp, vp, vp, vp, vp]), "vh_group_motion_inliers_mono": (i32, [vp, vp, vp, vp, vp]),
        "vh_match_inliers_mono": (i32, [vp, vp, vp, i32, vp]),
        "vh_refit_motion": (i32, [vp, i32, i32, vp, vp, vp, vp, vp, vp, vp]), "vh_group_refit_motion": (i32, [vp, vp, i32, vp, vp, vp, vp]),
        "vh_match_refit_motion": (i32, [vp, vp, i32, vp, vp, vp, vp]),
        "vh_group_post_device_dense": (i32, [vp, i32]), "vh_group_post_finish_device_dense": (i32, [vp, i32, vp, vp, vp, vp, i32, vp, vp]),
        "vh_gain": (i32, [i32, i32, vp, vp, vp, i64, vp, vp, vp, vp, vp, vp]), "vh_group_set_gain": (i32, [vp, i32]), "vh_set_gain": (i32, [vp, i32]),
        "vh_group_gain": (i32, [vp, vp, vp]), "vh_match_gain": (i32, [vp, vp, vp]), "vh_group_gain_indices": (i32, [vp, vp, vp, vp, vp]),
        "vh_match_gain_indices": (i32, [vp, vp, i32, vp, vp]),
        "vh_sequence_set_multi_stage": (i32, [vp, i32]), "vh_set_multi_stage_prior": (i32, [vp, i32]), "vh_group_set_multi_stage_prior": (i32, [vp, i32]),
        "vh_remove_outliers_pm_rule": (i32, [vp, i32, vp, vp]),
        "vh_remove_outliers_device_rule": (i32, [i32, i32, vp, i64, vp, i32, i32, f32, f32, vp, i32, vp, vp, vp, vp]),
        "vh_set_vote_rule": (i32, [vp, i32]), "vh_group_set_vote_rule": (i32, [vp, i32]),
        "vh_motion_covariance": (i32, [vp, i32, i32, vp, vp, vp, vp, vp, vp, vp]), "vh_group_motion_covariance": (i32, [vp, vp, vp, vp, vp, vp, vp, vp]),
        "vh_match_motion_covariance": (i32, [vp, vp, vp, vp, vp, vp, vp, vp]),
        "vh_refit_model_mono": (i32, [vp, i32, i32, vp, vp, vp, vp, vp, vp, vp]), "vh_group_refit_model_mono": (i32, [vp, vp, i32, vp, vp, vp, vp]),
        "vh_match_refit_model_mono": (i32, [vp, vp, i32, vp, vp, vp, vp]),
        "vh_pose_mono": (i32, [vp, i32, i32, vp, vp, vp, vp, vp, vp, vp]), "vh_group_pose_mono": (i32, [vp, vp, vp, vp, vp, vp]),
        "vh_match_pose_mono": (i32, [vp, vp, vp, vp, vp]),
        "vh_pose_mono_refined": (i32, [vp, i32, i32, vp, vp, vp, vp, vp, vp, vp, vp]), "vh_group_pose_mono_refined": (i32, [vp, vp, vp, vp, vp, vp, vp]),
        "vh_match_pose_mono_refined": (i32, [vp, vp, vp, vp, vp, vp]),
        "vh_group_post_device_tail": (i32, [vp, C.c_uint32]), "vh_group_post_device_shape": (i32, [vp, vp, vp]),
        "vh_group_post_finish_device_tail": (i32, [vp, i32, vp, vp, vp, vp, i32, vp, vp, vp]),
        "vh_default_scene_params": (None, [vp]), "vh_scene_points_stereo": (i32, [vp, vp, i32, i32, vp, vp, vp, vp, vp, vp, vp]),
        "vh_scene_points_mono": (i32, [vp, vp, i32, i32, vp, vp, vp, vp, vp, vp, vp]),
        "vh_group_scene_points_stereo": (i32, [vp, vp, vp, vp, vp]), "vh_match_scene_points_stereo": (i32, [vp, vp, vp, vp, vp]),
        "vh_group_scene_points_mono": (i32, [vp, vp, vp, vp, vp]), "vh_match_scene_points_mono": (i32, [vp, vp, vp, vp, vp]),
        "vh_group_get_scene_points": (i32, [vp, i32, vp, i32, vp]), "vh_group_get_scene_points_all": (i32, [vp, vp, i32, vp]),
        "vh_get_scene_points": (i32, [vp, vp, i32, vp]), "vh_group_scene_points_device": (i32, [vp, vp, vp]),
        "vh_default_landmark_params": (None, [vp]), "vh_landmarks_update": (i32, [vp, i32, i32, vp, vp, vp, vp, vp, vp, vp, vp, vp]),
        "vh_group_landmarks": (i32, [vp, vp, vp]), "vh_match_landmarks": (i32, [vp, vp, vp]),
        "vh_group_get_landmarks": (i32, [vp, i32, vp, i32, vp]), "vh_group_get_landmarks_all": (i32, [vp, vp, i32, vp]),
        "vh_get_landmarks": (i32, [vp, vp, i32, vp]), "vh_group_landmarks_device": (i32, [vp, vp, vp]),
        "vh_landmarks_chain": (i32, [vp, i32, i32, vp, vp, vp, vp, vp, i32, vp, vp, vp]), "vh_sequence_set_landmarks": (i32, [vp, i32]),
        "vh_default_traj_params": (None, [vp]), "vh_trajectory": (i32, [vp, i32, i32, vp, vp, vp, vp, vp, vp, vp]),
        "vh_group_set_trajectory": (i32, [vp, vp, vp]), "vh_sequence_set_trajectory": (i32, [vp, vp, vp]), "vh_set_trajectory": (i32, [vp, vp, vp]),
        "vh_group_trajectory": (i32, [vp, i32, vp]), "vh_match_trajectory": (i32, [vp, i32, vp]), "vh_group_get_poses": (i32, [vp, vp]),
        "vh_get_pose": (i32, [vp, vp]), "vh_group_poses_device": (i32, [vp, vp, vp]), "vh_group_set_pose": (i32, [vp, i32, vp]),
        "vh_group_scene_points_stereo_world": (i32, [vp, vp, vp, vp]), "vh_group_scene_points_mono_world": (i32, [vp, vp, vp, vp]),
        "vh_match_scene_points_stereo_world": (i32, [vp, vp, vp, vp]), "vh_match_scene_points_mono_world": (i32, [vp, vp, vp, vp]),
        "vh_default_traj_cov_params": (None, [vp]), "vh_trajectory_cov": (i32, [vp, vp, i32, i32, vp, vp, vp, vp, vp, vp, vp, vp, vp]),
        "vh_group_set_trajectory_covariance": (i32, [vp, vp, vp]), "vh_sequence_set_trajectory_covariance": (i32, [vp, vp, vp]),
        "vh_set_trajectory_covariance": (i32, [vp, vp, vp]), "vh_group_get_pose_covariances": (i32, [vp, vp]), "vh_get_pose_covariance": (i32, [vp, vp]),
        "vh_group_pose_covariances_device": (i32, [vp, vp, vp]),
        "vh_group_set_pose_covariance": (i32, [vp, i32, vp]),
    }


def _abi_ext_table():
    """The rows of the extension headers beside include/viso_hip.h (viso_hip_lmk_refit.h): the same library exports them,
    _lib() sets them in the same pass; they are kept out of ABI_SYMBOLS, which mirrors viso_hip.h alone."""
    vp, i32 = C.c_void_p, C.c_int32
    return {
        "vh_default_lmk_refit_params": (None, [vp]),
        "vh_refit_motion_landmarks": (i32, [vp, vp, i32, i32, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp]),
        "vh_group_refit_motion_landmarks": (i32, [vp, vp, vp, vp, i32, vp, vp, vp, vp, vp]),
        "vh_match_refit_motion_landmarks": (i32, [vp, vp, vp, vp, i32, vp, vp, vp, vp, vp]),
        "vh_group_get_refit_priors": (i32, [vp, i32, vp, i32, vp]),
    }


_ABI = _abi_table()
_ABI_EXT = _abi_ext_table()
#: every symbol include/viso_hip.h declares (checked by the CPU test-suite)
ABI_SYMBOLS = tuple(_ABI)


class Params(C.Structure):
    """POD mirror of Matcher::parameters (reference src/matcher.h:45-72)."""
    _fields_ = [(n, C.c_int32) for n in (
        "nms_n", "nms_tau", "match_binsize", "match_radius", "match_disp_tolerance",
        "outlier_disp_tolerance", "outlier_flow_tolerance", "multi_stage",
        "half_resolution", "refinement")] + [(n, C.c_double) for n in ("f", "cu", "cv", "base")]

    @classmethod
    def default(cls, **kw):
        """Matcher::parameters() defaults (reference src/matcher.h:60-71)."""
        p = cls(nms_n=2, nms_tau=50, match_binsize=50, match_radius=200,
                match_disp_tolerance=2, outlier_disp_tolerance=5, outlier_flow_tolerance=5,
                multi_stage=0, half_resolution=0, refinement=0)
        for k, v in kw.items():
            if not hasattr(p, k):
                raise AttributeError(k)
            setattr(p, k, v)
        return p


class VoteRule(C.Structure):
    """vh_vote_rule (include/viso_hip.h): the rule of the outlier vote, 16 bytes."""
    _fields_ = [("rule", C.c_int32), ("method", C.c_int32), ("flow_tolerance", C.c_float), ("disp_tolerance", C.c_float)]

    @classmethod
    def stock(cls, method: int, flow_tolerance: float = 5.0, disp_tolerance: float = 5.0):
        return cls(VOTE_STOCK, int(method), float(flow_tolerance), float(disp_tolerance))

    @classmethod
    def reference(cls):
        return cls(VOTE_REFERENCE, 0, 0.0, 0.0)


def _rule(rule):
    """None, a VoteRule or (rule, method, flow_tolerance, disp_tolerance) -> the pointer argument"""
    if rule is None:
        return None
    if not isinstance(rule, VoteRule):
        rule = VoteRule(*rule)
    return C.byref(rule)


class EgoParams(C.Structure):
    """VisualOdometryStereo::parameters + calibration (reference src/viso_stereo.h:31-43, src/viso.h:41-50)."""
    _fields_ = [("ransac_iters", C.c_int32), ("reweighting", C.c_int32), ("inlier_threshold", C.c_double),
                ("f", C.c_double), ("cu", C.c_double), ("cv", C.c_double), ("base", C.c_double)]

    @classmethod
    def default(cls, **kw):
        e = cls(ransac_iters=200, reweighting=1, inlier_threshold=2.0, f=1.0, cu=0.0, cv=0.0, base=1.0)
        for k, v in kw.items():
            if not hasattr(e, k):
                raise AttributeError(k)
            setattr(e, k, v)
        return e


class MonoParams(C.Structure):
    """VisualOdometryMono::parameters + calibration (reference src/viso_mono.h:32-46, src/viso.h:41-50)."""
    _fields_ = [("ransac_iters", C.c_int32), ("reserved_", C.c_int32), ("inlier_threshold", C.c_double), ("motion_threshold", C.c_double),
                ("height", C.c_double), ("pitch", C.c_double), ("f", C.c_double), ("cu", C.c_double), ("cv", C.c_double)]

    @classmethod
    def default(cls, **kw):
        e = cls(ransac_iters=2000, reserved_=0, inlier_threshold=0.00001, motion_threshold=100.0, height=1.0, pitch=0.0, f=1.0, cu=0.0, cv=0.0)
        for k, v in kw.items():
            if not hasattr(e, k):
                raise AttributeError(k)
            setattr(e, k, v)
        return e


class MonoModel(C.Structure):
    """vh_mono_model: the normalisation and the refit F the mono estimator arrived at (include/viso_hip.h)."""
    _fields_ = [("c", C.c_double * 4), ("s", C.c_double * 2), ("F", C.c_double * 9), ("valid", C.c_double)]


#: numpy layout of vh_mono_model, for arrays of models (one per list / stream)
MONO_MODEL_DTYPE = np.dtype([("c", "<f8", (4,)), ("s", "<f8", (2,)), ("F", "<f8", (9,)), ("valid", "<f8")])
# vh_mono_pose (152 bytes): what pose_mono / poseMono formed tr from
MONO_POSE_DTYPE = np.dtype([("R", "<f8", (9,)), ("t", "<f8", (3,)), ("scale", "<f8"), ("median", "<f8"), ("plane", "<f8"),
                            ("chirality", "<i4", (4,)), ("candidate", "<i4"), ("n_front", "<i4"), ("reason", "<i4"), ("reserved_", "<i4")])
# vh_mono_refine (288 bytes): what pose_mono / poseMono with refine=True made of the winner -- the tangent basis at the
# refined t, the 5 x 5 covariance of (w0, w1, w2, tau0, tau1), the sums of squared Sampson distances before and after
MONO_REFINE_DTYPE = np.dtype([("B", "<f8", (6,)), ("cov", "<f8", (25,)), ("ssr_start", "<f8"), ("ssr", "<f8"), ("moved_R", "<f8"),
                              ("moved_t", "<f8"), ("status", "<i4"), ("n_updates", "<i4")])


# vh_scene_point (32 bytes): one 3-d point per surviving record of scene_points_stereo / _mono / scenePoints
SCENE_POINT_DTYPE = np.dtype([("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("sigma_z", "<f4"), ("err", "<f4"), ("src_pos", "<i4"),
                              ("i1p", "<i4"), ("i1c", "<i4")])


class SceneParams(C.Structure):
    """vh_scene_params: the frame the points are given in (0 previous, 1 current left camera) and the three filters."""
    _fields_ = [("frame", C.c_int32), ("min_disp", C.c_float), ("max_depth", C.c_double), ("max_err", C.c_double)]

    @classmethod
    def default(cls, **kw):
        e = cls(frame=1, min_disp=0.0, max_depth=0.0, max_err=0.0)
        for k, v in kw.items():
            if not hasattr(e, k):
                raise AttributeError(k)
            setattr(e, k, v)
        return e


# vh_landmark_state (48 bytes): the sums of one track's accepted observations, one per record of a tracked list
LANDMARK_STATE_DTYPE = np.dtype([("sw", "<f8"), ("swx", "<f8"), ("swy", "<f8"), ("swz", "<f8"), ("n_obs", "<i4"), ("n_missed", "<i4"),
                                 ("reserved", "<i4", (2,))])
# vh_landmark (48 bytes): one fused point per track observed in the step (landmarks_update / landmarks)
LANDMARK_DTYPE = np.dtype([("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("sigma", "<f4"), ("n_obs", "<i4"), ("age", "<i4"),
                           ("birth_frame", "<i8"), ("birth_pos", "<i4"), ("src_pos", "<i4"), ("i1c", "<i4"), ("point_pos", "<i4")])


class LandmarkParams(C.Structure):
    """vh_landmark_params: the fewest observations of an emitted landmark, the longest gap a track's state survives (< 0: any)
    and the gate T = max_dist + gate_sigma * sigma_z (T <= 0: none)."""
    _fields_ = [("min_obs", C.c_int32), ("max_missed", C.c_int32), ("max_dist", C.c_double), ("gate_sigma", C.c_double)]

    @classmethod
    def default(cls, **kw):
        e = cls(min_obs=2, max_missed=3, max_dist=0.0, gate_sigma=0.0)
        for k, v in kw.items():
            if not hasattr(e, k):
                raise AttributeError(k)
            setattr(e, k, v)
        return e


#: policy of the trajectory for a row that is not accepted (vh_traj_params.on_fail) / the motion a handle steps under
TRAJ_HOLD, TRAJ_REPEAT = 0, 1
TRAJ_STEREO, TRAJ_MONO = 0, 1
#: rows of a chain one round of the trajectory kernel takes (csrc/vh_trajectory.h: VH_TRAJ_ROUND)
TRAJ_ROUND = 256
# vh_traj_pose (272 bytes): one per row of trajectory / trajectory(source)
TRAJ_POSE_DTYPE = np.dtype([("Tw_prev", "<f8", (4, 4)), ("Tw_cur", "<f8", (4, 4)), ("status", "<i4"), ("step", "<i4"), ("reserved", "<i4", (2,))])
# vh_traj_carry (272 bytes): what a chain carries from call to call
TRAJ_CARRY_DTYPE = np.dtype([("Tw", "<f8", (4, 4)), ("Tinv", "<f8", (4, 4)), ("step", "<i4"), ("has_tinv", "<i4"), ("reserved", "<i4", (2,))])


class TrajParams(C.Structure):
    """vh_traj_params: what a row that is not accepted does to the pose (TRAJ_HOLD: nothing; TRAJ_REPEAT: the last accepted
    step again)."""
    _fields_ = [("on_fail", C.c_int32), ("reserved", C.c_int32)]

    @classmethod
    def default(cls, **kw):
        e = cls(on_fail=TRAJ_HOLD, reserved=0)
        for k, v in kw.items():
            if not hasattr(e, k):
                raise AttributeError(k)
            setattr(e, k, v)
        return e


#: rows of a chain one round of the pose covariance kernel takes (csrc/vh_trajectory_cov.h: VH_TRAJ_COV_ROUND)
TRAJ_COV_ROUND = 128
# vh_traj_cov (304 bytes): one per row of trajectory_cov / getPoseCovariances
TRAJ_COV_DTYPE = np.dtype([("cov", "<f8", (6, 6)), ("status", "<i4"), ("step", "<i4"), ("n_filled", "<i4"), ("reserved", "<i4")])
# vh_traj_cov_carry (880 bytes): what a chain's covariance carries from call to call
TRAJ_COV_CARRY_DTYPE = np.dtype([("cov", "<f8", (6, 6)), ("Ad_last", "<f8", (6, 6)), ("Q_last", "<f8", (6, 6)), ("n_filled", "<i4"),
                                 ("has_ad", "<i4"), ("has_q", "<i4"), ("step", "<i4")])


class TrajCovParams(C.Structure):
    """vh_traj_cov_params: fill_scale, the share of the last own Q a step without a covariance of its own adds."""
    _fields_ = [("fill_scale", C.c_double), ("reserved", C.c_int32 * 2)]

    @classmethod
    def default(cls, **kw) -> "TrajCovParams":
        e = cls()
        _lib().vh_default_traj_cov_params(C.byref(e))
        for k, v in kw.items():
            setattr(e, k, v)
        return e


def _traj_S0(Sigma0, n):
    """None, or [n, 6, 6] doubles (one 6x6 serves every chain) -> [n, 36]"""
    if Sigma0 is None:
        return None
    s = np.asarray(Sigma0, np.float64)
    if s.shape == (6, 6):
        s = np.broadcast_to(s, (n, 6, 6))
    assert s.shape == (n, 6, 6), s.shape
    return np.ascontiguousarray(s).reshape(n, 36)


def _traj_T0(T0, n):
    """None, or [n, 4, 4] doubles (one 4x4 serves every chain) -> [n, 16]"""
    return _scene_Tw(T0, n)


def _scene_Tw(Tw, n):
    """None, or [n, 4, 4] doubles (one 4x4 serves every list)."""
    if Tw is None:
        return None
    Tw = np.asarray(Tw, np.float64)
    if Tw.shape == (4, 4):
        Tw = np.broadcast_to(Tw, (n, 4, 4))
    return np.ascontiguousarray(Tw).reshape(n, 16)


def _models(model, n):
    """`model` (a MONO_MODEL_DTYPE array, a MonoModel or a sequence of them) as a contiguous MONO_MODEL_DTYPE array [n]."""
    if isinstance(model, MonoModel):
        model = [model]
    if not isinstance(model, np.ndarray):
        model = np.frombuffer(b"".join(bytes(m) for m in model), MONO_MODEL_DTYPE)
    model = np.ascontiguousarray(model, MONO_MODEL_DTYPE).reshape(-1)
    assert len(model) == n, (len(model), n)
    return model


class PostDense(C.Structure):
    """vh_post_dense: the nullable output pointers of vh_group_post_finish_device_dense (include/viso_hip.h)."""
    _fields_ = [(n, C.c_void_p) for n in ("voted_counts", "inlier_counts", "tr_refit", "ok_refit", "n_updates", "model",
                                          "voted_pm", "flags", "inlier_pm", "src_pos")]


#: stages of vh_group_post_device_tail (StreamGroup.postDeviceTail): a bit mask
POST_TAIL_COV, POST_TAIL_MONO_REFIT, POST_TAIL_MONO_POSE, POST_TAIL_MONO_REFINE = 1, 2, 4, 8


class PostTail(C.Structure):
    """vh_post_tail: its size, then the nullable output pointers of vh_group_post_finish_device_tail (include/viso_hip.h)."""
    _fields_ = [("size", C.c_uint32), ("reserved", C.c_uint32)] + [
        (n, C.c_void_p) for n in ("cov", "ssr", "ok_cov", "model_refit", "ok_model", "w", "tr_pose", "ok_pose", "pose", "refine")]


class ReconParams(C.Structure):
    """Reconstruction's calibration and update's thresholds (reference src/reconstruction.h:55, :66)."""
    _fields_ = [("f", C.c_double), ("cu", C.c_double), ("cv", C.c_double), ("point_type", C.c_int32), ("min_track_length", C.c_int32),
                ("max_dist", C.c_double), ("min_angle", C.c_double)]

    @classmethod
    def default(cls, **kw):
        r = cls(f=1.0, cu=0.0, cv=0.0, point_type=1, min_track_length=2, max_dist=30.0, min_angle=2.0)
        for k, v in kw.items():
            if not hasattr(r, k):
                raise AttributeError(k)
            setattr(r, k, v)
        return r


#: vh_reconstruct_tracks' status values (include/viso_hip.h), in the order Reconstruction::update tests them
RECON_ACCEPTED, RECON_SHORT, RECON_INFINITY, RECON_TYPE, RECON_NOT_REFINED, RECON_FAR_OR_NARROW = range(6)
#: a lost track older than the history of a sequence handle's reconstruction: not solved
RECON_HISTORY = 6


#: Matcher::p_match (reference src/matcher.h:89-104), 48 bytes
P_MATCH_DTYPE = np.dtype([
    ("u1p", "<f4"), ("v1p", "<f4"), ("i1p", "<i4"),
    ("u2p", "<f4"), ("v2p", "<f4"), ("i2p", "<i4"),
    ("u1c", "<f4"), ("v1c", "<f4"), ("i1c", "<i4"),
    ("u2c", "<f4"), ("v2c", "<f4"), ("i2c", "<i4")])


#: vh_track (include/viso_hip.h), 24 bytes: one per match record of a tracked list
TRACK = np.dtype([("birth_frame", "<i8"), ("birth_pos", "<i4"), ("age", "<i4"), ("prev", "<i4"), ("reserved", "<i4")])


#: vh_recon_track (include/viso_hip.h), 56 bytes: one per lost track of SequenceGroup.reconstruct / reconstruct_lists
RECON_TRACK = np.dtype([("birth_frame", "<i8"), ("birth_pos", "<i4"), ("frames", "<i4"), ("lost_frame", "<i8"), ("status", "<i4"),
                        ("point", "<f4", (3,)), ("distance", "<f8"), ("angle", "<f8")])


class VisoHipError(RuntimeError):
    def __init__(self, code: int, where: str):
        self.code = code
        msg = _lib().vh_error_string(code).decode()
        last = _lib().vh_last_error().decode()
        super().__init__(f"{where}: {msg} ({code})" + (f" [{last}]" if last else ""))


def build(verbose: bool = False) -> str:
    """Compile every HIP source for gfx950 into libviso_hip.so (in-tree), and the -DVH_CHECK
    variant libviso_hip_check.so (index invariants verified on the device, csrc/vh_dev.h) and the
    -DVH_SNAKE=0 variant libviso_hip_nosnake.so that tests/ run a part of the suite on."""
    cmd = ["make", "-C", CSRC, "-j4"] + ([] if verbose else ["-s"])
    subprocess.check_call(cmd)
    subprocess.check_call(cmd + ["VARIANT=check"])
    # (only the two units that read the switch are compiled again; the other objects are the shipped build's)
    subprocess.check_call(cmd + ["VARIANT=nosnake", "EXTRA=-DVH_SNAKE=0", "ONLY=kernels_bin kernels_match"])
    return LIB_PATH


_LIB = None


def _lib():
    global _LIB
    if _LIB is None:
        if not os.path.exists(LIB_PATH):
            raise ImportError(
                f"{LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                "(there is no CPU fallback for the HIP path)")
        lib = C.CDLL(LIB_PATH)
        for name, proto in {**_ABI, **_ABI_EXT}.items():
            fn = getattr(lib, name)   # every declared symbol resolves, or the library is not the header's
            if proto is not None:
                fn.restype = proto[0]
                if proto[1] is not None:
                    fn.argtypes = proto[1]
        _LIB = lib
    return _LIB


def _check(rc: int, where: str, allow=()):
    if rc != VH_OK and rc not in allow:
        raise VisoHipError(rc, where)
    return rc


def _ptr(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _dims(dims):
    return (C.c_int32 * 3)(*[int(d) for d in dims])


def _feat(m):
    if m is None:
        return np.zeros((0, 12), np.int32), 0
    m = np.ascontiguousarray(m, dtype=np.int32).reshape(-1, 12)
    return m, m.shape[0]


def _fetch(name, rec, *lead, empty_raises=False):
    """The sized getters of the C ABI, `name`(*lead, out..., cap, &n): asked with no buffer the entry answers
    VH_ERR_CAPACITY and the length n, asked again it fills n records.  rec: the records' dtype (with a shape tail, as
    (np.int32, 12), for rows), or a list of dtypes for an entry that fills several arrays side by side -> the array, or a
    tuple of them.  empty_raises: an empty list whose first answer was an error other than the length raises it."""
    recs = rec if isinstance(rec, list) else [rec]
    fn = getattr(_lib(), name)
    n = C.c_int32(0)
    rc = _check(fn(*lead, *[None] * len(recs), 0, C.byref(n)), name, allow=(VH_ERR_CAPACITY,))
    out = [np.zeros(n.value, r) for r in recs]
    if n.value:
        _check(fn(*lead, *[_ptr(o) for o in out], n.value, C.byref(n)), name)
    elif empty_raises and rc != VH_OK:
        raise VisoHipError(rc, name)
    return tuple(out) if isinstance(rec, list) else out[0]


def _device_view(name, h, n_arrays=1):
    """`name`(h, &address..., &stride) -> (the device address of each of the handle's n_arrays arrays, stride in records)"""
    ptrs = [C.c_void_p() for _ in range(n_arrays)]
    stride = C.c_int64(0)
    _check(getattr(_lib(), name)(h, *[C.byref(p) for p in ptrs], C.byref(stride)), name)
    return (*[p.value for p in ptrs], stride.value)


def _packed(arrays, dtype, tail=(), empty=0):
    """a list of arrays of records (each of shape `tail`) -> (their concatenation, offsets [n + 1] in records).  empty: the
    records of the placeholder that stands in when there is no record at all -- the entries differ in whether they take
    an empty array's address there (0), or want one record to point at (1), and each keeps what it was written with."""
    arrays = [np.ascontiguousarray(a, dtype=dtype).reshape(-1, *tail) for a in arrays]
    offsets = np.zeros(len(arrays) + 1, np.int32)
    offsets[1:] = np.cumsum([len(a) for a in arrays])
    return (np.concatenate(arrays) if offsets[-1] else np.zeros((empty, *tail), dtype)), offsets


def _padded(lists, min_stride=1):
    """a list of p_match arrays -> (records [n, stride] with list l in row l, stride = the longest list, counts [n])"""
    lists = [np.ascontiguousarray(m, dtype=P_MATCH_DTYPE) for m in lists]
    stride = max([len(m) for m in lists] + [min_stride])
    pm = np.zeros((len(lists), stride), P_MATCH_DTYPE)
    for l, m in enumerate(lists):
        pm[l, :len(m)] = m
    return pm, stride, np.array([len(m) for m in lists], np.int32)


