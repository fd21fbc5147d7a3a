"""viso-hip: MI355X-native feature detection + matching behind the libviso2
`Matcher` surface of Chang-Tun-Yu/HLS-final-Visual-Odometry.

This package is the thin Python host mirror over the C ABI of
`libviso_hip.so` (include/viso_hip.h).  All compute happens in the hand-written
HIP kernels under csrc/; there is no CPU or PyTorch fallback: importing works
without a GPU (so the library and its exported symbols can be checked), any
compute call without a usable GPU raises `VisoHipError(VH_ERR_NO_DEVICE)`, and a
missing shared library raises at import.

The directory name contains hyphens, so load it with
`__graft_entry__.load_package()` (importlib under the name
`hls_final_visual_odometry_amd`).
"""
from __future__ import annotations

import ctypes as C
import os
import subprocess

import numpy as np

from . import synth  # noqa: F401  (synthetic KITTI-shaped frames)

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

#: every symbol include/viso_hip.h declares (checked by the CPU test-suite)
ABI_SYMBOLS = (
    "vh_abi_version", "vh_device_count", "vh_error_string", "vh_last_error", "vh_default_params",
    "vh_create", "vh_create_ex", "vh_destroy", "vh_set_intrinsics", "vh_push_back", "vh_push_back_device",
    "vh_match_features", "vh_remove_outliers", "vh_remove_outliers_pm", "vh_remove_outliers_device", "vh_bucket_features", "vh_get_matches", "vh_get_features", "vh_synchronize",
    "vh_set_stream", "vh_clear_stream", "vh_stream_wait_images", "vh_host_alloc", "vh_host_free", "vh_compute_features", "vh_filters", "vh_create_index", "vh_match_all", "vh_match_all_prior", "vh_match",
    "vh_group_create", "vh_group_destroy", "vh_group_streams", "vh_group_device_bytes", "vh_group_push_back_device",
    "vh_group_push_back", "vh_group_match_features", "vh_group_match_features_prior", "vh_group_remove_outliers", "vh_group_get_matches", "vh_group_get_matches_all", "vh_group_download_matches_async", "vh_group_wait_download", "vh_group_get_features",
    "vh_group_get_counts", "vh_group_synchronize", "vh_group_set_stream", "vh_group_clear_stream", "vh_group_stream_wait_images", "vh_group_profile_enable",
    "vh_group_profile_read", "vh_group_profile_reset", "vh_group_debug_fail_next_alloc", "vh_debug_vote_stack_slots",
    "vh_default_ego_params", "vh_estimate_motion_stereo", "vh_group_estimate_motion", "vh_group_search_stats",
    "vh_default_mono_params", "vh_estimate_motion_mono", "vh_group_estimate_motion_mono",
    "vh_group_post_begin", "vh_group_post_finish", "vh_group_post_finish_mono",
    "vh_group_post_device_config", "vh_group_post_begin_device", "vh_group_post_finish_device",
    "vh_sequence_create", "vh_sequence_push_back_device", "vh_sequence_push_back", "vh_sequence_position",
    "vh_refine_matches",
    "vh_set_multi_stage_matching", "vh_group_set_multi_stage_matching", "vh_get_sparse_matches", "vh_group_get_sparse_matches",
    "vh_prior_statistics", "vh_match_ranged",
    "vh_set_multi_stage_device", "vh_group_set_multi_stage_device", "vh_prior_statistics_device",
    "vh_set_track_linking", "vh_group_set_track_linking", "vh_get_tracks", "vh_group_get_tracks", "vh_group_get_tracks_all",
    "vh_group_tracks_device", "vh_link_tracks", "vh_track_carry_free", "vh_group_debug_fail_alloc_after",
    "vh_default_recon_params", "vh_reconstruct_tracks", "vh_reconstruct_last_kernel_ms",
    "vh_sequence_set_reconstruction", "vh_sequence_reconstruct", "vh_sequence_get_recon_tracks", "vh_reconstruct_lists",
    "vh_group_set_reconstruction", "vh_group_reconstruct", "vh_group_get_recon_tracks", "vh_group_get_recon_counts",
    "vh_group_debug_reconstruct_lists",
    "vh_motion_inliers", "vh_group_motion_inliers", "vh_match_inliers", "vh_group_get_inlier_flags", "vh_group_get_inlier_matches",
    "vh_group_get_inlier_matches_all", "vh_get_inlier_matches", "vh_group_inliers_device",
    "vh_estimate_motion_mono_model", "vh_group_estimate_motion_mono_model",
    "vh_motion_inliers_mono", "vh_group_motion_inliers_mono", "vh_match_inliers_mono",
    "vh_refit_motion", "vh_group_refit_motion", "vh_match_refit_motion",
    "vh_group_post_device_dense", "vh_group_post_finish_device_dense",
    "vh_gain", "vh_group_set_gain", "vh_set_gain", "vh_group_gain", "vh_match_gain", "vh_group_gain_indices", "vh_match_gain_indices",
    "vh_sequence_set_multi_stage", "vh_set_multi_stage_prior", "vh_group_set_multi_stage_prior",
    "vh_remove_outliers_pm_rule", "vh_remove_outliers_device_rule", "vh_set_vote_rule", "vh_group_set_vote_rule",
    "vh_motion_covariance", "vh_group_motion_covariance", "vh_match_motion_covariance",
    "vh_refit_model_mono", "vh_group_refit_model_mono", "vh_match_refit_model_mono",
    "vh_pose_mono", "vh_group_pose_mono", "vh_match_pose_mono",
    "vh_pose_mono_refined", "vh_group_pose_mono_refined", "vh_match_pose_mono_refined",
    "vh_group_post_device_tail", "vh_group_post_device_shape", "vh_group_post_finish_device_tail",
    "vh_default_scene_params", "vh_scene_points_stereo", "vh_scene_points_mono",
    "vh_group_scene_points_stereo", "vh_match_scene_points_stereo", "vh_group_scene_points_mono", "vh_match_scene_points_mono",
    "vh_group_get_scene_points", "vh_group_get_scene_points_all", "vh_get_scene_points", "vh_group_scene_points_device",
    "vh_default_landmark_params", "vh_landmarks_update", "vh_group_landmarks", "vh_match_landmarks",
    "vh_group_get_landmarks", "vh_group_get_landmarks_all", "vh_get_landmarks", "vh_group_landmarks_device",
    "vh_landmarks_chain", "vh_sequence_set_landmarks",
    "vh_default_traj_params", "vh_trajectory", "vh_group_set_trajectory", "vh_sequence_set_trajectory", "vh_set_trajectory",
    "vh_group_trajectory", "vh_match_trajectory", "vh_group_get_poses", "vh_get_pose", "vh_group_poses_device", "vh_group_set_pose",
    "vh_group_scene_points_stereo_world", "vh_group_scene_points_mono_world",
    "vh_match_scene_points_stereo_world", "vh_match_scene_points_mono_world",
    "vh_default_traj_cov_params", "vh_trajectory_cov", "vh_group_set_trajectory_covariance", "vh_sequence_set_trajectory_covariance",
    "vh_set_trajectory_covariance", "vh_group_get_pose_covariances", "vh_get_pose_covariance", "vh_group_pose_covariances_device",
    "vh_group_set_pose_covariance",
)


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
        lib.vh_error_string.restype = C.c_char_p
        lib.vh_error_string.argtypes = [C.c_int32]
        lib.vh_last_error.restype = C.c_char_p
        vp, i32, i64, f32, f64 = C.c_void_p, C.c_int32, C.c_int64, C.c_float, C.c_double
        sig = {
            "vh_create": [vp, i32, vp], "vh_create_ex": [vp, i32, i32, i32, vp], "vh_destroy": [vp],
            "vh_set_intrinsics": [vp, f64, f64, f64, f64],
            "vh_push_back": [vp, vp, vp, vp, i32], "vh_push_back_device": [vp, vp, vp, vp, i32],
            "vh_match_features": [vp, i32, vp], "vh_bucket_features": [vp, i32, f32, f32],
            "vh_get_matches": [vp, vp, i32, vp], "vh_get_features": [vp, i32, vp, i32, vp],
            "vh_synchronize": [vp], "vh_set_stream": [vp, vp], "vh_clear_stream": [vp], "vh_stream_wait_images": [vp, vp],
            "vh_remove_outliers": [vp], "vh_remove_outliers_pm": [vp, i32, vp], "vh_group_remove_outliers": [vp, i32],
            "vh_remove_outliers_device": [i32, i32, vp, i64, vp, i32, i32, f32, f32, vp, i32, vp, vp, vp],
            "vh_host_alloc": [i32, C.c_size_t, vp], "vh_host_free": [vp],
            "vh_compute_features": [vp, i32, vp, vp, vp, i32, vp, vp, i32, vp, vp, vp],
            "vh_filters": [i32, vp, i32, i32, vp, vp, vp, vp],
            "vh_create_index": [vp, i32, vp, vp, i32, vp, vp],
            "vh_match_all": [vp, i32, vp, vp, i32, vp, i32, i32, vp],
            "vh_match_all_prior": [vp, i32, vp, vp, i32, vp, i32, i32, f64, f64, vp],
            "vh_match": [vp, i32, vp, i32, vp, i32, vp, i32, vp, i32, vp, i32, vp, i32, vp],
            "vh_group_create": [vp, i32, i32, i32, i32, vp], "vh_group_destroy": [vp], "vh_group_streams": [vp],
            "vh_group_push_back_device": [vp, vp, vp, i64, vp, i32],
            "vh_group_push_back": [vp, vp, vp, i64, vp, i32],
            "vh_group_match_features": [vp, i32], "vh_group_match_features_prior": [vp, i32, vp], "vh_group_get_matches": [vp, i32, vp, i32, vp],
            "vh_group_get_matches_all": [vp, vp, i32, vp],
            "vh_group_download_matches_async": [vp, vp, i32, vp], "vh_group_wait_download": [vp],
            "vh_group_get_features": [vp, i32, i32, vp, i32, vp], "vh_group_get_counts": [vp, vp, vp],
            "vh_group_synchronize": [vp], "vh_group_set_stream": [vp, vp], "vh_group_clear_stream": [vp],
            "vh_group_stream_wait_images": [vp, vp],
            "vh_group_profile_enable": [vp, i32], "vh_group_profile_read": [vp, C.c_char_p, vp, vp],
            "vh_group_profile_reset": [vp], "vh_group_debug_fail_next_alloc": [vp], "vh_debug_vote_stack_slots": [i32],
            "vh_estimate_motion_stereo": [vp, i32, i32, vp, vp, vp, vp, vp, vp, vp],
            "vh_group_estimate_motion": [vp, vp, vp, vp, vp, vp],
            "vh_estimate_motion_mono": [vp, i32, i32, vp, vp, vp, vp, vp, vp, vp],
            "vh_group_estimate_motion_mono": [vp, vp, vp, vp, vp, vp],
            "vh_group_post_begin": [vp, i32],
            "vh_group_post_finish": [vp, i32, i32, f32, f32, i32, vp, vp, vp, vp, vp, vp, i32, vp, vp],
            "vh_group_post_finish_mono": [vp, i32, i32, f32, f32, i32, vp, vp, vp, vp, vp, vp, i32, vp, vp],
            "vh_group_post_device_config": [vp, i32, i32, i32],
            "vh_group_post_begin_device": [vp, i32, i32, f32, f32, vp, vp, vp, vp, i32],
            "vh_group_post_finish_device": [vp, i32, vp, vp, vp, vp, i32, vp],
            "vh_group_search_stats": [vp, vp, vp],
            "vh_sequence_create": [vp, i32, i32, i32, i32, vp],
            "vh_sequence_push_back_device": [vp, vp, vp, i64, vp, i32],
            "vh_sequence_push_back": [vp, vp, vp, i64, vp, i32],
            "vh_sequence_position": [vp, vp, vp],
            "vh_refine_matches": [vp, i32, i32, vp, vp, vp, vp, vp, vp, i32, vp],
            "vh_set_multi_stage_matching": [vp, i32], "vh_group_set_multi_stage_matching": [vp, i32],
            "vh_get_sparse_matches": [vp, vp, i32, vp], "vh_group_get_sparse_matches": [vp, i32, vp, i32, vp],
            "vh_prior_statistics": [vp, vp, i32, vp, i32, vp],
            "vh_set_multi_stage_device": [vp, i32], "vh_group_set_multi_stage_device": [vp, i32],
            "vh_prior_statistics_device": [vp, i32, vp, i32, i32, vp, i64, vp, vp],
            "vh_match_ranged": [vp, i32, vp, i32, vp, i32, vp, i32, vp, i32, vp, i32, vp, vp, i32, vp],
            "vh_set_track_linking": [vp, i32], "vh_group_set_track_linking": [vp, i32],
            "vh_remove_outliers_pm_rule": [vp, i32, vp, vp], "vh_set_vote_rule": [vp, i32], "vh_group_set_vote_rule": [vp, i32],
            "vh_remove_outliers_device_rule": [i32, i32, vp, i64, vp, i32, i32, f32, f32, vp, i32, vp, vp, vp, vp],
            "vh_get_tracks": [vp, vp, i32, vp], "vh_group_get_tracks": [vp, i32, vp, i32, vp],
            "vh_group_get_tracks_all": [vp, vp, i32, vp], "vh_group_tracks_device": [vp, vp, vp],
            "vh_link_tracks": [i32, i32, vp, i64, vp, i32, vp, vp, vp],
            "vh_group_debug_fail_alloc_after": [vp, i32],
            "vh_reconstruct_tracks": [vp, i32, i32, vp, i32, vp, vp, vp, vp, vp, vp],
            "vh_sequence_set_reconstruction": [vp, vp, i32], "vh_sequence_reconstruct": [vp, vp, vp, vp],
            "vh_sequence_get_recon_tracks": [vp, vp, i32, vp],
            "vh_reconstruct_lists": [vp, i32, i32, vp, i64, vp, i32, vp, vp, i32, vp],
            "vh_group_set_reconstruction": [vp, vp, i32], "vh_group_reconstruct": [vp, vp, vp, vp],
            "vh_group_get_recon_tracks": [vp, i32, vp, i32, vp], "vh_group_get_recon_counts": [vp, vp, vp],
            "vh_group_debug_reconstruct_lists": [vp, i32, i32, i32, vp, i64, vp, i32, vp, vp, i32, vp],
            "vh_motion_inliers": [vp, i32, i32, vp, vp, vp, vp, vp, vp, vp, vp],
            "vh_group_motion_inliers": [vp, vp, vp, vp, vp], "vh_match_inliers": [vp, vp, vp, i32, vp],
            "vh_group_get_inlier_flags": [vp, i32, vp, i32, vp], "vh_group_get_inlier_matches": [vp, i32, vp, vp, i32, vp],
            "vh_group_get_inlier_matches_all": [vp, vp, vp, i32, vp], "vh_get_inlier_matches": [vp, vp, vp, i32, vp],
            "vh_group_inliers_device": [vp, vp, vp, vp, vp],
            "vh_estimate_motion_mono_model": [vp, i32, i32, vp, vp, vp, vp, vp, vp, vp, vp],
            "vh_group_estimate_motion_mono_model": [vp, vp, vp, vp, vp, vp, vp],
            "vh_motion_inliers_mono": [vp, i32, i32, vp, vp, vp, vp, vp, vp, vp, vp],
            "vh_group_motion_inliers_mono": [vp, vp, vp, vp, vp], "vh_match_inliers_mono": [vp, vp, vp, i32, vp],
            "vh_refit_motion": [vp, i32, i32, vp, vp, vp, vp, vp, vp, vp],
            "vh_motion_covariance": [vp, i32, i32, vp, vp, vp, vp, vp, vp, vp],
            "vh_group_motion_covariance": [vp, vp, vp, vp, vp, vp, vp, vp], "vh_match_motion_covariance": [vp, vp, vp, vp, vp, vp, vp, vp],
            "vh_refit_model_mono": [vp, i32, i32, vp, vp, vp, vp, vp, vp, vp],
            "vh_group_refit_model_mono": [vp, vp, i32, vp, vp, vp, vp], "vh_match_refit_model_mono": [vp, vp, i32, vp, vp, vp, vp],
            "vh_pose_mono": [vp, i32, i32, vp, vp, vp, vp, vp, vp, vp],
            "vh_group_pose_mono": [vp, vp, vp, vp, vp, vp], "vh_match_pose_mono": [vp, vp, vp, vp, vp],
            "vh_pose_mono_refined": [vp, i32, i32, vp, vp, vp, vp, vp, vp, vp, vp],
            "vh_group_pose_mono_refined": [vp, vp, vp, vp, vp, vp, vp], "vh_match_pose_mono_refined": [vp, vp, vp, vp, vp, vp],
            "vh_group_refit_motion": [vp, vp, i32, vp, vp, vp, vp], "vh_match_refit_motion": [vp, vp, i32, vp, vp, vp, vp],
            "vh_group_post_device_dense": [vp, i32],
            "vh_group_post_finish_device_dense": [vp, i32, vp, vp, vp, vp, i32, vp, vp],
            "vh_group_post_device_tail": [vp, C.c_uint32], "vh_group_post_device_shape": [vp, vp, vp],
            "vh_group_post_finish_device_tail": [vp, i32, vp, vp, vp, vp, i32, vp, vp, vp],
            "vh_gain": [i32, i32, vp, vp, vp, i64, vp, vp, vp, vp, vp, vp],
            "vh_group_set_gain": [vp, i32], "vh_set_gain": [vp, i32],
            "vh_group_gain": [vp, vp, vp], "vh_match_gain": [vp, vp, vp],
            "vh_group_gain_indices": [vp, vp, vp, vp, vp], "vh_match_gain_indices": [vp, vp, i32, vp, vp],
            "vh_sequence_set_multi_stage": [vp, i32], "vh_set_multi_stage_prior": [vp, i32], "vh_group_set_multi_stage_prior": [vp, i32],
            "vh_scene_points_stereo": [vp, vp, i32, i32, vp, vp, vp, vp, vp, vp, vp],
            "vh_scene_points_mono": [vp, vp, i32, i32, vp, vp, vp, vp, vp, vp, vp],
            "vh_group_scene_points_stereo": [vp, vp, vp, vp, vp], "vh_match_scene_points_stereo": [vp, vp, vp, vp, vp],
            "vh_group_scene_points_mono": [vp, vp, vp, vp, vp], "vh_match_scene_points_mono": [vp, vp, vp, vp, vp],
            "vh_group_get_scene_points": [vp, i32, vp, i32, vp], "vh_group_get_scene_points_all": [vp, vp, i32, vp],
            "vh_get_scene_points": [vp, vp, i32, vp], "vh_group_scene_points_device": [vp, vp, vp],
            "vh_landmarks_update": [vp, i32, i32, vp, vp, vp, vp, vp, vp, vp, vp, vp],
            "vh_group_landmarks": [vp, vp, vp], "vh_match_landmarks": [vp, vp, vp],
            "vh_group_get_landmarks": [vp, i32, vp, i32, vp], "vh_group_get_landmarks_all": [vp, vp, i32, vp],
            "vh_get_landmarks": [vp, vp, i32, vp], "vh_group_landmarks_device": [vp, vp, vp],
            "vh_landmarks_chain": [vp, i32, i32, vp, vp, vp, vp, vp, i32, vp, vp, vp], "vh_sequence_set_landmarks": [vp, i32],
            "vh_trajectory": [vp, i32, i32, vp, vp, vp, vp, vp, vp, vp],
            "vh_group_set_trajectory": [vp, vp, vp], "vh_sequence_set_trajectory": [vp, vp, vp], "vh_set_trajectory": [vp, vp, vp],
            "vh_group_trajectory": [vp, i32, vp], "vh_match_trajectory": [vp, i32, vp],
            "vh_group_get_poses": [vp, vp], "vh_get_pose": [vp, vp], "vh_group_poses_device": [vp, vp, vp],
            "vh_group_set_pose": [vp, i32, vp],
            "vh_group_scene_points_stereo_world": [vp, vp, vp, vp], "vh_group_scene_points_mono_world": [vp, vp, vp, vp],
            "vh_match_scene_points_stereo_world": [vp, vp, vp, vp], "vh_match_scene_points_mono_world": [vp, vp, vp, vp],
            "vh_trajectory_cov": [vp, vp, i32, i32, vp, vp, vp, vp, vp, vp, vp, vp, vp],
            "vh_group_set_trajectory_covariance": [vp, vp, vp], "vh_sequence_set_trajectory_covariance": [vp, vp, vp],
            "vh_set_trajectory_covariance": [vp, vp, vp],
            "vh_group_get_pose_covariances": [vp, vp], "vh_get_pose_covariance": [vp, vp], "vh_group_pose_covariances_device": [vp, vp, vp],
            "vh_group_set_pose_covariance": [vp, i32, vp],
        }
        for name, args in sig.items():
            fn = getattr(lib, name)
            fn.argtypes = args
            fn.restype = None if name.endswith("destroy") else i32
        lib.vh_track_carry_free.argtypes = [vp]
        lib.vh_track_carry_free.restype = None
        lib.vh_default_recon_params.argtypes = [vp]
        lib.vh_default_recon_params.restype = None
        lib.vh_default_scene_params.argtypes = [vp]
        lib.vh_default_scene_params.restype = None
        lib.vh_default_landmark_params.argtypes = [vp]
        lib.vh_default_landmark_params.restype = None
        lib.vh_default_traj_params.argtypes = [vp]
        lib.vh_default_traj_params.restype = None
        lib.vh_default_traj_cov_params.argtypes = [vp]
        lib.vh_default_traj_cov_params.restype = None
        lib.vh_reconstruct_last_kernel_ms.argtypes = []
        lib.vh_reconstruct_last_kernel_ms.restype = f64
        lib.vh_group_device_bytes.argtypes = [vp]
        lib.vh_group_device_bytes.restype = i64
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


def device_count() -> int:
    """Visible HIP devices (0 when there is none)."""
    return max(0, _lib().vh_device_count())


def pinned_empty(shape, dtype=np.uint8, device: int = 0) -> np.ndarray:
    """numpy array over page-locked host memory (vh_host_alloc): image buffers whose
    upload in pushBack runs at PCIe rate.  Freed when the array is collected."""
    import weakref
    dt = np.dtype(dtype)
    n = int(np.prod(shape)) * dt.itemsize
    ptr = C.c_void_p()
    _check(_lib().vh_host_alloc(int(device), C.c_size_t(max(n, 1)), C.byref(ptr)), "vh_host_alloc")
    buf = (C.c_uint8 * max(n, 1)).from_address(ptr.value)
    arr = np.frombuffer(buf, dtype=dt, count=int(np.prod(shape))).reshape(shape)
    weakref.finalize(buf, _lib().vh_host_free, C.c_void_p(ptr.value))
    return arr


def abi_version() -> int:
    return _lib().vh_abi_version()


# --------------------------------------------------------------------------- one stream
class Matcher:
    """Host mirror of the reference's `Matcher` public surface
    (src/matcher.h:75-143): pushBack / matchFeatures / bucketFeatures /
    getMatches, same argument meaning, plus getFeatures for the parity checks."""

    def __init__(self, param: Params | None = None, device: int = 0, max_features: int = 0,
                 max_matches: int = 0, outlier_removal: bool = True):
        self.param = param if param is not None else Params.default()
        # matchFeatures ends with removeOutliers as the reference's does (src/matcher.cpp:108);
        # False gives the bare Matcher::matching result
        self.outlier_removal = bool(outlier_removal)
        h = C.c_void_p()
        _check(_lib().vh_create_ex(C.byref(self.param), device, max_features, max_matches, C.byref(h)), "vh_create")
        self._h = h

    def close(self):
        if getattr(self, "_h", None):
            _lib().vh_destroy(self._h)
            self._h = None

    __del__ = close

    def setIntrinsics(self, f, cu, cv, base):
        _check(_lib().vh_set_intrinsics(self._h, f, cu, cv, base), "vh_set_intrinsics")

    def pushBack(self, I1, I2=None, dims=None, replace=False):
        """I1/I2: (H, bpl) uint8 numpy arrays (host) -- Matcher::pushBack (src/matcher.cpp:51-91).
        Like the reference, a dimension mismatch is reported and the call returns False."""
        I1 = np.ascontiguousarray(I1, dtype=np.uint8)
        if I2 is not None:
            I2 = np.ascontiguousarray(I2, dtype=np.uint8)
        if dims is None:
            dims = [I1.shape[1], I1.shape[0], I1.shape[1]]
        rc = _lib().vh_push_back(self._h, _ptr(I1), _ptr(I2), _dims(dims), 1 if replace else 0)
        if rc == VH_ERR_INVALID_ARG:
            print("ERROR: Image dimension mismatch!")
            return False
        _check(rc, "vh_push_back")
        return True

    def pushBackDevice(self, ptr1: int, ptr2: int | None, dims, replace=False):
        _check(_lib().vh_push_back_device(self._h, C.c_void_p(ptr1), C.c_void_p(ptr2) if ptr2 else None,
                                          _dims(dims), 1 if replace else 0), "vh_push_back_device")

    def matchFeatures(self, method: int, Tr_delta=None):
        tr = None
        if Tr_delta is not None:
            tr = np.ascontiguousarray(Tr_delta, dtype=np.float64).reshape(16)
        _check(_lib().vh_match_features(self._h, int(method), _ptr(tr)), "vh_match_features")
        if self.outlier_removal:
            self.removeOutliers()

    def removeOutliers(self):
        """removeOutliers (src/remove_outliers.cpp:4-94), which the reference's matchFeatures
        runs right after matching (src/matcher.cpp:108); host side, flow and quad matches."""
        _check(_lib().vh_remove_outliers(self._h), "vh_remove_outliers")

    def bucketFeatures(self, max_features: int, bucket_width: float, bucket_height: float):
        _check(_lib().vh_bucket_features(self._h, int(max_features), float(bucket_width), float(bucket_height)),
               "vh_bucket_features")

    def getMatches(self) -> np.ndarray:
        n = C.c_int32(0)
        rc = _check(_lib().vh_get_matches(self._h, None, 0, C.byref(n)), "vh_get_matches", allow=(VH_ERR_CAPACITY,))
        out = np.zeros(n.value, P_MATCH_DTYPE)
        if n.value:
            _check(_lib().vh_get_matches(self._h, _ptr(out), n.value, C.byref(n)), "vh_get_matches")
        elif rc != VH_OK:  # an empty list from truncated feature sets is still an error
            raise VisoHipError(rc, "vh_get_matches")
        return out

    def setMultiStageMatching(self, on: bool = True):
        """Two-pass matching of stock libviso2 (vh_set_multi_stage_matching): before the first pushBack, with
        param.multi_stage = 1."""
        _check(_lib().vh_set_multi_stage_matching(self._h, 1 if on else 0), "vh_set_multi_stage_matching")

    def setMultiStageDevice(self, on: bool = True):
        """The vote and the statistics between the two passes on the GPU (vh_set_multi_stage_device): matchFeatures only
        queues work.  After setMultiStageMatching(True), before the first pushBack."""
        _check(_lib().vh_set_multi_stage_device(self._h, 1 if on else 0), "vh_set_multi_stage_device")

    def setMultiStagePrior(self, on: bool = True):
        """matchFeatures(2, Tr_delta) hands the motion estimate to both passes of multi-stage matching
        (vh_set_multi_stage_prior): after setMultiStageMatching(True), before the first pushBack."""
        _check(_lib().vh_set_multi_stage_prior(self._h, 1 if on else 0), "vh_set_multi_stage_prior")

    def getSparseMatches(self) -> np.ndarray:
        """The sparse list of pass 1 after the vote (multi-stage matching on)."""
        n = C.c_int32(0)
        _check(_lib().vh_get_sparse_matches(self._h, None, 0, C.byref(n)), "vh_get_sparse_matches", allow=(VH_ERR_CAPACITY,))
        out = np.zeros(n.value, P_MATCH_DTYPE)
        if n.value:
            _check(_lib().vh_get_sparse_matches(self._h, _ptr(out), n.value, C.byref(n)), "vh_get_sparse_matches")
        return out

    def setTrackLinking(self, on: bool = True):
        """Link every match list to the list of the previous pair on the GPU (vh_set_track_linking): before the first
        pushBack.  The tracks describe the list as matching left it: use outlier_removal=False, or link the voted lists
        with link_tracks()."""
        _check(_lib().vh_set_track_linking(self._h, 1 if on else 0), "vh_set_track_linking")

    def setVoteRule(self, rule: int = VOTE_STOCK):
        """The rule of every outlier vote of this handle (vh_set_vote_rule), before the first push: VOTE_REFERENCE or
        VOTE_STOCK -- the per-method rule under this handle's outlier_flow_tolerance / outlier_disp_tolerance."""
        _check(_lib().vh_set_vote_rule(self._h, int(rule)), "vh_set_vote_rule")

    def getTracks(self) -> np.ndarray:
        """One TRACK record per record of the last matchFeatures' list (vh_get_tracks)."""
        n = C.c_int32(0)
        rc = _check(_lib().vh_get_tracks(self._h, None, 0, C.byref(n)), "vh_get_tracks", allow=(VH_ERR_CAPACITY,))
        out = np.zeros(n.value, TRACK)
        if n.value:
            _check(_lib().vh_get_tracks(self._h, _ptr(out), n.value, C.byref(n)), "vh_get_tracks")
        elif rc != VH_OK:
            raise VisoHipError(rc, "vh_get_tracks")
        return out

    def motionInliers(self, ego: "EgoParams", tr, ok: bool = True) -> int:
        """VisualOdometryStereo::getInlier on the whole device-resident quad list under tr[6] (vh_match_inliers) -> the
        number of inliers; getInlierMatches() returns them."""
        tr = np.ascontiguousarray(tr, np.float64).reshape(6)
        n = C.c_int32(0)
        _check(_lib().vh_match_inliers(self._h, C.byref(ego), _ptr(tr), 1 if ok else 0, C.byref(n)), "vh_match_inliers")
        return n.value

    def motionInliersMono(self, mono: "MonoParams", model, ok: bool = True) -> int:
        """VisualOdometryMono::getInlier on the whole device-resident flow or quad list under a vh_mono_model
        (vh_match_inliers_mono) -> the number of inliers; getInlierMatches() returns them."""
        model = _models(model, 1)
        n = C.c_int32(0)
        _check(_lib().vh_match_inliers_mono(self._h, C.byref(mono), _ptr(model), 1 if ok else 0, C.byref(n)), "vh_match_inliers_mono")
        return n.value

    def refitMotion(self, ego: "EgoParams", reclassify: bool = False):
        """The reference's final optimisation (src/viso_stereo.cpp:126-139) on ALL inliers of the last motionInliers, from the
        motion it classified under (vh_match_refit_motion) -> (tr [6], ok, n_updates, count); reclassify: the list is
        classified again under the refined motion, and count / getInlierMatches() are that classification's."""
        tr = np.zeros(6, np.float64); ok = C.c_int32(0); nupd = C.c_int32(0); n = C.c_int32(0)
        _check(_lib().vh_match_refit_motion(self._h, C.byref(ego), 1 if reclassify else 0, _ptr(tr), C.byref(ok), C.byref(nupd), C.byref(n)),
               "vh_match_refit_motion")
        return tr, bool(ok.value), nupd.value, n.value

    def motionCovariance(self, ego: "EgoParams", tr=None, ok: bool = True):
        """The covariance of the stereo motion over ALL inliers of the last motionInliers / refitMotion(reclassify=True)
        (vh_match_motion_covariance) -> (cov [6, 6], ssr, ok, count).  tr None: under the motion the list was classified
        under, which is on the device; else under tr [6] / ok -- refitMotion's tr after reclassify=False."""
        cov = np.zeros((6, 6), np.float64); ssr = C.c_double(0); oko = C.c_int32(0); n = C.c_int32(0)
        okin = C.c_int32(1 if ok else 0)
        if tr is not None:
            tr = np.ascontiguousarray(tr, np.float64).reshape(6)
        _check(_lib().vh_match_motion_covariance(self._h, C.byref(ego), _ptr(tr) if tr is not None else None,
                                                 C.byref(okin) if tr is not None else None, _ptr(cov), C.byref(ssr), C.byref(oko),
                                                 C.byref(n)), "vh_match_motion_covariance")
        return cov, ssr.value, bool(oko.value), n.value

    def refitModelMono(self, mono: "MonoParams", reclassify: bool = False):
        """fundamentalMatrix (reference src/viso_mono.cpp:235-266) on ALL inliers of the last motionInliersMono, in the frame
        of the model it classified under (vh_match_refit_model_mono) -> (model [1] MONO_MODEL_DTYPE, ok, w [2] = the two
        smallest singular values w[8], w[7] of the moment matrix, count); reclassify: the list is classified again under
        the refined model, and count / getInlierMatches() are that classification's."""
        model = np.zeros(1, MONO_MODEL_DTYPE); ok = C.c_int32(0); w = np.zeros(2, np.float64); n = C.c_int32(0)
        _check(_lib().vh_match_refit_model_mono(self._h, C.byref(mono), 1 if reclassify else 0, _ptr(model), C.byref(ok), _ptr(w), C.byref(n)),
               "vh_match_refit_model_mono")
        return model, bool(ok.value), w, n.value

    def poseMono(self, mono: "MonoParams", pose: bool = False, refine: bool = False):
        """The mono pose (reference src/viso_mono.cpp:83-158: E, R|t, chirality, the ground-plane scale) over ALL inliers of
        the last motionInliersMono, under the model it classified under (vh_match_pose_mono) -> (tr [6], ok) and, with
        pose=True, the MONO_POSE_DTYPE record [1] as a third value.  refine=True: the winning R|t is refined by Gauss-Newton
        on the Sampson distance of every inlier before the scale tail (vh_match_pose_mono_refined), and the
        MONO_REFINE_DTYPE record [1] is one more value at the end."""
        tr = np.zeros(6, np.float64); ok = C.c_int32(0)
        rec = np.zeros(1, MONO_POSE_DTYPE)
        if refine:
            ref = np.zeros(1, MONO_REFINE_DTYPE)
            _check(_lib().vh_match_pose_mono_refined(self._h, C.byref(mono), _ptr(tr), C.byref(ok), _ptr(rec) if pose else None, _ptr(ref)),
                   "vh_match_pose_mono_refined")
            return (tr, bool(ok.value), rec, ref) if pose else (tr, bool(ok.value), ref)
        _check(_lib().vh_match_pose_mono(self._h, C.byref(mono), _ptr(tr), C.byref(ok), _ptr(rec) if pose else None), "vh_match_pose_mono")
        return (tr, bool(ok.value), rec) if pose else (tr, bool(ok.value))

    def scenePoints(self, e, sp: "SceneParams | None" = None, Tw=None) -> np.ndarray:
        """The 3-d point of every inlier of the current classification (vh_match_scene_points_stereo for an EgoParams: under
        the motion of the last motionInliers / refitMotion(reclassify=True); vh_match_scene_points_mono for a MonoParams:
        under the pose of the last poseMono) -> SCENE_POINT_DTYPE [n], in list order.  Tw: None or a 4x4 applied last."""
        sp = sp or SceneParams.default()
        tw = _scene_Tw(Tw, 1)
        n = C.c_int32(0)
        fn = "vh_match_scene_points_mono" if isinstance(e, MonoParams) else "vh_match_scene_points_stereo"
        _check(getattr(_lib(), fn)(self._h, C.byref(e), C.byref(sp), None if tw is None else _ptr(tw), C.byref(n)), fn)
        return self.getScenePoints()

    def setTrajectory(self, params: "TrajParams | None" = None, T0=None, on: bool = True):
        """Accumulate the camera's pose on the device (vh_set_trajectory): before the first pushBack.  T0: the start pose
        (None: the unit matrix); on=False switches the feature off."""
        tp = params or TrajParams.default()
        t0 = _traj_T0(T0, 1)
        _check(_lib().vh_set_trajectory(self._h, C.byref(tp) if on else None, _ptr(t0)), "vh_set_trajectory")

    def trajectory(self, source: int = TRAJ_STEREO) -> np.ndarray:
        """One step of the pose under the motion of the current classification (vh_match_trajectory; TRAJ_STEREO: the
        motion of motionInliers / refitMotion(reclassify=True), TRAJ_MONO: poseMono's) -> TRAJ_POSE_DTYPE [1].  A
        repeated call for the same pair recomputes the step."""
        out = np.zeros(1, TRAJ_POSE_DTYPE)
        _check(_lib().vh_match_trajectory(self._h, source, _ptr(out)), "vh_match_trajectory")
        return out

    def getPoses(self) -> np.ndarray:
        """The record of the last trajectory(), valid until the next pushBack (vh_get_pose) -> TRAJ_POSE_DTYPE [1]."""
        out = np.zeros(1, TRAJ_POSE_DTYPE)
        _check(_lib().vh_get_pose(self._h, _ptr(out)), "vh_get_pose")
        return out

    def setPose(self, T):
        """The chain continues from the 4x4 T (vh_group_set_pose)."""
        t = np.ascontiguousarray(T, np.float64).reshape(16)
        _check(_lib().vh_group_set_pose(self._h, 0, _ptr(t)), "vh_group_set_pose")

    def setTrajectoryCovariance(self, params: "TrajCovParams | None" = None, Sigma0=None, on: bool = True):
        """Propagate the pose's covariance with the pose (vh_set_trajectory_covariance): behind setTrajectory, before the
        first pushBack.  Sigma0: the start covariance 6x6 (None: zero); on=False switches it off.  trajectory() then needs
        motionCovariance(ego) (tr None) of the current classification in front of it."""
        tcp = params or TrajCovParams.default()
        _check(_lib().vh_set_trajectory_covariance(self._h, C.byref(tcp) if on else None, _ptr(_traj_S0(Sigma0, 1))),
               "vh_set_trajectory_covariance")

    def getPoseCovariances(self) -> np.ndarray:
        """The covariance record of the last trajectory() (vh_get_pose_covariance) -> TRAJ_COV_DTYPE [1]."""
        out = np.zeros(1, TRAJ_COV_DTYPE)
        _check(_lib().vh_get_pose_covariance(self._h, _ptr(out)), "vh_get_pose_covariance")
        return out

    def setPoseCovariance(self, Sigma):
        """The chain's covariance continues from the 6x6 Sigma (vh_group_set_pose_covariance)."""
        s = np.ascontiguousarray(Sigma, np.float64).reshape(36)
        _check(_lib().vh_group_set_pose_covariance(self._h, 0, _ptr(s)), "vh_group_set_pose_covariance")

    def scenePointsWorld(self, e, sp: "SceneParams | None" = None) -> np.ndarray:
        """scenePoints with Tw taken from the trajectory's pose on the device: Tw_prev for sp.frame 0, Tw_cur for 1
        (vh_match_scene_points_stereo_world / _mono_world); after trajectory() of the current match."""
        sp = sp or SceneParams.default()
        n = C.c_int32(0)
        fn = "vh_match_scene_points_mono_world" if isinstance(e, MonoParams) else "vh_match_scene_points_stereo_world"
        _check(getattr(_lib(), fn)(self._h, C.byref(e), C.byref(sp), C.byref(n)), fn)
        return self.getScenePoints()

    def getScenePoints(self) -> np.ndarray:
        """The points of the last scenePoints, valid until the next matchFeatures (vh_get_scene_points)."""
        n = C.c_int32(0)
        _check(_lib().vh_get_scene_points(self._h, None, 0, C.byref(n)), "vh_get_scene_points", allow=(VH_ERR_CAPACITY,))
        out = np.zeros(n.value, SCENE_POINT_DTYPE)
        if n.value:
            _check(_lib().vh_get_scene_points(self._h, _ptr(out), n.value, C.byref(n)), "vh_get_scene_points")
        return out

    def landmarks(self, params: "LandmarkParams | None" = None) -> np.ndarray:
        """The scene points of the last scenePoints fused along the feature tracks (vh_match_landmarks; setTrackLinking, and
        a scenePoints Tw that takes every step's points into one common frame) -> LANDMARK_DTYPE [n], in list order."""
        lp = params or LandmarkParams.default()
        n = C.c_int32(0)
        _check(_lib().vh_match_landmarks(self._h, C.byref(lp), C.byref(n)), "vh_match_landmarks")
        return self.getLandmarks()

    def getLandmarks(self) -> np.ndarray:
        """The landmarks of the last landmarks(), valid until the next matchFeatures (vh_get_landmarks)."""
        n = C.c_int32(0)
        _check(_lib().vh_get_landmarks(self._h, None, 0, C.byref(n)), "vh_get_landmarks", allow=(VH_ERR_CAPACITY,))
        out = np.zeros(n.value, LANDMARK_DTYPE)
        if n.value:
            _check(_lib().vh_get_landmarks(self._h, _ptr(out), n.value, C.byref(n)), "vh_get_landmarks")
        return out

    def setGain(self, on: bool = True):
        """Keep the pushed left images on the device for getGain (vh_set_gain): before the first pushBack."""
        _check(_lib().vh_set_gain(self._h, 1 if on else 0), "vh_set_gain")

    def getGain(self, indices=None):
        """Matcher::getGain (reference src/matcher.h:148): the gain between the previous and the current left image over
        the positions `indices` of getMatches(), or over the inliers of the last motionInliers(Mono) when None
        (vh_match_gain_indices / vh_match_gain) -> (gain np.float32, num)."""
        g = C.c_float(0); n = C.c_int32(0)
        if indices is None:
            _check(_lib().vh_match_gain(self._h, C.byref(g), C.byref(n)), "vh_match_gain")
        else:
            idx = np.ascontiguousarray(indices, np.int32).reshape(-1)
            _check(_lib().vh_match_gain_indices(self._h, _ptr(idx) if len(idx) else None, len(idx), C.byref(g), C.byref(n)), "vh_match_gain_indices")
        return np.float32(g.value), n.value

    def getInlierMatches(self):
        """-> (the inlier records in list order, their positions in getMatches()) of the last motionInliers(Mono)."""
        n = C.c_int32(0)
        _check(_lib().vh_get_inlier_matches(self._h, None, None, 0, C.byref(n)), "vh_get_inlier_matches", allow=(VH_ERR_CAPACITY,))
        out = np.zeros(n.value, P_MATCH_DTYPE); pos = np.zeros(n.value, np.int32)
        if n.value:
            _check(_lib().vh_get_inlier_matches(self._h, _ptr(out), _ptr(pos), n.value, C.byref(n)), "vh_get_inlier_matches")
        return out, pos

    def getFeatures(self, which: int) -> np.ndarray:
        n = C.c_int32(0)
        _check(_lib().vh_get_features(self._h, which, None, 0, C.byref(n)), "vh_get_features", allow=(VH_ERR_CAPACITY,))
        out = np.zeros((n.value, 12), np.int32)
        if n.value:
            _check(_lib().vh_get_features(self._h, which, _ptr(out), n.value, C.byref(n)), "vh_get_features")
        return out

    def synchronize(self):
        _check(_lib().vh_synchronize(self._h), "vh_synchronize")

    def setStream(self, hip_stream: int | None):
        """Order every pushBack after `hip_stream` (a hipStream_t handle; 0 is the legacy
        default stream, a stream like any other); None removes the ordering."""
        if hip_stream is None:
            _check(_lib().vh_clear_stream(self._h), "vh_clear_stream")
        else:
            _check(_lib().vh_set_stream(self._h, C.c_void_p(int(hip_stream))), "vh_set_stream")

    def streamWaitImages(self, hip_stream: int):
        """Make `hip_stream` wait (device side) until the last pushBackDevice's images were consumed."""
        _check(_lib().vh_stream_wait_images(self._h, C.c_void_p(int(hip_stream))), "vh_stream_wait_images")


# ------------------------------------------------------------------ S streams in lock step
class StreamGroup:
    """S independent camera streams stepped together (vh_group_*): the
    multi-stream configuration, one sequence per stream, no exchange between
    streams.  Images are device pointers (e.g. torch `tensor.data_ptr()`)."""

    def __init__(self, n_streams: int, param: Params | None = None, device: int = 0,
                 max_features: int = 0, max_matches: int = 0):
        self.param = param if param is not None else Params.default()
        self.S = int(n_streams)
        h = C.c_void_p()
        _check(_lib().vh_group_create(C.byref(self.param), device, self.S, max_features, max_matches, C.byref(h)),
               "vh_group_create")
        self._h = h

    def close(self):
        if getattr(self, "_h", None):
            _lib().vh_group_destroy(self._h)
            self._h = None

    __del__ = close

    def pushBackDevice(self, ptr1: int, ptr2: int | None, stride_bytes: int, dims, replace=False):
        _check(_lib().vh_group_push_back_device(self._h, C.c_void_p(ptr1), C.c_void_p(ptr2) if ptr2 else None,
                                                int(stride_bytes), _dims(dims), 1 if replace else 0),
               "vh_group_push_back_device")

    def pushBack(self, I1, I2=None, dims=None, replace=False):
        """I1/I2: (S, H, bpl) uint8 numpy arrays."""
        I1 = np.ascontiguousarray(I1, dtype=np.uint8)
        assert I1.ndim == 3 and I1.shape[0] == self.S
        if I2 is not None:
            I2 = np.ascontiguousarray(I2, dtype=np.uint8)
        if dims is None:
            dims = [I1.shape[2], I1.shape[1], I1.shape[2]]
        _check(_lib().vh_group_push_back(self._h, _ptr(I1), _ptr(I2), I1.shape[1] * I1.shape[2], _dims(dims),
                                         1 if replace else 0), "vh_group_push_back")

    def matchFeatures(self, method: int):
        _check(_lib().vh_group_match_features(self._h, int(method)), "vh_group_match_features")

    def deviceBytes(self) -> int:
        """Device memory held by the group (after the first pushBack)."""
        return int(_lib().vh_group_device_bytes(self._h))

    def removeOutliers(self, host_threads: int = 0):
        """Matcher.removeOutliers for every stream, on `host_threads` host workers (0: all)."""
        _check(_lib().vh_group_remove_outliers(self._h, int(host_threads)), "vh_group_remove_outliers")

    def matchFeaturesPrior(self, method: int, Tr_delta):
        """matchFeatures with a motion prior per stream: Tr_delta [S, 4, 4] (vh_group_match_features_prior)."""
        tr = np.ascontiguousarray(Tr_delta, dtype=np.float64).reshape(self.S, 16)
        _check(_lib().vh_group_match_features_prior(self._h, int(method), _ptr(tr)), "vh_group_match_features_prior")

    def getMatches(self, stream: int) -> np.ndarray:
        n = C.c_int32(0)
        rc = _check(_lib().vh_group_get_matches(self._h, stream, None, 0, C.byref(n)), "vh_group_get_matches",
                    allow=(VH_ERR_CAPACITY,))
        out = np.zeros(n.value, P_MATCH_DTYPE)
        if n.value:
            _check(_lib().vh_group_get_matches(self._h, stream, _ptr(out), n.value, C.byref(n)), "vh_group_get_matches")
        elif rc != VH_OK:
            raise VisoHipError(rc, "vh_group_get_matches")
        return out

    def setMultiStageMatching(self, on: bool = True):
        """Two-pass matching of stock libviso2 for every stream (vh_group_set_multi_stage_matching): before the first
        pushBack, with param.multi_stage = 1; not on a SequenceGroup."""
        _check(_lib().vh_group_set_multi_stage_matching(self._h, 1 if on else 0), "vh_group_set_multi_stage_matching")

    def setMultiStageDevice(self, on: bool = True):
        """The vote and the statistics between the two passes on the GPU for every stream
        (vh_group_set_multi_stage_device): after setMultiStageMatching(True), before the first pushBack."""
        _check(_lib().vh_group_set_multi_stage_device(self._h, 1 if on else 0), "vh_group_set_multi_stage_device")

    def setMultiStagePrior(self, on: bool = True):
        """matchFeaturesPrior hands the motion estimates to both passes of multi-stage matching
        (vh_group_set_multi_stage_prior): after multi-stage matching was switched on, before the first pushBack."""
        _check(_lib().vh_group_set_multi_stage_prior(self._h, 1 if on else 0), "vh_group_set_multi_stage_prior")

    def getSparseMatches(self, stream: int) -> np.ndarray:
        """The sparse list of pass 1 after the vote (multi-stage matching on)."""
        n = C.c_int32(0)
        _check(_lib().vh_group_get_sparse_matches(self._h, stream, None, 0, C.byref(n)), "vh_group_get_sparse_matches",
               allow=(VH_ERR_CAPACITY,))
        out = np.zeros(n.value, P_MATCH_DTYPE)
        if n.value:
            _check(_lib().vh_group_get_sparse_matches(self._h, stream, _ptr(out), n.value, C.byref(n)), "vh_group_get_sparse_matches")
        return out

    def setTrackLinking(self, on: bool = True):
        """Link every stream's (row's) match lists to their predecessors on the GPU (vh_group_set_track_linking): before
        the first pushBack; also on a SequenceGroup."""
        _check(_lib().vh_group_set_track_linking(self._h, 1 if on else 0), "vh_group_set_track_linking")

    def setVoteRule(self, rule: int = VOTE_STOCK):
        """The rule of every outlier vote of this handle (vh_group_set_vote_rule), before the first push: VOTE_REFERENCE or
        VOTE_STOCK -- the per-method rule under this handle's outlier_flow_tolerance / outlier_disp_tolerance."""
        _check(_lib().vh_group_set_vote_rule(self._h, int(rule)), "vh_group_set_vote_rule")

    def getTracks(self, stream: int) -> np.ndarray:
        """One TRACK record per record of the stream's (row's) list of the last matchFeatures (vh_group_get_tracks)."""
        n = C.c_int32(0)
        rc = _check(_lib().vh_group_get_tracks(self._h, stream, None, 0, C.byref(n)), "vh_group_get_tracks", allow=(VH_ERR_CAPACITY,))
        out = np.zeros(n.value, TRACK)
        if n.value:
            _check(_lib().vh_group_get_tracks(self._h, stream, _ptr(out), n.value, C.byref(n)), "vh_group_get_tracks")
        elif rc != VH_OK:
            raise VisoHipError(rc, "vh_group_get_tracks")
        return out

    def getTracksAll(self, out: np.ndarray | None = None, cap_per_stream: int | None = None):
        """-> (records [S, cap_per_stream] TRACK, counts [S]) as getMatchesAll (vh_group_get_tracks_all)."""
        if out is None:
            if cap_per_stream is None:
                cap_per_stream = int(self.getCounts()[1].max(initial=0))
            out = np.zeros((self.S, max(cap_per_stream, 1)), TRACK)
        assert out.dtype == TRACK and out.ndim == 2 and out.shape[0] == self.S and out.flags.c_contiguous
        counts = np.zeros(self.S, np.int32)
        _check(_lib().vh_group_get_tracks_all(self._h, _ptr(out), out.shape[1], _ptr(counts)), "vh_group_get_tracks_all")
        return out, counts

    def tracksDevice(self):
        """-> (device address of stream 0's track records, stride in records): valid until the next matchFeatures."""
        ptr = C.c_void_p(); stride = C.c_int64(0)
        _check(_lib().vh_group_tracks_device(self._h, C.byref(ptr), C.byref(stride)), "vh_group_tracks_device")
        return ptr.value, stride.value

    def getFeatures(self, stream: int, which: int) -> np.ndarray:
        n = C.c_int32(0)
        _check(_lib().vh_group_get_features(self._h, stream, which, None, 0, C.byref(n)), "vh_group_get_features",
               allow=(VH_ERR_CAPACITY,))
        out = np.zeros((n.value, 12), np.int32)
        if n.value:
            _check(_lib().vh_group_get_features(self._h, stream, which, _ptr(out), n.value, C.byref(n)),
                   "vh_group_get_features")
        return out

    def getMatchesAll(self, out: np.ndarray | None = None, cap_per_stream: int | None = None):
        """-> (records [S, cap_per_stream] P_MATCH_DTYPE, counts [S]); one wait for the whole group.
        Pass `out` (e.g. from pinned_empty) to reuse a buffer."""
        if out is None:
            if cap_per_stream is None:
                cap_per_stream = int(self.getCounts()[1].max(initial=0))
            out = np.zeros((self.S, max(cap_per_stream, 1)), P_MATCH_DTYPE)
        assert out.dtype == P_MATCH_DTYPE and out.ndim == 2 and out.shape[0] == self.S and out.flags.c_contiguous
        counts = np.zeros(self.S, np.int32)
        _check(_lib().vh_group_get_matches_all(self._h, _ptr(out), out.shape[1], _ptr(counts)), "vh_group_get_matches_all")
        return out, counts

    def downloadMatchesAsync(self, out: np.ndarray, counts: np.ndarray):
        """Start the asynchronous download of all streams' match lists into page-locked
        `out` [S, cap] / `counts` [S] (pinned_empty); waitDownload() before reading them."""
        assert out.dtype == P_MATCH_DTYPE and out.ndim == 2 and out.shape[0] == self.S and out.flags.c_contiguous
        assert counts.dtype == np.int32 and counts.shape == (self.S,) and counts.flags.c_contiguous
        _check(_lib().vh_group_download_matches_async(self._h, _ptr(out), out.shape[1], _ptr(counts)),
               "vh_group_download_matches_async")

    def waitDownload(self):
        _check(_lib().vh_group_wait_download(self._h), "vh_group_wait_download")

    def getCounts(self):
        nf = np.zeros((self.S, 4), np.int32)
        nm = np.zeros(self.S, np.int32)
        _check(_lib().vh_group_get_counts(self._h, _ptr(nf), _ptr(nm)), "vh_group_get_counts")
        return nf, nm

    def synchronize(self):
        _check(_lib().vh_group_synchronize(self._h), "vh_group_synchronize")

    def setStream(self, hip_stream: int | None):
        """Order every pushBack after `hip_stream` (a hipStream_t handle; 0 is the legacy
        default stream, a stream like any other); None removes the ordering."""
        if hip_stream is None:
            _check(_lib().vh_group_clear_stream(self._h), "vh_group_clear_stream")
        else:
            _check(_lib().vh_group_set_stream(self._h, C.c_void_p(int(hip_stream))), "vh_group_set_stream")

    def streamWaitImages(self, hip_stream: int):
        """Make `hip_stream` wait (device side) until the last pushBackDevice's images were consumed."""
        _check(_lib().vh_group_stream_wait_images(self._h, C.c_void_p(int(hip_stream))), "vh_group_stream_wait_images")

    def estimateMotion(self, ego: "EgoParams", rand3):
        """VisualOdometryStereo::estimateMotion (reference src/viso_stereo.cpp:54-157) on every stream's
        device-resident quad matches; rand3 [S, ransac_iters, 3] int32 rand() values -> (tr [S,6], ok [S], n_inliers [S])."""
        rand3 = np.ascontiguousarray(rand3, np.int32)
        assert rand3.shape == (self.S, ego.ransac_iters, 3)
        tr = np.zeros((self.S, 6), np.float64); ok = np.zeros(self.S, np.int32); ninl = np.zeros(self.S, np.int32)
        _check(_lib().vh_group_estimate_motion(self._h, C.byref(ego), _ptr(rand3), _ptr(tr), _ptr(ok), _ptr(ninl)), "vh_group_estimate_motion")
        return tr, ok.astype(bool), ninl

    def motionInliers(self, ego: "EgoParams", tr, ok) -> np.ndarray:
        """VisualOdometryStereo::getInlier (reference src/viso_stereo.cpp:159-177) on every stream's whole device-resident
        quad list under tr [S, 6] / ok [S], e.g. from estimateMotion (vh_group_motion_inliers) -> inliers per stream [S]."""
        tr = np.ascontiguousarray(tr, np.float64); ok = np.ascontiguousarray(ok).astype(np.int32)
        assert tr.shape == (self.S, 6) and ok.shape == (self.S,)
        counts = np.zeros(self.S, np.int32)
        _check(_lib().vh_group_motion_inliers(self._h, C.byref(ego), _ptr(tr), _ptr(ok), _ptr(counts)), "vh_group_motion_inliers")
        return counts

    def refitMotion(self, ego: "EgoParams", reclassify: bool = False):
        """The reference's final optimisation (src/viso_stereo.cpp:126-139) on every stream's compacted inlier list of the last
        motionInliers, from the tr / ok it classified under (vh_group_refit_motion) -> (tr [S, 6], ok [S], n_updates [S],
        counts [S]); reclassify: the lists are classified again under the refined motions (queued behind the refit), and
        counts and the getters are that classification's."""
        tr = np.zeros((self.S, 6), np.float64); ok = np.zeros(self.S, np.int32); nupd = np.zeros(self.S, np.int32)
        counts = np.zeros(self.S, np.int32)
        _check(_lib().vh_group_refit_motion(self._h, C.byref(ego), 1 if reclassify else 0, _ptr(tr), _ptr(ok), _ptr(nupd), _ptr(counts)),
               "vh_group_refit_motion")
        return tr, ok.astype(bool), nupd, counts

    def motionCovariance(self, ego: "EgoParams", tr=None, ok=None):
        """The covariance of every stream's stereo motion over its compacted inlier list (vh_group_motion_covariance)
        -> (cov [S, 6, 6], ssr [S], ok [S], counts [S]).  tr None (then ok None): under the tr / ok the lists were
        classified under -- after refitMotion(reclassify=True) the refined motions -- which are on the device; else under
        tr [S, 6] / ok [S], e.g. refitMotion's results after reclassify=False.  One without the other: VH_ERR_INVALID_ARG."""
        cov = np.zeros((self.S, 6, 6), np.float64); ssr = np.zeros(self.S, np.float64); oko = np.zeros(self.S, np.int32)
        counts = np.zeros(self.S, np.int32)
        if tr is not None:
            tr = np.ascontiguousarray(tr, np.float64)
            assert tr.shape == (self.S, 6)
        if ok is not None:
            ok = np.ascontiguousarray(ok).astype(np.int32).reshape(self.S)
        _check(_lib().vh_group_motion_covariance(self._h, C.byref(ego), None if tr is None else _ptr(tr), None if ok is None else _ptr(ok),
                                                 _ptr(cov), _ptr(ssr), _ptr(oko), _ptr(counts)), "vh_group_motion_covariance")
        return cov, ssr, oko.astype(bool), counts

    def motionInliersMono(self, mono: "MonoParams", model, ok) -> np.ndarray:
        """VisualOdometryMono::getInlier (reference src/viso_mono.cpp:268-315) on every stream's whole device-resident flow
        or quad list under model [S] (MONO_MODEL_DTYPE) / ok [S], e.g. from estimateMotionMono(model=True)
        (vh_group_motion_inliers_mono) -> inliers per stream [S]; the getters are motionInliers'."""
        model = _models(model, self.S)
        ok = np.ascontiguousarray(ok).astype(np.int32).reshape(self.S)
        counts = np.zeros(self.S, np.int32)
        _check(_lib().vh_group_motion_inliers_mono(self._h, C.byref(mono), _ptr(model), _ptr(ok), _ptr(counts)), "vh_group_motion_inliers_mono")
        return counts

    def refitModelMono(self, mono: "MonoParams", reclassify: bool = False):
        """fundamentalMatrix (reference src/viso_mono.cpp:235-266) on every stream's compacted inlier list of the last
        motionInliersMono, in the frame of the model / ok it classified under (vh_group_refit_model_mono) -> (model [S]
        MONO_MODEL_DTYPE, ok [S], w [S, 2] = the two smallest singular values w[8], w[7] of the moment matrix, counts [S]);
        reclassify: the lists are classified again under the refined models (queued behind the refit), and counts and the
        getters are that classification's."""
        model = np.zeros(self.S, MONO_MODEL_DTYPE); ok = np.zeros(self.S, np.int32); w = np.zeros((self.S, 2), np.float64)
        counts = np.zeros(self.S, np.int32)
        _check(_lib().vh_group_refit_model_mono(self._h, C.byref(mono), 1 if reclassify else 0, _ptr(model), _ptr(ok), _ptr(w), _ptr(counts)),
               "vh_group_refit_model_mono")
        return model, ok.astype(bool), w, counts

    def poseMono(self, mono: "MonoParams", pose: bool = False, refine: bool = False):
        """The mono pose (reference src/viso_mono.cpp:83-158: E, R|t, chirality, the ground-plane scale) over every stream's
        compacted inlier list of the last motionInliersMono, under the model / ok it classified under -- after
        refitModelMono(reclassify=True) the refined model with its inliers (vh_group_pose_mono) -> (tr [S, 6], ok [S],
        counts [S]) and, with pose=True, the MONO_POSE_DTYPE records [S] as a fourth value.  refine=True: every winning R|t
        is refined by Gauss-Newton on the Sampson distance of every inlier before the scale tail
        (vh_group_pose_mono_refined), and the MONO_REFINE_DTYPE records [S] are one more value at the end."""
        tr = np.zeros((self.S, 6), np.float64); ok = np.zeros(self.S, np.int32); counts = np.zeros(self.S, np.int32)
        rec = np.zeros(self.S, MONO_POSE_DTYPE)
        if refine:
            ref = np.zeros(self.S, MONO_REFINE_DTYPE)
            _check(_lib().vh_group_pose_mono_refined(self._h, C.byref(mono), _ptr(tr), _ptr(ok), _ptr(rec) if pose else None, _ptr(ref),
                                                     _ptr(counts)), "vh_group_pose_mono_refined")
            return (tr, ok.astype(bool), counts, rec, ref) if pose else (tr, ok.astype(bool), counts, ref)
        _check(_lib().vh_group_pose_mono(self._h, C.byref(mono), _ptr(tr), _ptr(ok), _ptr(rec) if pose else None, _ptr(counts)), "vh_group_pose_mono")
        return (tr, ok.astype(bool), counts, rec) if pose else (tr, ok.astype(bool), counts)

    def scenePoints(self, e, sp: "SceneParams | None" = None, Tw=None) -> np.ndarray:
        """The 3-d point of every inlier of every stream's current classification, left on the device: with an EgoParams
        the stereo form (vh_group_scene_points_stereo, under the motion the stereo classification was made under -- after
        refitMotion(reclassify=True) the refined one), with a MonoParams the mono form (vh_group_scene_points_mono, under
        the pose of the last poseMono); the other kind of classification is VH_ERR_STATE.  Tw: None, one 4x4 or [S, 4, 4],
        applied last.  -> counts [S]; getScenePoints(stream) / getScenePointsAll / scenePointsDevice give the points."""
        sp = sp or SceneParams.default()
        tw = _scene_Tw(Tw, self.S)
        counts = np.zeros(self.S, np.int32)
        fn = "vh_group_scene_points_mono" if isinstance(e, MonoParams) else "vh_group_scene_points_stereo"
        _check(getattr(_lib(), fn)(self._h, C.byref(e), C.byref(sp), None if tw is None else _ptr(tw), _ptr(counts)), fn)
        return counts

    def setTrajectory(self, params: "TrajParams | None" = None, T0=None, on: bool = True):
        """Accumulate every stream's pose on the device (vh_group_set_trajectory; a SequenceGroup: one pose along the rows
        of its chunks, vh_sequence_set_trajectory): before the first pushBack.  T0: None, one 4x4 or [S, 4, 4] (a
        SequenceGroup: one 4x4); on=False switches the feature off."""
        tp = params or TrajParams.default()
        seq = isinstance(self, SequenceGroup)
        t0 = _traj_T0(T0, 1 if seq else self.S)
        fn = "vh_sequence_set_trajectory" if seq else "vh_group_set_trajectory"
        _check(getattr(_lib(), fn)(self._h, C.byref(tp) if on else None, _ptr(t0)), fn)

    def trajectory(self, source: int = TRAJ_STEREO) -> np.ndarray:
        """One step of every pose under the motions of the current classification (vh_group_trajectory; TRAJ_STEREO: the
        motion of motionInliers / refitMotion(reclassify=True), TRAJ_MONO: poseMono's) -> TRAJ_POSE_DTYPE [S] (a
        SequenceGroup: one record per row of the chunk, walked as one chain).  A repeated call for the same pair
        recomputes the step."""
        out = np.zeros(self.S, TRAJ_POSE_DTYPE)
        _check(_lib().vh_group_trajectory(self._h, source, _ptr(out)), "vh_group_trajectory")
        return out

    def getPoses(self) -> np.ndarray:
        """The records of the last trajectory(), valid until the next pushBack (vh_group_get_poses) -> TRAJ_POSE_DTYPE [S]."""
        out = np.zeros(self.S, TRAJ_POSE_DTYPE)
        _check(_lib().vh_group_get_poses(self._h, _ptr(out)), "vh_group_get_poses")
        return out

    def posesDevice(self):
        """-> (device address of the records of the last trajectory(), stride in records)"""
        d = C.c_void_p(); stride = C.c_int64(0)
        _check(_lib().vh_group_poses_device(self._h, C.byref(d), C.byref(stride)), "vh_group_poses_device")
        return d.value, stride.value

    def setPose(self, stream: int, T):
        """The chain of `stream` (a SequenceGroup: 0) continues from the 4x4 T (vh_group_set_pose)."""
        t = np.ascontiguousarray(T, np.float64).reshape(16)
        _check(_lib().vh_group_set_pose(self._h, stream, _ptr(t)), "vh_group_set_pose")

    def setTrajectoryCovariance(self, params: "TrajCovParams | None" = None, Sigma0=None, on: bool = True):
        """Propagate every pose's covariance with the pose (vh_group_set_trajectory_covariance; a SequenceGroup:
        vh_sequence_set_trajectory_covariance): behind setTrajectory, before the first pushBack.  Sigma0: None, one 6x6 or
        [S, 6, 6] (a SequenceGroup: one 6x6); on=False switches it off.  trajectory() then needs motionCovariance(ego)
        (tr None) of the current classification in front of it."""
        tcp = params or TrajCovParams.default()
        seq = isinstance(self, SequenceGroup)
        fn = "vh_sequence_set_trajectory_covariance" if seq else "vh_group_set_trajectory_covariance"
        _check(getattr(_lib(), fn)(self._h, C.byref(tcp) if on else None, _ptr(_traj_S0(Sigma0, 1 if seq else self.S))), fn)

    def getPoseCovariances(self) -> np.ndarray:
        """The covariance records of the last trajectory() (vh_group_get_pose_covariances) -> TRAJ_COV_DTYPE [S]."""
        out = np.zeros(self.S, TRAJ_COV_DTYPE)
        _check(_lib().vh_group_get_pose_covariances(self._h, _ptr(out)), "vh_group_get_pose_covariances")
        return out

    def poseCovariancesDevice(self):
        """-> (device address of the covariance records of the last trajectory(), stride in records)"""
        d = C.c_void_p(); stride = C.c_int64(0)
        _check(_lib().vh_group_pose_covariances_device(self._h, C.byref(d), C.byref(stride)), "vh_group_pose_covariances_device")
        return d.value, stride.value

    def setPoseCovariance(self, stream: int, Sigma):
        """The covariance of the chain of `stream` (a SequenceGroup: 0) continues from the 6x6 Sigma
        (vh_group_set_pose_covariance)."""
        s = np.ascontiguousarray(Sigma, np.float64).reshape(36)
        _check(_lib().vh_group_set_pose_covariance(self._h, stream, _ptr(s)), "vh_group_set_pose_covariance")

    def scenePointsWorld(self, e, sp: "SceneParams | None" = None) -> np.ndarray:
        """scenePoints with Tw taken from the trajectory's poses on the device: Tw_prev for sp.frame 0, Tw_cur for 1
        (vh_group_scene_points_stereo_world / _mono_world); after trajectory() of the current match.  -> counts [S]"""
        sp = sp or SceneParams.default()
        counts = np.zeros(self.S, np.int32)
        fn = "vh_group_scene_points_mono_world" if isinstance(e, MonoParams) else "vh_group_scene_points_stereo_world"
        _check(getattr(_lib(), fn)(self._h, C.byref(e), C.byref(sp), _ptr(counts)), fn)
        return counts

    def getScenePoints(self, stream: int) -> np.ndarray:
        """The stream's points of the last scenePoints in list order, SCENE_POINT_DTYPE [n] (vh_group_get_scene_points)."""
        n = C.c_int32(0)
        _check(_lib().vh_group_get_scene_points(self._h, stream, None, 0, C.byref(n)), "vh_group_get_scene_points", allow=(VH_ERR_CAPACITY,))
        out = np.zeros(n.value, SCENE_POINT_DTYPE)
        if n.value:
            _check(_lib().vh_group_get_scene_points(self._h, stream, _ptr(out), n.value, C.byref(n)), "vh_group_get_scene_points")
        return out

    def getScenePointsAll(self, cap_per_stream: int):
        """-> (points [S, cap_per_stream], counts [S]) (vh_group_get_scene_points_all)."""
        out = np.zeros((self.S, max(cap_per_stream, 1)), SCENE_POINT_DTYPE); counts = np.zeros(self.S, np.int32)
        _check(_lib().vh_group_get_scene_points_all(self._h, _ptr(out), out.shape[1], _ptr(counts)), "vh_group_get_scene_points_all")
        return out, counts

    def scenePointsDevice(self):
        """-> (device address of stream 0's points, stride in records): valid until the next matchFeatures."""
        d = C.c_void_p(); stride = C.c_int64(0)
        _check(_lib().vh_group_scene_points_device(self._h, C.byref(d), C.byref(stride)), "vh_group_scene_points_device")
        return d.value, stride.value

    def landmarks(self, params: "LandmarkParams | None" = None) -> np.ndarray:
        """The scene points of the last scenePoints fused along every stream's feature tracks (vh_group_landmarks;
        setTrackLinking, and a scenePoints Tw that takes every step's points into one common frame) -> counts [S];
        getLandmarks(stream) / getLandmarksAll / landmarksDevice give the landmarks.  A SequenceGroup: after setLandmarks(True),
        else VH_ERR_UNSUPPORTED."""
        lp = params or LandmarkParams.default()
        counts = np.zeros(self.S, np.int32)
        _check(_lib().vh_group_landmarks(self._h, C.byref(lp), _ptr(counts)), "vh_group_landmarks")
        return counts

    def getLandmarks(self, stream: int) -> np.ndarray:
        """The stream's landmarks of the last landmarks() in list order, LANDMARK_DTYPE [n] (vh_group_get_landmarks)."""
        n = C.c_int32(0)
        _check(_lib().vh_group_get_landmarks(self._h, stream, None, 0, C.byref(n)), "vh_group_get_landmarks", allow=(VH_ERR_CAPACITY,))
        out = np.zeros(n.value, LANDMARK_DTYPE)
        if n.value:
            _check(_lib().vh_group_get_landmarks(self._h, stream, _ptr(out), n.value, C.byref(n)), "vh_group_get_landmarks")
        return out

    def getLandmarksAll(self, cap_per_stream: int):
        """-> (landmarks [S, cap_per_stream], counts [S]) (vh_group_get_landmarks_all)."""
        out = np.zeros((self.S, max(cap_per_stream, 1)), LANDMARK_DTYPE); counts = np.zeros(self.S, np.int32)
        _check(_lib().vh_group_get_landmarks_all(self._h, _ptr(out), out.shape[1], _ptr(counts)), "vh_group_get_landmarks_all")
        return out, counts

    def landmarksDevice(self):
        """-> (device address of stream 0's landmarks, stride in records): valid until the next matchFeatures."""
        d = C.c_void_p(); stride = C.c_int64(0)
        _check(_lib().vh_group_landmarks_device(self._h, C.byref(d), C.byref(stride)), "vh_group_landmarks_device")
        return d.value, stride.value

    def setGain(self, on: bool = True):
        """Keep the pushed left images of every stream (sequence handle: frame) on the device for gain()
        (vh_group_set_gain): before the first push."""
        _check(_lib().vh_group_set_gain(self._h, 1 if on else 0), "vh_group_set_gain")

    def gain(self, indices=None):
        """Matcher::getGain (reference src/matcher.h:148) for every stream (sequence handle: row): over the inlier
        positions of the current classification (indices None, vh_group_gain) or over `indices`, one array of positions
        into getMatches(s) per stream (vh_group_gain_indices) -> (gain float32 [S], num int32 [S])."""
        gain = np.zeros(self.S, np.float32); num = np.zeros(self.S, np.int32)
        if indices is None:
            _check(_lib().vh_group_gain(self._h, _ptr(gain), _ptr(num)), "vh_group_gain")
            return gain, num
        lists = [np.ascontiguousarray(q, np.int32).reshape(-1) for q in indices]
        assert len(lists) == self.S
        off = np.zeros(self.S + 1, np.int32)
        off[1:] = np.cumsum([len(q) for q in lists])
        idx = np.concatenate(lists) if off[-1] else np.zeros(1, np.int32)
        _check(_lib().vh_group_gain_indices(self._h, _ptr(idx), _ptr(off), _ptr(gain), _ptr(num)), "vh_group_gain_indices")
        return gain, num

    def getInlierFlags(self, stream: int) -> np.ndarray:
        """One byte per record of the stream's list: 1 = inlier of the last motionInliers (vh_group_get_inlier_flags)."""
        n = C.c_int32(0)
        _check(_lib().vh_group_get_inlier_flags(self._h, stream, None, 0, C.byref(n)), "vh_group_get_inlier_flags", allow=(VH_ERR_CAPACITY,))
        out = np.zeros(n.value, np.uint8)
        if n.value:
            _check(_lib().vh_group_get_inlier_flags(self._h, stream, _ptr(out), n.value, C.byref(n)), "vh_group_get_inlier_flags")
        return out

    def getInlierMatches(self, stream: int):
        """-> (the stream's inlier records in list order, their positions in getMatches(stream)) (vh_group_get_inlier_matches)."""
        n = C.c_int32(0)
        _check(_lib().vh_group_get_inlier_matches(self._h, stream, None, None, 0, C.byref(n)), "vh_group_get_inlier_matches",
               allow=(VH_ERR_CAPACITY,))
        out = np.zeros(n.value, P_MATCH_DTYPE); pos = np.zeros(n.value, np.int32)
        if n.value:
            _check(_lib().vh_group_get_inlier_matches(self._h, stream, _ptr(out), _ptr(pos), n.value, C.byref(n)), "vh_group_get_inlier_matches")
        return out, pos

    def getInlierMatchesAll(self, cap_per_stream: int):
        """-> (records [S, cap_per_stream], positions [S, cap_per_stream], counts [S]) (vh_group_get_inlier_matches_all)."""
        out = np.zeros((self.S, max(cap_per_stream, 1)), P_MATCH_DTYPE); pos = np.zeros((self.S, max(cap_per_stream, 1)), np.int32)
        counts = np.zeros(self.S, np.int32)
        _check(_lib().vh_group_get_inlier_matches_all(self._h, _ptr(out), _ptr(pos), out.shape[1], _ptr(counts)), "vh_group_get_inlier_matches_all")
        return out, pos, counts

    def inliersDevice(self):
        """-> (device addresses of stream 0's flags, inlier records and positions, stride in elements): valid until the
        next matchFeatures (vh_group_inliers_device)."""
        f = C.c_void_p(); m = C.c_void_p(); q = C.c_void_p(); stride = C.c_int64(0)
        _check(_lib().vh_group_inliers_device(self._h, C.byref(f), C.byref(m), C.byref(q), C.byref(stride)), "vh_group_inliers_device")
        return f.value, m.value, q.value, stride.value

    def postBegin(self, cap_per_stream: int):
        """Start the download of this step's match lists into an internal page-locked slot (vh_group_post_begin)."""
        _check(_lib().vh_group_post_begin(self._h, int(cap_per_stream)), "vh_group_post_begin")

    def postFinish(self, age: int, max_features: int, bucket_width: float, bucket_height: float, host_threads: int = 0,
                   ego: "EgoParams" = None, rand3=None, want_lists: bool = True, list_cap: int = 0, mono: "MonoParams" = None, rand8=None):
        """removeOutliers + bucketFeatures (+ the stereo estimateMotion when `ego` is given, the monocular one when
        `mono` is) of the step begun `age` begins ago (vh_group_post_finish / vh_group_post_finish_mono)
        -> dict(tr, ok, n_inliers, lists, host_ms)."""
        S = self.S
        tr = np.zeros((S, 6), np.float64); ok = np.zeros(S, np.int32); ninl = np.zeros(S, np.int32)
        counts = np.zeros(S, np.int32); ms = C.c_double(0.0)
        out = None
        if want_lists:
            list_cap = int(list_cap) if list_cap else 4096
            out = np.zeros((S, list_cap), P_MATCH_DTYPE)
        r3 = None
        if ego is not None:
            r3 = np.ascontiguousarray(rand3, np.int32)
            assert r3.shape == (S, ego.ransac_iters, 3)
        if mono is not None:
            assert ego is None
            r8 = np.ascontiguousarray(rand8, np.int32)
            assert r8.shape == (S, mono.ransac_iters, 8)
            _check(_lib().vh_group_post_finish_mono(self._h, int(age), int(max_features), C.c_float(bucket_width), C.c_float(bucket_height),
                                                    int(host_threads), C.byref(mono), _ptr(r8), _ptr(tr), _ptr(ok),
                                                    _ptr(ninl), _ptr(out), int(list_cap), _ptr(counts), C.byref(ms)), "vh_group_post_finish_mono")
        else:
            _check(_lib().vh_group_post_finish(self._h, int(age), int(max_features), C.c_float(bucket_width), C.c_float(bucket_height),
                                               int(host_threads), C.byref(ego) if ego is not None else None, _ptr(r3), _ptr(tr), _ptr(ok),
                                               _ptr(ninl), _ptr(out), int(list_cap), _ptr(counts), C.byref(ms)), "vh_group_post_finish")
        lists = [out[s, :counts[s]].copy() for s in range(S)] if want_lists else None
        return {"tr": tr, "ok": ok.astype(bool), "n_inliers": ninl, "lists": lists, "counts": counts, "host_ms": ms.value}

    def postDeviceConfig(self, steps_per_batch: int = 64, batches: int = 3, lanes_per_wave: int = 16):
        """Shape of the device post stage's pipeline (vh_group_post_device_config); the defaults are the library's own
        (64 steps per batch, 3 batches, 16 lists per wave: the throughput-optimal shape, up to a second of latency)."""
        _check(_lib().vh_group_post_device_config(self._h, int(steps_per_batch), int(batches), int(lanes_per_wave)), "vh_group_post_device_config")

    def postDeviceDense(self, mode: int):
        """Dense inliers and the motion refit as stages of the device post chain (vh_group_post_device_dense): 0 off (the
        default), 1 classify every stream's voted list under the batch's motion, 2 and refit on the inliers (stereo
        estimator), 3 and classify again under the refined motion.  Not while steps are in flight."""
        _check(_lib().vh_group_post_device_dense(self._h, int(mode)), "vh_group_post_device_dense")
        self._dense_mode = int(mode)

    def postDeviceTail(self, stages: int):
        """The covariance, the mono refit and the mono pose as stages of the device post chain behind the dense ones
        (vh_group_post_device_tail): a mask of POST_TAIL_COV (stereo estimator, dense mode >= 1), POST_TAIL_MONO_REFIT,
        POST_TAIL_MONO_POSE and POST_TAIL_MONO_REFINE (mono estimator, dense mode 1; REFINE needs POSE); 0 off (the
        default).  Not while steps are in flight."""
        _check(_lib().vh_group_post_device_tail(self._h, int(stages)), "vh_group_post_device_tail")
        self._tail_mask = int(stages)

    def postDeviceShape(self):
        """-> (steps per batch, batches) in effect (vh_group_post_device_shape): the first postBeginDevice of a ring may
        have halved the steps per batch postDeviceConfig asked for; before it, the configured shape."""
        steps, batches = C.c_int32(0), C.c_int32(0)
        _check(_lib().vh_group_post_device_shape(self._h, C.byref(steps), C.byref(batches)), "vh_group_post_device_shape")
        return steps.value, batches.value

    def postBeginDevice(self, cap_per_stream: int, max_features: int, bucket_width: float, bucket_height: float,
                        ego: "EgoParams" = None, rand3=None, mono: "MonoParams" = None, rand8=None, want_lists: bool = False):
        """This step's match lists enter the device post stage: removeOutliers -> bucketFeatures -> estimateMotion, all on
        the GPU (vh_group_post_begin_device)."""
        r3 = r8 = None
        if ego is not None:
            r3 = np.ascontiguousarray(rand3, np.int32)
            assert r3.shape == (self.S, ego.ransac_iters, 3)
        if mono is not None:
            r8 = np.ascontiguousarray(rand8, np.int32)
            assert r8.shape == (self.S, mono.ransac_iters, 8)
        _check(_lib().vh_group_post_begin_device(self._h, int(cap_per_stream), int(max_features), C.c_float(bucket_width), C.c_float(bucket_height),
                                                 C.byref(ego) if ego is not None else None, _ptr(r3),
                                                 C.byref(mono) if mono is not None else None, _ptr(r8), 1 if want_lists else 0),
               "vh_group_post_begin_device")
        # what the steps in flight were begun with: postFinishDevice(dense=...) asks for what such a step produced
        steps = self.__dict__.setdefault("_dense_steps", [])
        steps.append((getattr(self, "_dense_mode", 0), mono is not None))
        del steps[:-(256 * 64)]
        tails = self.__dict__.setdefault("_tail_steps", [])   # and postFinishDevice(tail=...) likewise
        tails.append(getattr(self, "_tail_mask", 0))
        del tails[:-(256 * 64)]

    def postFinishDevice(self, age: int, want_lists: bool = False, list_cap: int = 4096, estimator: bool = True, strict: bool = True,
                         dense=None, tail=None):
        """Results of the step begun `age` begins ago (vh_group_post_finish_device) -> dict(tr, ok, n_inliers, lists, counts).
        strict=False: a refused list does not raise; its stream reports counts = -1 and the dict carries the code as "rc".
        dense (vh_group_post_finish_device_dense, after postDeviceDense(mode >= 1)): a tuple of "counts" -- adds voted_counts
        [S], inlier_counts [S], with modes 2 and 3 tr_refit [S, 6], ok_refit [S], n_updates [S], with the monocular estimator
        model [S] -- and "lists" -- adds voted, flags, inliers, src_pos: one array per stream (empty where the count is
        -1; every list must fit list_cap).  "refit" / "model" ask for those outputs whatever the step was begun with.
        tail (vh_group_post_finish_device_tail, after postDeviceTail(mask)): names out of "cov" -- adds cov [S, 6, 6], ssr
        [S], ok_cov [S] --, "mono_refit" -- model_refit [S], ok_model [S], w [S, 2] --, "pose" -- tr_pose [S, 6], ok_pose
        [S], pose [S] (MONO_POSE_DTYPE) -- and "refine" -- refine [S] (MONO_REFINE_DTYPE); () adds what the step was begun
        with, a name asks for its outputs whatever the step was begun with."""
        S = self.S
        tr = np.zeros((S, 6), np.float64); ok = np.zeros(S, np.int32); ninl = np.zeros(S, np.int32); counts = np.zeros(S, np.int32)
        out = np.zeros((S, int(list_cap)), P_MATCH_DTYPE) if want_lists else None
        args = (self._h, int(age), _ptr(tr) if estimator else None, _ptr(ok) if estimator else None,
                _ptr(ninl) if estimator else None, _ptr(out), int(list_cap) if want_lists else 0, _ptr(counts))
        extra_t = {}
        if tail is not None:
            tail = (tail,) if isinstance(tail, str) else tuple(tail)
            assert set(tail) <= {"cov", "mono_refit", "pose", "refine"}, tail
            tails = getattr(self, "_tail_steps", [])
            mask = tails[-1 - int(age)] if int(age) < len(tails) else 0
            if mask & POST_TAIL_COV or "cov" in tail:
                extra_t.update(cov=np.zeros((S, 6, 6), np.float64), ssr=np.zeros(S, np.float64), ok_cov=np.zeros(S, np.int32))
            if mask & POST_TAIL_MONO_REFIT or "mono_refit" in tail:
                extra_t.update(model_refit=np.zeros(S, MONO_MODEL_DTYPE), ok_model=np.zeros(S, np.int32), w=np.zeros((S, 2), np.float64))
            if mask & POST_TAIL_MONO_POSE or "pose" in tail:
                extra_t.update(tr_pose=np.zeros((S, 6), np.float64), ok_pose=np.zeros(S, np.int32), pose=np.zeros(S, MONO_POSE_DTYPE))
            if mask & POST_TAIL_MONO_REFINE or "refine" in tail:
                extra_t["refine"] = np.zeros(S, MONO_REFINE_DTYPE)
        if dense is None and tail is None:
            name = "vh_group_post_finish_device"
            rc = _lib().vh_group_post_finish_device(*args)
        else:
            name = "vh_group_post_finish_device_dense"
            dargs = args + (None,)
            if dense is not None:
                dense = (dense,) if isinstance(dense, str) else tuple(dense)
                assert dense and set(dense) <= {"counts", "lists", "refit", "model"}, dense
                steps = getattr(self, "_dense_steps", [])
                mode, mono = steps[-1 - int(age)] if int(age) < len(steps) else (0, False)
                cap = int(list_cap)
                extra = {"voted_counts": np.zeros(S, np.int32), "inlier_counts": np.zeros(S, np.int32)}
                if mode >= 2 or "refit" in dense:
                    extra.update(tr_refit=np.zeros((S, 6), np.float64), ok_refit=np.zeros(S, np.int32), n_updates=np.zeros(S, np.int32))
                if mono or "model" in dense:
                    extra["model"] = np.zeros(S, MONO_MODEL_DTYPE)
                if "lists" in dense:
                    extra.update(voted_pm=np.zeros((S, cap), P_MATCH_DTYPE), flags=np.zeros((S, cap), np.uint8),
                                 inlier_pm=np.zeros((S, cap), P_MATCH_DTYPE), src_pos=np.zeros((S, cap), np.int32))
                d = PostDense(**{k: v.ctypes.data for k, v in extra.items()})
                dargs = args[:6] + (cap if (want_lists or "lists" in dense) else 0, args[7], C.byref(d))
            if tail is None:
                rc = _lib().vh_group_post_finish_device_dense(*dargs)
            else:
                name = "vh_group_post_finish_device_tail"
                pt = PostTail(size=C.sizeof(PostTail), **{k: v.ctypes.data for k, v in extra_t.items()})
                rc = _lib().vh_group_post_finish_device_tail(*(dargs + (C.byref(pt),)))
        if strict or rc in (VH_ERR_INVALID_ARG, VH_ERR_STATE, VH_ERR_HIP, VH_ERR_NO_DEVICE):
            _check(rc, name)
        lists = [out[s, :max(int(counts[s]), 0)].copy() for s in range(S)] if want_lists else None
        res = {"tr": tr, "ok": ok.astype(bool), "n_inliers": ninl, "lists": lists, "counts": counts, "rc": rc}
        if dense is not None:
            nv, ni = np.maximum(extra["voted_counts"], 0), np.maximum(extra["inlier_counts"], 0)
            if "ok_refit" in extra:
                extra["ok_refit"] = extra["ok_refit"].astype(bool)
            if "lists" in dense:
                extra["voted"] = [extra["voted_pm"][s, :nv[s]].copy() for s in range(S)]
                extra["flags"] = [extra["flags"][s, :nv[s]].copy() for s in range(S)]
                extra["inliers"] = [extra["inlier_pm"][s, :ni[s]].copy() for s in range(S)]
                extra["src_pos"] = [extra["src_pos"][s, :ni[s]].copy() for s in range(S)]
                del extra["voted_pm"], extra["inlier_pm"]
            res.update(extra)
        for k in ("ok_cov", "ok_model", "ok_pose"):
            if k in extra_t:
                extra_t[k] = extra_t[k].astype(bool)
        res.update(extra_t)
        return res

    def estimateMotionMono(self, mono: "MonoParams", rand8, model: bool = False):
        """VisualOdometryMono::estimateMotion (reference src/viso_mono.cpp:41-160) on every stream's device-resident
        flow (or quad) matches; rand8 [S, ransac_iters, 8] int32 rand() values -> (tr [S,6], ok [S], n_inliers [S]);
        model=True: and the models [S] (MONO_MODEL_DTYPE, vh_group_estimate_motion_mono_model) as a fourth value."""
        rand8 = np.ascontiguousarray(rand8, np.int32)
        assert rand8.shape == (self.S, mono.ransac_iters, 8)
        tr = np.zeros((self.S, 6), np.float64); ok = np.zeros(self.S, np.int32); ninl = np.zeros(self.S, np.int32)
        if model:
            mo = np.zeros(self.S, MONO_MODEL_DTYPE)
            _check(_lib().vh_group_estimate_motion_mono_model(self._h, C.byref(mono), _ptr(rand8), _ptr(tr), _ptr(ok), _ptr(ninl), _ptr(mo)),
                   "vh_group_estimate_motion_mono_model")
            return tr, ok.astype(bool), ninl, mo
        _check(_lib().vh_group_estimate_motion_mono(self._h, C.byref(mono), _ptr(rand8), _ptr(tr), _ptr(ok), _ptr(ninl)), "vh_group_estimate_motion_mono")
        return tr, ok.astype(bool), ninl

    def searchStats(self):
        """-> (speculative loops in use?, last observed share of re-searched queries or -1)."""
        sp = C.c_int32(0); rate = C.c_double(-1.0)
        _check(_lib().vh_group_search_stats(self._h, C.byref(sp), C.byref(rate)), "vh_group_search_stats")
        return bool(sp.value), rate.value

    def setReconstruction(self, recon: "ReconParams | None", history_steps: int = 0):
        """3-d points from the tracks that end, per stream and step, gathered on the device (vh_group_set_reconstruction):
        before the first push only; switches track linking on.  history_steps >= 1: lost tracks older than that come back
        RECON_HISTORY.  recon None: off."""
        _check(_lib().vh_group_set_reconstruction(self._h, C.byref(recon) if recon is not None else None, int(history_steps)),
               "vh_group_set_reconstruction")

    def reconstruct(self, Trs) -> list:
        """The lost tracks of the step of the last match call (vh_group_reconstruct), once per match call, before the next
        one.  Trs [S, 4, 4]: every stream's motion over this step.  -> S RECON_TRACK arrays, each sorted by (lost_frame,
        birth_frame, birth_pos)."""
        tr = np.ascontiguousarray(Trs, dtype=np.float64).reshape(-1, 16)
        assert tr.shape[0] == self.S, (tr.shape, self.S)
        nt, na = C.c_int32(0), C.c_int32(0)
        _check(_lib().vh_group_reconstruct(self._h, _ptr(tr), C.byref(nt), C.byref(na)), "vh_group_reconstruct")
        counts = self.getReconCounts()[0]
        out = []
        for s in range(self.S):
            rec = np.zeros(int(counts[s]), RECON_TRACK)
            n = C.c_int32(0)
            _check(_lib().vh_group_get_recon_tracks(self._h, s, _ptr(rec) if len(rec) else None, len(rec), C.byref(n)), "vh_group_get_recon_tracks")
            out.append(rec[:n.value])
        return out

    def getReconCounts(self):
        """-> (records [S], accepted records [S]) of the last reconstruct call."""
        nt, na = np.zeros(self.S, np.int32), np.zeros(self.S, np.int32)
        _check(_lib().vh_group_get_recon_counts(self._h, _ptr(nt), _ptr(na)), "vh_group_get_recon_counts")
        return nt, na

    def debugFailNextAlloc(self):
        """Test hook: the group's next device allocation fails once."""
        _check(_lib().vh_group_debug_fail_next_alloc(self._h), "vh_group_debug_fail_next_alloc")

    def debugFailAllocAfter(self, skip: int):
        """Test hook: the group's device allocation after `skip` more successful ones fails once."""
        _check(_lib().vh_group_debug_fail_alloc_after(self._h, int(skip)), "vh_group_debug_fail_alloc_after")

    def profileEnable(self, on: bool = True):
        _check(_lib().vh_group_profile_enable(self._h, 1 if on else 0), "vh_group_profile_enable")

    def profileReset(self):
        _check(_lib().vh_group_profile_reset(self._h), "vh_group_profile_reset")

    def profileRead(self, name: str):
        ms = C.c_double(0)
        n = C.c_int64(0)
        _check(_lib().vh_group_profile_read(self._h, name.encode(), C.byref(ms), C.byref(n)), "vh_group_profile_read")
        return ms.value, n.value


# ------------------------------------------------------------------ one camera's consecutive frames in lock step
class SequenceGroup(StreamGroup):
    """Consecutive frames of ONE camera in the rows of a group (vh_sequence_*): each push brings a chunk of
    n <= max_frames frames, and after matching row r holds the pair frame F+r-1 -> frame F+r (F = position()[0]), row 0
    linking to the last frame of the previous chunk.  Row 0 of a sequence's first chunk and the rows >= n of a short
    chunk are empty.  Every StreamGroup getter and post step reads "stream s" as "row s"; self.S is max_frames."""

    def __init__(self, max_frames: int, param: Params | None = None, device: int = 0,
                 max_features: int = 0, max_matches: int = 0):
        self.param = param if param is not None else Params.default()
        self.S = int(max_frames)
        h = C.c_void_p()
        _check(_lib().vh_sequence_create(C.byref(self.param), device, self.S, max_features, max_matches, C.byref(h)),
               "vh_sequence_create")
        self._h = h

    def pushBack(self, I1, I2=None, dims=None):
        """I1/I2: (n, H, bpl) uint8 numpy arrays, frames F .. F+n-1 of the sequence (I2 None: mono)."""
        I1 = np.ascontiguousarray(I1, dtype=np.uint8)
        assert I1.ndim == 3 and 1 <= I1.shape[0] <= self.S
        if I2 is not None:
            I2 = np.ascontiguousarray(I2, dtype=np.uint8)
            assert I2.shape == I1.shape
        if dims is None:
            dims = [I1.shape[2], I1.shape[1], I1.shape[2]]
        _check(_lib().vh_sequence_push_back(self._h, _ptr(I1), _ptr(I2), I1.shape[1] * I1.shape[2], _dims(dims),
                                            I1.shape[0]), "vh_sequence_push_back")

    def pushBackDevice(self, ptr1: int, ptr2: int | None, stride_bytes: int, dims, n_frames: int):
        """Frame F+r at ptr1 + r * stride_bytes (and ptr2 + ...; None: mono), device memory."""
        _check(_lib().vh_sequence_push_back_device(self._h, C.c_void_p(ptr1), C.c_void_p(ptr2) if ptr2 else None,
                                                   int(stride_bytes), _dims(dims), int(n_frames)),
               "vh_sequence_push_back_device")

    def position(self):
        """-> (index within the sequence of row 0's current frame, rows valid in the last push)."""
        first = C.c_int64(0); n = C.c_int32(0)
        _check(_lib().vh_sequence_position(self._h, C.byref(first), C.byref(n)), "vh_sequence_position")
        return first.value, n.value

    def matchFeaturesPrior(self, method: int, Tr_delta):
        """matchFeatures with a motion prior per row of the last chunk: Tr_delta [n, 4, 4]."""
        n = self.position()[1]
        tr = np.ascontiguousarray(Tr_delta, dtype=np.float64).reshape(-1, 16)
        assert tr.shape[0] == n, (tr.shape, n)
        _check(_lib().vh_group_match_features_prior(self._h, int(method), _ptr(tr)), "vh_group_match_features_prior")

    def setMultiStage(self, mode: int):
        """Two-pass matching of stock libviso2 on every row (vh_sequence_set_multi_stage): 0 off, 1 with the vote and the
        statistics on the host, 2 with both on the device.  Before the first pushBack, with param.multi_stage = 1;
        getSparseMatches(row) then returns the voted sparse list of a row."""
        _check(_lib().vh_sequence_set_multi_stage(self._h, int(mode)), "vh_sequence_set_multi_stage")
        self._ms_mode = int(mode)

    def setMultiStageMatching(self, on: bool = True):
        """setMultiStage(1) / setMultiStage(0) (the group's own entry refuses a sequence handle)."""
        self.setMultiStage(1 if on else 0)

    def setMultiStageDevice(self, on: bool = True):
        """setMultiStage(2), or back to setMultiStage(1): after setMultiStageMatching(True), as on a group."""
        if not getattr(self, "_ms_mode", 0):
            raise VisoHipError(VH_ERR_STATE, "vh_sequence_set_multi_stage")
        self.setMultiStage(2 if on else 1)

    def setLandmarks(self, on: bool = True):
        """Landmarks along the rows of a chunk (vh_sequence_set_landmarks): before the first pushBack, with setTrackLinking.
        landmarks() then fuses the scene points of the last scenePoints along the tracks of the chunk's rows, row 0
        continuing the previous chunk's last row; getLandmarks(row) / getLandmarksAll / landmarksDevice serve rows."""
        _check(_lib().vh_sequence_set_landmarks(self._h, 1 if on else 0), "vh_sequence_set_landmarks")

    def setReconstruction(self, recon: "ReconParams | None", history_frames: int = 0):
        """3-d points from the tracks that end, gathered on the device (vh_sequence_set_reconstruction): before the first
        push only; switches track linking on.  history_frames >= 1: lost tracks older than that come back RECON_HISTORY.
        recon None: off."""
        _check(_lib().vh_sequence_set_reconstruction(self._h, C.byref(recon) if recon is not None else None, int(history_frames)),
               "vh_sequence_set_reconstruction")

    def reconstruct(self, Trs) -> np.ndarray:
        """The lost tracks of the chunk of the last match call (vh_sequence_reconstruct), once per matched chunk, before the
        next match call.  Trs [rows, 4, 4]: the motion frame F+r-1 -> F+r per row of that chunk (rows without a pair are not
        read).  -> RECON_TRACK array sorted by (lost_frame, birth_frame, birth_pos)."""
        tr = np.ascontiguousarray(Trs, dtype=np.float64).reshape(-1, 16)
        nt, na = C.c_int32(0), C.c_int32(0)
        _check(_lib().vh_sequence_reconstruct(self._h, _ptr(tr) if len(tr) else None, C.byref(nt), C.byref(na)), "vh_sequence_reconstruct")
        out = np.zeros(nt.value, RECON_TRACK)
        n = C.c_int32(0)
        _check(_lib().vh_sequence_get_recon_tracks(self._h, _ptr(out) if nt.value else None, nt.value, C.byref(n)), "vh_sequence_get_recon_tracks")
        return out[:n.value]


# ------------------------------------------------------------------ stateless primitives
def compute_features(param: Params, img, dims, device: int = 0, planes: bool = False, cap: int | None = None):
    """Matcher::computeFeatures (reference src/matcher.cpp:585-672) ->
    (max1 [n1,12], max2 [n2,12][, I_du, I_dv])."""
    img = np.ascontiguousarray(img, dtype=np.uint8)
    if cap is None:
        cap = 4 * (dims[0] // (param.nms_n + 1) + 1) * (dims[1] // (param.nms_n + 1) + 1)
    m1 = np.zeros((cap, 12), np.int32)
    m2 = np.zeros((cap, 12), np.int32)
    n1, n2 = C.c_int32(0), C.c_int32(0)
    du = dv = None
    if planes:
        if param.half_resolution:
            w2 = dims[0] // 2
            shape = (dims[1] // 2, w2 + 15 - (w2 - 1) % 16)
        else:
            shape = (dims[1], dims[2])
        du = np.zeros(shape, np.uint8)
        dv = np.zeros(shape, np.uint8)
    _check(_lib().vh_compute_features(C.byref(param), device, _ptr(img), _dims(dims), _ptr(m1), cap, C.byref(n1),
                                      _ptr(m2), cap, C.byref(n2), _ptr(du), _ptr(dv)), "vh_compute_features")
    r = (m1[:n1.value].copy(), m2[:n2.value].copy())
    return r + (du, dv) if planes else r


def filters(img, device: int = 0):
    """sobel5x5 / blob5x5 / checkerboard5x5 (reference src/filter.h:80-96) on
    the valid interior -> (du, dv, f1, f2)."""
    img = np.ascontiguousarray(img, dtype=np.uint8)
    h, bpl = img.shape
    du = np.empty((h, bpl), np.uint8); dv = np.empty((h, bpl), np.uint8)
    f1 = np.empty((h, bpl), np.int16); f2 = np.empty((h, bpl), np.int16)
    _check(_lib().vh_filters(device, _ptr(img), bpl, h, _ptr(du), _ptr(dv), _ptr(f1), _ptr(f2)), "vh_filters")
    return du, dv, f1, f2


def create_index(param: Params, dims, m, device: int = 0):
    """Matcher::createIndexVector (reference src/matcher.cpp:194-214) as CSR."""
    m, n = _feat(m)
    ubn = -(-int(dims[0]) // param.match_binsize)
    vbn = -(-int(dims[1]) // param.match_binsize)
    bs = np.zeros(4 * ubn * vbn + 1, np.int32)
    lst = np.zeros(max(n, 1), np.int32)
    _check(_lib().vh_create_index(C.byref(param), device, _dims(dims), _ptr(m), n, _ptr(bs), _ptr(lst)), "vh_create_index")
    return bs, lst[:n]


def match_all(param: Params, dims, m1, m2, flow: bool = True, device: int = 0):
    """Matcher::findMatch (reference src/matcher.cpp:216-272) for every query."""
    m1, n1 = _feat(m1)
    m2, n2 = _feat(m2)
    best = np.zeros(max(n1, 1), np.int32)
    _check(_lib().vh_match_all(C.byref(param), device, _dims(dims), _ptr(m1), n1, _ptr(m2), n2, 1 if flow else 0,
                               _ptr(best)), "vh_match_all")
    return best[:n1]


def match_all_prior(param: Params, dims, m1, m2, u_: float, v_: float, flow: bool = True, device: int = 0):
    """Matcher::findMatch with the u_,v_ prediction term (reference src/matcher.cpp:257-262)."""
    m1, n1 = _feat(m1)
    m2, n2 = _feat(m2)
    best = np.zeros(max(n1, 1), np.int32)
    _check(_lib().vh_match_all_prior(C.byref(param), device, _dims(dims), _ptr(m1), n1, _ptr(m2), n2,
                                     1 if flow else 0, float(u_), float(v_), _ptr(best)), "vh_match_all_prior")
    return best[:n1]


def estimate_motion_stereo(ego: EgoParams, match_lists, rand3, device: int = 0):
    """VisualOdometryStereo::estimateMotion (reference src/viso_stereo.cpp:54-157), batched over
    `match_lists` (a list of p_match arrays); rand3 [n_sets, ransac_iters, 3] int32 rand() values.
    -> (tr [n,6], ok [n] bool, [inlier index arrays])."""
    lists = [np.ascontiguousarray(m, dtype=P_MATCH_DTYPE) for m in match_lists]
    n = len(lists)
    offsets = np.zeros(n + 1, np.int32)
    offsets[1:] = np.cumsum([len(m) for m in lists])
    pm = np.concatenate(lists) if offsets[-1] else np.zeros(0, P_MATCH_DTYPE)
    rand3 = np.ascontiguousarray(rand3, np.int32)
    assert rand3.shape == (n, ego.ransac_iters, 3)
    tr = np.zeros((n, 6), np.float64); ok = np.zeros(n, np.int32); ninl = np.zeros(n, np.int32)
    inl = np.zeros(max(int(offsets[-1]), 1), np.int32)
    _check(_lib().vh_estimate_motion_stereo(C.byref(ego), device, n, _ptr(pm), _ptr(offsets), _ptr(rand3), _ptr(tr), _ptr(ok),
                                            _ptr(ninl), _ptr(inl)), "vh_estimate_motion_stereo")
    return tr, ok.astype(bool), [inl[offsets[s]:offsets[s] + ninl[s]].copy() for s in range(n)]


def motion_inliers(ego: EgoParams, match_lists, tr, ok, device: int = 0):
    """VisualOdometryStereo::getInlier (reference src/viso_stereo.cpp:159-177) on whole quad lists under given motions:
    `match_lists` (a list of p_match arrays), tr [n, 6], ok [n] (vh_motion_inliers).
    -> ([flags uint8 per list], n_inliers [n], [inlier records per list], [their positions per list])."""
    lists = [np.ascontiguousarray(m, dtype=P_MATCH_DTYPE) for m in match_lists]
    n = len(lists)
    offsets = np.zeros(n + 1, np.int32)
    offsets[1:] = np.cumsum([len(m) for m in lists])
    total = int(offsets[-1])
    pm = np.concatenate(lists) if total else np.zeros(0, P_MATCH_DTYPE)
    tr = np.ascontiguousarray(tr, np.float64).reshape(n, 6); ok = np.ascontiguousarray(ok).astype(np.int32).reshape(n)
    flags = np.zeros(max(total, 1), np.uint8); ninl = np.zeros(max(n, 1), np.int32)
    out = np.zeros(max(total, 1), P_MATCH_DTYPE); pos = np.zeros(max(total, 1), np.int32)
    _check(_lib().vh_motion_inliers(C.byref(ego), device, n, _ptr(pm), _ptr(offsets), _ptr(tr), _ptr(ok), _ptr(flags), _ptr(ninl),
                                    _ptr(out), _ptr(pos)), "vh_motion_inliers")
    sl = [slice(int(offsets[s]), int(offsets[s]) + int(ninl[s])) for s in range(n)]
    return ([flags[offsets[s]:offsets[s + 1]].copy() for s in range(n)], ninl[:n],
            [out[q].copy() for q in sl], [pos[q].copy() for q in sl])


def gain(match_lists, index_lists, I_prev, I_cur, dims, device: int = 0):
    """Matcher::getGain (reference src/matcher.h:148) for n lists in one call (vh_gain): `match_lists` (p_match arrays),
    `index_lists` (int32 positions into each), I_prev / I_cur: uint8 [n, H, bpl] (or [H, bpl] for one list), the previous
    and current left images at full resolution, dims = (W, H, bpl) -> (gain float32 [n], num int32 [n])."""
    lists = [np.ascontiguousarray(m, dtype=P_MATCH_DTYPE) for m in match_lists]
    idxs = [np.ascontiguousarray(q, np.int32).reshape(-1) for q in index_lists]
    n = len(lists)
    assert len(idxs) == n
    W, H, bpl = (int(d) for d in dims)
    Ip = np.ascontiguousarray(I_prev, np.uint8).reshape(n, H, bpl); Ic = np.ascontiguousarray(I_cur, np.uint8).reshape(n, H, bpl)
    offsets = np.zeros(n + 1, np.int32); ioff = np.zeros(n + 1, np.int32)
    offsets[1:] = np.cumsum([len(m) for m in lists]); ioff[1:] = np.cumsum([len(q) for q in idxs])
    pm = np.concatenate(lists) if offsets[-1] else np.zeros(1, P_MATCH_DTYPE)
    idx = np.concatenate(idxs) if ioff[-1] else np.zeros(1, np.int32)
    out = np.zeros(max(n, 1), np.float32); num = np.zeros(max(n, 1), np.int32)
    _check(_lib().vh_gain(device, n, _dims(dims), _ptr(Ip), _ptr(Ic), H * bpl, _ptr(pm), _ptr(offsets), _ptr(idx), _ptr(ioff), _ptr(out),
                          _ptr(num)), "vh_gain")
    return out[:n], num[:n]


def refit_motion(ego: EgoParams, match_lists, tr, ok, device: int = 0):
    """The reference's final optimisation (src/viso_stereo.cpp:126-139: updateParameters with eps 1e-8 until it converges, at
    most 102 times) on whole quad lists, every record active, from the starts tr [n, 6] / ok [n] (vh_refit_motion).
    -> (tr [n, 6], ok [n] bool, n_updates [n])."""
    lists = [np.ascontiguousarray(m, dtype=P_MATCH_DTYPE) for m in match_lists]
    n = len(lists)
    offsets = np.zeros(n + 1, np.int32)
    offsets[1:] = np.cumsum([len(m) for m in lists])
    pm = np.concatenate(lists) if int(offsets[-1]) else np.zeros(0, P_MATCH_DTYPE)
    tr = np.ascontiguousarray(tr, np.float64).reshape(n, 6); ok = np.ascontiguousarray(ok).astype(np.int32).reshape(n)
    tr_out = np.zeros((max(n, 1), 6), np.float64); ok_out = np.zeros(max(n, 1), np.int32); nupd = np.zeros(max(n, 1), np.int32)
    _check(_lib().vh_refit_motion(C.byref(ego), device, n, _ptr(pm), _ptr(offsets), _ptr(tr), _ptr(ok), _ptr(tr_out), _ptr(ok_out),
                                  _ptr(nupd)), "vh_refit_motion")
    return tr_out[:n], ok_out[:n].astype(bool), nupd[:n]


def motion_covariance(ego: EgoParams, match_lists, tr, ok, device: int = 0):
    """The 6x6 covariance sigma^2 (J^T J)^-1 of stereo motions over whole quad lists, every record active, at the motions
    tr [n, 6] / ok [n] (vh_motion_covariance): J and the residuals as the reference's computeResidualsAndJacobian forms
    them at tr, sigma^2 = ssr / (4 N - 6).  -> (cov [n, 6, 6], ssr [n], ok [n] bool)."""
    lists = [np.ascontiguousarray(m, dtype=P_MATCH_DTYPE) for m in match_lists]
    n = len(lists)
    offsets = np.zeros(n + 1, np.int32)
    offsets[1:] = np.cumsum([len(m) for m in lists])
    pm = np.concatenate(lists) if int(offsets[-1]) else np.zeros(0, P_MATCH_DTYPE)
    tr = np.ascontiguousarray(tr, np.float64).reshape(n, 6); ok = np.ascontiguousarray(ok).astype(np.int32).reshape(n)
    cov = np.zeros((max(n, 1), 6, 6), np.float64); ssr = np.zeros(max(n, 1), np.float64); ok_out = np.zeros(max(n, 1), np.int32)
    _check(_lib().vh_motion_covariance(C.byref(ego), device, n, _ptr(pm), _ptr(offsets), _ptr(tr), _ptr(ok), _ptr(cov), _ptr(ssr),
                                       _ptr(ok_out)), "vh_motion_covariance")
    return cov[:n], ssr[:n], ok_out[:n].astype(bool)


def _scene_points(fn, e, match_lists, motion, ok, sp, Tw, device):
    lists = [np.ascontiguousarray(m, dtype=P_MATCH_DTYPE) for m in match_lists]
    n = len(lists)
    offsets = np.zeros(n + 1, np.int32)
    offsets[1:] = np.cumsum([len(m) for m in lists])
    total = int(offsets[-1])
    pm = np.concatenate(lists) if total else np.zeros(0, P_MATCH_DTYPE)
    ok = np.ascontiguousarray(ok).astype(np.int32).reshape(n)
    sp = sp or SceneParams.default()
    tw = _scene_Tw(Tw, n)
    out = np.zeros(max(total, 1), SCENE_POINT_DTYPE); counts = np.zeros(max(n, 1), np.int32)
    _check(getattr(_lib(), fn)(C.byref(e), C.byref(sp), device, n, _ptr(pm), _ptr(offsets), _ptr(motion), _ptr(ok),
                               None if tw is None else _ptr(tw), _ptr(out), _ptr(counts)), fn)
    return [out[int(offsets[s]):int(offsets[s]) + int(counts[s])].copy() for s in range(n)], counts[:n]


def scene_points_stereo(ego: EgoParams, match_lists, tr, ok, sp: "SceneParams | None" = None, Tw=None, device: int = 0):
    """The 3-d point of every record of whole quad lists under the motions tr [n, 6] / ok [n] (vh_scene_points_stereo): the
    previous pair's point as getInlier forms it, moved by tr for sp.frame = 1, with its reprojection error and sigma_z;
    records behind the camera, non-finite ones and those the filters of `sp` cut are dropped, survivors keep list order.
    Tw: None, one 4x4 or [n, 4, 4], applied last.  -> ([SCENE_POINT_DTYPE array per list], counts [n])."""
    tr = np.ascontiguousarray(tr, np.float64).reshape(len(match_lists), 6)
    return _scene_points("vh_scene_points_stereo", ego, match_lists, tr, ok, sp, Tw, device)


def scene_points_mono(mono: MonoParams, match_lists, pose, ok, sp: "SceneParams | None" = None, Tw=None, device: int = 0):
    """The triangulated point of every record of whole flow / quad lists under the poses `pose` (MONO_POSE_DTYPE [n], as
    pose_mono returns them: R, t and scale are read) / ok [n] (vh_scene_points_mono), scaled to metres.
    -> ([SCENE_POINT_DTYPE array per list], counts [n])."""
    pose = np.ascontiguousarray(pose, MONO_POSE_DTYPE).reshape(len(match_lists))
    return _scene_points("vh_scene_points_mono", mono, match_lists, pose, ok, sp, Tw, device)


def _packed(arrays, dtype):
    """a list of arrays -> (their concatenation, offsets [n + 1])"""
    arrays = [np.ascontiguousarray(a, dtype=dtype).reshape(-1) for a in arrays]
    offsets = np.zeros(len(arrays) + 1, np.int32)
    offsets[1:] = np.cumsum([len(a) for a in arrays])
    return (np.concatenate(arrays) if offsets[-1] else np.zeros(0, dtype)), offsets


def landmarks_update(tracks, points, prev_state=None, params: "LandmarkParams | None" = None, device: int = 0):
    """One step of the landmarks for n independent lists (vh_landmarks_update): `tracks` (TRACK arrays, one per list), `points`
    (SCENE_POINT_DTYPE arrays whose src_pos number the records of the same list, strictly increasing, all in one common
    frame), prev_state (None, or LANDMARK_STATE_DTYPE arrays, one per predecessor list -- what the step before returned).
    -> ([LANDMARK_DTYPE array per list], [LANDMARK_STATE_DTYPE array per list])."""
    n = len(tracks)
    assert len(points) == n and (prev_state is None or len(prev_state) == n)
    lp = params or LandmarkParams.default()
    trk, roff = _packed(tracks, TRACK)
    pts, poff = _packed(points, SCENE_POINT_DTYPE)
    prev, voff = _packed(prev_state, LANDMARK_STATE_DTYPE) if prev_state is not None else (None, None)
    total = int(roff[-1])
    state = np.zeros(max(total, 1), LANDMARK_STATE_DTYPE); out = np.zeros(max(total, 1), LANDMARK_DTYPE)
    counts = np.zeros(max(n, 1), np.int32)
    _check(_lib().vh_landmarks_update(C.byref(lp), device, n, _ptr(trk), _ptr(roff), _ptr(pts), _ptr(poff),
                                      None if prev is None else _ptr(prev), None if voff is None else _ptr(voff),
                                      _ptr(state), _ptr(out), _ptr(counts)), "vh_landmarks_update")
    return ([out[int(roff[s]):int(roff[s]) + int(counts[s])].copy() for s in range(n)],
            [state[int(roff[s]):int(roff[s + 1])].copy() for s in range(n)])


def landmarks_chain(tracks, points, carry=None, params: "LandmarkParams | None" = None, device: int = 0):
    """The landmarks of n lists that are the rows of one chain (vh_landmarks_chain): list s's prev indexes list s - 1 of the
    same call (what link_tracks returns), list 0's indexes `carry` (None, or a LANDMARK_STATE_DTYPE array: the last list's
    states of the call before).  tracks / points as landmarks_update's.
    -> ([LANDMARK_DTYPE array per list], [LANDMARK_STATE_DTYPE array per list])."""
    n = len(tracks)
    assert len(points) == n
    lp = params or LandmarkParams.default()
    trk, roff = _packed(tracks, TRACK)
    pts, poff = _packed(points, SCENE_POINT_DTYPE)
    cs = None if carry is None else np.ascontiguousarray(carry, LANDMARK_STATE_DTYPE).reshape(-1)
    total = int(roff[-1])
    state = np.zeros(max(total, 1), LANDMARK_STATE_DTYPE); out = np.zeros(max(total, 1), LANDMARK_DTYPE)
    counts = np.zeros(max(n, 1), np.int32)
    _check(_lib().vh_landmarks_chain(C.byref(lp), device, n, _ptr(trk), _ptr(roff), _ptr(pts), _ptr(poff),
                                     None if cs is None or not len(cs) else _ptr(cs), 0 if cs is None else len(cs),
                                     _ptr(state), _ptr(out), _ptr(counts)), "vh_landmarks_chain")
    return ([out[int(roff[s]):int(roff[s]) + int(counts[s])].copy() for s in range(n)],
            [state[int(roff[s]):int(roff[s + 1])].copy() for s in range(n)])


def trajectory(tr_chains, ok_chains, T0=None, carry=None, params: "TrajParams | None" = None, device: int = 0):
    """Poses accumulated along n chains of rows (vh_trajectory): tr_chains a list of [rows, 6] arrays, ok_chains of [rows]
    int arrays (0: not ok, < 0: the row holds no pair).  T0: None, one 4x4 or [n, 4, 4]; carry: None or a TRAJ_CARRY_DTYPE
    array [n] (what an earlier call returned: T0 is then not read).
    -> ([TRAJ_POSE_DTYPE array per chain], TRAJ_CARRY_DTYPE [n])."""
    n = len(tr_chains)
    assert len(ok_chains) == n
    tp = params or TrajParams.default()
    off = np.zeros(n + 1, np.int32)
    off[1:] = np.cumsum([len(t) for t in tr_chains])
    total = int(off[-1])
    tr = np.zeros((max(total, 1), 6), np.float64); ok = np.zeros(max(total, 1), np.int32)
    for c in range(n):
        tr[off[c]:off[c + 1]] = np.asarray(tr_chains[c], np.float64).reshape(-1, 6)
        ok[off[c]:off[c + 1]] = np.asarray(ok_chains[c]).astype(np.int32)
    t0 = _traj_T0(T0, n)
    cin = None if carry is None else np.ascontiguousarray(carry, TRAJ_CARRY_DTYPE).reshape(-1)
    assert cin is None or len(cin) == n
    out = np.zeros(max(total, 1), TRAJ_POSE_DTYPE); cout = np.zeros(max(n, 1), TRAJ_CARRY_DTYPE)
    _check(_lib().vh_trajectory(C.byref(tp), device, n, _ptr(off), _ptr(tr), _ptr(ok), _ptr(t0), _ptr(cin), _ptr(out), _ptr(cout)),
           "vh_trajectory")
    return [out[int(off[c]):int(off[c + 1])].copy() for c in range(n)], cout[:n]


def trajectory_cov(tr_chains, ok_chains, cov_chains, ok_cov_chains, Sigma0=None, carry=None, params: "TrajParams | None" = None,
                   cov_params: "TrajCovParams | None" = None, device: int = 0):
    """The pose's covariance propagated along n chains of rows (vh_trajectory_cov): tr_chains / ok_chains as trajectory()'s,
    cov_chains a list of [rows, 6, 6] motion covariances, ok_cov_chains of [rows] int arrays.  Sigma0: None, one 6x6 or
    [n, 6, 6]; carry: None or a TRAJ_COV_CARRY_DTYPE array [n] (Sigma0 is then not read).
    -> ([TRAJ_COV_DTYPE array per chain], TRAJ_COV_CARRY_DTYPE [n])."""
    n = len(tr_chains)
    assert len(ok_chains) == n and len(cov_chains) == n and len(ok_cov_chains) == n
    tp = params or TrajParams.default()
    tcp = cov_params or TrajCovParams.default()
    off = np.zeros(n + 1, np.int32)
    off[1:] = np.cumsum([len(t) for t in tr_chains])
    total = int(off[-1])
    tr = np.zeros((max(total, 1), 6), np.float64); ok = np.zeros(max(total, 1), np.int32)
    cov = np.zeros((max(total, 1), 36), np.float64); okc = np.zeros(max(total, 1), np.int32)
    for c in range(n):
        tr[off[c]:off[c + 1]] = np.asarray(tr_chains[c], np.float64).reshape(-1, 6)
        ok[off[c]:off[c + 1]] = np.asarray(ok_chains[c]).astype(np.int32)
        cov[off[c]:off[c + 1]] = np.asarray(cov_chains[c], np.float64).reshape(-1, 36)
        okc[off[c]:off[c + 1]] = np.asarray(ok_cov_chains[c]).astype(np.int32)
    s0 = _traj_S0(Sigma0, n)
    cin = None if carry is None else np.ascontiguousarray(carry, TRAJ_COV_CARRY_DTYPE).reshape(-1)
    assert cin is None or len(cin) == n
    out = np.zeros(max(total, 1), TRAJ_COV_DTYPE); cout = np.zeros(max(n, 1), TRAJ_COV_CARRY_DTYPE)
    _check(_lib().vh_trajectory_cov(C.byref(tp), C.byref(tcp), device, n, _ptr(off), _ptr(tr), _ptr(ok), _ptr(cov), _ptr(okc), _ptr(s0),
                                    _ptr(cin), _ptr(out), _ptr(cout)), "vh_trajectory_cov")
    return [out[int(off[c]):int(off[c + 1])].copy() for c in range(n)], cout[:n]


def estimate_motion_mono(mono: MonoParams, match_lists, rand8, device: int = 0, model: bool = False):
    """VisualOdometryMono::estimateMotion (reference src/viso_mono.cpp:41-160), batched over `match_lists`;
    rand8 [n_sets, ransac_iters, 8] int32 rand() values.  -> (tr [n,6], ok [n] bool, [inlier index arrays]);
    model=True: and the models [n] (MONO_MODEL_DTYPE, vh_estimate_motion_mono_model) as a fourth value."""
    lists = [np.ascontiguousarray(m, dtype=P_MATCH_DTYPE) for m in match_lists]
    n = len(lists)
    offsets = np.zeros(n + 1, np.int32)
    offsets[1:] = np.cumsum([len(m) for m in lists])
    pm = np.concatenate(lists) if offsets[-1] else np.zeros(0, P_MATCH_DTYPE)
    rand8 = np.ascontiguousarray(rand8, np.int32)
    assert rand8.shape == (n, mono.ransac_iters, 8)
    tr = np.zeros((n, 6), np.float64); ok = np.zeros(n, np.int32); ninl = np.zeros(n, np.int32)
    inl = np.zeros(max(int(offsets[-1]), 1), np.int32)
    if model:
        mo = np.zeros(max(n, 1), MONO_MODEL_DTYPE)
        _check(_lib().vh_estimate_motion_mono_model(C.byref(mono), device, n, _ptr(pm), _ptr(offsets), _ptr(rand8), _ptr(tr), _ptr(ok),
                                                    _ptr(ninl), _ptr(inl), _ptr(mo)), "vh_estimate_motion_mono_model")
    else:
        _check(_lib().vh_estimate_motion_mono(C.byref(mono), device, n, _ptr(pm), _ptr(offsets), _ptr(rand8), _ptr(tr), _ptr(ok),
                                              _ptr(ninl), _ptr(inl)), "vh_estimate_motion_mono")
    res = (tr, ok.astype(bool), [inl[offsets[s]:offsets[s] + ninl[s]].copy() for s in range(n)])
    return res + (mo[:n],) if model else res


def motion_inliers_mono(mono: MonoParams, match_lists, model, ok, device: int = 0):
    """VisualOdometryMono::getInlier (reference src/viso_mono.cpp:268-315) on whole flow or quad lists under given models:
    `match_lists` (a list of p_match arrays), model [n] (MONO_MODEL_DTYPE), ok [n] (vh_motion_inliers_mono).
    -> ([flags uint8 per list], n_inliers [n], [inlier records per list], [their positions per list])."""
    lists = [np.ascontiguousarray(m, dtype=P_MATCH_DTYPE) for m in match_lists]
    n = len(lists)
    offsets = np.zeros(n + 1, np.int32)
    offsets[1:] = np.cumsum([len(m) for m in lists])
    total = int(offsets[-1])
    pm = np.concatenate(lists) if total else np.zeros(0, P_MATCH_DTYPE)
    model = _models(model, n) if n else np.zeros(1, MONO_MODEL_DTYPE)
    ok = np.ascontiguousarray(ok).astype(np.int32).reshape(n)
    flags = np.zeros(max(total, 1), np.uint8); ninl = np.zeros(max(n, 1), np.int32)
    out = np.zeros(max(total, 1), P_MATCH_DTYPE); pos = np.zeros(max(total, 1), np.int32)
    _check(_lib().vh_motion_inliers_mono(C.byref(mono), device, n, _ptr(pm), _ptr(offsets), _ptr(model), _ptr(ok), _ptr(flags), _ptr(ninl),
                                         _ptr(out), _ptr(pos)), "vh_motion_inliers_mono")
    sl = [slice(int(offsets[s]), int(offsets[s]) + int(ninl[s])) for s in range(n)]
    return ([flags[offsets[s]:offsets[s + 1]].copy() for s in range(n)], ninl[:n],
            [out[q].copy() for q in sl], [pos[q].copy() for q in sl])


def refit_model_mono(mono: MonoParams, match_lists, model, ok, device: int = 0):
    """fundamentalMatrix (reference src/viso_mono.cpp:235-266) over whole flow or quad lists, every record active, in the
    normalised frame of model [n] (MONO_MODEL_DTYPE) / ok [n] (vh_refit_model_mono): c, s copied, F refitted on all records.
    -> (model [n], ok [n] bool, w [n, 2]: the two smallest singular values w[8], w[7] of the 9x9 moment matrix)."""
    lists = [np.ascontiguousarray(m, dtype=P_MATCH_DTYPE) for m in match_lists]
    n = len(lists)
    offsets = np.zeros(n + 1, np.int32)
    offsets[1:] = np.cumsum([len(m) for m in lists])
    pm = np.concatenate(lists) if int(offsets[-1]) else np.zeros(0, P_MATCH_DTYPE)
    model = _models(model, n) if n else np.zeros(1, MONO_MODEL_DTYPE)
    ok = np.ascontiguousarray(ok).astype(np.int32).reshape(n)
    model_out = np.zeros(max(n, 1), MONO_MODEL_DTYPE); ok_out = np.zeros(max(n, 1), np.int32); w = np.zeros((max(n, 1), 2), np.float64)
    _check(_lib().vh_refit_model_mono(C.byref(mono), device, n, _ptr(pm), _ptr(offsets), _ptr(model), _ptr(ok), _ptr(model_out), _ptr(ok_out),
                                      _ptr(w)), "vh_refit_model_mono")
    return model_out[:n], ok_out[:n].astype(bool), w[:n]


def pose_mono(mono: MonoParams, match_lists, model, ok, device: int = 0, refine: bool = False):
    """The rest of VisualOdometryMono::estimateMotion after the refit (reference src/viso_mono.cpp:83-158) over whole flow or
    quad lists under model [n] (MONO_MODEL_DTYPE) / ok [n] (vh_pose_mono): E, the four (R, t) candidates, the chirality count
    of every record, the ground-plane vote over the points in front.  -> (tr [n, 6], ok [n] bool, pose [n] MONO_POSE_DTYPE).
    refine=True: the winning R|t of every list is refined by Gauss-Newton on the Sampson distance of every record before
    the scale tail (vh_pose_mono_refined); the MONO_REFINE_DTYPE records [n] (the 5 x 5 covariance of the refined pose among
    them) are a fourth value."""
    lists = [np.ascontiguousarray(m, dtype=P_MATCH_DTYPE) for m in match_lists]
    n = len(lists)
    offsets = np.zeros(n + 1, np.int32)
    offsets[1:] = np.cumsum([len(m) for m in lists])
    pm = np.concatenate(lists) if int(offsets[-1]) else np.zeros(0, P_MATCH_DTYPE)
    model = _models(model, n) if n else np.zeros(1, MONO_MODEL_DTYPE)
    ok = np.ascontiguousarray(ok).astype(np.int32).reshape(n)
    tr = np.zeros((max(n, 1), 6), np.float64); ok_out = np.zeros(max(n, 1), np.int32); pose = np.zeros(max(n, 1), MONO_POSE_DTYPE)
    if refine:
        ref = np.zeros(max(n, 1), MONO_REFINE_DTYPE)
        _check(_lib().vh_pose_mono_refined(C.byref(mono), device, n, _ptr(pm), _ptr(offsets), _ptr(model), _ptr(ok), _ptr(tr), _ptr(ok_out),
                                           _ptr(pose), _ptr(ref)), "vh_pose_mono_refined")
        return tr[:n], ok_out[:n].astype(bool), pose[:n], ref[:n]
    _check(_lib().vh_pose_mono(C.byref(mono), device, n, _ptr(pm), _ptr(offsets), _ptr(model), _ptr(ok), _ptr(tr), _ptr(ok_out), _ptr(pose)),
           "vh_pose_mono")
    return tr[:n], ok_out[:n].astype(bool), pose[:n]


def remove_outliers(pm, rule=None) -> np.ndarray:
    """removeOutliers (reference src/remove_outliers.cpp:4-94) on p_match records; host only.  rule: None (the reference's
    vote) or a VoteRule (VoteRule.stock(method, flow_tolerance, disp_tolerance): stock libviso2's per-method rule)."""
    pm = np.ascontiguousarray(pm, dtype=P_MATCH_DTYPE).copy()
    n = C.c_int32(0)
    if rule is None:
        _check(_lib().vh_remove_outliers_pm(_ptr(pm), len(pm), C.byref(n)), "vh_remove_outliers_pm")
    else:
        _check(_lib().vh_remove_outliers_pm_rule(_ptr(pm), len(pm), _rule(rule), C.byref(n)), "vh_remove_outliers_pm_rule")
    return pm[:n.value].copy()


def remove_outliers_device(lists, lanes_per_wave: int = 1, max_features: int = 0, bucket_width: float = 50.0, bucket_height: float = 50.0,
                           device: int = 0, out_cap: int = 0, strict: bool = True, with_counts: bool = False, rule=None):
    """removeOutliers (and bucketFeatures when max_features >= 1) of several match lists at once on the GPU
    (vh_remove_outliers_device) -> (lists, triangles per list, sweep kernel ms).  rule: as remove_outliers.  strict=False: an error code does not
    raise; the healthy lists are returned (a refused list comes back empty) with the code as a fourth element.
    with_counts: out_counts as the call left them (the length a list that did not fit out_cap needs) as a last element."""
    lists = [np.ascontiguousarray(m, dtype=P_MATCH_DTYPE) for m in lists]
    n = len(lists)
    stride = max([len(m) for m in lists] + [1])
    pm = np.zeros((n, stride), P_MATCH_DTYPE)
    for l, m in enumerate(lists):
        pm[l, :len(m)] = m
    counts = np.array([len(m) for m in lists], np.int32)
    out_cap = int(out_cap) if out_cap else stride
    out = np.zeros((n, out_cap), P_MATCH_DTYPE)
    oc = np.zeros(n, np.int32); ntri = np.zeros(n, np.int32); ms = C.c_float(0.0)
    args = (device, n, _ptr(pm), stride, _ptr(counts), int(lanes_per_wave), int(max_features), C.c_float(bucket_width), C.c_float(bucket_height),
            _ptr(out), out_cap, _ptr(oc), _ptr(ntri), C.byref(ms))
    rc = _lib().vh_remove_outliers_device(*args) if rule is None else _lib().vh_remove_outliers_device_rule(*args, _rule(rule))
    tail = (oc.copy(),) if with_counts else ()
    if strict:
        _check(rc, "vh_remove_outliers_device")
        return ([out[l, :oc[l]].copy() for l in range(n)], ntri, ms.value) + tail
    return ([out[l, :oc[l]].copy() if oc[l] <= out_cap else out[l, :0].copy() for l in range(n)], ntri, ms.value, rc) + tail


class TrackCarry:
    """The opaque carry of link_tracks(): the last list of a call and its tracks, for the next call to continue."""

    def __init__(self, handle):
        import weakref
        self._h = handle
        weakref.finalize(self, _lib().vh_track_carry_free, C.c_void_p(handle.value))


def link_tracks(lists, n_index: int, carry: "TrackCarry | None" = None, device: int = 0):
    """Feature tracks over caller-owned match lists (vh_link_tracks): list l continues list l - 1, list 0 the last
    list of the call that returned `carry`.  -> ([TRACK array per list], carry for the next call)."""
    lists = [np.ascontiguousarray(m, dtype=P_MATCH_DTYPE) for m in lists]
    n = len(lists)
    stride = max([len(m) for m in lists] + [1])
    pm = np.zeros((n, stride), P_MATCH_DTYPE)
    for l, m in enumerate(lists):
        pm[l, :len(m)] = m
    counts = np.array([len(m) for m in lists], np.int32)
    out = np.zeros((n, stride), TRACK)
    h = C.c_void_p()
    _check(_lib().vh_link_tracks(device, n, _ptr(pm), stride, _ptr(counts), int(n_index), carry._h if carry is not None else None,
                                 C.byref(h), _ptr(out)), "vh_link_tracks")
    return [out[l, :counts[l]].copy() for l in range(n)], TrackCarry(h)


def reconstruct_tracks(recon: ReconParams, Trs, first_frame, offsets, pixels, n_frames: int | None = None, metrics: bool = True,
                       device: int = 0):
    """What Reconstruction::update computes for its lost tracks (reference src/reconstruction.cpp:131-142), for all given
    tracks in one launch (vh_reconstruct_tracks).  Trs [n_frames - 1, 4, 4]: the Tr of update k (frame k -> k + 1); track t
    was seen in frames first_frame[t] .. at pixels[offsets[t]:offsets[t + 1]] = (u, v).
    -> (points [n, 3] float32, status [n] int32 (RECON_*), metrics [n, 2] float64 (distance, angle) or None)."""
    tr = np.ascontiguousarray(Trs, dtype=np.float64).reshape(-1, 16)
    first = np.ascontiguousarray(first_frame, dtype=np.int32).reshape(-1)
    off = np.ascontiguousarray(offsets, dtype=np.int32).reshape(-1)
    px = np.ascontiguousarray(pixels, dtype=np.float32).reshape(-1, 2)
    n = len(first)
    if len(off) != n + 1 or (n > 0 and len(px) < off[-1]):
        raise ValueError(f"reconstruct_tracks: {n} tracks need {n + 1} offsets and offsets[-1] pixels (got {len(off)}, {len(px)})")
    nf = tr.shape[0] + 1 if n_frames is None else int(n_frames)
    if tr.shape[0] < nf - 1:
        raise ValueError(f"reconstruct_tracks: {nf} frames need {nf - 1} Trs (got {tr.shape[0]})")
    pts = np.zeros((n, 3), np.float32); st = np.zeros(n, np.int32)
    met = np.zeros((n, 2), np.float64) if metrics else None
    _check(_lib().vh_reconstruct_tracks(C.byref(recon), int(device), nf, _ptr(tr), n, _ptr(first), _ptr(off), _ptr(px), _ptr(pts),
                                        _ptr(st), _ptr(met)), "vh_reconstruct_tracks")
    return pts, st, met


def reconstruct_lists(recon: ReconParams, lists, Trs, n_index: int, device: int = 0) -> np.ndarray:
    """A whole fresh drive from caller-owned match lists (vh_reconstruct_lists): list l is update l of a new
    Reconstruction, Trs[l] its Tr; linked by the rule of link_tracks, every lost track gathered and solved on the device.
    -> RECON_TRACK array sorted by (lost_frame, birth_frame, birth_pos)."""
    lists = [np.ascontiguousarray(m, dtype=P_MATCH_DTYPE) for m in lists]
    n = len(lists)
    tr = np.ascontiguousarray(Trs, dtype=np.float64).reshape(-1, 16)
    if tr.shape[0] != n:
        raise ValueError(f"reconstruct_lists: {n} lists need as many Trs (got {tr.shape[0]})")
    stride = max([len(m) for m in lists] + [1])
    pm = np.zeros((n, stride), P_MATCH_DTYPE)
    for l, m in enumerate(lists):
        pm[l, :len(m)] = m
    counts = np.array([len(m) for m in lists], np.int32)
    cap = int(counts.sum())   # every record ends at most one track
    out = np.zeros(max(cap, 1), RECON_TRACK)
    got = C.c_int32(0)
    _check(_lib().vh_reconstruct_lists(C.byref(recon), int(device), n, _ptr(pm), stride, _ptr(counts), int(n_index), _ptr(tr), _ptr(out), cap,
                                       C.byref(got)), "vh_reconstruct_lists")
    return out[:got.value].copy()


def debug_group_reconstruct_lists(recon: ReconParams, streams, Trs, n_index: int, device: int = 0) -> list:
    """Test hook (vh_group_debug_reconstruct_lists): the group form of the gather kernels on caller-owned lists.  streams:
    S sequences of n lists each, Trs [S, n, 4, 4]; every stream a fresh drive, all through one kernel sequence.
    -> S RECON_TRACK arrays."""
    S, n = len(streams), len(streams[0])
    tr = np.ascontiguousarray(Trs, dtype=np.float64).reshape(-1, 16)
    assert all(len(ls) == n for ls in streams) and tr.shape[0] == S * n, (S, n, tr.shape)
    stride = max(1, max(len(m) for ls in streams for m in ls))
    pm = np.zeros((S * n, stride), P_MATCH_DTYPE)
    for k, m in enumerate(m for ls in streams for m in ls):
        pm[k, :len(m)] = m
    counts = np.array([len(m) for ls in streams for m in ls], np.int32)
    cap = int(counts.sum())
    out = np.zeros(max(cap, 1), RECON_TRACK)
    got = np.zeros(S, np.int32)
    _check(_lib().vh_group_debug_reconstruct_lists(C.byref(recon), int(device), S, n, _ptr(pm), stride, _ptr(counts), int(n_index), _ptr(tr),
                                                   _ptr(out), cap, _ptr(got)), "vh_group_debug_reconstruct_lists")
    ends = np.cumsum(got)
    return [out[e - c:e].copy() for e, c in zip(ends, got)]


def reconstruct_last_kernel_ms() -> float:
    """Device time of the kernel of this thread's last reconstruct_tracks call (HIP events), -1 before the first."""
    return float(_lib().vh_reconstruct_last_kernel_ms())


class Reconstruction:
    """Host mirror of the reference's `Reconstruction` (src/reconstruction.h:35-110): setCalibration, update, getPoints.
    The association of matches to tracks is update's, statement for statement (src/reconstruction.cpp:72-145), on the
    host; every lost track's point is computed on the GPU (reconstruct_tracks).  updateMany runs several consecutive
    updates with ONE launch: points never feed back into the association, so the result is that of the single updates.
    The entry is stateless: every call rebuilds the tables of all frames so far on the host (a third of a microsecond per
    frame), so update() once per frame costs O(N^2) of that over a drive of N frames; prefer updateMany per chunk."""

    def __init__(self, device: int = 0):
        self.device = int(device)
        self.recon = ReconParams.default()
        self.Trs = []      # Tr of every update so far: frame k -> k + 1
        self.tracks = []   # active tracks: [pixels (list of (u, v)), first_frame, last_frame, last_idx]
        self.points = []   # accepted points, float32 [3] each

    def setCalibration(self, f: float, cu: float, cv: float):
        self.recon.f, self.recon.cu, self.recon.cv = float(f), float(cu), float(cv)

    def associate(self, p_matched, current_frame: int):
        """src/reconstruction.cpp:75-145 without the points: extends / starts tracks from one match list and returns the
        lost tracks, in track order, as (first_frame, pixels).  The reference indexes its table with i1p and last_idx
        unchecked; here a match with i1p < 0 starts a new track and a track with last_idx < 0 is not entered."""
        pm = np.ascontiguousarray(p_matched, dtype=P_MATCH_DTYPE)
        tracks = self.tracks
        track_idx_max = 0
        if len(pm):
            track_idx_max = max(track_idx_max, int(pm["i1p"].max()))
        for t in tracks:
            if t[3] > track_idx_max:
                track_idx_max = t[3]
        track_idx = [-1] * (track_idx_max + 1)
        for i, t in enumerate(tracks):
            if t[3] >= 0:
                track_idx[t[3]] = i          # in track order: the later track wins a shared last_idx
        for i1p, i1c, u1p, v1p, u1c, v1c in zip(pm["i1p"].tolist(), pm["i1c"].tolist(), pm["u1p"], pm["v1p"], pm["u1c"], pm["v1c"]):
            idx = track_idx[i1p] if i1p >= 0 else -1
            if idx >= 0 and tracks[idx][2] == current_frame - 1:
                t = tracks[idx]
                t[0].append((u1c, v1c)); t[2] = current_frame; t[3] = i1c
            else:
                tracks.append([[(u1p, v1p), (u1c, v1c)], current_frame - 1, current_frame, i1c])
        lost = [(t[1], t[0]) for t in tracks if t[2] != current_frame]
        self.tracks = [t for t in tracks if t[2] == current_frame]
        return lost

    def updateMany(self, lists, Trs, point_type: int = 1, min_track_length: int = 2, max_dist: float = 30.0, min_angle: float = 2.0):
        """len(lists) consecutive updates; the lost tracks of all of them are solved in one launch."""
        Trs = np.ascontiguousarray(Trs, dtype=np.float64).reshape(-1, 4, 4)
        if len(Trs) != len(lists):
            raise ValueError(f"updateMany: {len(lists)} lists need as many Trs (got {len(Trs)})")
        lost = []
        for pm, Tr in zip(lists, Trs):
            self.Trs.append(Tr.copy())
            lost += self.associate(pm, len(self.Trs))
        if not lost:
            return
        r = self.recon
        r.point_type, r.min_track_length, r.max_dist, r.min_angle = int(point_type), int(min_track_length), float(max_dist), float(min_angle)
        first = np.array([f for f, _ in lost], np.int32)
        offsets = np.zeros(len(lost) + 1, np.int32)
        offsets[1:] = np.cumsum([len(px) for _, px in lost])
        pixels = np.array([uv for _, px in lost for uv in px], np.float32).reshape(-1, 2)
        pts, st, _ = reconstruct_tracks(r, np.array(self.Trs), first, offsets, pixels, metrics=False, device=self.device)
        self.points += [p for p in pts[st == RECON_ACCEPTED]]

    def update(self, p_matched, Tr, point_type: int = 1, min_track_length: int = 2, max_dist: float = 30.0, min_angle: float = 2.0):
        """Reconstruction::update (src/reconstruction.cpp:59-151)."""
        self.updateMany([p_matched], [Tr], point_type, min_track_length, max_dist, min_angle)

    def getPoints(self) -> np.ndarray:
        """-> [n, 3] float32 (point3d x, y, z), in the order the reference appends them."""
        return np.array(self.points, np.float32).reshape(-1, 3)


def match(param: Params, dims, method: int, m1p=None, m2p=None, m1c=None, m2c=None, device: int = 0, cap=None):
    """Matcher::matching (reference src/matcher.cpp:274-344) on given feature arrays."""
    sets = [_feat(m) for m in (m1p, m2p, m1c, m2c)]
    if cap is None:
        cap = max(s[1] for s in sets) + 1
    out = np.zeros(cap, P_MATCH_DTYPE)
    n = C.c_int32(0)
    _check(_lib().vh_match(C.byref(param), device, _dims(dims), int(method),
                           _ptr(sets[0][0]), sets[0][1], _ptr(sets[1][0]), sets[1][1],
                           _ptr(sets[2][0]), sets[2][1], _ptr(sets[3][0]), sets[3][1],
                           _ptr(out), cap, C.byref(n)), "vh_match")
    return out[:n.value].copy()


def prior_statistics(param: Params, dims, method: int, pm) -> np.ndarray:
    """computePriorStatistics of multi-stage matching (vh_prior_statistics; host only) -> ranges [nb, 4, 4] float32:
    per statistics bin (v_bin * ubn + u_bin) and stage u_min, u_max, v_min, v_max."""
    pm = np.ascontiguousarray(pm, dtype=P_MATCH_DTYPE)
    ubn = -(-int(dims[0]) // param.match_binsize)
    vbn = -(-int(dims[1]) // param.match_binsize)
    out = np.zeros((ubn * vbn, 4, 4), np.float32)
    _check(_lib().vh_prior_statistics(C.byref(param), _dims(dims), int(method), _ptr(pm) if len(pm) else None, len(pm), _ptr(out)),
           "vh_prior_statistics")
    return out


def prior_statistics_device(param: Params, dims, method: int, lists, device: int = 0, stride: int = 0) -> np.ndarray:
    """prior_statistics of several lists in one launch on the GPU (vh_prior_statistics_device) -> ranges
    [n_lists, nb, 4, 4] float32.  stride: record slots per list in the array handed over (default: the longest list)."""
    lists = [np.ascontiguousarray(m, dtype=P_MATCH_DTYPE) for m in lists]
    n = len(lists)
    stride = max([len(m) for m in lists] + [1, int(stride)])
    pm = np.zeros((n, stride), P_MATCH_DTYPE)
    for l, m in enumerate(lists):
        pm[l, :len(m)] = m
    counts = np.array([len(m) for m in lists], np.int32)
    ubn = -(-int(dims[0]) // param.match_binsize)
    vbn = -(-int(dims[1]) // param.match_binsize)
    out = np.zeros((n, ubn * vbn, 4, 4), np.float32)
    _check(_lib().vh_prior_statistics_device(C.byref(param), device, _dims(dims), int(method), n, _ptr(pm), stride, _ptr(counts), _ptr(out)),
           "vh_prior_statistics_device")
    return out


def match_ranged(param: Params, dims, method: int, ranges, m1p=None, m2p=None, m1c=None, m2c=None, device: int = 0, cap=None):
    """Matcher::matching with use_prior = true (vh_match_ranged): every stage searches inside ranges [nb, 4, 4] of the
    driving feature's statistics bin."""
    sets = [_feat(m) for m in (m1p, m2p, m1c, m2c)]
    if cap is None:
        cap = max(s[1] for s in sets) + 1
    ubn = -(-int(dims[0]) // param.match_binsize)
    vbn = -(-int(dims[1]) // param.match_binsize)
    ranges = np.ascontiguousarray(ranges, dtype=np.float32)
    assert ranges.shape == (ubn * vbn, 4, 4), ranges.shape
    out = np.zeros(cap, P_MATCH_DTYPE)
    n = C.c_int32(0)
    _check(_lib().vh_match_ranged(C.byref(param), device, _dims(dims), int(method),
                                  _ptr(sets[0][0]), sets[0][1], _ptr(sets[1][0]), sets[1][1],
                                  _ptr(sets[2][0]), sets[2][1], _ptr(sets[3][0]), sets[3][1],
                                  _ptr(ranges), _ptr(out), cap, C.byref(n)), "vh_match_ranged")
    return out[:n.value].copy()


def refine_matches(param: Params, dims, method: int, pm, I1p=None, I2p=None, I1c=None, I2c=None, device: int = 0):
    """Stock libviso2's match refinement (param.refinement: 1 pixel, 2 sub-pixel) on the
    records pm with the full-resolution images of the pair -> the refined records that are kept, in order."""
    pm = np.ascontiguousarray(pm, dtype=P_MATCH_DTYPE).copy()
    imgs = [None if I is None else np.ascontiguousarray(I, dtype=np.uint8) for I in (I1p, I2p, I1c, I2c)]
    n = C.c_int32(0)
    _check(_lib().vh_refine_matches(C.byref(param), device, int(method), _dims(dims), *[_ptr(I) for I in imgs],
                                    _ptr(pm) if len(pm) else None, len(pm), C.byref(n)), "vh_refine_matches")
    return pm[:n.value].copy()
