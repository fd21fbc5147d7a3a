"""The handles of the binding: Matcher (one stream), StreamGroup (S streams in lock step) and SequenceGroup (one
camera's consecutive frames in the rows of a group)."""
from __future__ import annotations

from ._abi import *  # noqa: F401,F403  (constants, structures, dtypes)
from ._abi import _check, _device_view, _dims, _fetch, _lib, _models, _packed, _ptr, _scene_Tw, _traj_S0, _traj_T0


class _Handle:
    """What Matcher and StreamGroup share: the life of the handle, the stream it is ordered after and its switches.
    _ABI is what the C symbols of the class begin with: a shared method calls _ABI + the rest of the name."""
    _ABI = None

    def _call(self, name, *args):
        name = self._ABI + name
        return _check(getattr(_lib(), name)(self._h, *args), name)

    def _switch(self, name, on):
        """the on/off setters of the ABI: `name`(h, 1 or 0)"""
        self._call(name, 1 if on else 0)

    def close(self):
        if getattr(self, "_h", None):
            getattr(_lib(), self._ABI + "destroy")(self._h)
            self._h = None

    __del__ = close

    def synchronize(self):
        self._call("synchronize")

    def setStream(self, hip_stream: int | None):
        """Order every pushBack after `hip_stream` (a hipStream_t handle; 0 is the legacy
        default stream, a stream like any other); None removes the ordering."""
        if hip_stream is None:
            self._call("clear_stream")
        else:
            self._call("set_stream", C.c_void_p(int(hip_stream)))

    def streamWaitImages(self, hip_stream: int):
        """Make `hip_stream` wait (device side) until the last pushBackDevice's images were consumed."""
        self._call("stream_wait_images", C.c_void_p(int(hip_stream)))


# --------------------------------------------------------------------------- one stream
class Matcher(_Handle):
    """Host mirror of the reference's `Matcher` public surface
    (src/matcher.h:75-143): pushBack / matchFeatures / bucketFeatures /
    getMatches, same argument meaning, plus getFeatures for the parity checks."""
    _ABI = "vh_"

    def __init__(self, param: Params | None = None, device: int = 0, max_features: int = 0,
                 max_matches: int = 0, outlier_removal: bool = True):
        self.param = param if param is not None else Params.default()
        # matchFeatures ends with removeOutliers as the reference's does (src/matcher.cpp:108);
        # False gives the bare Matcher::matching result
        self.outlier_removal = bool(outlier_removal)
        h = C.c_void_p()
        _check(_lib().vh_create_ex(C.byref(self.param), device, max_features, max_matches, C.byref(h)), "vh_create")
        self._h = h

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
        # an empty list from truncated feature sets is still an error
        return _fetch("vh_get_matches", P_MATCH_DTYPE, self._h, empty_raises=True)

    def setMultiStageMatching(self, on: bool = True):
        """Two-pass matching of stock libviso2 (vh_set_multi_stage_matching): before the first pushBack, with
        param.multi_stage = 1."""
        self._switch("set_multi_stage_matching", on)

    def setMultiStageDevice(self, on: bool = True):
        """The vote and the statistics between the two passes on the GPU (vh_set_multi_stage_device): matchFeatures only
        queues work.  After setMultiStageMatching(True), before the first pushBack."""
        self._switch("set_multi_stage_device", on)

    def setMultiStagePrior(self, on: bool = True):
        """matchFeatures(2, Tr_delta) hands the motion estimate to both passes of multi-stage matching
        (vh_set_multi_stage_prior): after setMultiStageMatching(True), before the first pushBack."""
        self._switch("set_multi_stage_prior", on)

    def getSparseMatches(self) -> np.ndarray:
        """The sparse list of pass 1 after the vote (multi-stage matching on)."""
        return _fetch("vh_get_sparse_matches", P_MATCH_DTYPE, self._h)

    def setTrackLinking(self, on: bool = True):
        """Link every match list to the list of the previous pair on the GPU (vh_set_track_linking): before the first
        pushBack.  The tracks describe the list as matching left it: use outlier_removal=False, or link the voted lists
        with link_tracks()."""
        self._switch("set_track_linking", on)

    def setVoteRule(self, rule: int = VOTE_STOCK):
        """The rule of every outlier vote of this handle (vh_set_vote_rule), before the first push: VOTE_REFERENCE or
        VOTE_STOCK -- the per-method rule under this handle's outlier_flow_tolerance / outlier_disp_tolerance."""
        self._call("set_vote_rule", int(rule))

    def getTracks(self) -> np.ndarray:
        """One TRACK record per record of the last matchFeatures' list (vh_get_tracks)."""
        return _fetch("vh_get_tracks", TRACK, self._h, empty_raises=True)

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
        return _fetch("vh_get_scene_points", SCENE_POINT_DTYPE, self._h)

    def landmarks(self, params: "LandmarkParams | None" = None) -> np.ndarray:
        """The scene points of the last scenePoints fused along the feature tracks (vh_match_landmarks; setTrackLinking, and
        a scenePoints Tw that takes every step's points into one common frame) -> LANDMARK_DTYPE [n], in list order."""
        lp = params or LandmarkParams.default()
        n = C.c_int32(0)
        _check(_lib().vh_match_landmarks(self._h, C.byref(lp), C.byref(n)), "vh_match_landmarks")
        return self.getLandmarks()

    def getLandmarks(self) -> np.ndarray:
        """The landmarks of the last landmarks(), valid until the next matchFeatures (vh_get_landmarks)."""
        return _fetch("vh_get_landmarks", LANDMARK_DTYPE, self._h)

    def setGain(self, on: bool = True):
        """Keep the pushed left images on the device for getGain (vh_set_gain): before the first pushBack."""
        self._switch("set_gain", on)

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
        return _fetch("vh_get_inlier_matches", [P_MATCH_DTYPE, np.int32], self._h)

    def getFeatures(self, which: int) -> np.ndarray:
        return _fetch("vh_get_features", (np.int32, 12), self._h, which)


# ------------------------------------------------------------------ S streams in lock step
class StreamGroup(_Handle):
    """S independent camera streams stepped together (vh_group_*): the
    multi-stream configuration, one sequence per stream, no exchange between
    streams.  Images are device pointers (e.g. torch `tensor.data_ptr()`)."""
    _ABI = "vh_group_"
    # what a SequenceGroup does otherwise: the entries that switch the trajectory on, and the chains they start
    _SET_TRAJECTORY, _SET_TRAJECTORY_COVARIANCE = "vh_group_set_trajectory", "vh_group_set_trajectory_covariance"

    def _chains(self):
        """poses the trajectory carries: one per stream"""
        return self.S

    def __init__(self, n_streams: int, param: Params | None = None, device: int = 0,
                 max_features: int = 0, max_matches: int = 0):
        self.param = param if param is not None else Params.default()
        self.S = int(n_streams)
        h = C.c_void_p()
        _check(_lib().vh_group_create(C.byref(self.param), device, self.S, max_features, max_matches, C.byref(h)),
               "vh_group_create")
        self._h = h

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
        return _fetch("vh_group_get_matches", P_MATCH_DTYPE, self._h, stream, empty_raises=True)

    def setMultiStageMatching(self, on: bool = True):
        """Two-pass matching of stock libviso2 for every stream (vh_group_set_multi_stage_matching): before the first
        pushBack, with param.multi_stage = 1; not on a SequenceGroup."""
        self._switch("set_multi_stage_matching", on)

    def setMultiStageDevice(self, on: bool = True):
        """The vote and the statistics between the two passes on the GPU for every stream
        (vh_group_set_multi_stage_device): after setMultiStageMatching(True), before the first pushBack."""
        self._switch("set_multi_stage_device", on)

    def setMultiStagePrior(self, on: bool = True):
        """matchFeaturesPrior hands the motion estimates to both passes of multi-stage matching
        (vh_group_set_multi_stage_prior): after multi-stage matching was switched on, before the first pushBack."""
        self._switch("set_multi_stage_prior", on)

    def getSparseMatches(self, stream: int) -> np.ndarray:
        """The sparse list of pass 1 after the vote (multi-stage matching on)."""
        return _fetch("vh_group_get_sparse_matches", P_MATCH_DTYPE, self._h, stream)

    def setTrackLinking(self, on: bool = True):
        """Link every stream's (row's) match lists to their predecessors on the GPU (vh_group_set_track_linking): before
        the first pushBack; also on a SequenceGroup."""
        self._switch("set_track_linking", on)

    def setVoteRule(self, rule: int = VOTE_STOCK):
        """The rule of every outlier vote of this handle (vh_group_set_vote_rule), before the first push: VOTE_REFERENCE or
        VOTE_STOCK -- the per-method rule under this handle's outlier_flow_tolerance / outlier_disp_tolerance."""
        self._call("set_vote_rule", int(rule))

    def getTracks(self, stream: int) -> np.ndarray:
        """One TRACK record per record of the stream's (row's) list of the last matchFeatures (vh_group_get_tracks)."""
        return _fetch("vh_group_get_tracks", TRACK, self._h, stream, empty_raises=True)

    def _fetch_all(self, name, recs, cap_per_stream, out=None):
        """The getters of all streams at once, `name`(h, out..., cap, counts): arrays [S, max(cap_per_stream, 1)] of the
        dtypes `recs`, or the caller's `out` for the first -> (the arrays..., counts [S])"""
        if out is None:
            bufs = [np.zeros((self.S, max(cap_per_stream, 1)), r) for r in recs]
        else:
            assert out.dtype == recs[0] and out.ndim == 2 and out.shape[0] == self.S and out.flags.c_contiguous
            bufs = [out]
        counts = np.zeros(self.S, np.int32)
        _check(getattr(_lib(), name)(self._h, *[_ptr(b) for b in bufs], bufs[0].shape[1], _ptr(counts)), name)
        return (*bufs, counts)

    def getTracksAll(self, out: np.ndarray | None = None, cap_per_stream: int | None = None):
        """-> (records [S, cap_per_stream] TRACK, counts [S]) as getMatchesAll (vh_group_get_tracks_all)."""
        if out is None and cap_per_stream is None:
            cap_per_stream = int(self.getCounts()[1].max(initial=0))
        return self._fetch_all("vh_group_get_tracks_all", [TRACK], cap_per_stream, out)

    def tracksDevice(self):
        """-> (device address of stream 0's track records, stride in records): valid until the next matchFeatures."""
        return _device_view("vh_group_tracks_device", self._h)

    def getFeatures(self, stream: int, which: int) -> np.ndarray:
        return _fetch("vh_group_get_features", (np.int32, 12), self._h, stream, which)

    def getMatchesAll(self, out: np.ndarray | None = None, cap_per_stream: int | None = None):
        """-> (records [S, cap_per_stream] P_MATCH_DTYPE, counts [S]); one wait for the whole group.
        Pass `out` (e.g. from pinned_empty) to reuse a buffer."""
        if out is None and cap_per_stream is None:
            cap_per_stream = int(self.getCounts()[1].max(initial=0))
        return self._fetch_all("vh_group_get_matches_all", [P_MATCH_DTYPE], cap_per_stream, out)

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
        t0 = _traj_T0(T0, self._chains())
        fn = self._SET_TRAJECTORY
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
        return _device_view("vh_group_poses_device", self._h)

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
        fn = self._SET_TRAJECTORY_COVARIANCE
        _check(getattr(_lib(), fn)(self._h, C.byref(tcp) if on else None, _ptr(_traj_S0(Sigma0, self._chains()))), fn)

    def getPoseCovariances(self) -> np.ndarray:
        """The covariance records of the last trajectory() (vh_group_get_pose_covariances) -> TRAJ_COV_DTYPE [S]."""
        out = np.zeros(self.S, TRAJ_COV_DTYPE)
        _check(_lib().vh_group_get_pose_covariances(self._h, _ptr(out)), "vh_group_get_pose_covariances")
        return out

    def poseCovariancesDevice(self):
        """-> (device address of the covariance records of the last trajectory(), stride in records)"""
        return _device_view("vh_group_pose_covariances_device", self._h)

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
        return _fetch("vh_group_get_scene_points", SCENE_POINT_DTYPE, self._h, stream)

    def getScenePointsAll(self, cap_per_stream: int):
        """-> (points [S, cap_per_stream], counts [S]) (vh_group_get_scene_points_all)."""
        return self._fetch_all("vh_group_get_scene_points_all", [SCENE_POINT_DTYPE], cap_per_stream)

    def scenePointsDevice(self):
        """-> (device address of stream 0's points, stride in records): valid until the next matchFeatures."""
        return _device_view("vh_group_scene_points_device", self._h)

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
        return _fetch("vh_group_get_landmarks", LANDMARK_DTYPE, self._h, stream)

    def getLandmarksAll(self, cap_per_stream: int):
        """-> (landmarks [S, cap_per_stream], counts [S]) (vh_group_get_landmarks_all)."""
        return self._fetch_all("vh_group_get_landmarks_all", [LANDMARK_DTYPE], cap_per_stream)

    def landmarksDevice(self):
        """-> (device address of stream 0's landmarks, stride in records): valid until the next matchFeatures."""
        return _device_view("vh_group_landmarks_device", self._h)

    def setGain(self, on: bool = True):
        """Keep the pushed left images of every stream (sequence handle: frame) on the device for gain()
        (vh_group_set_gain): before the first push."""
        self._switch("set_gain", on)

    def gain(self, indices=None):
        """Matcher::getGain (reference src/matcher.h:148) for every stream (sequence handle: row): over the inlier
        positions of the current classification (indices None, vh_group_gain) or over `indices`, one array of positions
        into getMatches(s) per stream (vh_group_gain_indices) -> (gain float32 [S], num int32 [S])."""
        gain = np.zeros(self.S, np.float32); num = np.zeros(self.S, np.int32)
        if indices is None:
            _check(_lib().vh_group_gain(self._h, _ptr(gain), _ptr(num)), "vh_group_gain")
            return gain, num
        idx, off = _packed(indices, np.int32, empty=1)   # one element to point at when no stream has a position
        assert len(off) == self.S + 1
        _check(_lib().vh_group_gain_indices(self._h, _ptr(idx), _ptr(off), _ptr(gain), _ptr(num)), "vh_group_gain_indices")
        return gain, num

    def getInlierFlags(self, stream: int) -> np.ndarray:
        """One byte per record of the stream's list: 1 = inlier of the last motionInliers (vh_group_get_inlier_flags)."""
        return _fetch("vh_group_get_inlier_flags", np.uint8, self._h, stream)

    def getInlierMatches(self, stream: int):
        """-> (the stream's inlier records in list order, their positions in getMatches(stream)) (vh_group_get_inlier_matches)."""
        return _fetch("vh_group_get_inlier_matches", [P_MATCH_DTYPE, np.int32], self._h, stream)

    def getInlierMatchesAll(self, cap_per_stream: int):
        """-> (records [S, cap_per_stream], positions [S, cap_per_stream], counts [S]) (vh_group_get_inlier_matches_all)."""
        return self._fetch_all("vh_group_get_inlier_matches_all", [P_MATCH_DTYPE, np.int32], cap_per_stream)

    def inliersDevice(self):
        """-> (device addresses of stream 0's flags, inlier records and positions, stride in elements): valid until the
        next matchFeatures (vh_group_inliers_device)."""
        return _device_view("vh_group_inliers_device", self._h, 3)

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
        self._switch("profile_enable", on)

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
    _SET_TRAJECTORY, _SET_TRAJECTORY_COVARIANCE = "vh_sequence_set_trajectory", "vh_sequence_set_trajectory_covariance"

    def _chains(self):
        """one pose along the rows of the chunks"""
        return 1

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

