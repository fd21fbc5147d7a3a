"""The motion refit on the landmarks (include/viso_hip_lmk_refit.h): an extension module beside
the binding's three, not re-exported by the package -- import it as `<package>._lmk_refit`.  It holds the record and parameter layouts, the stateless entry and the handle entries as
functions over a Matcher / StreamGroup, in the call idioms of _abi."""
from __future__ import annotations

from ._abi import *  # noqa: F401,F403  (constants, structures, dtypes)
from ._abi import _ABI_EXT, _check, _fetch, _lib, _packed, _ptr, _scene_Tw

#: every symbol include/viso_hip_lmk_refit.h declares (checked by the CPU test-suite); their prototypes are rows of _abi's
#: extension table, set by _abi._lib() with all others
ABI_SYMBOLS = tuple(_ABI_EXT)


# vh_refit_prior (32 bytes): the point a record entered refit_motion_landmarks / refitMotionLandmarks with
REFIT_PRIOR_DTYPE = np.dtype([("X", "<f8"), ("Y", "<f8"), ("Z", "<f8"), ("source", "<i4"), ("reason", "<i4")])


class LandmarkRefitParams(C.Structure):
    """vh_lmk_refit_params: the fewest observations of a landmark the refit uses, and the gate on its depth over the
    record's own (max_depth_ratio <= 1: none)."""
    _fields_ = [("min_obs", C.c_int32), ("reserved", C.c_int32), ("max_depth_ratio", C.c_double)]

    @classmethod
    def default(cls, **kw):
        e = cls(min_obs=2, reserved=0, max_depth_ratio=0.0)
        for k, v in kw.items():
            if not hasattr(e, k):
                raise AttributeError(k)
            setattr(e, k, v)
        return e


def refit_motion_landmarks(ego: EgoParams, match_lists, prev_pos, prev_state, Tw_prev, tr, ok,
                           params: "LandmarkRefitParams | None" = None, device: int = 0):
    """refit_motion with the landmarks as the 3-d prior (vh_refit_motion_landmarks): prev_pos (int32 arrays, one per list:
    every record's position in its predecessor list, vh_track.prev), prev_state (None, or LANDMARK_STATE_DTYPE arrays, one
    per predecessor list), Tw_prev (one 4x4 or [n, 4, 4]: the previous camera to the world).
    -> (tr [n, 6], ok [n] bool, n_updates [n], n_used [n], [REFIT_PRIOR_DTYPE array per list])."""
    pm, offsets = _packed(match_lists, P_MATCH_DTYPE)
    n, total = len(offsets) - 1, int(offsets[-1])
    assert len(prev_pos) == n and (prev_state is None or len(prev_state) == n)
    rp = params or LandmarkRefitParams.default()
    ppos, poff = _packed(prev_pos, np.int32)
    assert np.array_equal(poff, offsets)
    prev, voff = _packed(prev_state, LANDMARK_STATE_DTYPE) if prev_state is not None else (None, None)
    tw = _scene_Tw(Tw_prev, n)
    tr = np.ascontiguousarray(tr, np.float64).reshape(n, 6); ok = np.ascontiguousarray(ok).astype(np.int32).reshape(n)
    tr_out = np.zeros((max(n, 1), 6), np.float64); ok_out = np.zeros(max(n, 1), np.int32); nupd = np.zeros(max(n, 1), np.int32)
    used = np.zeros(max(n, 1), np.int32); prior = np.zeros(max(total, 1), REFIT_PRIOR_DTYPE)
    _check(_lib().vh_refit_motion_landmarks(C.byref(ego), C.byref(rp), device, n, _ptr(pm), _ptr(offsets), _ptr(ppos),
                                            None if prev is None else _ptr(prev), None if voff is None else _ptr(voff), _ptr(tw),
                                            _ptr(tr), _ptr(ok), _ptr(tr_out), _ptr(ok_out), _ptr(nupd), _ptr(used), _ptr(prior)),
           "vh_refit_motion_landmarks")
    return (tr_out[:n], ok_out[:n].astype(bool), nupd[:n], used[:n],
            [prior[int(offsets[s]):int(offsets[s + 1])].copy() for s in range(n)])


def matchRefitMotionLandmarks(m, ego: "EgoParams", params: "LandmarkRefitParams | None" = None, Tw_prev=None, reclassify: bool = False):
    """On a Matcher `m`: refitMotion with the landmarks of the last landmarks() on the predecessor list as the 3-d points of
    the records they belong to (vh_match_refit_motion_landmarks; setTrackLinking) -> (tr [6], ok, n_updates, n_used, count).
    Tw_prev: the 4x4 pose of the previous camera in the landmarks' frame; None: the trajectory's (setTrajectory)."""
    rp = params or LandmarkRefitParams.default()
    tw = _scene_Tw(Tw_prev, 1)
    tr = np.zeros(6, np.float64); ok = C.c_int32(0); nupd = C.c_int32(0); used = C.c_int32(0); n = C.c_int32(0)
    _check(_lib().vh_match_refit_motion_landmarks(m._h, C.byref(ego), C.byref(rp), _ptr(tw), 1 if reclassify else 0, _ptr(tr),
                                                  C.byref(ok), C.byref(nupd), C.byref(used), C.byref(n)), "vh_match_refit_motion_landmarks")
    return tr, bool(ok.value), nupd.value, used.value, n.value


def groupRefitMotionLandmarks(g, ego: "EgoParams", params: "LandmarkRefitParams | None" = None, Tw_prev=None, reclassify: bool = False):
    """On a StreamGroup `g`: refitMotion with the landmarks of the last landmarks() on every stream's predecessor list as the
    3-d points of the records they belong to (vh_group_refit_motion_landmarks; setTrackLinking) -> (tr [S, 6], ok [S],
    n_updates [S], n_used [S], counts [S]).  Tw_prev: one 4x4 or [S, 4, 4], the previous cameras' poses in the landmarks'
    frame; None: the trajectory's (setTrajectory).  Without valid landmark states the result is refitMotion's and n_used is 0."""
    rp = params or LandmarkRefitParams.default()
    S = g.S
    tw = _scene_Tw(Tw_prev, S)
    tr = np.zeros((S, 6), np.float64); ok = np.zeros(S, np.int32); nupd = np.zeros(S, np.int32)
    used = np.zeros(S, np.int32); counts = np.zeros(S, np.int32)
    _check(_lib().vh_group_refit_motion_landmarks(g._h, C.byref(ego), C.byref(rp), _ptr(tw), 1 if reclassify else 0, _ptr(tr),
                                                  _ptr(ok), _ptr(nupd), _ptr(used), _ptr(counts)), "vh_group_refit_motion_landmarks")
    return tr, ok.astype(bool), nupd, used, counts


def getRefitPriors(h, stream: int = 0) -> np.ndarray:
    """The point every inlier of `stream` of a StreamGroup (a Matcher: stream 0) entered the last refit on the landmarks
    with, REFIT_PRIOR_DTYPE [n] in the order of the list the fit read, valid until the next matchFeatures
    (vh_group_get_refit_priors)."""
    return _fetch("vh_group_get_refit_priors", REFIT_PRIOR_DTYPE, h._h, stream)
