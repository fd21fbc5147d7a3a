"""The stateless entries of the binding: every call brings its inputs and takes its results, no handle in between."""
from __future__ import annotations

from ._abi import *  # noqa: F401,F403  (constants, structures, dtypes)
from ._abi import _check, _dims, _feat, _lib, _models, _packed, _padded, _ptr, _rule, _scene_Tw, _traj_S0, _traj_T0


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
    pm, offsets = _packed(match_lists, P_MATCH_DTYPE)
    n = len(offsets) - 1
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
    pm, offsets = _packed(match_lists, P_MATCH_DTYPE)
    n, total = len(offsets) - 1, int(offsets[-1])
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
    # (one-element placeholders: what this entry has always handed over for "no records" / "no positions"; vh_gain
    # reads neither, and the other entries' empty arrays are what they were written and tested with)
    pm, offsets = _packed(match_lists, P_MATCH_DTYPE, empty=1)
    idx, ioff = _packed(index_lists, np.int32, empty=1)
    n = len(offsets) - 1
    assert len(ioff) == n + 1
    W, H, bpl = (int(d) for d in dims)
    Ip = np.ascontiguousarray(I_prev, np.uint8).reshape(n, H, bpl); Ic = np.ascontiguousarray(I_cur, np.uint8).reshape(n, H, bpl)
    out = np.zeros(max(n, 1), np.float32); num = np.zeros(max(n, 1), np.int32)
    _check(_lib().vh_gain(device, n, _dims(dims), _ptr(Ip), _ptr(Ic), H * bpl, _ptr(pm), _ptr(offsets), _ptr(idx), _ptr(ioff), _ptr(out),
                          _ptr(num)), "vh_gain")
    return out[:n], num[:n]


def refit_motion(ego: EgoParams, match_lists, tr, ok, device: int = 0):
    """The reference's final optimisation (src/viso_stereo.cpp:126-139: updateParameters with eps 1e-8 until it converges, at
    most 102 times) on whole quad lists, every record active, from the starts tr [n, 6] / ok [n] (vh_refit_motion).
    -> (tr [n, 6], ok [n] bool, n_updates [n])."""
    pm, offsets = _packed(match_lists, P_MATCH_DTYPE)
    n = len(offsets) - 1
    tr = np.ascontiguousarray(tr, np.float64).reshape(n, 6); ok = np.ascontiguousarray(ok).astype(np.int32).reshape(n)
    tr_out = np.zeros((max(n, 1), 6), np.float64); ok_out = np.zeros(max(n, 1), np.int32); nupd = np.zeros(max(n, 1), np.int32)
    _check(_lib().vh_refit_motion(C.byref(ego), device, n, _ptr(pm), _ptr(offsets), _ptr(tr), _ptr(ok), _ptr(tr_out), _ptr(ok_out),
                                  _ptr(nupd)), "vh_refit_motion")
    return tr_out[:n], ok_out[:n].astype(bool), nupd[:n]


def motion_covariance(ego: EgoParams, match_lists, tr, ok, device: int = 0):
    """The 6x6 covariance sigma^2 (J^T J)^-1 of stereo motions over whole quad lists, every record active, at the motions
    tr [n, 6] / ok [n] (vh_motion_covariance): J and the residuals as the reference's computeResidualsAndJacobian forms
    them at tr, sigma^2 = ssr / (4 N - 6).  -> (cov [n, 6, 6], ssr [n], ok [n] bool)."""
    pm, offsets = _packed(match_lists, P_MATCH_DTYPE)
    n = len(offsets) - 1
    tr = np.ascontiguousarray(tr, np.float64).reshape(n, 6); ok = np.ascontiguousarray(ok).astype(np.int32).reshape(n)
    cov = np.zeros((max(n, 1), 6, 6), np.float64); ssr = np.zeros(max(n, 1), np.float64); ok_out = np.zeros(max(n, 1), np.int32)
    _check(_lib().vh_motion_covariance(C.byref(ego), device, n, _ptr(pm), _ptr(offsets), _ptr(tr), _ptr(ok), _ptr(cov), _ptr(ssr),
                                       _ptr(ok_out)), "vh_motion_covariance")
    return cov[:n], ssr[:n], ok_out[:n].astype(bool)


def _scene_points(fn, e, match_lists, motion, ok, sp, Tw, device):
    pm, offsets = _packed(match_lists, P_MATCH_DTYPE)
    n, total = len(offsets) - 1, int(offsets[-1])
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
    tr, off = _packed(tr_chains, np.float64, (6,), empty=1)   # (the chain entries get one zero row when no chain has a row)
    ok, ok_off = _packed(ok_chains, np.int32, empty=1)
    assert np.array_equal(ok_off, off)
    total = int(off[-1])
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
    tr, off = _packed(tr_chains, np.float64, (6,), empty=1)   # (one zero row each when no chain has a row, as trajectory's)
    packs = [_packed(ok_chains, np.int32, empty=1), _packed(cov_chains, np.float64, (36,), empty=1),
             _packed(ok_cov_chains, np.int32, empty=1)]
    assert all(np.array_equal(o, off) for _, o in packs)
    ok, cov, okc = (a for a, _ in packs)
    total = int(off[-1])
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
    pm, offsets = _packed(match_lists, P_MATCH_DTYPE)
    n = len(offsets) - 1
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
    pm, offsets = _packed(match_lists, P_MATCH_DTYPE)
    n, total = len(offsets) - 1, int(offsets[-1])
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
    pm, offsets = _packed(match_lists, P_MATCH_DTYPE)
    n = len(offsets) - 1
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
    pm, offsets = _packed(match_lists, P_MATCH_DTYPE)
    n = len(offsets) - 1
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
    pm, stride, counts = _padded(lists)
    n = len(counts)
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
    pm, stride, counts = _padded(lists)
    n = len(counts)
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
    pm, stride, counts = _padded(lists)
    n = len(counts)
    tr = np.ascontiguousarray(Trs, dtype=np.float64).reshape(-1, 16)
    if tr.shape[0] != n:
        raise ValueError(f"reconstruct_lists: {n} lists need as many Trs (got {tr.shape[0]})")
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
    pm, stride, counts = _padded([m for ls in streams for m in ls])
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
        pixels, offsets = _packed([px for _, px in lost], np.float32, (2,))
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
    pm, stride, counts = _padded(lists, max(1, int(stride)))
    n = len(counts)
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
