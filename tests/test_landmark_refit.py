"""Motion refit on the landmarks: vh_refit_motion's loop with the fused landmark of a record's track
as its 3-d point.  tests/lmk_refit_oracle.py is the restatement (the rule in numpy, refit_oracle's loop over the points);
tests/cpp/lmk_refit_check.cpp compiles csrc/vh_refit_prior.h and vh_ego.h for the host.  The CPU part ties the two together
and checks the premises of the GPU cases; the GPU part holds the kernels to the restatement: priors and n_used byte for
byte, ok and n_updates exactly, tr within the project's bound (rtol 1e-9, atol 1e-12, tests/test_egomotion.py), derived as
tests/test_motion_refit.py derives it -- the host program summing in the kernel's order differs from the sequential sums by
less than a tenth of it (asserted below), the rest is the room for the device's sin and cos.  Handles are held to the
stateless entry byte for byte on the lists and states their getters return.

The restatement is not independent of a copy: refit_oracle.rows takes no points, and that module may not change, so
lmk_refit_oracle.rows_points repeats its row arithmetic with X, Y, Z passed in and is swapped in for refit_oracle.rows
while refit_oracle's own loop, normal equations and solve run.  test_rows_with_own_points_are_refit_oracles_rows holds
the copy to refit_oracle.rows' bytes where the points are the records' own; for other points nothing but the shared
header on the host (tests/cpp/lmk_refit_check.cpp, byte-equal on every parity list) stands beside it."""
import ctypes as C
import importlib
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import landmark_oracle as lo
import lmk_refit_oracle as lr
import refit_oracle as ro
import test_motion_inliers as mi
import test_motion_refit as mr
import test_post_dense as pd
import test_sequence_recon as sr
from conftest import ROOT
from egomotion_scene import KITTI, rot

SYMBOLS = ("vh_default_lmk_refit_params", "vh_refit_motion_landmarks", "vh_group_refit_motion_landmarks", "vh_match_refit_motion_landmarks",
           "vh_group_get_refit_priors")
QUAD = mr.QUAD
TR = mr.TR
Cal = mr.Cal
ptr, expect, within_bound = mr.ptr, mr.expect, mr.within_bound
I32MAX = 2 ** 31 - 1
POSE = np.eye(4)
POSE[:3, :3] = rot(0.02, -0.3, 0.01)
POSE[:3, 3] = (3.0, -0.5, 12.0)


def ext(pkg):
    """the binding's extension module of this feature (not re-exported by the package)"""
    return importlib.import_module(pkg.__name__ + "._lmk_refit")


# ------------------------------------------------------------------------------------------------------------ cases
def states_for(pm, n_prev, Tw, seed, cal, n_obs=(1, 2, 3, 5), noise=0.01):
    """(prev_pos [n], states [n_prev]): a state is continued by at most one record (the link rule) and holds that
    record's own point, moved a little and taken to the world by Tw -- a landmark near where the record's track is.
    Records 1 and 2 continue the states 0 and n_prev - 1, every 7th record has a position outside (-1, n_prev, INT32_MAX),
    the records left over when the states run out have -1."""
    rng = np.random.default_rng(seed)
    n = len(pm)
    X, Y, Z = lr.own_points(pm, cal)
    ppos = np.full(n, -1, np.int32)
    free = [i for i in range(n) if i % 7]
    states = list(rng.permutation(n_prev)) if n_prev > 0 else []
    for fixed in (0, n_prev - 1):                      # first and last state: records 1 and 2
        if fixed in states and len(states) > 1:
            states.remove(fixed); states.insert(0 if fixed == 0 else 1, fixed)
    for i, p in zip(free, states):
        ppos[i] = p
    outside = (-1, n_prev, I32MAX)
    for i in range(0, n, 7):
        ppos[i] = outside[(i // 7) % 3]
    st = np.zeros(max(n_prev, 0), lo.STATE)
    for i in range(n):
        p = int(ppos[i])
        if 0 <= p < n_prev:
            P = np.array([X[i], Y[i], Z[i]]) + rng.normal(0, noise, 3) * max(Z[i], 1.0) / 20
            m = Tw[:3, :3] @ P + Tw[:3, 3]
            w = rng.uniform(0.5, 40.0)
            st[p] = (w, w * m[0], w * m[1], w * m[2], n_obs[p % len(n_obs)], 0, (0, 0))
    return ppos, st


def special_states(st, ppos, Tw):
    """sw = 0, a NaN swx, a +inf sw, a landmark behind the camera and one at Z = 0 on the states the first records use"""
    used = [int(p) for p in ppos if 0 <= p < len(st)]
    uniq = list(dict.fromkeys(used))[:5]
    for k, p in enumerate(uniq):
        if k == 4 and not np.array_equal(Tw, np.eye(4)):
            continue                     # (Z = 0 is exact under the unit pose only)
        st[p]["n_obs"] = 5
        if k == 0:
            st[p]["sw"] = 0.0
        elif k == 1:
            st[p]["swx"] = np.nan
        elif k == 2:
            st[p]["sw"] = np.inf
        else:
            P = np.array([1.0, 2.0, -3.0 if k == 3 else 0.0])
            m = Tw[:3, :3] @ P + Tw[:3, 3] if k == 3 else Tw[:3, 3] + Tw[:3, :3] @ P
            st[p]["sw"] = 1.0; st[p]["swx"], st[p]["swy"], st[p]["swz"] = m
    return st


_CASES = {}
#: the list of the depth gate: the records GATE_AT have their landmark at GATE_SCALE times their own depth -- on the upper
#: bound of max_depth_ratio = 2, on the lower, outside above, outside below
GATE_SEED, GATE_AT, GATE_SCALE = 412, np.array([10, 110, 210, 290]), np.array([2.0, 0.5, 2.5, 0.4])
#: seed of a list's states where 900 + k does not do, chosen on the CPU so that test_case_premises holds
STATE_SEEDS = {5: 1005}


def calls(oracle, ob):
    """The stateless calls: [(name, rp kwargs, lists)] with lists of (pm, prev_pos, states or None, Tw, start, ok_in)."""
    if "c" in _CASES:
        return _CASES["c"]
    cal = Cal(reweighting=0, **KITTI)
    lists, starts, oks = mr.parity_lists(oracle, ob)
    main = []
    for k, (pm, start, ok) in enumerate(zip(lists, starts, oks)):
        n_prev = (257, 1, 0, None, 257, 300)[k % 6] if len(pm) != 3073 else 3073
        Tw = np.eye(4) if k % 2 == 0 else POSE
        seed = STATE_SEEDS.get(k, 900 + k)
        if n_prev is None:
            ppos, st = states_for(pm, 0, Tw, seed, cal)[0], None
        else:
            ppos, st = states_for(pm, n_prev, Tw, seed, cal)
            if k in (10, 11, 12):
                st = special_states(st, ppos, Tw)
        main.append((pm, ppos, st, Tw, start, int(ok)))
    # every record on a landmark (list 13, 777 records: one state each) / every record falling back (list 15: n_obs below min_obs)
    pm = lists[13]
    X, Y, Z = lr.own_points(pm, cal)
    st = np.zeros(len(pm), lo.STATE)
    rng = np.random.default_rng(78)     # (chosen on the CPU so that test_case_premises holds)
    P = np.stack([X, Y, Z], 1) + rng.normal(0, 0.02, (len(pm), 3))
    M = P @ POSE[:3, :3].T + POSE[:3, 3]
    st["sw"] = 4.0; st["swx"], st["swy"], st["swz"] = 4.0 * M[:, 0], 4.0 * M[:, 1], 4.0 * M[:, 2]; st["n_obs"] = 4
    main[13] = (pm, np.arange(len(pm), dtype=np.int32), st, POSE, starts[13], 1)
    pm = lists[15]
    st = states_for(pm, 40, np.eye(4), 55, cal, n_obs=(1,))[1]
    main[15] = (pm, np.arange(len(pm), dtype=np.int32), st, np.eye(4), starts[15], 1)
    # min_obs = 1 and 3 with n_obs = min_obs - 1 and min_obs; max_depth_ratio 1 (no gate) and 2 with records exactly on both bounds
    pm = mr.noisy(300, GATE_SEED)
    X, Y, Z = lr.own_points(pm, cal)
    st = np.zeros(300, lo.STATE)
    scale = np.ones(300)
    scale[GATE_AT] = GATE_SCALE                       # (along the ray; the products by 2, 0.5 are exact: on the bounds to the bit)
    st["sw"] = 1.0; st["swx"], st["swy"], st["swz"] = X * scale, Y * scale, Z * scale
    st["n_obs"] = np.array([0, 1, 2, 3])[np.arange(300) % 4]
    st["n_obs"][GATE_AT] = 3
    gate = (pm, np.arange(300, dtype=np.int32), st, np.eye(4), np.array(TR) + 1e-3, 1)
    _CASES["c"] = [("main", dict(), main), ("one", dict(min_obs=1, max_depth_ratio=1.0), main[7:9]),
                   ("gate", dict(min_obs=3, max_depth_ratio=2.0), [gate]), ("gate1", dict(min_obs=1, max_depth_ratio=2.0), [gate])]
    return _CASES["c"]


def expectation(oracle, ob, rw):
    """the restatement's (priors, tr, ok, n_updates, steps) of every list of every call under reweighting rw, once"""
    if ("want", rw) not in _CASES:
        cal = Cal(reweighting=rw, **KITTI)
        out = {}
        for name, kw, lists in calls(oracle, ob):
            rows = []
            for pm, ppos, st, Tw, start, ok in lists:
                pr = lr.priors(pm, ppos, st, Tw, cal, kw.get("min_obs", 2), kw.get("max_depth_ratio", 0.0))
                rows.append((pr,) + tuple(lr.refit(pm, pr, start, cal, ok=bool(ok))))
            out[name] = rows
        _CASES["want", rw] = out
    return _CASES["want", rw]


def host_check(exe, tmp, pm, ppos, st, Tw, start, cal, kw, lanes):
    """tests/cpp/lmk_refit_check.cpp on one list -> (priors, tr [6], ok, n_updates, n_used)"""
    fin, fout = str(tmp / "in"), str(tmp / "out")
    with open(fin, "wb") as fh:
        fh.write(np.array([cal.f, cal.cu, cal.cv, cal.base, cal.reweighting, *start, kw.get("min_obs", 2), kw.get("max_depth_ratio", 0.0),
                           *np.asarray(Tw, np.float64).reshape(16)], np.float64).tobytes())
        fh.write(np.array([len(pm), lanes, -1 if st is None else len(st)], np.int64).tobytes())
        fh.write(pm.tobytes()); fh.write(np.ascontiguousarray(ppos, np.int32).tobytes())
        if st is not None:
            fh.write(st.tobytes())
    subprocess.check_call([exe, fin, fout], timeout=120)
    raw = open(fout, "rb").read()
    k = 32 * len(pm)
    tail = np.frombuffer(raw[k + 48:], np.int32)
    return np.frombuffer(raw[:k], lr.PRIOR), np.frombuffer(raw[k:k + 48], np.float64), int(tail[0]), int(tail[1]), int(tail[2])


# ------------------------------------------------------------------------------------------------------------ CPU
def test_symbols_and_host_refusals(pkg):
    """Declared, exported, mirrored; the record is 32 bytes; n_sets = 0 and lists without records are VH_OK without a
    device; null pointers, min_obs = 0, reserved != 0 and one of prev / prev_offsets alone are VH_ERR_INVALID_ARG."""
    text = open(os.path.join(ROOT, "include", "viso_hip_lmk_refit.h")).read()
    header = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    lib = ext(pkg)._lib()
    assert sorted(set(re.findall(r"\b(vh_[a-z0-9_]+)\s*\(", header))) == sorted(SYMBOLS) == sorted(ext(pkg).ABI_SYMBOLS)
    for name in SYMBOLS:
        assert hasattr(C.CDLL(pkg.LIB_PATH), name), name
    assert ext(pkg).REFIT_PRIOR_DTYPE.itemsize == 32 == lr.PRIOR.itemsize and C.sizeof(ext(pkg).LandmarkRefitParams) == 16
    rp = ext(pkg).LandmarkRefitParams(9, 9, 9.0)
    lib.vh_default_lmk_refit_params(C.byref(rp))
    assert (rp.min_obs, rp.reserved, rp.max_depth_ratio) == (2, 0, 0.0)
    for fn in ("refit_motion_landmarks", "matchRefitMotionLandmarks", "groupRefitMotionLandmarks", "getRefitPriors"):
        assert callable(getattr(ext(pkg), fn)), fn
    e = pkg.EgoParams.default(**KITTI)
    pm = np.zeros(8, pkg.P_MATCH_DTYPE); off = np.array([0, 8], np.int32); pp = np.zeros(8, np.int32)
    st = np.zeros(2, pkg.LANDMARK_STATE_DTYPE); voff = np.array([0, 2], np.int32)
    Tw = np.eye(4).reshape(1, 16).copy(); tr = np.zeros((1, 6)); ok = np.ones(1, np.int32)
    tro = np.full((2, 6), 7.0); oko = np.full(2, 7, np.int32); nu = np.full(2, 7, np.int32); used = np.full(2, 7, np.int32)
    pr = np.zeros(8, ext(pkg).REFIT_PRIOR_DTYPE)
    call = lib.vh_refit_motion_landmarks
    assert call(C.byref(e), C.byref(rp), 0, 0, *[None] * 13) == pkg.VH_OK
    empty = np.array([3, 3, 3], np.int32)
    assert call(C.byref(e), C.byref(rp), 0, 2, None, ptr(empty), None, None, None, ptr(np.zeros((2, 16))), ptr(np.zeros((2, 6))),
                ptr(np.ones(2, np.int32)), ptr(tro), ptr(oko), ptr(nu), ptr(used), None) == pkg.VH_OK
    assert not tro.any() and not oko.any() and not nu.any() and not used.any()
    inv = pkg.VH_ERR_INVALID_ARG
    good = [C.byref(e), C.byref(rp), 0, 1, ptr(pm), ptr(off), ptr(pp), ptr(st), ptr(voff), ptr(Tw), ptr(tr), ptr(ok), ptr(tro), ptr(oko),
            ptr(nu), ptr(used), ptr(pr)]
    for k in (0, 1, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15):     # (7, 8: one of prev / prev_offsets alone)
        args = list(good); args[k] = None
        assert call(*args) == inv, k
    args = list(good); args[3] = -1
    assert call(*args) == inv
    for bad in (ext(pkg).LandmarkRefitParams(0, 0, 0.0), ext(pkg).LandmarkRefitParams(2, 1, 0.0)):
        args = list(good); args[1] = C.byref(bad)
        assert call(*args) == inv
    assert lib.vh_group_refit_motion_landmarks(None, C.byref(e), C.byref(rp), None, 0, ptr(tro), ptr(oko), ptr(nu), ptr(used), ptr(nu)) == inv
    assert lib.vh_group_get_refit_priors(None, 0, None, 0, None) == inv


def test_rows_with_own_points_are_refit_oracles_rows():
    """lmk_refit_oracle.rows_points fed the records' own points gives refit_oracle.rows' bytes, both reweightings."""
    pm = mr.noisy(500, 3)
    for rw in (0, 1):
        cal = Cal(reweighting=rw, **KITTI)
        X, Y, Z = lr.own_points(pm, cal)
        for a, b in zip(lr.rows_points(pm, X, Y, Z, TR, cal), ro.rows(pm, TR, cal)):
            assert a.tobytes() == b.tobytes(), rw


def test_case_premises(ob, oracle):
    """On the restatement alone: every converging list has a last step of at most 5e-9 and a step before it of at least
    2e-8; every reason 0..5 occurs; one list has every record on a landmark, one every record falling back (and equals
    the plain refit's bytes); records lie exactly on both bounds of the depth gate and are used."""
    reasons = set()
    for rw in (0, 1):
        want = expectation(oracle, ob, rw)
        for name, kw, lists in calls(oracle, ob):
            for k, ((pm, ppos, st, Tw, start, ok), (pr, tr, okw, nupd, steps)) in enumerate(zip(lists, want[name])):
                reasons |= set(pr["reason"].tolist())
                if len(pm) < 6 or not ok:
                    assert not okw and nupd == 0
                    continue
                assert okw and 1 <= nupd <= 20 and steps[-1] <= 5e-9, (rw, name, k, steps)
                assert nupd == 1 or steps[-2] >= 2e-8, (rw, name, k, steps)
        main = want["main"]
        assert len(main[13][0]) == 777 and main[13][0]["source"].all()
        assert not main[15][0]["source"].any() and set(main[15][0]["reason"].tolist()) == {2}
        plain = ro.refit(calls(oracle, ob)[0][2][15][0], calls(oracle, ob)[0][2][15][4], Cal(reweighting=rw, **KITTI))
        assert np.asarray(main[15][1]).tobytes() == np.asarray(plain[0]).tobytes() and main[15][3] == plain[2]
        for g in (want["gate"][0][0], want["gate1"][0][0]):
            assert g["source"][GATE_AT].tolist() == [1, 1, 0, 0] and g["reason"][GATE_AT].tolist() == [0, 0, 5, 5]
            assert (g["Z"][GATE_AT[:2]] / lr.own_points(calls(oracle, ob)[2][2][0][0], Cal(reweighting=0, **KITTI))[2][GATE_AT[:2]]).tolist() == [2.0, 0.5]
    assert reasons == {0, 1, 2, 3, 4, 5}, reasons


def test_header_on_the_host_equals_the_restatement(tmp_path, ob, oracle):
    """csrc/vh_refit_prior.h and vh_ego.h compiled for the host with -ffp-contract=off: the priors are the restatement's byte
    for byte; summed record after record tr, ok and n_updates are too; summed in the kernel's shape ok and n_updates are
    equal and tr differs by less than a tenth of the project's bound.  The largest difference is printed."""
    exe = str(tmp_path / "lmk_refit_check")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", os.path.join(ROOT, "tests", "cpp", "lmk_refit_check.cpp"), "-lm", "-o", exe])
    worst = 0.0
    for rw in (0, 1):
        cal = Cal(reweighting=rw, **KITTI)
        want = expectation(oracle, ob, rw)
        for name, kw, lists in calls(oracle, ob):
            for k, ((pm, ppos, st, Tw, start, ok), (pr, tr, okw, nupd, _)) in enumerate(zip(lists, want[name])):
                if not ok:
                    continue
                got = host_check(exe, tmp_path, pm, ppos, st, Tw, start, cal, kw, 0)
                assert got[0].tobytes() == pr.tobytes(), (rw, name, k)
                assert (got[2], got[3], got[4]) == (int(okw), nupd, int(pr["source"].sum())), (rw, name, k)
                assert got[1].tobytes() == np.asarray(tr, np.float64).tobytes(), (rw, name, k)
                shaped = host_check(exe, tmp_path, pm, ppos, st, Tw, start, cal, kw, 256)
                assert shaped[0].tobytes() == pr.tobytes() and (shaped[2], shaped[3]) == (int(okw), nupd), (rw, name, k)
                worst = max(worst, float(np.abs(shaped[1] - tr).max(initial=0.0)))
    print(f"kernel-shaped sums against sequential sums: largest |tr| difference {worst:.3e}")
    assert worst < 0.1 * mr.ATOL, worst


def simulate(seed, steps=6, n=400, noise=0.3):
    """A static scene seen over `steps` steps of TR: per step the plain refit and the refit on the landmarks fused by
    landmark_oracle from the steps before (points taken to the world by this fit's own accumulated pose), both from a zero
    start.  -> (translation errors plain, prior; rotation errors plain, prior) over the steps that had landmarks"""
    rng = np.random.default_rng(seed)
    cal = Cal(reweighting=1, **KITTI)
    f, cu, cv, base = KITTI["f"], KITTI["cu"], KITTI["cv"], KITTI["base"]
    R, t = rot(*TR[:3]), np.array(TR[3:])
    Z = rng.uniform(12, 70, n)
    P = np.stack([rng.uniform(-0.6, 0.6, n) * Z, rng.uniform(-0.2, 0.2, n) * Z, Z + 8.0], 1)   # in camera 0

    def project(Q):
        v = np.stack([f * Q[:, 0] / Q[:, 2] + cu, f * Q[:, 1] / Q[:, 2] + cv, f * (Q[:, 0] - base) / Q[:, 2] + cu, f * Q[:, 1] / Q[:, 2] + cv], 1)
        return v + rng.uniform(-noise, noise, v.shape)

    trk = np.zeros(n, lo.TRACK); trk["prev"] = np.arange(n)
    lp = lo.params(min_obs=1, max_missed=-1)
    pose = np.eye(4)                      # camera k-1 to the world, accumulated from the prior fit's own motions
    state, prev_obs = None, project(P)
    et_p, et_l, er_p, er_l = [], [], [], []
    for k in range(steps):
        P = P @ R.T + t
        cur_obs = project(P)
        pm = np.zeros(n, mr.P_MATCH)
        for j, name in enumerate(("u1p", "v1p", "u2p", "v2p")):
            pm[name] = prev_obs[:, j].astype(np.float32)
        for j, name in enumerate(("u1c", "v1c", "u2c", "v2c")):
            pm[name] = cur_obs[:, j].astype(np.float32)
        plain = ro.refit(pm, np.zeros(6), cal)
        pr = lr.priors(pm, trk["prev"], state, pose, cal, 1, 0.0)
        fit = lr.refit(pm, pr, np.zeros(6), cal)
        assert plain[1] and fit[1]
        if state is not None:
            et_p.append(np.abs(plain[0][3:] - t).max()); et_l.append(np.abs(fit[0][3:] - t).max())
            er_p.append(np.abs(plain[0][:3] - TR[:3]).max()); er_l.append(np.abs(fit[0][:3] - TR[:3]).max())
        T = np.eye(4); T[:3, :3] = rot(*fit[0][:3]); T[:3, 3] = fit[0][3:]
        pose = pose @ np.linalg.inv(T)    # camera k to the world
        d = np.maximum(cur_obs[:, 0] - cur_obs[:, 2], 1e-4)
        C3 = np.stack([(cur_obs[:, 0] - cu) * base / d, (cur_obs[:, 1] - cv) * base / d, f * base / d], 1)   # this step's points, camera k
        Wp = C3 @ pose[:3, :3].T + pose[:3, 3]
        pts = np.zeros(n, lo.POINT)
        pts["x"], pts["y"], pts["z"] = Wp[:, 0], Wp[:, 1], Wp[:, 2]
        pts["sigma_z"] = C3[:, 2] ** 2 / (f * base) * 0.3
        pts["src_pos"] = np.arange(n)
        _, state = lo.update(trk, pts, state, lp)
        prev_obs = cur_obs
    return et_p, et_l, er_p, er_l


def test_accuracy_on_a_static_scene():
    """Fixed seeds, on the restatement alone: the median translation and rotation error of the fit on the landmarks is not
    larger than the plain refit's on the same records.  The ratios are printed (profiles/landmark_refit.md has them)."""
    acc = [[], [], [], []]
    for seed in (1, 2, 3, 4):
        for a, v in zip(acc, simulate(seed)):
            a.extend(v)
    mt_p, mt_l, mr_p, mr_l = (float(np.median(a)) for a in acc)
    print(f"median translation error: plain {mt_p:.3e}, landmarks {mt_l:.3e}, ratio {mt_l / mt_p:.3f}; "
          f"rotation: plain {mr_p:.3e}, landmarks {mr_l:.3e}, ratio {mr_l / mr_p:.3f}")
    assert mt_l <= mt_p and mr_l <= mr_p


# ------------------------------------------------------------------------------------------------------------ GPU, stateless
def run_call(pkg, rw, kw, lists):
    e = pkg.EgoParams.default(reweighting=rw, **KITTI)
    rp = ext(pkg).LandmarkRefitParams.default(**kw)
    has_prev = any(l[2] is not None for l in lists)
    prev = [np.zeros(0, lo.STATE) if l[2] is None else l[2] for l in lists] if has_prev else None
    return ext(pkg).refit_motion_landmarks(e, [l[0] for l in lists], [l[1] for l in lists], prev, np.stack([l[3] for l in lists]),
                                      np.stack([l[4] for l in lists]), [l[5] for l in lists], rp)


def check_call(got, want, what):
    tr, ok, nupd, used, priors = got
    for k, (pr, tr_w, ok_w, n_w, _) in enumerate(want):
        assert priors[k].tobytes() == pr.tobytes(), (what, k, "priors")
        assert int(used[k]) == int(pr["source"].sum()), (what, k, "n_used")
        assert bool(ok[k]) == bool(ok_w) and int(nupd[k]) == n_w, (what, k, ok[k], ok_w, nupd[k], n_w)
        assert within_bound(tr[k], tr_w), (what, k, tr[k], tr_w)


@pytest.mark.gpu
@pytest.mark.parametrize("rw", [0, 1])
def test_gpu_stateless_parity(rw, pkg, ob, oracle, gpu):
    """17 lists in one call (lengths 0 .. 9000, ok_in = 0 among them; predecessor lists of 0, 1, 257 and 3073 states and
    none; prev_pos -1, 0, n_prev - 1, n_prev, INT32_MAX; sw = 0, NaN swx, +inf sw, behind the camera, Z = 0; the unit pose
    and a general one), the calls with min_obs 1 and 3 and the depth gate at 1 and 2, then lists 7 and 8 alone (2 per call)
    and list 11 alone (a short call behind a long one would differ if anything was left over)."""
    want = expectation(oracle, ob, rw)
    for name, kw, lists in calls(oracle, ob):
        check_call(run_call(pkg, rw, kw, lists), want[name], (name, rw))
    main = calls(oracle, ob)[0][2]
    check_call(run_call(pkg, rw, {}, main[7:9]), want["main"][7:9], ("two", rw))
    check_call(run_call(pkg, rw, {}, main[1:2]), want["main"][1:2], ("short behind long", rw))
    check_call(run_call(pkg, rw, {}, main[11:12]), want["main"][11:12], ("one", rw))
    # NULL predecessors: every record falls back, the bytes are vh_refit_motion's
    e = pkg.EgoParams.default(reweighting=rw, **KITTI)
    sub = [l for l in main if l[5] and len(l[0]) >= 6][:4]
    got = ext(pkg).refit_motion_landmarks(e, [l[0] for l in sub], [l[1] for l in sub], None, np.eye(4), np.stack([l[4] for l in sub]), [1] * len(sub))
    plain = pkg.refit_motion(e, [l[0] for l in sub], np.stack([l[4] for l in sub]), [1] * len(sub))
    assert got[0].tobytes() == plain[0].tobytes() and np.array_equal(got[1], plain[1]) and np.array_equal(got[2], plain[2])
    assert not got[3].any() and all((p["reason"] == 1).all() for p in got[4])
    # the list whose states are all below min_obs: the same bytes again
    l = main[15]
    got = run_call(pkg, rw, {}, [l])
    plain = pkg.refit_motion(e, [l[0]], l[4][None], [1])
    assert got[0].tobytes() == plain[0].tobytes() and got[3][0] == 0


@pytest.mark.gpu
def test_gpu_identity_pose_gives_the_means(pkg, ob, oracle, gpu):
    """Under the unit matrix the prior of a used record is the landmark's mean bit for bit."""
    pm, ppos, st, Tw, start, ok = calls(oracle, ob)[0][2][4]
    assert np.array_equal(Tw, np.eye(4))
    pr = run_call(pkg, 0, {}, [(pm, ppos, st, Tw, start, ok)])[4][0]
    use = np.flatnonzero(pr["source"])
    assert len(use) > 5
    s = st[ppos[use]]
    for k, name in (("X", "swx"), ("Y", "swy"), ("Z", "swz")):
        assert (pr[k][use] == s[name] / s["sw"]).all()


@pytest.mark.gpu
def test_child_checking_build(pkg, gpu):
    """The stateless cases once more on libviso_hip_check.so (-DVH_CHECK)."""
    assert os.path.exists(pkg.CHECK_LIB_PATH), "build() makes it"
    env = dict(os.environ, VISO_HIP_LIB=pkg.CHECK_LIB_PATH)
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-q", "-x", "-m", "gpu", "-k", "stateless_parity"],
                       env=env, capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "2 passed" in r.stdout and " skipped" not in r.stdout, r.stdout[-2000:]
    assert "VH_CHECK" not in r.stderr


# ------------------------------------------------------------------------------------------------------------ GPU, handles
@pytest.mark.gpu
def test_gpu_group_of_three_and_lone_matcher(pkg, ob, gpu):
    """A group of 3 streams over 5 steps of match, estimate, inliers, this refit (reclassify), trajectory, scenePointsWorld,
    landmarks: step 1 equals refitMotion with n_used = 0; later steps use landmarks and equal the stateless entry fed from
    getInlierMatches, getTracks, the previous step's states and the poses, byte for byte, Tw_prev given and NULL alike; a
    re-matched pair repeats its bytes; a step without a landmarks call breaks the chain (n_used = 0).  A lone matcher
    equals stream 0 of a group of one."""
    fr, dims = pd.frames_of(pkg), pd.dims_of(pkg)
    e = pd.ego_of(pkg)
    S = pd.S
    rp = ext(pkg).LandmarkRefitParams.default(min_obs=1)
    lp = pkg.LandmarkParams.default(min_obs=1)
    g = pkg.StreamGroup(S, pkg.Params.default())
    g.setTrackLinking(True); g.setTrajectory()
    g.profileEnable(True)
    state, used_total, n_calls = None, 0, 0
    for t in range(6):
        pd.push(g, fr, t, dims)
        if t == 0:
            continue
        g.matchFeatures(QUAD)
        tr0, ok0, _ = g.estimateMotion(e, mi.rand3_of(ob, e, S))
        g.motionInliers(e, tr0, ok0.astype(np.int32))
        lists = [g.getInlierMatches(s) for s in range(S)]
        tracks = [g.getTracks(s) for s in range(S)]
        plain = g.refitMotion(e, reclassify=False)
        got = ext(pkg).groupRefitMotionLandmarks(g, e, rp); n_calls += 1                      # Tw_prev NULL: the trajectory's
        priors = [ext(pkg).getRefitPriors(g, s) for s in range(S)]
        Tw_prev = np.stack([np.eye(4)] * S) if t == 1 else poses["Tw_cur"]
        given = ext(pkg).groupRefitMotionLandmarks(g, e, rp, Tw_prev); n_calls += 1
        for a, b in zip(got, given):
            assert np.asarray(a).tobytes() == np.asarray(b).tobytes(), t
        assert all(a.tobytes() == ext(pkg).getRefitPriors(g, s).tobytes() for s, a in enumerate(priors))
        for s in range(S):
            pm, src = lists[s]
            want = ext(pkg).refit_motion_landmarks(e, [pm], [tracks[s]["prev"][src]], None if state is None else [state[s]], Tw_prev[s], tr0[s][None],
                                              [int(ok0[s])], rp)
            assert got[0][s].tobytes() == want[0][0].tobytes() and got[1][s] == want[1][0] and got[2][s] == want[2][0], (t, s)
            assert got[3][s] == want[3][0] and priors[s].tobytes() == want[4][0].tobytes() and len(priors[s]) == len(pm), (t, s)
        if state is None:                                                       # no states: refitMotion's bytes
            assert not got[3].any() and got[0].tobytes() == plain[0].tobytes() and np.array_equal(got[2], plain[2])
        else:
            used_total += int(got[3].sum())
        final = ext(pkg).groupRefitMotionLandmarks(g, e, rp, reclassify=True); n_calls += 1
        assert final[0].tobytes() == got[0].tobytes() and np.array_equal(final[4], g.motionInliers(e, final[0], final[1].astype(np.int32)))
        poses = g.trajectory()
        g.scenePointsWorld(e)
        if t == 3:                                                              # no landmarks call: the chain of states breaks
            state = None
            continue
        tracks = [g.getTracks(s) for s in range(S)]
        points = [g.getScenePoints(s) for s in range(S)]
        g.landmarks(lp)
        state = pkg.landmarks_update(tracks, points, state, lp)[1]
        if t == 5:                                                              # the pair matched again: the same bytes
            g.matchFeatures(QUAD)
            g.motionInliers(e, tr0, ok0.astype(np.int32))
            again = ext(pkg).groupRefitMotionLandmarks(g, e, rp, Tw_prev)
            assert all(np.asarray(a).tobytes() == np.asarray(b).tobytes() for a, b in zip(again, got))
    g.synchronize()
    assert used_total > 0
    assert g.profileRead("refit_prior")[1] == n_calls + 1 and g.profileRead("refit_prior_fit")[1] == n_calls + 1
    g.close()
    frames = sr.frames_of(pkg, 4, 91)
    e = mi.hego(pkg, inlier_threshold=2.5)
    g1 = pkg.StreamGroup(1, pkg.Params.default()); g1.setTrackLinking(True); g1.setTrajectory()
    m = pkg.Matcher(pkg.Params.default(), outlier_removal=False); m.setTrackLinking(True); m.setTrajectory()
    used = 0
    for t, (left, right) in enumerate(frames):
        g1.pushBack(left[None], right[None], sr.dims_of(pkg)); m.pushBack(left, right, sr.dims_of(pkg))
        if t == 0:
            continue
        g1.matchFeatures(QUAD); g1.motionInliers(e, np.array([mi.TR2]), np.ones(1, np.int32))
        m.matchFeatures(QUAD); m.motionInliers(e, mi.TR2)
        if t == 1:                                                              # no states yet: refitMotion's bytes
            plain = m.refitMotion(e)
            first = ext(pkg).matchRefitMotionLandmarks(m, e, rp)
            assert first[0].tobytes() == plain[0].tobytes() and first[1:3] == plain[1:3] and first[3] == 0 and first[4] == plain[3]
        a = ext(pkg).groupRefitMotionLandmarks(g1, e, rp, reclassify=True)
        b = ext(pkg).matchRefitMotionLandmarks(m, e, rp, reclassify=True)
        assert a[0][0].tobytes() == b[0].tobytes() and (bool(a[1][0]), int(a[2][0]), int(a[3][0]), int(a[4][0])) == b[1:], t
        assert ext(pkg).getRefitPriors(g1, 0).tobytes() == ext(pkg).getRefitPriors(m).tobytes()
        assert t == 1 or b[3] > 0, t
        used += b[3]
        g1.trajectory(); g1.scenePointsWorld(e); g1.landmarks(lp)
        m.trajectory(); m.scenePointsWorld(e); m.landmarks(lp)
    assert used > 0
    g1.close(); m.close()


@pytest.mark.gpu
def test_gpu_state_rules_memory_and_failed_allocation(pkg, gpu):
    """VH_ERR_UNSUPPORTED on a sequence handle, ahead of a null argument; VH_ERR_STATE before a classification, with track
    linking off, where the classification read a host-replaced list (a Matcher with outlier removal), on flow lists and
    under a mono classification (quad and flow), with Tw_prev NULL and the trajectory off, after the next push, and from getRefitPriors before a call and after the next match; the
    block is counted to the byte; a refused allocation is VH_ERR_HIP before any launch and the repeated call succeeds."""
    dims = sr.dims_of(pkg)
    frames = [sr.frames_of(pkg, 3, seed) for seed in (85, 86)]
    e = mi.hego(pkg, inlier_threshold=2.5)
    rp = ext(pkg).LandmarkRefitParams.default()
    state = pkg.VH_ERR_STATE
    S, MM = 2, 4096
    push = lambda g, t: g.pushBack(np.stack([f[t][0] for f in frames]), np.stack([f[t][1] for f in frames]), dims)  # noqa: E731
    classify = lambda g: (g.matchFeatures(QUAD), g.motionInliers(e, np.array([mi.TR2] * S), np.ones(S, np.int32)))  # noqa: E731
    sq = pkg.SequenceGroup(4, pkg.Params.default()); sq.setTrackLinking(True)
    expect(pkg, pkg.VH_ERR_UNSUPPORTED, lambda: ext(pkg).groupRefitMotionLandmarks(sq, e, rp, np.eye(4)))
    out = np.zeros(4 * 6); cnt = np.zeros(4, np.int32)                        # checked first: before a null argument
    assert ext(pkg)._lib().vh_group_refit_motion_landmarks(sq._h, None, None, None, 0, ptr(out), ptr(cnt), ptr(cnt), ptr(cnt), ptr(cnt)) == pkg.VH_ERR_UNSUPPORTED
    sq.close()
    # where the classification read a list replaced on the host: its positions are not the tracked list's
    m = pkg.Matcher(pkg.Params.default(), outlier_removal=True); m.setTrackLinking(True)
    for t in range(2):
        m.pushBack(frames[0][t][0], frames[0][t][1], dims)
    m.matchFeatures(QUAD)
    assert m.motionInliers(e, mi.TR2) > 6
    m.refitMotion(e)                                                          # (the plain refit takes such a list)
    expect(pkg, state, lambda: ext(pkg).matchRefitMotionLandmarks(m, e, rp, np.eye(4)))
    m.close()
    # the cases inherited from refitMotion, with linking on and a tracked list: flow lists, a mono classification
    q = pkg.StreamGroup(S, pkg.Params.default(), max_matches=MM); q.setTrackLinking(True)
    push(q, 0); push(q, 1)
    model = np.zeros(S, pkg.MONO_MODEL_DTYPE)
    mono = pkg.MonoParams.default(f=mi.HCAL["f"], cu=mi.HCAL["cu"], cv=mi.HCAL["cv"])
    call = lambda: ext(pkg).groupRefitMotionLandmarks(q, e, rp, np.eye(4))  # noqa: E731
    q.matchFeatures(mr.FLOW)
    q.motionInliersMono(mono, model, np.zeros(S, np.int32))
    expect(pkg, state, call)                                                  # flow lists under a mono classification
    q.matchFeatures(QUAD)
    q.motionInliersMono(mono, model, np.zeros(S, np.int32))
    assert len(q.getTracks(0)) == len(q.getMatches(0))                        # (a tracked list of the current pair exists)
    expect(pkg, state, call)                                                  # a mono classification of quad lists
    q.motionInliers(e, np.array([mi.TR2] * S), np.ones(S, np.int32))
    assert not call()[3].any()                                                # ... and the stereo one is taken
    q.close()
    off = pkg.StreamGroup(S, pkg.Params.default(), max_matches=MM)            # linking off
    push(off, 0); push(off, 1); classify(off)
    expect(pkg, state, lambda: ext(pkg).groupRefitMotionLandmarks(off, e, rp, np.eye(4)))
    off.close()
    g = pkg.StreamGroup(S, pkg.Params.default(), max_matches=MM)
    g.setTrackLinking(True)
    g.profileEnable(True)
    expect(pkg, state, lambda: ext(pkg).groupRefitMotionLandmarks(g, e, rp, np.eye(4)))       # nothing pushed
    push(g, 0); push(g, 1)
    g.matchFeatures(QUAD)
    expect(pkg, state, lambda: ext(pkg).groupRefitMotionLandmarks(g, e, rp, np.eye(4)))       # no classification
    classify(g)
    expect(pkg, state, lambda: ext(pkg).groupRefitMotionLandmarks(g, e, rp))                  # Tw_prev NULL, the trajectory off
    expect(pkg, state, lambda: ext(pkg).getRefitPriors(g, 0))
    expect(pkg, pkg.VH_ERR_INVALID_ARG, lambda: ext(pkg).groupRefitMotionLandmarks(g, e, ext(pkg).LandmarkRefitParams.default(min_obs=0), np.eye(4)))
    g.synchronize()
    bytes0 = g.deviceBytes()
    g.debugFailNextAlloc()
    expect(pkg, pkg.VH_ERR_HIP, lambda: ext(pkg).groupRefitMotionLandmarks(g, e, rp, np.eye(4)))
    g.synchronize()
    assert g.deviceBytes() == bytes0 and g.profileRead("refit_prior")[1] == 0
    plain = g.refitMotion(e)
    bytes1 = g.deviceBytes()
    got = ext(pkg).groupRefitMotionLandmarks(g, e, rp, np.eye(4))
    assert got[0].tobytes() == plain[0].tobytes() and not got[3].any()
    _, _, _, stride = g.inliersDevice()
    up = lambda b: (b + 255) // 256 * 256  # noqa: E731
    block = up(32 * S * stride) + up(128 * S) + up(4 * S) + up(48 * S) + 2 * up(4 * S)
    assert g.deviceBytes() == bytes1 + block, (g.deviceBytes() - bytes1, block)
    ext(pkg).groupRefitMotionLandmarks(g, e, rp, np.eye(4))
    g.synchronize()
    assert g.deviceBytes() == bytes1 + block and g.profileRead("refit_prior")[1] == 2 == g.profileRead("refit_prior_fit")[1]
    assert len(ext(pkg).getRefitPriors(g, 1)) == len(g.getInlierMatches(1)[0])
    push(g, 2)
    expect(pkg, state, lambda: ext(pkg).groupRefitMotionLandmarks(g, e, rp, np.eye(4)))       # pushed: the pair the lists belong to is over
    g.matchFeatures(QUAD)
    expect(pkg, state, lambda: ext(pkg).getRefitPriors(g, 0))                            # the priors end with the next match
    g.close()


# ------------------------------------------------------------------------------------------------------------ GPU, poisoned
@pytest.mark.gpu
def test_gpu_edges_on_fresh_buffers(pkg, ob, oracle, gpu):
    """The cases a stale buffer would hide: the empty list, ok_in = 0, the shortest lists, a short call behind a long one --
    every output compared with the restatement (run once more by the child below on poisoned buffers)."""
    want = expectation(oracle, ob, 1)["main"]
    main = calls(oracle, ob)[0][2]
    for idx in ([12], [0, 1, 2, 3], [6], [2]):
        check_call(run_call(pkg, 1, {}, [main[k] for k in idx]), [want[k] for k in idx], idx)


@pytest.mark.gpu
def test_gpu_child_on_poisoned_buffers(gpu):
    """DESIGN.md section 4.0's rule for new output arrays: ONE child process with VH_POISON=1 runs this file's edge cases on
    buffers that start as 0xA5 bytes."""
    cmd = [sys.executable, "-m", "pytest", os.path.abspath(__file__), "-q", "-x", "-m", "gpu", "-k", "edges_on_fresh"]
    r = subprocess.run(cmd, env=dict(os.environ, VH_POISON="1"), capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    assert "1 passed" in r.stdout and " skipped" not in r.stdout, r.stdout[-2000:]
