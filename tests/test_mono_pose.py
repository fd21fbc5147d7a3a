"""The mono pose on whole lists: vh_pose_mono, vh_group_pose_mono, vh_match_pose_mono -- the rest
of VisualOdometryMono::estimateMotion after the refit (reference src/viso_mono.cpp:83-158) over every record of whole
lists, under the model the lists were classified under.  The contract is restated in tests/mono_pose_oracle.py.

The GPU bound.  R, t and median are restated operation for operation with contraction off and use no function of the
device library: expected bit-equal.  tr, scale and plane pass through the device's sin / cos (d), exp (the vote's sums,
which only pick the plane) and asin: rtol 1e-9, atol 1e-12, the project's bound for this arithmetic (tests/test_mono.py).
The input condition: the restatement's vote margin is at least MARGIN_FLOOR on every list that reaches the vote (the
seeds are chosen so; the smallest over the lists below is 2.9e-6, at 1 300 records); the tolerance is not loosened to admit a tie.

Measured on the CPU (test_restatement_noisy_dense_against_bucketed prints them), 0.3 px noise, 2 000 records: the bucketed
estimator's pose is (2.3e-4 rad, 0.036 m) from the truth, the pose of the refit model over the 1 859 dense inliers
(2.3e-4 rad, 0.043 m)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import mono_inlier_oracle as mo
import mono_pose_oracle as mp
import mono_refit_oracle as mr
import test_mono_inliers as tm    # its helpers: hmono, rand8_of, restated_model
import test_motion_inliers as ti  # its helpers: the stereo scene of the handle tests
import test_sequence_recon as sr  # its helpers: the synthetic frames, expect()
from conftest import ROOT

SYMBOLS = ("vh_pose_mono", "vh_group_pose_mono", "vh_match_pose_mono")
SCOPES = ("mono_pose_head", "mono_pose_tri", "mono_pose_front", "mono_pose_rank", "mono_pose_vote", "mono_pose_finish")
FIELDS = ("R", "t", "scale", "median", "plane", "chirality", "candidate", "n_front", "reason", "reserved_")
OFFSETS = (0, 72, 96, 104, 112, 120, 136, 140, 144, 148)
FLOW, QUAD, STEREO = sr.FLOW, sr.QUAD, sr.STEREO
MARGIN_FLOOR = 1e-6
ROT_TOL, TRANS_TOL = 0.003, 0.15   # tests/test_mono.py: the scale comes from the road plane, looser
# one lane short of a wave, one over, one short of a workgroup trip, one over, more than two LDS tiles of 512 elements
LENGTHS = {9: 300, 10: 300, 11: 300, 63: 305, 64: 304, 65: 305, 255: 306, 256: 383, 257: 309, 600: 313, 1300: 305}   # length -> seed
ptr, expect = sr.ptr, sr.expect
_CACHE = {}


def dtype():
    return ti._parity_dtype()


def params(mod, **kw):
    return tm.mono_params(mod, **{**dict(pitch=mp.PITCH), **kw})


@pytest.fixture(autouse=True)
def entries(pkg):
    """Every test here is about the pose entries, the restatement's own included (it is their yardstick): without them in
    the library's ABI none of it passes."""
    assert all(name in pkg.ABI_SYMBOLS and hasattr(pkg._lib(), name) for name in SYMBOLS)


def true_model(pm, tr=mr.MOTION):
    """The list's own normalisation and the true F in that frame."""
    nrm = mo.normalise(pm)
    return dict(c=nrm[0], s=nrm[1], F=mr.normalised_F(mr.true_F(tr), nrm[0], nrm[1]), valid=1.0)


SLOW = tuple(mr.MOTION[:3]) + tuple(0.05 * np.array(mr.MOTION[3:]))   # a twentieth of the translation: depths of hundreds of baselines


def lists():
    """name -> (pm, model, ok_in): a list per length, and the refused ones."""
    if "lists" not in _CACHE:
        out = {}
        for n, seed in LENGTHS.items():
            pm = mp.ground_scene(dtype(), n, seed)
            out[n] = (pm, true_model(pm) if n >= 10 else true_model(mp.ground_scene(dtype(), 64, seed)), 1)
        pm = mp.ground_scene(dtype(), 64, 200)
        out["ok0"] = (pm, dict(c=np.full(4, np.nan), s=np.full(2, np.inf), F=np.full(9, np.nan), valid=0.0), 0)     # reason 1
        out["nanF"] = (pm, dict(true_model(pm), F=np.full(9, np.nan)), 1)                                            # reason 3: no candidate counts a point
        pm = mp.ground_scene(dtype(), 14, 400, swapped=7)
        out["behind"] = (pm, true_model(pm), 1)                                                                      # reason 4: 8 points in front
        pm = mp.ground_scene(dtype(), 64, 402, noise=0.0, tr=SLOW)
        out["slow"] = (pm, true_model(pm, SLOW), 1)                                                                  # reason 5
        pm = mp.ground_scene(dtype(), 255, 441)
        model = true_model(pm)
        pm["v1c"][131] = np.nan
        out["nanrec"] = (pm, model, 1)       # a NaN record is in front of no camera: the pose of the other 254
        _CACHE["lists"] = out
    return _CACHE["lists"]


def expectation(ob, oracle):
    if "want" not in _CACHE:
        e = params(ob)
        _CACHE["want"] = {k: mp.pose(oracle.svd, pm, m, e, ok=bool(ok)) for k, (pm, m, ok) in lists().items()}
    return _CACHE["want"]


# ------------------------------------------------------------------------------------------------------------ CPU
def test_symbols_layout_and_argument_errors(pkg, tmp_path):
    """Every new symbol is declared, exported and mirrored; vh_abi_version stays 1; vh_mono_pose is 152 bytes with the
    header's offsets in the C compiler's layout and in the numpy mirror; n_sets = 0 and lists without records are VH_OK
    without a device; null and negative arguments are VH_ERR_INVALID_ARG."""
    header = open(os.path.join(ROOT, "include", "viso_hip.h")).read()
    lib = pkg._lib()
    for name in SYMBOLS:
        assert name + "(" in header and hasattr(C.CDLL(pkg.LIB_PATH), name) and name in pkg.ABI_SYMBOLS, name
    assert all(s in header for s in SCOPES)
    assert pkg.abi_version() == 1
    assert callable(pkg.pose_mono) and "poseMono" in vars(pkg.Matcher)
    assert "poseMono" in vars(pkg.StreamGroup) and hasattr(pkg.SequenceGroup, "poseMono")
    dt = pkg.MONO_POSE_DTYPE
    assert dt.names == FIELDS and dt.itemsize == 152 and tuple(dt.fields[n][1] for n in FIELDS) == OFFSETS
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "viso_hip.h"\nint main(void) {\n  printf("%zu", sizeof(vh_mono_pose));\n'
                   + "".join(f'  printf(" %zu", offsetof(vh_mono_pose, {n}));\n' for n in FIELDS) + '  return 0;\n}\n')
    exe = str(tmp_path / "layout")
    subprocess.check_call(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), str(src), "-o", exe])
    assert [int(v) for v in subprocess.check_output([exe], timeout=60).decode().split()] == [152] + list(OFFSETS)
    e = params(pkg)
    pm = np.zeros(12, pkg.P_MATCH_DTYPE)
    off = np.array([0, 12], np.int32)
    model = np.zeros(1, pkg.MONO_MODEL_DTYPE); ok = np.ones(1, np.int32)
    tr = np.full((1, 6), 7.0); okout = np.full(1, 7, np.int32); pose = np.zeros(1, dt)
    inv = pkg.VH_ERR_INVALID_ARG
    call = lib.vh_pose_mono
    assert call(C.byref(e), 0, 0, None, None, None, None, None, None, None) == pkg.VH_OK
    empty = np.array([3, 3, 3], np.int32)
    tr2 = np.full((2, 6), 7.0); ok2 = np.full(2, 7, np.int32); p2 = np.zeros(2, dt); p2["scale"] = 5
    assert call(C.byref(e), 0, 2, None, ptr(empty), ptr(np.zeros(2, pkg.MONO_MODEL_DTYPE)), ptr(np.array([1, 0], np.int32)), ptr(tr2), ptr(ok2), ptr(p2)) == pkg.VH_OK
    assert ok2.tolist() == [0, 0] and not tr2.any() and p2["reason"].tolist() == [2, 1] and p2["candidate"].tolist() == [-1, -1]
    assert not p2["scale"].any() and not p2["R"].any() and not p2["chirality"].any()
    assert pkg.pose_mono(e, [], [], [])[1].shape == (0,)
    good = [C.byref(e), 0, 1, ptr(pm), ptr(off), ptr(model), ptr(ok), ptr(tr), ptr(okout), ptr(pose)]
    for k in (0, 3, 4, 5, 6, 7, 8):     # (the pose output is optional)
        assert call(*[None if j == k else a for j, a in enumerate(good)]) == inv, k
    assert call(C.byref(e), 0, -1, *good[3:]) == inv
    assert call(*good[:4], ptr(np.array([12, 0], np.int32)), *good[5:]) == inv
    assert call(*good[:4], ptr(np.array([-1, 3], np.int32)), *good[5:]) == inv
    n = np.zeros(1, np.int32)
    assert lib.vh_group_pose_mono(None, C.byref(e), ptr(tr), ptr(okout), ptr(pose), ptr(n)) == inv
    assert lib.vh_match_pose_mono(None, C.byref(e), ptr(tr), ptr(okout), ptr(pose)) == inv


def bucketed(ob, oracle):
    """A bucketed list of 200 records of a noisy scene of 2 000, the pinned estimator's result and model for it."""
    if "bucketed" not in _CACHE:
        pm = mp.ground_scene(dtype(), 2000, 11)
        rng = np.random.default_rng(12)
        few = pm[np.sort(rng.permutation(2000)[:200])]
        e = params(ob)
        ok, tr, inl = oracle.estimate_motion_mono(e, few, oracle.draw_samples_n(len(few), 8, e.ransac_iters))
        _CACHE["bucketed"] = (pm, few, bool(ok), np.array(tr), mo.model_of(oracle.svd, few, inl))
    return _CACHE["bucketed"]


def test_restatement_is_the_pinned_estimators_tail(ob, oracle):
    """On a bucketed list with the pinned estimator's model for it (the refit over its inlier set), the restatement's ok and
    tr are the pinned estimator's: bit for bit on the CPU (both use the C library's exp / asin / cos); the project's bound
    rtol 1e-9, atol 1e-12 is asserted first.  The same on a noise-free list and on one the estimator refuses."""
    _, few, ok, tr, model = bucketed(ob, oracle)
    e = params(ob)
    got = mp.pose(oracle.svd, few, model, e)
    assert ok and got["ok"] and got["reason"] == 0
    assert np.allclose(got["tr"], tr, rtol=1e-9, atol=1e-12)
    assert got["tr"].tobytes() == tr.tobytes()
    for pm in (mp.ground_scene(dtype(), 300, 5, noise=0.0), mp.ground_scene(dtype(), 64, 402, noise=0.0, tr=SLOW)):
        ok, tr, inl = oracle.estimate_motion_mono(e, pm, oracle.draw_samples_n(len(pm), 8, e.ransac_iters))
        got = mp.pose(oracle.svd, pm, mo.model_of(oracle.svd, pm, inl), e)
        assert bool(ok) == got["ok"] and got["tr"].tobytes() == np.array(tr).tobytes(), (ok, got["reason"])


def test_restatement_recovers_the_truth_without_noise(ob, oracle):
    """A ground plane 1.65 m below a camera pitched by -0.03 rad plus general points at 5 .. 50 m, forward-plus-sideways
    translation and a small rotation, exact projections rounded to float, the true F: the restatement's tr is the motion
    within the tolerances tests/test_mono.py holds its scene to, every point is in front under the winner alone."""
    e = params(ob)
    for n, seed in ((500, 1), (2000, 2), (40, 3)):
        pm = mp.ground_scene(dtype(), n, seed, noise=0.0)
        got = mp.pose(oracle.svd, pm, true_model(pm), e)
        rot, trans = mp.distance_to_truth(got["tr"])
        print(f"n = {n}: rotation {rot:.3e}, translation {trans:.3e}, margin {got['margin']:.3e}")
        assert got["ok"] and rot <= ROT_TOL and trans <= TRANS_TOL
        assert got["n_front"] == n and got["chirality"][got["candidate"]] == n and got["chirality"].sum() == n
        assert abs(np.linalg.norm(got["t"]) - 1) < 1e-12 and abs(got["scale"] * got["plane"] - e.height) < 1e-12


def test_restatement_noisy_dense_against_bucketed(ob, oracle):
    """0.3 px noise, 2 000 records: the pose from the refit model over the dense inliers and the bucketed estimator's pose,
    each one's distance to the truth (printed; measured: bucketed 2.3e-4 rad / 0.036 m, dense 2.3e-4 rad / 0.043 m -- the
    scale is the ground-plane vote's in both, and it dominates).  Asserted: both within the noise-free tolerances."""
    pm, few, ok, tr_b, model = bucketed(ob, oracle)
    e = params(ob)
    flags, _ = mo.inliers(pm, model, tm.THR)
    refined, ok_r, _ = mr.refit(oracle.svd, pm[flags == 1], model)
    assert ok and ok_r
    flags2, _ = mo.inliers(pm, refined, tm.THR)
    got = mp.pose(oracle.svd, pm[flags2 == 1], refined, e)
    assert got["ok"]
    d_b, d_d = mp.distance_to_truth(tr_b), mp.distance_to_truth(got["tr"])
    print(f"bucketed ({len(few)} records): rotation {d_b[0]:.3e}, translation {d_b[1]:.3e}; dense ({int(flags2.sum())} inliers): "
          f"rotation {d_d[0]:.3e}, translation {d_d[1]:.3e}")
    assert d_b[0] <= ROT_TOL and d_b[1] <= TRANS_TOL and d_d[0] <= ROT_TOL and d_d[1] <= TRANS_TOL


def test_device_functions_on_the_host_equal_the_restatement(tmp_path, ob, oracle):
    """csrc/vh_mono_pose.h compiled for the host with -ffp-contract=off: E, the candidates and the projection matrices are
    the restatement's byte for byte, the triangulated direction of every record under every candidate byte for byte up to
    its sign (the device takes it without U); a NaN record gives a NaN w."""
    exe = str(tmp_path / "mono_pose_check")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", os.path.join(ROOT, "tests", "cpp", "mono_pose_check.cpp"), "-lm", "-o", exe])
    dt = np.dtype([("c", "<f8", (4,)), ("s", "<f8", (2,)), ("F", "<f8", (9,)), ("valid", "<f8")])
    e = params(ob)
    for k in (10, 65, 257, "behind", "slow", "nanrec"):
        pm, model, _ = lists()[k]
        fin, fout = str(tmp_path / f"in{k}"), str(tmp_path / f"out{k}")
        with open(fin, "wb") as fh:
            fh.write(mo.as_array([model], dt).tobytes()); fh.write(np.array([e.f, e.cu, e.cv]).tobytes())
            fh.write(np.int64(len(pm)).tobytes()); fh.write(pm.tobytes())
        subprocess.check_call([exe, fin, fout], timeout=60)
        got = np.fromfile(fout, np.float64)
        parts = {}
        mp.pose(oracle.svd, pm, model, e, parts=parts)
        head = np.concatenate([parts["E"].reshape(9), parts["Ra"].reshape(9), parts["Rb"].reshape(9), parts["t0"], parts["P1"].reshape(12), parts["P2"].reshape(48)])
        assert got[:90].tobytes() == head.tobytes(), k
        X = got[90:].reshape(4, len(pm), 4)
        for c in range(4):
            want = parts["X"][c]
            bad = np.isnan(want[:, 3])
            assert np.isnan(X[c][bad, 3]).all() and bad.sum() == (1 if k == "nanrec" else 0), (k, c)
            same = [X[c][i].tobytes() == want[i].tobytes() or (-X[c][i]).tobytes() == want[i].tobytes() for i in np.nonzero(~bad)[0]]
            assert all(same), (k, c, int(np.sum(same)), len(same))


# ------------------------------------------------------------------------------------------------------------ GPU
def pose_bytes(res, k):
    return res[0][k].tobytes() + bytes([int(res[1][k])]) + res[2][k].tobytes()


def check_list(name, want, tr, ok, pose, what):
    """One list's device result against the restatement."""
    assert bool(ok) == want["ok"] and pose["reason"] == want["reason"], (what, pose["reason"], want["reason"])
    assert pose["candidate"] == want["candidate"] and pose["n_front"] == want["n_front"] and pose["reserved_"] == 0, what
    assert np.array_equal(pose["chirality"], want["chirality"]), (what, pose["chirality"], want["chirality"])
    assert pose["R"].tobytes() == np.asarray(want["R"], np.float64).tobytes(), (what, pose["R"], want["R"])
    assert pose["t"].tobytes() == np.asarray(want["t"], np.float64).tobytes(), (what, pose["t"], want["t"])
    assert np.float64(pose["median"]).tobytes() == np.float64(want["median"]).tobytes(), (what, pose["median"], want["median"])
    if want["margin"] is not None:
        assert want["margin"] >= MARGIN_FLOOR, (what, want["margin"])
    for got, ref in ((tr, want["tr"]), (pose["scale"], want["scale"]), (pose["plane"], want["plane"])):
        assert np.allclose(got, ref, rtol=1e-9, atol=1e-12), (what, got, ref)
    if not ok:
        assert not tr.any(), what
    return tr.tobytes() == want["tr"].tobytes() and float(pose["plane"]) == want["plane"]


def call_stateless(pkg, names, **kw):
    L = lists()
    return pkg.pose_mono(params(pkg, **kw), [L[k][0] for k in names], mo.as_array([L[k][1] for k in names], pkg.MONO_MODEL_DTYPE), [L[k][2] for k in names])


GROUPS = ((9, 1300, "ok0", 65, 10, "nanF"), (600, "behind", 63, 256, "slow"), (257, 64, "nanrec", 255, 1300, 11))


@pytest.mark.gpu
def test_gpu_stateless(pkg, ob, oracle, gpu):
    """vh_pose_mono on lists of 9 .. 1 300 records and on the refused ones (reasons 1, 2, 3, 4, 5 and a list with a NaN
    record), one list per call and in three calls of mixed lists: integers equal to the restatement's, R, t, median bit for
    bit, tr / scale / plane within rtol 1e-9; the same bytes alone, among other lists and from two runs.  Reason 6 needs a
    plane coordinate below 1e-20 to win the vote: no input without contortion, not tested.  Reason 7 on its own: below."""
    want = expectation(ob, oracle)
    alone = {}
    exact = []
    for k in lists():
        res = call_stateless(pkg, [k])
        assert pose_bytes(res, 0) == pose_bytes(call_stateless(pkg, [k]), 0), k
        exact.append(check_list(k, want[k], res[0][0], res[1][0], res[2][0], f"alone {k}"))
        alone[k] = res
    assert [want[k]["reason"] for k in (9, "ok0", "nanF", "behind", "slow", "nanrec")] == [2, 1, 3, 4, 5, 0]
    assert all(want[n]["ok"] for n in LENGTHS if n >= 10)
    for names in GROUPS:
        res = call_stateless(pkg, names)
        again = call_stateless(pkg, names)
        for j, k in enumerate(names):
            assert pose_bytes(res, j) == pose_bytes(again, j), (names, k)
            assert pose_bytes(res, j) == pose_bytes(alone[k], 0), (names, k)      # a refused neighbour changes nothing
    print(f"tr and plane bit-equal to the restatement on {sum(exact)} of {len(exact)} lists")
    # the NaN record counts for nothing: the pose of the list without it
    pm, m, _ = lists()["nanrec"]
    rest = pkg.pose_mono(params(pkg), [np.delete(pm, 131)], mo.as_array([m], pkg.MONO_MODEL_DTYPE), [1])
    assert pose_bytes(rest, 0) == pose_bytes(alone["nanrec"], 0)
    # ransac_iters and inlier_threshold are not read; pose = NULL gives the same tr
    assert pose_bytes(call_stateless(pkg, [257], ransac_iters=1, inlier_threshold=9.0), 0) == pose_bytes(alone[257], 0)


@pytest.mark.gpu
def test_gpu_reason_7(pkg, ob, oracle, gpu):
    """A non-finite tr: with an infinite camera height every list that reaches the end has reason 7, ok = 0, tr = 0, the
    fields as computed (scale infinite); the lists refused earlier keep their reasons.  (The parameters belong to the call:
    such a list cannot sit among good ones.)"""
    names = (64, "slow", 257, 9)
    res = call_stateless(pkg, names, height=np.inf)
    e = params(ob, height=np.inf)
    for j, k in enumerate(names):
        pm, m, ok = lists()[k]
        want = mp.pose(oracle.svd, pm, m, e, ok=bool(ok))
        check_list(k, want, res[0][j], res[1][j], res[2][j], f"height inf {k}")
    assert res[2]["reason"].tolist() == [7, 5, 7, 2] and np.isinf(res[2]["scale"][0]) and not res[0].any()


@pytest.mark.gpu
def test_gpu_tie_to_the_estimator(pkg, ob, oracle, gpu):
    """pose_mono on a bucketed list with the model estimate_motion_mono(model=True) returned for it: that call's tr and ok
    (rtol 1e-9; printed: whether bit for bit) and the restatement's winner."""
    _, few, ok_w, tr_w, _ = bucketed(ob, oracle)
    e = params(pkg)
    tr, ok, inl, models = pkg.estimate_motion_mono(e, [few], tm.rand8_of(ob, e, 1), model=True)
    assert ok[0] and ok_w and np.allclose(tr[0], tr_w, rtol=1e-9, atol=1e-12)
    got = pkg.pose_mono(e, [few], models, [1])
    want = mp.pose(oracle.svd, few, mo.from_array(models[0]), params(ob))
    assert got[1][0] and np.allclose(got[0][0], tr[0], rtol=1e-9, atol=0) and got[2][0]["candidate"] == want["candidate"]
    assert want["margin"] >= MARGIN_FLOOR
    print(f"pose_mono against the estimator's own tail: bit-equal = {got[0][0].tobytes() == tr[0].tobytes()}")


def pose_path(pkg, ob, g, what, rows=None):
    """estimateMotionMono(model=True) -> motionInliersMono -> refitModelMono(reclassify) -> poseMono on a group's current
    lists: every stream equals the stateless form on the lists the inlier getters return, byte for byte."""
    e = tm.hmono(pkg, inlier_threshold=3e-5)
    S = g.S
    _, _, _, models = g.estimateMotionMono(e, tm.rand8_of(ob, e, S), model=True)
    ok0 = models["valid"].astype(np.int32)
    g.motionInliersMono(e, models, ok0)
    seen = []
    for refit in (False, True):
        if refit:
            models, okr, _, counts = g.refitModelMono(e, reclassify=True)
            ok0 = okr.astype(np.int32)
        inl = [g.getInlierMatches(s)[0] for s in range(S)]
        tr, ok, counts, pose = g.poseMono(e, pose=True)
        want = pkg.pose_mono(e, inl, models, ok0)
        assert np.array_equal(counts, [len(x) for x in inl]), what
        for s in range(S):
            assert pose_bytes((tr, ok, pose), s) == pose_bytes(want, s), (what, refit, s, pose[s], want[2][s])
        tr2, ok2, _ = g.poseMono(e)                      # pose = NULL: the same tr
        assert tr2.tobytes() == tr.tobytes() and np.array_equal(ok2, ok)
        assert all(g.getInlierMatches(s)[0].tobytes() == inl[s].tobytes() for s in range(S)), what   # the classification is untouched
        seen.append(pose["reason"].tolist())
        if rows is not None:   # a sequence handle: rows without a pair hold nothing
            assert all(pose["reason"][r] in (1, 2) and not tr[r].any() for r in range(S) if r not in rows), (what, pose["reason"], rows)
    print(f"{what}: reasons {seen}")
    return seen


@pytest.mark.gpu
@pytest.mark.parametrize("method", [FLOW, QUAD])
def test_gpu_group_of_three(method, pkg, ob, gpu):
    """A plain group of S = 3 (one stream of constant images: empty lists) on flow and on quad lists."""
    dims = sr.dims_of(pkg)
    frames = [sr.frames_of(pkg, 3, seed) for seed in (81, 82, 83)]
    frames[1] = [(np.full_like(a, 90), np.full_like(b, 90)) for a, b in frames[1]]
    g = pkg.StreamGroup(3, pkg.Params.default())
    for t in range(3):
        g.pushBack(np.stack([f[t][0] for f in frames]), np.stack([f[t][1] for f in frames]) if method == QUAD else None, dims)
        if t == 0:
            continue
        g.matchFeatures(method)
        seen = pose_path(pkg, ob, g, f"group m{method} t{t}")
        assert all(r[1] in (1, 2) for r in seen)
        assert any(r[0] not in (1, 2) for r in seen)      # a stream with images gets past the refusals that need no record
    g.close()


@pytest.mark.gpu
def test_gpu_sequence_handle_and_lone_matcher(pkg, ob, gpu):
    """A sequence handle across one chunk boundary (chunks of 4 and 2 frames) and a lone matcher."""
    dims = sr.dims_of(pkg)
    frames = sr.frames_of(pkg, 6, 84)
    g = pkg.SequenceGroup(4, pkg.Params.default())
    g.pushBack(np.stack([frames[t][0] for t in range(4)]), None, dims)
    g.matchFeatures(FLOW)
    pose_path(pkg, ob, g, "sequence chunk 0", rows=(1, 2, 3))
    g.pushBack(np.stack([frames[t][0] for t in range(4, 6)]), None, dims)
    g.matchFeatures(FLOW)
    pose_path(pkg, ob, g, "sequence chunk 1", rows=(0, 1))
    g.close()
    m = pkg.Matcher(pkg.Params.default(), outlier_removal=False)
    for left, _ in frames[:2]:
        m.pushBack(left, None, dims)
    m.matchFeatures(FLOW)
    pm = m.getMatches()
    e = tm.hmono(pkg, inlier_threshold=3e-5)
    models = pkg.estimate_motion_mono(e, [pm], tm.rand8_of(ob, e, 1), model=True)[3]
    assert models["valid"][0] == 1.0
    m.motionInliersMono(e, models)
    m2, ok2, _, _ = m.refitModelMono(e, reclassify=True)
    inl = m.getInlierMatches()[0]
    tr, ok, pose = m.poseMono(e, pose=True)
    want = pkg.pose_mono(e, [inl], m2, [int(ok2)])
    assert tr.tobytes() == want[0][0].tobytes() and ok == want[1][0] and pose[0].tobytes() == want[2][0].tobytes()
    assert m.poseMono(e)[0].tobytes() == tr.tobytes()
    m.close()


@pytest.mark.gpu
def test_gpu_state_rules_off_state_and_failed_allocation(pkg, ob, gpu):
    """VH_ERR_STATE before a classification, after a stereo classification and after a push; a handle that never calls the
    entry holds the bytes of one that only classifies and has no mono_pose launch; a refused allocation is VH_ERR_HIP before
    any launch, leaves the bytes and the classification as they were, and the repeated call gives what the stateless form
    gives; the block is 16 bytes per record slot and 972 per stream, allocated once."""
    dims = sr.dims_of(pkg)
    frames = [sr.frames_of(pkg, 3, seed) for seed in (85, 86)]
    e = tm.hmono(pkg, inlier_threshold=3e-5)
    ego = ti.hego(pkg, inlier_threshold=2.5)
    state = pkg.VH_ERR_STATE
    MM = 4096
    seen = {}
    for name in ("off", "on"):
        g = pkg.StreamGroup(2, pkg.Params.default(), max_matches=MM)
        g.profileEnable(True)
        expect(pkg, state, lambda: g.poseMono(e))                        # nothing pushed
        for t in range(2):
            g.pushBack(np.stack([f[t][0] for f in frames]), np.stack([f[t][1] for f in frames]), dims)
        g.matchFeatures(QUAD)
        expect(pkg, state, lambda: g.poseMono(e))                        # not classified yet
        g.motionInliers(ego, np.array([ti.TR2] * 2), np.ones(2, np.int32))
        expect(pkg, state, lambda: g.poseMono(e))                        # the current result is a stereo classification
        _, _, _, models = g.estimateMotionMono(e, tm.rand8_of(ob, e, 2), model=True)
        ok0 = models["valid"].astype(np.int32)
        g.motionInliersMono(e, models, ok0)
        bytes0 = g.deviceBytes()
        if name == "on":
            inl = [g.getInlierMatches(s)[0] for s in range(2)]
            want = pkg.pose_mono(e, inl, models, ok0)
            g.debugFailNextAlloc()
            expect(pkg, pkg.VH_ERR_HIP, lambda: g.poseMono(e))
            assert g.deviceBytes() == bytes0 and all(g.profileRead(s)[1] == 0 for s in SCOPES)
            assert all(g.getInlierMatches(s)[0].tobytes() == inl[s].tobytes() for s in range(2))   # the handle is as it was
            tr, ok, _, pose = g.poseMono(e, pose=True)                   # the repeated call
            assert all(pose_bytes((tr, ok, pose), s) == pose_bytes(want, s) for s in range(2))
            lo = 16 * 2 * MM + 972 * 2
            assert lo <= g.deviceBytes() - bytes0 <= lo + 6 * 255, (g.deviceBytes() - bytes0, lo)
            bytes1 = g.deviceBytes()
            g.poseMono(e); g.poseMono(e, pose=True)
            assert g.deviceBytes() == bytes1                             # one block, allocated once
        g.synchronize()
        seen[name] = (bytes0, [g.profileRead(s)[1] for s in SCOPES])
        g.pushBack(np.stack([f[2][0] for f in frames]), np.stack([f[2][1] for f in frames]), dims)
        expect(pkg, state, lambda: g.poseMono(e))                        # pushed: the pair the lists belong to is over
        g.close()
    assert seen["off"][0] == seen["on"][0] and seen["off"][1] == [0] * 6 and seen["on"][1] == [3] * 6
