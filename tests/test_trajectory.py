"""The trajectory: vh_trajectory on caller-owned chains of rows, and vh_group_trajectory with the
_world scene-point entries on plain groups, lone matchers and sequence handles.

The bounds.  Where every rotation is zero, sin and cos are exact, T's entries are 0, 1 and the translation, and nothing of
any math library enters: the device must give the float64 restatement (tests/trajectory_oracle.py) byte for byte.  For
general motions the device's sin / cos may differ from the host's in the last place, so every element is held to
16 x d_ref of the longdouble restatement, d_ref being the float64 restatement's own largest distance from the longdouble
one over these very chains, relative to max(1, |element|) -- the factor the covariance and mono-refit tests give the device
over a restatement's own error.  Handles are held to the stateless form byte for byte: same kernel, same inputs."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import test_motion_inliers as mi
import test_mono_inliers as tm
import test_post_dense as pd
import test_sequence_landmarks as sl
import test_sequence_recon as sr
import trajectory_oracle as to
from conftest import ROOT

SYMBOLS = ("vh_default_traj_params", "vh_trajectory", "vh_group_set_trajectory", "vh_sequence_set_trajectory", "vh_set_trajectory",
           "vh_group_trajectory", "vh_match_trajectory", "vh_group_get_poses", "vh_get_pose", "vh_group_poses_device", "vh_group_set_pose",
           "vh_group_scene_points_stereo_world", "vh_group_scene_points_mono_world", "vh_match_scene_points_stereo_world",
           "vh_match_scene_points_mono_world")
R = 256                                     # VH_TRAJ_ROUND: asserted against the header and the package below
LENGTHS = (1, 0, 2, R - 1, R, R + 1, 2 * R + 1)   # an empty chain among them
QUAD, FLOW = 2, 0
T0 = np.array([[0.0, -1.0, 0.0, 3.5], [1.0, 0.0, 0.0, -2.25], [0.0, 0.0, 1.0, 0.75], [0.0, 0.0, 0.0, 1.0]])
_CACHE = {}


def ptr(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def expect(pkg, code, fn):
    with pytest.raises(pkg.VisoHipError) as ei:
        fn()
    assert ei.value.code == code, (ei.value.code, code)


def ok_pattern(n, seed):
    """mixed ok: mostly accepted, runs of failures, a failure in front of and behind every round boundary, a row without
    a pair now and then"""
    rng = np.random.default_rng(seed)
    ok = (rng.random(n) < 0.75).astype(np.int32)
    for b in range(R, n, R):
        ok[b - 1] = 1; ok[b] = 0                      # REPEAT across the boundary needs the round before's Tinv
    ok[rng.random(n) < 0.03] = -1
    return ok


def translation_chains(seed=5):
    """rx = ry = rz = 0; translations on a grid of 1 / 128 m and below 1 m: the full pivoting then only ever divides by the
    1s of T (a larger |t| would become a pivot and 1 / t rounds), and every sum is exact in float64"""
    rng = np.random.default_rng(seed)
    trs, oks = [], []
    for c, n in enumerate(LENGTHS):
        tr = np.zeros((n, 6))
        tr[:, 3:] = rng.integers(-127, 128, (n, 3)) / 128.0
        trs.append(tr); oks.append(ok_pattern(n, seed + c))
    if len(oks[0]):
        oks[0][0] = 0                                  # REPEAT before any accepted row: holds
    return trs, oks


def general_chains(seed=11):
    """|r| <= 0.05 rad, |t| <= 2 m"""
    rng = np.random.default_rng(seed)
    trs, oks = [], []
    for c, n in enumerate(LENGTHS):
        tr = np.concatenate([rng.uniform(-0.05, 0.05, (n, 3)), rng.uniform(-2, 2, (n, 3))], 1)
        trs.append(tr); oks.append(ok_pattern(n, seed + 100 + c))
    return trs, oks


def oracle_chains(trs, oks, on_fail, ft=np.float64, T0s=None):
    return [to.chain(t, o, None if T0s is None else T0s[c], None, on_fail, ft) for c, (t, o) in enumerate(zip(trs, oks))]


def general_reference():
    """-> (float64 results, longdouble results, d_ref) over general_chains(), HOLD"""
    if "gen" not in _CACHE:
        trs, oks = general_chains()
        w64 = oracle_chains(trs, oks, to.HOLD)
        wld = oracle_chains(trs, oks, to.HOLD, np.longdouble)
        d = max(float(max(to.rel_diff(a[0][f], b[0][f]) for f in ("Tw_prev", "Tw_cur"))) for a, b in zip(w64, wld))
        _CACHE["gen"] = (w64, wld, d)
    return _CACHE["gen"]


def same_records(got, want, what):
    assert got.dtype == want.dtype and len(got) == len(want), (what, len(got), len(want))
    if got.tobytes() != want.tobytes():
        for f in ("status", "step", "Tw_prev", "Tw_cur"):
            bad = [r for r in range(len(got)) if got[f][r].tobytes() != want[f][r].tobytes()]
            assert not bad, (what, f, bad[:5], got[f][bad[0]], want[f][bad[0]])
        raise AssertionError(what)


# ------------------------------------------------------------------------------------------------------------ CPU
def test_symbols_layout_and_host_refusals(pkg):
    """Every symbol is declared, exported and in ABI_SYMBOLS, vh_abi_version stays 1; the records are 272 bytes; the round
    length is the header's; both units are in the Makefile's SRCS; the Python layer has its entries; n_chains = 0 and
    chains without rows are VH_OK without a device (the carry goes from the start to carry_out); the refusals."""
    header = open(os.path.join(ROOT, "include", "viso_hip.h")).read()
    lib = pkg._lib()
    for name in SYMBOLS:
        assert name + "(" in header and hasattr(C.CDLL(pkg.LIB_PATH), name) and name in pkg.ABI_SYMBOLS, name
    assert pkg.abi_version() == 1
    assert pkg.TRAJ_POSE_DTYPE.itemsize == 272 == to.POSE.itemsize and pkg.TRAJ_CARRY_DTYPE.itemsize == 272 == to.CARRY.itemsize
    assert pkg.TRAJ_POSE_DTYPE == to.POSE and pkg.TRAJ_CARRY_DTYPE == to.CARRY
    assert f"#define VH_TRAJ_ROUND {R}\n" in open(os.path.join(pkg.CSRC, "vh_trajectory.h")).read() and pkg.TRAJ_ROUND == R
    srcs = open(os.path.join(pkg.CSRC, "Makefile")).read().split("SRCS", 1)[1].split("ONLY", 1)[0]
    assert "kernels_trajectory.hip" in srcs and "engine_trajectory.hip" in srcs
    for cls in (pkg.Matcher, pkg.StreamGroup, pkg.SequenceGroup):
        assert all(hasattr(cls, n) for n in ("setTrajectory", "trajectory", "getPoses", "setPose", "scenePointsWorld")), cls
    tp = pkg.TrajParams.default()
    assert tp.on_fail == pkg.TRAJ_HOLD
    assert lib.vh_trajectory(C.byref(tp), 0, 0, None, None, None, None, None, None, None) == pkg.VH_OK
    off = np.zeros(3, np.int32); cout = np.zeros(2, to.CARRY)
    t0 = np.stack([T0, np.eye(4)]).reshape(2, 16).copy()
    assert lib.vh_trajectory(C.byref(tp), 0, 2, ptr(off), None, None, ptr(t0), None, None, ptr(cout)) == pkg.VH_OK
    assert np.array_equal(cout["Tw"][0], T0) and np.array_equal(cout["Tw"][1], np.eye(4)) and not cout["has_tinv"].any() and not cout["step"].any()
    inv = pkg.VH_ERR_INVALID_ARG
    off = np.array([0, 1], np.int32); tr = np.zeros((1, 6)); ok = np.ones(1, np.int32); out = np.zeros(1, to.POSE)
    assert lib.vh_trajectory(None, 0, 1, ptr(off), ptr(tr), ptr(ok), None, None, ptr(out), None) == inv
    assert lib.vh_trajectory(C.byref(pkg.TrajParams.default(on_fail=2)), 0, 1, ptr(off), ptr(tr), ptr(ok), None, None, ptr(out), None) == inv
    assert lib.vh_trajectory(C.byref(tp), 0, -1, ptr(off), ptr(tr), ptr(ok), None, None, ptr(out), None) == inv
    assert lib.vh_trajectory(C.byref(tp), 0, 1, None, ptr(tr), ptr(ok), None, None, ptr(out), None) == inv
    assert lib.vh_trajectory(C.byref(tp), 0, 1, ptr(off), None, ptr(ok), None, None, ptr(out), None) == inv
    assert lib.vh_trajectory(C.byref(tp), 0, 1, ptr(off), ptr(tr), ptr(ok), None, None, None, None) == inv
    assert lib.vh_trajectory(C.byref(tp), 0, 1, ptr(np.array([1, 0], np.int32)), ptr(tr), ptr(ok), None, None, ptr(out), None) == inv
    assert lib.vh_group_set_trajectory(None, C.byref(tp), None) == inv and lib.vh_group_trajectory(None, 0, None) == inv


def test_restatement_against_the_demo_loop_and_d_ref():
    """The float64 restatement equals the literal pose @ inv(T) loop (numpy's own inverse and product) to within d_ref;
    d_ref itself -- float64 against longdouble over the GPU tests' own chains -- is computed and printed, and is what
    one expects of a product chain of up to 2R + 1 well-conditioned matrices: below 1e-12."""
    trs, oks = general_chains()
    w64, wld, d_ref = general_reference()
    print(f"d_ref = {d_ref:.3e} over chains of {LENGTHS} rows")
    assert 0 < d_ref < 1e-12
    worst = 0.0
    for (res, _), tr, ok in zip(w64, trs, oks):
        if len(tr):
            worst = max(worst, float(to.rel_diff(res["Tw_cur"], to.demo_loop(tr, ok))))
    print(f"float64 restatement against the demo loop: {worst:.3e}")
    assert worst <= d_ref
    for (a, _), (b, _) in zip(w64, wld):
        assert np.array_equal(a["status"], b["status"]) and np.array_equal(a["step"], b["step"])


def test_pure_translations_are_exact_sums():
    """rx = ry = rz = 0: Tinv is [I | -t] and the pose is the start minus the sum of the accepted translations, exactly;
    Tw_prev of row r is Tw_cur of row r - 1; step counts the accepted rows."""
    trs, oks = translation_chains()
    for on_fail in (to.HOLD, to.REPEAT):
        for tr, ok in zip(trs, oks):
            res, (P, last, step) = to.chain(tr, ok, None, None, on_fail)
            pos, lastt, steps = np.zeros(3), None, 0
            for r in range(len(tr)):
                assert np.array_equal(res["Tw_prev"][r][:3, 3], pos)
                if ok[r] > 0:
                    lastt = tr[r, 3:]; pos = pos - lastt; steps += 1
                elif ok[r] == 0 and on_fail == to.REPEAT and lastt is not None:
                    pos = pos - lastt
                want = np.eye(4); want[:3, 3] = pos
                assert res["Tw_cur"][r].tobytes() == (want + 0.0).tobytes(), (on_fail, r)
                assert res["step"][r] == steps and res["status"][r] == (0 if ok[r] > 0 else 1 if ok[r] == 0 else 4)


HAND_TR = np.array([[0, 0, 0, 1.0, 0, 0],            # accepted
                    [0, 0, 0, 9.0, 9.0, 9.0],        # ok = 0
                    [0, np.nan, 0, 1.0, 0, 0],       # NaN
                    [0.01, 0, 0, 1e300, 0, 0],       # the elimination refuses: the pivots behind 1e300 fall below 1e-20
                    [0, 0, 0, np.inf, 0, 0],         # inf
                    [0, 0, 0, 7.0, 7.0, 7.0],        # no pair
                    [0, 0, 0, 0, 2.0, 0]])           # accepted
HAND_OK = np.array([1, 0, 1, 1, 1, -1, 1], np.int32)
HAND_STATUS = [0, 1, 2, 3, 2, 4, 0]


def test_policies_and_status_codes_on_hand_made_rows():
    hold, _ = to.chain(HAND_TR, HAND_OK, None, None, to.HOLD)
    rep, carry = to.chain(HAND_TR, HAND_OK, None, None, to.REPEAT)
    assert hold["status"].tolist() == HAND_STATUS == rep["status"].tolist()
    assert hold["step"].tolist() == [1, 1, 1, 1, 1, 1, 2] == rep["step"].tolist()
    assert hold["Tw_cur"][:, :3, 3].tolist() == [[-1, 0, 0]] * 6 + [[-1, -2, 0]]
    # REPEAT: rows 1 - 4 each step by the last accepted (-1, 0, 0) again, the row without a pair holds
    assert rep["Tw_cur"][:, 0, 3].tolist() == [-1, -2, -3, -4, -5, -5, -5] and rep["Tw_cur"][6, 1, 3] == -2
    assert np.array_equal(carry[1], np.array([[1, 0, 0, 0], [0, 1, 0, -2.0], [0, 0, 1, 0], [0, 0, 0, 1]]))
    first, _ = to.chain(HAND_TR[1:3], HAND_OK[1:3], T0, None, to.REPEAT)       # nothing accepted yet: holds
    assert all(first["Tw_cur"][r].tobytes() == T0.tobytes() for r in range(2)) and first["step"].tolist() == [0, 0]


def run_check(tmp_path, exe, name, tr, ok, on_fail, T0m):
    fin, fout = str(tmp_path / (name + ".in")), str(tmp_path / (name + ".out"))
    with open(fin, "wb") as fh:
        fh.write(np.array([on_fail, len(tr)], np.int32).tobytes()); fh.write(np.asarray(T0m, np.float64).tobytes())
        fh.write(np.ascontiguousarray(tr, np.float64).tobytes()); fh.write(np.ascontiguousarray(ok, np.int32).tobytes())
    subprocess.check_call([exe, fin, fout], timeout=60)
    raw = np.fromfile(fout, np.uint8)
    return raw[:272 * len(tr)].view(to.POSE), raw[272 * len(tr):].view(to.CARRY)


def test_header_on_the_host(tmp_path):
    """csrc/vh_trajectory.h compiled for the host (tests/cpp/trajectory_check.cpp): byte for byte the float64 restatement
    on the exact cases -- pure translations under both policies, the hand-made rows -- records and carry; on general motions
    status and step are equal and the elements agree up to libm (both use the host's sin / cos here: 4 x d_ref)."""
    exe = str(tmp_path / "trajectory_check")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", os.path.join(ROOT, "tests", "cpp", "trajectory_check.cpp"), "-lm", "-o", exe])
    trs, oks = translation_chains()
    for on_fail in (to.HOLD, to.REPEAT):
        for c, (tr, ok) in enumerate(list(zip(trs, oks)) + [(HAND_TR, HAND_OK)]):
            res, carry = to.chain(tr, ok, T0 if c % 2 else None, None, on_fail)
            got, gc = run_check(tmp_path, exe, f"t{on_fail}_{c}", tr, ok, on_fail, T0 if c % 2 else np.eye(4))
            same_records(got, to.records(res), ("host exact", on_fail, c))
            assert gc.tobytes() == to.carry_record(carry).tobytes(), (on_fail, c)
    trs, oks = general_chains()
    w64, _, d_ref = general_reference()
    for c, (tr, ok) in enumerate(zip(trs, oks)):
        got, _ = run_check(tmp_path, exe, f"g{c}", tr, ok, to.HOLD, np.eye(4))
        assert np.array_equal(got["status"], w64[c][0]["status"]) and np.array_equal(got["step"], w64[c][0]["step"])
        assert float(to.rel_diff(got["Tw_cur"], w64[c][0]["Tw_cur"])) <= 4 * d_ref


def test_drift_of_the_rotation():
    """RtR - I after 4 096 accepted general rows on the float64 restatement: measured and printed (DESIGN.md section 4.23
    records it); nothing re-orthonormalises, so it only has to stay a rounding-sized number: 4 096 rows x 2^-52 x 16."""
    rng = np.random.default_rng(23)
    tr = np.concatenate([rng.uniform(-0.05, 0.05, (4096, 3)), rng.uniform(-2, 2, (4096, 3))], 1)
    res, _ = to.chain(tr, np.ones(4096, np.int32))
    Rm = res["Tw_cur"][-1][:3, :3]
    drift = float(np.abs(Rm.T @ Rm - np.eye(3)).max())
    print(f"drift of RtR - I after 4096 rows: {drift:.3e}")
    assert res["step"][-1] == 4096 and drift < 4096 * 2.0 ** -52 * 16


# ------------------------------------------------------------------------------------------------------------ GPU, stateless
@pytest.mark.gpu
def test_gpu_pure_translations_byte_equal(pkg, gpu):
    """Chains of 1, 0, 2, R - 1, R, R + 1 and 2R + 1 rows in one call, mixed ok, both policies, with and without T0: records
    and carry byte for byte the float64 restatement; the hand-made rows likewise."""
    trs, oks = translation_chains()
    trs, oks = trs + [HAND_TR], oks + [HAND_OK]
    T0s = np.stack([T0 if c % 2 else np.eye(4) for c in range(len(trs))])
    for on_fail in (to.HOLD, to.REPEAT):
        for t0 in (None, T0s):
            got, carry = pkg.trajectory(trs, oks, t0, None, pkg.TrajParams.default(on_fail=on_fail))
            want = oracle_chains(trs, oks, on_fail, np.float64, t0)
            for c in range(len(trs)):
                same_records(got[c], to.records(want[c][0]), ("translations", on_fail, t0 is not None, c))
                assert carry[c:c + 1].tobytes() == to.carry_record(want[c][1]).tobytes(), (on_fail, c)
    assert got[-1]["status"].tolist() == HAND_STATUS


@pytest.mark.gpu
def test_gpu_general_motions_within_16_d_ref(pkg, gpu):
    """General motions: status and step equal, every element within 16 x d_ref of the longdouble restatement; the share
    of that room actually used is printed.  The same bytes on a second run, and for a chain alone as among the others."""
    trs, oks = general_chains()
    _, wld, d_ref = general_reference()
    got, carry = pkg.trajectory(trs, oks)
    worst = 0.0
    for c in range(len(trs)):
        assert np.array_equal(got[c]["status"], wld[c][0]["status"]) and np.array_equal(got[c]["step"], wld[c][0]["step"]), c
        for f in ("Tw_prev", "Tw_cur"):
            worst = max(worst, float(to.rel_diff(got[c][f], wld[c][0][f])))
    print(f"d_ref = {d_ref:.3e}; the device's largest distance {worst:.3e} = {worst / (16 * d_ref):.1%} of 16 x d_ref")
    assert worst <= 16 * d_ref
    again, carry2 = pkg.trajectory(trs, oks)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(got, again)) and carry.tobytes() == carry2.tobytes()
    c = len(trs) - 1
    alone, ca = pkg.trajectory(trs[c:], oks[c:])
    assert alone[0].tobytes() == got[c].tobytes() and ca.tobytes() == carry[c:].tobytes()


@pytest.mark.gpu
def test_gpu_two_calls_joined_by_the_carry(pkg, gpu):
    """Two calls, the second starting from the first's carry, equal one call over the concatenation -- split in front of,
    on and behind a round boundary, under REPEAT (the last accepted Tinv crosses the split), from a T0 that is not the unit
    matrix; general motions and translations."""
    for trs, oks in (general_chains(3), translation_chains(4)):
        tr, ok = trs[-1], oks[-1].copy()
        for cut in (1, R - 1, R, R + 1):
            ok[cut - 1] = 1; ok[cut] = 0                  # the row behind the split repeats the row in front of it
            tp = pkg.TrajParams.default(on_fail=pkg.TRAJ_REPEAT)
            whole, cw = pkg.trajectory([tr], [ok], T0, None, tp)
            a, ca = pkg.trajectory([tr[:cut]], [ok[:cut]], T0, None, tp)
            b, cb = pkg.trajectory([tr[cut:]], [ok[cut:]], None, ca, tp)
            assert np.concatenate([a[0], b[0]]).tobytes() == whole[0].tobytes() and cb.tobytes() == cw.tobytes(), cut
            assert not np.array_equal(whole[0]["Tw_cur"][cut], whole[0]["Tw_prev"][cut])   # (it did repeat)


# ------------------------------------------------------------------------------------------------------------ GPU, handles
def stateless_step(pkg, tr, ok, carry, tp=None):
    """one row per chain from `carry` -> (records [S], carry)"""
    got, c = pkg.trajectory([t[None] for t in tr], [[int(o)] for o in ok], None, carry, tp)
    return np.concatenate(got), c


def start_carry(S, T0m=None):
    c = np.zeros(S, to.CARRY)
    c["Tw"] = np.eye(4) if T0m is None else T0m
    return c


def check_world(pkg, g, e, what, rows):
    """scenePointsWorld byte for byte scenePoints(Tw = the poses' matrix of that frame), both frames"""
    poses = g.getPoses()
    total = 0
    for frame, field in ((0, "Tw_prev"), (1, "Tw_cur")):
        sp = pkg.SceneParams.default(frame=frame)
        cw = g.scenePointsWorld(e, sp)
        got = [g.getScenePoints(s) for s in rows]
        ch = g.scenePoints(e, sp, poses[field])
        want = [g.getScenePoints(s) for s in rows]
        assert np.array_equal(cw, ch) and all(a.tobytes() == b.tobytes() for a, b in zip(got, want)), (what, frame)
        total += int(cw.sum())
    return total


@pytest.mark.gpu
def test_gpu_group_of_three_and_lone_matcher(pkg, ob, gpu):
    """A group of 3 streams over 3 steps under REPEAT from a T0 per stream: trajectory(STEREO) byte for byte the stateless
    form fed the handle's own tr / ok and the carry of the step before; a second call behind refitMotion(reclassify=True)
    equals one step from the same base under the refined motion; getPoses serves the records; scenePointsWorld equals
    scenePoints(Tw = getPoses()[...]) for both frames; setPose re-anchors.  A lone matcher likewise."""
    fr, dims = pd.frames_of(pkg), pd.dims_of(pkg)
    e = pd.ego_of(pkg)
    S = pd.S
    tp = pkg.TrajParams.default(on_fail=pkg.TRAJ_REPEAT)
    T0s = np.stack([np.eye(4), T0, np.eye(4)])
    g = pkg.StreamGroup(S, pkg.Params.default())
    g.setTrajectory(tp, T0s)
    g.profileEnable(True)
    expect(pkg, pkg.VH_ERR_STATE, lambda: g.trajectory())                       # nothing pushed
    carry, total, calls = start_carry(S, T0s), 0, 0
    for t in range(3):
        pd.push(g, fr, t, dims)
        if t == 0:
            expect(pkg, pkg.VH_ERR_STATE, lambda: g.setTrajectory(tp))          # after the first push
            continue
        g.matchFeatures(QUAD)
        expect(pkg, pkg.VH_ERR_STATE, lambda: g.trajectory())                   # no classification yet
        expect(pkg, pkg.VH_ERR_STATE, lambda: g.getPoses())
        tr0, ok0, _ = g.estimateMotion(e, mi.rand3_of(ob, e, S))
        g.motionInliers(e, tr0, ok0.astype(np.int32))
        expect(pkg, pkg.VH_ERR_STATE, lambda: g.scenePointsWorld(e))            # no trajectory behind this match call
        expect(pkg, pkg.VH_ERR_STATE, lambda: g.trajectory(pkg.TRAJ_MONO))      # the wrong kind of classification
        got = g.trajectory(pkg.TRAJ_STEREO); calls += 1
        want, _ = stateless_step(pkg, tr0, ok0, carry, tp)
        same_records(got, want, f"group t{t}")
        tr, ok, _, _ = g.refitMotion(e, reclassify=True)
        expect(pkg, pkg.VH_ERR_STATE, lambda: g.scenePointsWorld(e))            # classified again: the poses are the old motion's
        got = g.trajectory(); calls += 1
        want, c2 = stateless_step(pkg, tr, ok, carry, tp)                       # one step from the latched base, not two
        same_records(got, want, f"group t{t} refit")
        assert g.getPoses().tobytes() == got.tobytes()
        d, stride = g.posesDevice()
        assert stride == 1 and mi.hip_read(d, S, to.POSE).tobytes() == got.tobytes()
        total += check_world(pkg, g, e, f"group t{t}", range(S))
        base, carry = carry, c2
    assert total > 0 and carry["step"].max() >= 2 and (got["status"] == 1).any()   # (the stream of constant images never is ok)
    # re-anchoring inside a pair: stream 1 steps from the new pose with step 0 and nothing to repeat, the others once more
    # from the base of this very pair
    g.setPose(1, np.eye(4))
    expect(pkg, pkg.VH_ERR_STATE, lambda: g.getPoses())
    base = base.copy(); base[1] = start_carry(1)[0]
    got = g.trajectory(); calls += 1
    same_records(got, stateless_step(pkg, tr, ok, base, tp)[0], "re-anchored")
    g.synchronize()
    assert g.profileRead("trajectory")[1] == calls
    g.close()

    frames = sr.frames_of(pkg, 3, 74)
    e = mi.hego(pkg, inlier_threshold=2.5)
    m = pkg.Matcher(pkg.Params.default(), outlier_removal=True)
    m.setTrajectory(None, T0)
    carry = start_carry(1, T0)
    for t, (left, right) in enumerate(frames):
        m.pushBack(left, right, sr.dims_of(pkg))
        if t == 0:
            continue
        m.matchFeatures(QUAD)
        n = m.motionInliers(e, mi.TR2)
        got = m.trajectory()
        want, c1 = stateless_step(pkg, np.array([mi.TR2]), [1], carry)
        same_records(got, want, f"matcher t{t}")
        tr, ok, _, _ = m.refitMotion(e, reclassify=True)
        got = m.trajectory()
        want, carry = stateless_step(pkg, np.asarray(tr)[None], [int(ok)], carry)
        same_records(got, want, f"matcher t{t} refit")
        assert m.getPoses().tobytes() == got.tobytes() and got["step"][0] == t and n > 6
        pts = m.scenePointsWorld(e)
        assert len(pts) > 0 and pts.tobytes() == m.scenePoints(e, Tw=got["Tw_cur"][0]).tobytes()
        pts = m.scenePointsWorld(e, pkg.SceneParams.default(frame=0))
        assert pts.tobytes() == m.scenePoints(e, pkg.SceneParams.default(frame=0), got["Tw_prev"][0]).tobytes()
    m.close()


@pytest.mark.gpu
def test_gpu_replace_push_and_unstepped_pair(pkg, gpu):
    """A lone matcher: step, replace push (getPoses and the _world entry are VH_ERR_STATE), match, step under another
    motion -- byte for byte ONE step from the base of the replaced pair, not two.  Then a pair that is pushed and matched
    but never stepped, and a shifted push behind it: the next step starts from the pose the last stepped pair left."""
    frames = sr.frames_of(pkg, 5, 74)
    dims = sr.dims_of(pkg)
    e = mi.hego(pkg, inlier_threshold=2.5)
    other = np.array(mi.TR2, np.float64) + np.array([0.002, -0.001, 0.003, 0.25, -0.125, 0.5])
    m = pkg.Matcher(pkg.Params.default(), outlier_removal=True)
    m.setTrajectory(None, T0)
    base = start_carry(1, T0)
    for left, right in frames[:2]:
        m.pushBack(left, right, dims)
    m.matchFeatures(QUAD)
    m.motionInliers(e, mi.TR2)
    got = m.trajectory()
    want, _ = stateless_step(pkg, np.array([mi.TR2]), [1], base)
    same_records(got, want, "before the replace push")
    m.pushBack(frames[2][0], frames[2][1], dims, True)
    expect(pkg, pkg.VH_ERR_STATE, lambda: m.getPoses())
    m.matchFeatures(QUAD)
    m.motionInliers(e, other)
    expect(pkg, pkg.VH_ERR_STATE, lambda: m.scenePointsWorld(e))
    got = m.trajectory()
    want, carry = stateless_step(pkg, other[None], [1], base)
    same_records(got, want, "behind the replace push")
    assert got["step"][0] == 1 and got["Tw_prev"][0].tobytes() == T0.tobytes()
    m.pushBack(frames[3][0], frames[3][1], dims)                                # a pair that is never stepped
    m.matchFeatures(QUAD)
    m.motionInliers(e, mi.TR2)
    m.pushBack(frames[4][0], frames[4][1], dims)
    m.matchFeatures(QUAD)
    m.motionInliers(e, mi.TR2)
    got = m.trajectory()
    want, _ = stateless_step(pkg, np.array([mi.TR2]), [1], carry)
    same_records(got, want, "behind the unstepped pair")
    assert got["step"][0] == 2 and got["Tw_prev"][0].tobytes() == carry["Tw"][0].tobytes()
    m.close()


@pytest.mark.gpu
def test_gpu_group_mono_source(pkg, ob, gpu):
    """The mono source behind poseMono on flow lists: VH_ERR_STATE before the pose, then byte for byte the stateless form
    fed poseMono's tr / ok; scenePointsWorld of the mono kind equals scenePoints with the poses' matrices."""
    dims = sr.dims_of(pkg)
    frames = [sr.frames_of(pkg, 3, seed) for seed in (81, 82, 83)]
    frames[1] = [(np.full_like(a, 90), np.full_like(b, 90)) for a, b in frames[1]]
    e = tm.hmono(pkg, inlier_threshold=3e-5, motion_threshold=1e300)
    g = pkg.StreamGroup(3, pkg.Params.default())
    g.setTrajectory()
    carry, total = start_carry(3), 0
    for t in range(3):
        g.pushBack(np.stack([f[t][0] for f in frames]), None, dims)
        if t == 0:
            continue
        g.matchFeatures(FLOW)
        _, _, _, models = g.estimateMotionMono(e, tm.rand8_of(ob, e, 3), model=True)
        g.motionInliersMono(e, models, models["valid"].astype(np.int32))
        expect(pkg, pkg.VH_ERR_STATE, lambda: g.trajectory(pkg.TRAJ_MONO))      # no pose yet for this classification
        expect(pkg, pkg.VH_ERR_STATE, lambda: g.trajectory(pkg.TRAJ_STEREO))
        tr, ok, _ = g.poseMono(e)
        got = g.trajectory(pkg.TRAJ_MONO)
        want, carry = stateless_step(pkg, tr, ok, carry)
        same_records(got, want, f"mono t{t}")
        total += check_world(pkg, g, e, f"mono t{t}", range(3))
    assert total > 0 and carry["step"].max() >= 1
    g.close()


@pytest.mark.gpu
def test_gpu_sequence_handle_two_chunks(pkg, gpu):
    """SequenceGroup(4), chunks of 4 and 2 frames, track linking, landmarks and trajectory on: the rows' poses byte for
    byte ONE stateless chain over all rows (row 0 of the first chunk holds no pair: status 4; the rows behind the short
    chunk: status 4, the pose held); a repeated call gives the same bytes; landmarks() behind scenePointsWorld byte for
    byte landmarks() behind scenePoints given the same matrices; the whole path runs under the profile scopes motion
    inliers .. trajectory .. scene_points .. landmarks without a pose going up."""
    dims = sr.dims_of(pkg)
    frames = sr.frames_of(pkg, 6, sl.SEED)
    e = mi.hego(pkg, inlier_threshold=2.5)
    lp = sl.lparams(pkg, sl.HANDLE_LP)
    ROWS = sl.ROWS
    g = pkg.SequenceGroup(ROWS, pkg.Params.default(), max_matches=sl.MM)
    g.setTrackLinking(True); g.setLandmarks(True); g.setTrajectory(None, T0)
    g.profileEnable(True)
    assert pkg._lib().vh_group_set_trajectory(g._h, C.byref(pkg.TrajParams.default()), None) == pkg.VH_ERR_UNSUPPORTED
    all_tr, all_ok, got_rows, landmarks = [], [], [], 0
    for F, n in ((0, 4), (4, 2)):
        sr.push(g, frames, F, n, dims)
        g.matchFeatures(QUAD)
        tr = sl.motions(F)
        g.motionInliers(e, tr, np.ones(ROWS, np.int32))
        got = g.trajectory()
        assert g.trajectory().tobytes() == got.tobytes() == g.getPoses().tobytes()
        assert (got["status"][n:] == 4).all() and all(got["Tw_cur"][r].tobytes() == got["Tw_cur"][n - 1].tobytes() for r in range(n, ROWS))
        got_rows.append(got[:n])
        all_tr.append(tr[:n]); all_ok.append(np.array([-1 if F + r == 0 else 1 for r in range(n)], np.int32))
        g.scenePointsWorld(e)
        a = sl.rows_landmarks(g, lp)
        g.scenePoints(e, None, got["Tw_cur"])
        b = sl.rows_landmarks(g, lp)
        sl.same(a, b, f"landmarks of chunk {F}")
        landmarks += sum(len(x) for x in a)
    want, _ = pkg.trajectory([np.concatenate(all_tr)], [np.concatenate(all_ok)], T0)
    same_records(np.concatenate(got_rows), want[0], "sequence rows")
    assert want[0]["status"].tolist() == [4, 0, 0, 0, 0, 0] and want[0]["step"][-1] == 5 and landmarks > 0
    g.synchronize()
    assert g.profileRead("trajectory")[1] == 4 and g.profileRead("scene_points")[1] == 4
    g.close()


@pytest.mark.gpu
def test_gpu_switch_off_and_the_block(pkg, ob, gpu):
    """Off: trajectory() and the _world entries are VH_ERR_STATE, no "trajectory" launch is profiled and deviceBytes equals
    that of a handle with the switch on that has not stepped yet; on: the first call adds exactly the documented block, once;
    a refused allocation is VH_ERR_HIP, leaves the bytes as they were, and the repeated call is right."""
    fr, dims = pd.frames_of(pkg), pd.dims_of(pkg)
    e = pd.ego_of(pkg)
    S = pd.S
    hs = []
    for on in (False, True):
        g = pkg.StreamGroup(S, pkg.Params.default())
        if on:
            g.setTrajectory()
        g.profileEnable(True)
        for t in range(2):
            pd.push(g, fr, t, dims)
        g.matchFeatures(QUAD)
        tr0, ok0, _ = g.estimateMotion(e, mi.rand3_of(ob, e, S))
        g.motionInliers(e, tr0, ok0.astype(np.int32))
        g.synchronize()
        hs.append(g)
    off, on = hs
    expect(pkg, pkg.VH_ERR_STATE, lambda: off.trajectory())
    expect(pkg, pkg.VH_ERR_STATE, lambda: off.scenePointsWorld(e))
    expect(pkg, pkg.VH_ERR_STATE, lambda: off.getPoses())
    expect(pkg, pkg.VH_ERR_STATE, lambda: off.setPose(0, np.eye(4)))
    off.synchronize()
    assert off.profileRead("trajectory")[1] == 0 and off.deviceBytes() == on.deviceBytes()
    bytes0 = on.deviceBytes()
    on.debugFailNextAlloc()
    expect(pkg, pkg.VH_ERR_HIP, lambda: on.trajectory())
    on.synchronize()
    assert on.deviceBytes() == bytes0 and on.profileRead("trajectory")[1] == 0
    got = on.trajectory()
    same_records(got, stateless_step(pkg, tr0, ok0, start_carry(S))[0], "after the refused allocation")
    on.trajectory()
    up = lambda b: (b + 255) // 256 * 256  # noqa: E731
    assert on.deviceBytes() == bytes0 + 3 * up(272 * S)
    off.close(); on.close()
