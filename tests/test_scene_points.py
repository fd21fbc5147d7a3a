"""Scene points: one 3-d point per record of whole lists, stereo and mono, compacted in list order
-- vh_scene_points_stereo / _mono on caller-owned lists, vh_group_scene_points_* / vh_match_scene_points_* on the compacted
inlier lists of a handle's classification.  tests/scene_points_oracle.py restates the contract in double and in long double.

The GPU bound.  The device computes in double what the restatement computes in double; the two differ only where the
device library's sin / cos differ from libm's (the stereo rotation at a non-zero motion) -- orders of magnitude below half
a float ulp -- so the one rounding to float can flip by at most one ulp, and does so rarely: every float within 1 ulp, at
most 1 % of them different at all.  At tr = 0 (sin and cos of 0 are exact) and in the mono form (no function of the device
library but sqrt, the pose handed to both sides) nothing differs in the arithmetic: stereo at tr = 0 is asserted byte for
byte, mono within 1 ulp with the bit-equal share printed.  Thresholds keep a relative margin of at least 1e-6 to every
record, asserted on the restatement, so that no filter compare can flip.

The handle forms store src_pos as the struct documents it -- the position in the list the classification ran on -- while
the stateless form on the getters' inlier list can only number that list: the handle tests map the stateless src_pos
through the getter's positions and then compare byte for byte.

Measured on the CPU.  test_stereo_truth: the restatement's largest miss on the noise-free scene is 8.4e-4 m (frame 0) and
8.4e-4 m (frame 1) at depths up to 60 m -- the float pixel coordinates, not the formula.  test_double_against_long_double:
d_ref = 7.5e-14 (the stereo lists set it; the mono form stays below); floats that differ between the two forms: 0 of
235 915."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import mono_pose_oracle as mp
import scene_points_oracle as so
import test_mono_inliers as tm
import test_mono_pose as tp
import test_motion_inliers as mi
import test_motion_refit as mr
import test_post_dense as pd
import test_sequence_recon as sr
from conftest import ROOT
from egomotion_scene import KITTI, rot

SYMBOLS = ("vh_default_scene_params", "vh_scene_points_stereo", "vh_scene_points_mono", "vh_group_scene_points_stereo",
           "vh_match_scene_points_stereo", "vh_group_scene_points_mono", "vh_match_scene_points_mono", "vh_group_get_scene_points",
           "vh_group_get_scene_points_all", "vh_get_scene_points", "vh_group_scene_points_device")
FIELDS = ("x", "y", "z", "sigma_z", "err", "src_pos", "i1p", "i1c")
QUAD, FLOW = sr.QUAD, sr.FLOW
Cal, ptr, expect, noisy = mr.Cal, mr.ptr, mr.expect, mr.noisy
TR = np.array(mr.TR)
TRUTH_BOUND = 8.5e-4          # metres: the restatement's own largest miss on the noise-free scene, measured here
# the wave, workgroup (= tile of 256) and multi-tile edges of the compaction
LENGTHS = (0, 1, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 2049)
TW = np.eye(4)
TW[:3, :3] = rot(0.1, -0.2, 0.3); TW[:3, 3] = (1.0, -2.0, 3.0)
LIMITS = dict(min_disp=8.0, max_depth=40.0, max_err=0.35)
_CACHE = {}


@pytest.fixture(autouse=True)
def entries(pkg):
    """Every test here is about the scene-point entries, the restatement's own included (it is their yardstick)."""
    assert all(name in pkg.ABI_SYMBOLS and hasattr(pkg._lib(), name) for name in SYMBOLS)


def cal():
    return Cal(**KITTI)


def lists():
    if "lists" not in _CACHE:
        _CACHE["lists"] = [noisy(n, 700 + k) for k, n in enumerate(LENGTHS)]
    return _CACHE["lists"]


#: (tr, frame, Tw, limits) of the stereo parity tests
SETTINGS = ((np.zeros(6), 1, None, {}), (np.zeros(6), 0, None, {}), (TR, 0, None, {}), (TR, 1, None, {}), (TR, 0, TW, {}), (TR, 1, TW, {}),
            (TR, 1, None, LIMITS), (TR, 0, TW, LIMITS))


def want_stereo(k, T=np.float64):
    if ("stereo", k, T) not in _CACHE:
        tr, frame, Tw, lim = SETTINGS[k]
        _CACHE["stereo", k, T] = [so.stereo(pm, tr, cal(), so.params(frame=frame, **lim), Tw=Tw, T=T) for pm in lists()]
    return _CACHE["stereo", k, T]


def mono_cases(ob, oracle):
    """name -> (pm, pose dict, ok): the lists of tests/test_mono_pose.py under the restatement's pose for each"""
    if "mono" not in _CACHE:
        want = tp.expectation(ob, oracle)
        _CACHE["mono"] = {k: (pm, want[k], bool(want[k]["ok"])) for k, (pm, _, _) in tp.lists().items()}
    return _CACHE["mono"]


def want_mono(ob, oracle, frame, Tw, T=np.float64):
    key = ("wmono", frame, Tw is not None, T)
    if key not in _CACHE:
        e = tp.params(ob)
        _CACHE[key] = {k: so.mono(oracle.svd, pm, pose, e, so.params(frame=frame), Tw=Tw, ok=ok, T=T) for k, (pm, pose, ok) in mono_cases(ob, oracle).items()}
    return _CACHE[key]


def pose_array(pkg, poses):
    out = np.zeros(len(poses), pkg.MONO_POSE_DTYPE)
    for j, p in enumerate(poses):
        out["R"][j] = p["R"]; out["t"][j] = p["t"]; out["scale"][j] = p["scale"]; out["reason"][j] = p["reason"]
    return out


def scene_params(pkg, frame=1, **lim):
    return pkg.SceneParams.default(frame=frame, **lim)


# ------------------------------------------------------------------------------------------------------------ CPU
def test_symbols_layout_and_argument_errors(pkg, tmp_path):
    """Every new symbol is declared, exported and mirrored; vh_abi_version stays 1; vh_scene_point is 32 bytes and
    vh_scene_params 24 in the C compiler's layout and in the mirrors; the defaults are frame 1 and no filter; n_sets = 0 and
    lists without records are VH_OK with zero counts without a device; null, negative and out-of-range arguments are
    VH_ERR_INVALID_ARG."""
    header = open(os.path.join(ROOT, "include", "viso_hip.h")).read()
    lib = pkg._lib()
    for name in SYMBOLS:
        assert name + "(" in header and hasattr(C.CDLL(pkg.LIB_PATH), name) and name in pkg.ABI_SYMBOLS, name
    assert '"scene_points"' in header and pkg.abi_version() == 1
    assert callable(pkg.scene_points_stereo) and callable(pkg.scene_points_mono)
    for cls in (pkg.Matcher, pkg.StreamGroup):
        assert "scenePoints" in vars(cls) and "getScenePoints" in vars(cls)
    assert hasattr(pkg.SequenceGroup, "scenePoints")
    dt = pkg.SCENE_POINT_DTYPE
    assert dt.names == FIELDS and dt.itemsize == 32 and dt == so.POINT and C.sizeof(pkg.SceneParams) == 24
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "viso_hip.h"\nint main(void) {\n'
                   '  printf("%zu %zu", sizeof(vh_scene_point), sizeof(vh_scene_params));\n'
                   + "".join(f'  printf(" %zu", offsetof(vh_scene_point, {n}));\n' for n in FIELDS)
                   + "".join(f'  printf(" %zu", offsetof(vh_scene_params, {n}));\n' for n in ("frame", "min_disp", "max_depth", "max_err"))
                   + '  return 0;\n}\n')
    exe = str(tmp_path / "layout")
    subprocess.check_call(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), str(src), "-o", exe])
    assert [int(v) for v in subprocess.check_output([exe], timeout=60).decode().split()] == [32, 24, 0, 4, 8, 12, 16, 20, 24, 28, 0, 4, 8, 16]
    sp = pkg.SceneParams(frame=7, min_disp=7, max_depth=7, max_err=7)
    lib.vh_default_scene_params(C.byref(sp))
    assert (sp.frame, sp.min_disp, sp.max_depth, sp.max_err) == (1, 0.0, 0.0, 0.0)
    inv = pkg.VH_ERR_INVALID_ARG
    pm = np.zeros(8, pkg.P_MATCH_DTYPE); off = np.array([0, 8], np.int32); ok = np.ones(1, np.int32)
    out = np.zeros(8, dt); counts = np.full(2, 7, np.int32)
    empty = np.array([3, 3, 3], np.int32)
    for call, e, motion in ((lib.vh_scene_points_stereo, pkg.EgoParams.default(**KITTI), np.zeros((2, 6))),
                            (lib.vh_scene_points_mono, tp.params(pkg), np.zeros(2, pkg.MONO_POSE_DTYPE))):
        assert call(C.byref(e), C.byref(sp), 0, 0, None, None, None, None, None, None, None) == pkg.VH_OK
        counts[:] = 7
        assert call(C.byref(e), C.byref(sp), 0, 2, None, ptr(empty), ptr(motion), ptr(np.ones(2, np.int32)), None, None, ptr(counts)) == pkg.VH_OK
        assert counts.tolist() == [0, 0]
        good = [C.byref(e), C.byref(sp), 0, 1, ptr(pm), ptr(off), ptr(motion), ptr(ok), None, ptr(out), ptr(counts)]
        for k in (0, 1, 4, 5, 6, 7, 9, 10):      # (Tw is optional)
            assert call(*[None if j == k else a for j, a in enumerate(good)]) == inv, k
        assert call(*good[:3], -1, *good[4:]) == inv
        for bad in ([8, 0], [-1, 7]):
            assert call(*good[:5], ptr(np.array(bad, np.int32)), *good[6:]) == inv
        for frame in (-1, 2):
            assert call(good[0], C.byref(pkg.SceneParams.default(frame=frame)), *good[2:]) == inv
    assert pkg.scene_points_stereo(pkg.EgoParams.default(**KITTI), [], np.zeros((0, 6)), [])[1].shape == (0,)
    n = C.c_int32(0)
    e = pkg.EgoParams.default(**KITTI)
    assert lib.vh_group_scene_points_stereo(None, C.byref(e), C.byref(sp), None, C.byref(n)) == inv
    assert lib.vh_match_scene_points_mono(None, C.byref(tp.params(pkg)), C.byref(sp), None, C.byref(n)) == inv
    assert lib.vh_group_get_scene_points(None, 0, None, 0, C.byref(n)) == inv and lib.vh_group_scene_points_device(None, None, None) == inv


def test_stereo_truth():
    """On a noise-free list (exact projections of known 3-d points before and after the scene's motion, rounded to float)
    the stereo restatement recovers the scene's points in both frames: no record is dropped, src_pos counts up, the
    largest miss is printed and lies within 4 x TRUTH_BOUND = 4 x 8.5e-4 m, the restatement's own largest miss measured
    here (the float pixel coordinates at disparities down to 6 px limit it, not the formula); err stays below 1e-3 px."""
    n, seed = 3000, 41
    pm = noisy(n, seed, noise=0.0)
    rng = np.random.default_rng(seed)            # the scene's own draws
    Z = rng.uniform(4, 60, n)
    P = np.stack([rng.uniform(-1, 1, n) * Z * 0.9, rng.uniform(-0.3, 0.25, n) * Z, Z], 1)
    Q = P @ rot(*TR[:3]).T + TR[3:]
    assert (Q[:, 2] > 2.0).all()
    for frame, truth in ((0, P), (1, Q)):
        got = so.stereo(pm, TR, cal(), so.params(frame=frame))
        assert got["keep"].all() and np.array_equal(got["points"]["src_pos"], np.arange(n))
        miss = float(np.abs(got["wide"][:, :3] - truth).max())
        print(f"frame {frame}: largest miss {miss:.3e} m, largest err {got['wide'][:, 4].max():.3e} px")
        assert miss <= 4 * TRUTH_BOUND and got["wide"][:, 4].max() < 1e-3
        assert np.allclose(got["wide"][:, 3], truth[:, 2] ** 2 / (KITTI["f"] * KITTI["base"]), rtol=1e-3)


def test_mono_tie_to_the_pinned_oracle(ob, oracle):
    """On the lists of tests/test_mono_pose.py with frame = 0 and no limits the mono restatement keeps exactly the points
    mono_pose_oracle counts in front, and its points before the scale -- (x * scale) / scale is not x bit for bit, so the
    restatement is run under scale = 1, where the product is exact -- give mono_pose_oracle's median bit for bit."""
    e = tp.params(ob)
    seen = 0
    for k, (pm, pose, ok) in mono_cases(ob, oracle).items():
        got = so.mono(oracle.svd, pm, pose, e, so.params(frame=0), ok=ok)
        if not ok:
            assert len(got["points"]) == 0
            continue
        assert len(got["points"]) == pose["n_front"], k
        unit = so.mono(oracle.svd, pm, dict(pose, scale=1.0), e, so.params(frame=0))
        assert unit["wide"][:, :3].tobytes() == unit["raw"].tobytes() == got["raw"].tobytes(), k
        dist = np.abs(unit["wide"][:, 0]) + np.abs(unit["wide"][:, 1]) + np.abs(unit["wide"][:, 2])
        assert np.float64(mp.median_by_rank(dist)).tobytes() == np.float64(pose["median"]).tobytes(), k
        seen += 1
    assert seen >= 11


def test_double_against_long_double(ob, oracle):
    """The double form against the long double form over every list and setting of the GPU tests: d_ref, the largest
    difference relative to the point's norm, is printed (measured: 7.5e-14); the two keep the same records; at most 1 % of
    the float outputs differ, none by more than 1 float ulp (measured: 0 of 235 915)."""
    if np.finfo(np.longdouble).eps >= np.finfo(np.float64).eps:
        pytest.skip("no wider arithmetic on this platform")
    d_ref, differ, total, worst = 0.0, 0, 0, 0
    pairs = []
    for k in range(len(SETTINGS)):
        pairs += list(zip(want_stereo(k), want_stereo(k, np.longdouble)))
    d_stereo = max(so.deviation(a, b) for a, b in pairs)
    for frame, Tw in ((0, None), (1, None), (1, TW)):
        a, b = want_mono(ob, oracle, frame, Tw), want_mono(ob, oracle, frame, Tw, np.longdouble)
        pairs += [(a[k], b[k]) for k in a]
    for a, b in pairs:
        assert np.array_equal(a["keep"], b["keep"])
        d_ref = max(d_ref, so.deviation(a, b))
        d, t, w = so.float_differences(a, b)
        differ += d; total += t; worst = max(worst, w)
    print(f"d_ref = {d_ref:.2e} (stereo alone {d_stereo:.2e}); floats that differ: {differ} of {total}, worst {worst} ulp")
    assert np.isfinite(d_ref) and d_ref < 1e-9 and total > 10000
    assert differ <= 0.01 * total and worst <= 1


# ------------------------------------------------------------------------------------------------------------ GPU
def run_stereo(pkg, sel, k):
    tr, frame, Tw, lim = SETTINGS[k]
    L = lists()
    pts, counts = pkg.scene_points_stereo(pkg.EgoParams.default(**KITTI), [L[i] for i in sel], np.array([tr] * len(sel)), np.ones(len(sel), np.int32),
                                          scene_params(pkg, frame, **lim), Tw)
    assert [len(p) for p in pts] == counts.tolist()
    return pts


def compare(got, want, what, exact=False):
    """integers and counts equal; floats byte-equal (exact) or within 1 ulp -> (floats that differ, floats compared)"""
    assert len(got) == len(want["points"]), (what, len(got), len(want["points"]))
    for name in ("src_pos", "i1p", "i1c"):
        assert np.array_equal(got[name], want["points"][name]), (what, name)
    if exact:
        assert got.tobytes() == want["points"].tobytes(), what
        return 0, 5 * len(got)
    d, t, w = so.float_differences(dict(points=got), want)
    assert w <= 1, (what, w)
    return d, t


@pytest.mark.gpu
def test_gpu_lengths_alone_and_mixed(pkg, gpu):
    """Lists of 0 .. 2 049 records at tr = 0, frame 1: each alone and all in one call, twice -- the same bytes from run to
    run and whatever else the call holds; every field byte-equal to the restatement (no transcendental value enters)."""
    want = want_stereo(0)
    sel = list(range(len(LENGTHS)))
    mixed, again = run_stereo(pkg, sel, 0), run_stereo(pkg, sel[::-1], 0)[::-1]
    for i in sel:
        alone = run_stereo(pkg, [i], 0)[0]
        assert alone.tobytes() == run_stereo(pkg, [i], 0)[0].tobytes() == mixed[i].tobytes() == again[i].tobytes(), LENGTHS[i]
        compare(alone, want[i], f"n = {LENGTHS[i]}", exact=True)
        assert len(alone) == LENGTHS[i]          # (this scene has no record to drop)
    for i, p in enumerate(run_stereo(pkg, sel, 1)):
        compare(p, want_stereo(1)[i], f"frame 0 n = {LENGTHS[i]}", exact=True)


@pytest.mark.gpu
def test_gpu_stereo_at_the_scenes_motion(pkg, gpu):
    """Both frames, with and without a rigid Tw, with and without the three filters: integers and counts equal, every float
    within 1 ulp, at most 1 % of them different (printed); the filters cut something and keep something, and hold a
    relative margin of at least 1e-6 to every record."""
    sel = list(range(len(LENGTHS)))
    for k in range(2, len(SETTINGS)):
        want = want_stereo(k)
        differ = total = 0
        for i, p in enumerate(run_stereo(pkg, sel, k)):
            d, t = compare(p, want[i], f"setting {k} n = {LENGTHS[i]}")
            differ += d; total += t
            assert want[i]["margin"] >= 1e-6, (k, i, want[i]["margin"])
        if SETTINGS[k][3]:
            kept = sum(len(w["points"]) for w in want)
            assert 0 < kept < sum(LENGTHS), kept
        print(f"setting {k}: {differ} of {total} floats differ from the restatement")
        assert differ <= 0.01 * total


@pytest.mark.gpu
def test_gpu_identity_tw_and_ignored_parameters(pkg, gpu):
    """Tw = identity gives the bytes of Tw = NULL; ransac_iters, reweighting and inlier_threshold are not read."""
    L = [lists()[i] for i in (4, 7, 11)]
    tr = np.array([TR] * 3); ok = np.ones(3, np.int32)
    e = pkg.EgoParams.default(**KITTI)
    for frame in (0, 1):
        sp = scene_params(pkg, frame)
        a = pkg.scene_points_stereo(e, L, tr, ok, sp)[0]
        b = pkg.scene_points_stereo(e, L, tr, ok, sp, np.eye(4))[0]
        c = pkg.scene_points_stereo(pkg.EgoParams.default(ransac_iters=1, reweighting=0, inlier_threshold=9.0, **KITTI), L, tr, ok, sp, np.array([np.eye(4)] * 3))[0]
        assert all(x.tobytes() == y.tobytes() == z.tobytes() and len(x) for x, y, z in zip(a, b, c))


@pytest.mark.gpu
def test_gpu_edge_records(pkg, gpu):
    """The kept set is the restatement's exactly: records with u1p - u2p <= 0 (clamped: kept at a depth of kilometres
    without a limit, removed by max_depth), a NaN coordinate, points behind the camera under a half turn; a list with
    ok = 0 among good ones has count 0 and leaves its neighbours' bytes unchanged (its tr, NaN, is not read); each of
    min_disp, max_depth and max_err alone cuts a known, non-empty subset."""
    e = pkg.EgoParams.default(**KITTI)
    base = noisy(600, 733)
    bad = base.copy()
    bad["u2p"][10] = bad["u1p"][10]; bad["u2p"][300] = bad["u1p"][300] + 5     # zero and negative disparity
    bad["v1c"][77] = np.nan; bad["u1p"][78] = np.nan
    cases = [("plain", bad, TR, {}), ("depth", bad, TR, dict(max_depth=60.5)), ("disp", base, TR, dict(min_disp=12.0)),
             ("err", base, TR, dict(max_err=0.3)), ("turn", base, np.array([0.0, 3.0, 0.0, 0.0, 0.0, 0.0]), {})]
    for name, pm, tr, lim in cases:
        for frame in (0, 1):
            want = so.stereo(pm, tr, cal(), so.params(frame=frame, **lim))
            got = pkg.scene_points_stereo(e, [pm], tr[None], [1], scene_params(pkg, frame, **lim))[0][0]
            assert np.array_equal(got["src_pos"], want["points"]["src_pos"]), (name, frame)
            assert want["margin"] >= 1e-6 and so.float_differences(dict(points=got), want)[2] <= 1
            keep = want["keep"]
            if name == "plain":
                assert not keep[77] and not keep[78] and keep[10] and keep[300] and keep.sum() == 598
                assert want["wide"][:, 2].max() > 1e5          # the clamped records, kilometres away
            if name == "depth":
                assert not keep[10] and not keep[300] and 500 < keep.sum() <= 596
            if name in ("disp", "err"):
                assert 0 < keep.sum() < 600
            if name == "turn":
                assert keep.all() if frame == 0 else not keep.any()
    # ok = 0 among good ones
    L = [lists()[5], base, lists()[8]]
    trs = np.array([TR, [np.nan] * 6, TR])
    pts, counts = pkg.scene_points_stereo(e, L, trs, [1, 0, 1])
    alone = [pkg.scene_points_stereo(e, [L[j]], TR[None], [1])[0][0] for j in (0, 2)]
    assert counts.tolist() == [255, 0, 1023] and pts[0].tobytes() == alone[0].tobytes() and pts[2].tobytes() == alone[1].tobytes()


@pytest.mark.gpu
def test_gpu_mono(pkg, ob, oracle, gpu):
    """vh_scene_points_mono on the lists of tests/test_mono_pose.py (9 .. 1 300 records, the refused ones included) under the
    restatement's pose for each: with frame = 0 and no limits the counts are the pose's points in front; integers equal,
    floats within 1 ulp (the bit-equal share is printed), both frames and with a rigid Tw; a refused pose gives count 0;
    the same bytes alone and among other lists."""
    cases = mono_cases(ob, oracle)
    names = list(cases)
    e = tp.params(pkg)
    args = ([cases[k][0] for k in names], pose_array(pkg, [cases[k][1] for k in names]), [int(cases[k][2]) for k in names])
    for frame, Tw in ((0, None), (1, None), (1, TW)):
        want = want_mono(ob, oracle, frame, Tw)
        pts, counts = pkg.scene_points_mono(e, *args, scene_params(pkg, frame), Tw)
        differ = total = 0
        for j, k in enumerate(names):
            d, t = compare(pts[j], want[k], f"mono {k} frame {frame}")
            differ += d; total += t
            if frame == 0:
                assert counts[j] == cases[k][1]["n_front"] * int(cases[k][2]), k
            if not cases[k][2]:
                assert counts[j] == 0
            assert not pts[j]["sigma_z"].any()
        print(f"mono frame {frame}, Tw {Tw is not None}: {total - differ} of {total} floats bit-equal to the restatement")
        assert differ <= 0.01 * total
    for k in (1300, 65, "nanrec"):
        j = names.index(k)
        alone = pkg.scene_points_mono(e, [args[0][j]], args[1][j:j + 1], [args[2][j]], scene_params(pkg, 1), TW)[0][0]
        assert alone.tobytes() == pts[j].tobytes(), k
    assert sum(1 for k in names if not cases[k][2]) >= 5 and counts.max() > 1000


def mapped(points, pos):
    """the stateless form's points on an inlier list, src_pos mapped to the list the classification ran on"""
    out = points.copy()
    out["src_pos"] = pos[points["src_pos"]]
    return out


def check_handle_stereo(pkg, ob, g, e, what, rows=None):
    """estimateMotion, motionInliers, refitMotion(reclassify), then scenePoints: every stream byte for byte the stateless
    form on the getters' inlier lists under the refined motion, both frames and with Tw; the getters' capacity rule."""
    S = g.S
    tr0, ok0, _ = g.estimateMotion(e, mi.rand3_of(ob, e, S))
    g.motionInliers(e, tr0, ok0.astype(np.int32))
    tr, ok, _, _ = g.refitMotion(e, reclassify=True)
    inl = [g.getInlierMatches(s) for s in range(S)]
    total = 0
    for frame, Tw in ((1, None), (0, TW)):
        sp = scene_params(pkg, frame, max_depth=50.0)
        counts = g.scenePoints(e, sp, Tw)
        want = pkg.scene_points_stereo(e, [x[0] for x in inl], tr, ok.astype(np.int32), sp, Tw)[0]
        for s in range(S):
            got = g.getScenePoints(s)
            assert len(got) == counts[s] and got.tobytes() == mapped(want[s], inl[s][1]).tobytes(), (what, frame, s)
        if rows is not None:
            assert all(counts[r] == 0 for r in range(S) if r not in rows), (what, counts)
        total += int(counts.sum())
        cap = int(counts.max())
        out, c2 = g.getScenePointsAll(cap)
        assert np.array_equal(c2, counts) and all(out[s, :counts[s]].tobytes() == g.getScenePoints(s).tobytes() for s in range(S))
        if cap > 1:
            expect(pkg, pkg.VH_ERR_CAPACITY, lambda: g.getScenePointsAll(cap - 1))
            s = int(np.argmax(counts)); n = C.c_int32(0); few = np.zeros(cap - 1, pkg.SCENE_POINT_DTYPE)
            assert pkg._lib().vh_group_get_scene_points(g._h, s, ptr(few), cap - 1, C.byref(n)) == pkg.VH_ERR_CAPACITY
            assert n.value == cap and few.tobytes() == g.getScenePoints(s)[:cap - 1].tobytes()
    assert all(g.getInlierMatches(s)[0].tobytes() == inl[s][0].tobytes() for s in range(S)), what   # the classification is untouched
    return total


def check_handle_mono(pkg, ob, g, what, rows=None):
    """estimateMotionMono(model) -> motionInliersMono -> poseMono -> scenePoints under the pose left on the device."""
    e = tm.hmono(pkg, inlier_threshold=3e-5, motion_threshold=1e300)   # (the synthetic frames move little: no refusal for that)
    S = g.S
    _, _, _, models = g.estimateMotionMono(e, tm.rand8_of(ob, e, S), model=True)
    g.motionInliersMono(e, models, models["valid"].astype(np.int32))
    expect(pkg, pkg.VH_ERR_STATE, lambda: g.scenePoints(e))            # no pose yet for this classification
    tr, ok, _, pose = g.poseMono(e, pose=True)
    inl = [g.getInlierMatches(s) for s in range(S)]
    total = 0
    for frame, Tw in ((0, None), (1, TW)):
        sp = scene_params(pkg, frame)
        counts = g.scenePoints(e, sp, Tw)
        want = pkg.scene_points_mono(e, [x[0] for x in inl], pose, ok.astype(np.int32), sp, Tw)[0]
        for s in range(S):
            got = g.getScenePoints(s)
            assert len(got) == counts[s] and got.tobytes() == mapped(want[s], inl[s][1]).tobytes(), (what, frame, s)
            if frame == 0:
                assert counts[s] == (pose["n_front"][s] if ok[s] else 0), (what, s)
        if rows is not None:
            assert all(counts[r] == 0 for r in range(S) if r not in rows), (what, counts)
        total += int(counts.sum())
    expect(pkg, pkg.VH_ERR_STATE, lambda: g.scenePoints(pkg.EgoParams.default(**KITTI)))   # the wrong kind of classification
    g.motionInliersMono(e, models, models["valid"].astype(np.int32))
    expect(pkg, pkg.VH_ERR_STATE, lambda: g.scenePoints(e))            # classified again: the pose belongs to the lists before
    print(f"{what}: {total} points, pose reasons {pose['reason'].tolist()}")
    return total


@pytest.mark.gpu
def test_gpu_group_of_three_stereo(pkg, ob, gpu):
    """A group of S = 3 on quad lists (one stream of constant images: empty lists), after refitMotion(reclassify=True)."""
    fr, dims = pd.frames_of(pkg), pd.dims_of(pkg)
    e = pd.ego_of(pkg)
    g = pkg.StreamGroup(pd.S, pkg.Params.default())
    total = 0
    for t in range(3):
        pd.push(g, fr, t, dims)
        if t == 0:
            continue
        g.matchFeatures(QUAD)
        total += check_handle_stereo(pkg, ob, g, e, f"group t{t}")
        assert g.getScenePoints(1).shape == (0,)
    assert total > 0
    g.close()


@pytest.mark.gpu
def test_gpu_group_of_three_mono(pkg, ob, gpu):
    """A group of S = 3 on flow lists (one stream of constant images), after poseMono."""
    dims = sr.dims_of(pkg)
    frames = [sr.frames_of(pkg, 3, seed) for seed in (81, 82, 83)]
    frames[1] = [(np.full_like(a, 90), np.full_like(b, 90)) for a, b in frames[1]]
    g = pkg.StreamGroup(3, pkg.Params.default())
    total = 0
    for t in range(3):
        g.pushBack(np.stack([f[t][0] for f in frames]), None, dims)
        if t == 0:
            continue
        g.matchFeatures(FLOW)
        total += check_handle_mono(pkg, ob, g, f"group mono t{t}")
    assert total > 0
    g.close()


@pytest.mark.gpu
def test_gpu_sequence_handle_and_lone_matcher(pkg, ob, gpu):
    """A sequence handle across a chunk boundary (chunks of 4 and 2 frames; rows without a pair: count 0), stereo and mono,
    and a lone matcher, each byte for byte the stateless form."""
    dims = sr.dims_of(pkg)
    frames = sr.frames_of(pkg, 6, 74)
    e = mi.hego(pkg, inlier_threshold=2.5)
    g = pkg.SequenceGroup(4, pkg.Params.default())
    sr.push(g, frames, 0, 4, dims)
    g.matchFeatures(QUAD)
    check_handle_stereo(pkg, ob, g, e, "sequence chunk 0", rows=(1, 2, 3))
    check_handle_mono(pkg, ob, g, "sequence mono chunk 0", rows=(1, 2, 3))
    sr.push(g, frames, 4, 2, dims)
    g.matchFeatures(QUAD)
    check_handle_stereo(pkg, ob, g, e, "sequence chunk 1", rows=(0, 1))
    g.close()
    m = pkg.Matcher(pkg.Params.default(), outlier_removal=True)
    for left, right in frames[:2]:
        m.pushBack(left, right, dims)
    m.matchFeatures(QUAD)
    n = m.motionInliers(e, mi.TR2)
    tr, ok, _, _ = m.refitMotion(e, reclassify=True)
    inl, pos = m.getInlierMatches()
    got = m.scenePoints(e, Tw=TW)
    want = pkg.scene_points_stereo(e, [inl], tr[None], [int(ok)], None, TW)[0][0]
    assert n > 6 and len(got) > 0 and got.tobytes() == mapped(want, pos).tobytes() == m.getScenePoints().tobytes()
    m.close()


@pytest.mark.gpu
def test_gpu_state_rules_memory_and_failed_allocation(pkg, ob, gpu):
    """VH_ERR_STATE before a classification, for the mono entry without a pose, for the wrong kind of classification, after
    the next push; the getters before any points; vh_group_device_bytes is unchanged until the first call, a refused
    allocation is VH_ERR_HIP before any launch and leaves the handle as it was, the repeated call adds exactly the
    documented block -- 32 bytes per record slot, 4 per tile of 256 slots, 128 + 4 per stream, each array rounded up to 256
    -- once; profile scope "scene_points"."""
    dims = sr.dims_of(pkg)
    frames = [sr.frames_of(pkg, 3, seed) for seed in (85, 86)]
    e = mi.hego(pkg, inlier_threshold=2.5)
    mono = tm.hmono(pkg, inlier_threshold=3e-5)
    state = pkg.VH_ERR_STATE
    S, MM = 2, 4096
    g = pkg.StreamGroup(S, pkg.Params.default(), max_matches=MM)
    g.profileEnable(True)
    expect(pkg, state, lambda: g.scenePoints(e))                       # nothing pushed
    for t in range(2):
        g.pushBack(np.stack([f[t][0] for f in frames]), np.stack([f[t][1] for f in frames]), dims)
    g.matchFeatures(QUAD)
    expect(pkg, state, lambda: g.scenePoints(e))                       # not classified yet
    expect(pkg, state, lambda: g.getScenePoints(0))
    tr = np.array([mi.TR2] * S); ok = np.ones(S, np.int32)
    g.motionInliers(e, tr, ok)
    expect(pkg, state, lambda: g.scenePoints(mono))                    # a stereo classification: the mono entry refuses
    expect(pkg, state, lambda: g.scenePointsDevice())
    inl = [g.getInlierMatches(s) for s in range(S)]
    g.synchronize()
    bytes0 = g.deviceBytes()
    g.debugFailNextAlloc()
    expect(pkg, pkg.VH_ERR_HIP, lambda: g.scenePoints(e))
    g.synchronize()
    assert g.deviceBytes() == bytes0 and g.profileRead("scene_points")[1] == 0
    assert all(g.getInlierMatches(s)[0].tobytes() == inl[s][0].tobytes() for s in range(S))
    counts = g.scenePoints(e)                                          # the repeated call
    want = pkg.scene_points_stereo(e, [x[0] for x in inl], tr, ok)[0]
    assert all(g.getScenePoints(s).tobytes() == mapped(want[s], inl[s][1]).tobytes() for s in range(S)) and counts.sum() > 0
    _, stride = g.scenePointsDevice()
    up = lambda b: (b + 255) // 256 * 256  # noqa: E731
    block = up(32 * S * stride) + up(4 * S * ((stride + 255) // 256)) + up(128 * S) + up(4 * S)
    assert stride >= MM and g.deviceBytes() == bytes0 + block, (g.deviceBytes() - bytes0, block)
    g.scenePoints(e, scene_params(pkg, 0), TW)
    g.synchronize()
    assert g.deviceBytes() == bytes0 + block and g.profileRead("scene_points")[1] == 2
    _, _, _, models = g.estimateMotionMono(mono, tm.rand8_of(ob, mono, S), model=True)
    g.motionInliersMono(mono, models, models["valid"].astype(np.int32))
    expect(pkg, state, lambda: g.scenePoints(mono))                    # a mono classification without a pose
    expect(pkg, state, lambda: g.scenePoints(e))                       # ... and the stereo entry refuses it
    g.poseMono(mono)
    g.scenePoints(mono)
    assert g.deviceBytes() >= bytes0 + block
    g.pushBack(np.stack([f[2][0] for f in frames]), np.stack([f[2][1] for f in frames]), dims)
    expect(pkg, state, lambda: g.scenePoints(mono))                    # pushed: the pair the lists belong to is over
    g.matchFeatures(QUAD)
    expect(pkg, state, lambda: g.getScenePoints(0))                    # the points end with the next match
    g.close()
