"""Dense list stages on lists longer than one scan round (DESIGN.md sections 4.10, 4.11, 4.20 - 4.22).

Every whole-list stage ends in one compaction pattern: a survivor count per tile, and one workgroup per list that scans
those counts in rounds of 256 tiles, carrying `base` from round to round.  inlier_scan_kernel (tiles of 1 024 records)
starts its second round at 262 145 records, scene_scan_kernel (tiles of 256; scene points and both landmark forms) at
65 537.  The other test files stay far below both; this one goes past them: lists of exactly one round, one round and one
tile, and three rounds, alone and between other lists' rows, on the stateless entries and on the getters of a lone
matcher at the suite's own 4K configurations.

The device post chain is not covered and need not be: its vote caps every list at 65 535 records and its dense stages
use 1 024-record tiles, so none of its lists reaches a second round.  This is about the stateless entries and the handle
getters.

Expected values come from the numpy restatements the other files use, unchanged (inlier_oracle, mono_inlier_oracle,
scene_points_oracle, landmark_oracle), under the rules those files already use: stereo inliers byte for byte but for the
records within 1e-9 of the threshold (near_threshold), mono inliers byte for byte, stereo scene points byte for byte at
tr = 0 (no transcendental value enters, so no filter compare can flip and no margin is needed), landmarks byte for byte;
at a non-zero motion and in the mono scene-point form test_scene_points.compare (integers equal, floats within 1 ulp).

Records.  The stereo lists are test_motion_refit.noisy's (the vectorised builder of the dense stereo tests; the per-record
Python loops of egomotion_scene.scene would take minutes at 10^6 records), the flow lists mono_pose_oracle.ground_scene's
under test_mono_pose.true_model, each at a noise level that leaves a mixed outcome; tracks and points are
test_sequence_landmarks.build's.  The mono scene-point restatement triangulates record by record and takes about 1 s
for 65 537 records here, so the one mono case the round boundary asks for is in.

test_long_lists_are_not_vacuous asserts on the restatements alone that every span of 256 consecutive tiles of every long
list keeps between 30 % and 70 % of its records, that the tile counts differ, and that the lists cross the boundaries
they are there for.  The CPU part of this file (building the lists and every restatement) takes about 6 s."""
import numpy as np
import pytest

import inlier_oracle as io
import landmark_oracle as lo
import mono_inlier_oracle as mo
import mono_pose_oracle as mp
import mono_refit_oracle as mfo
import scene_points_oracle as so
import test_mono_inliers as tm
import test_mono_pose as tp
import test_motion_inliers as mi
import test_motion_refit as mr
import test_scene_points as tsp
import test_sequence_landmarks as sl
from egomotion_scene import KITTI

ROUND = 256                        # tiles per round of both scan kernels
INLIER_TILE, SCENE_TILE = 1024, 256   # VH_INLIER_TILE, SCN_T
INLIER_LONG = (262144, 262145, 524289)  # one full round; a second round of one tile; three rounds
SCENE_LONG = (65536, 65537, 131073)
# seeds of the long lists; the third of each is one for which the restatement keeps the list's last record -- the one
# record of the third round -- so that round's count is not zero (asserted in test_long_lists_are_not_vacuous)
STEREO_SEEDS, FLOW_SEEDS, SCENE_SEEDS = (8100, 8101, 8103), (8200, 8201, 8203), (8300, 8301, 8305)
STEREO_NOISE, FLOW_NOISE = 1.1, 1.0
THR = tm.THR
SCENE_LIMITS = dict(min_disp=7.0, max_depth=48.0, max_err=0.55)
MONO_LIMITS = dict(max_err=0.25)
TW = tsp.TW
ZERO = np.zeros(6)
LANDMARK_ROWS = (131073, 131073, 65537, 300)  # rows of one chain; the last is the second call's, through the carry
SHORT_ROWS = (300, 257, 280, 40)              # the short chain beside it
N_CARRY = 140000
LP = lo.params(min_obs=2, max_missed=1, max_dist=0.5, gate_sigma=3.0)
_CACHE = {}


def cached(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def tiles_of(n, tile):
    return (n + tile - 1) // tile


def span_fractions(keep, tile):
    """-> (the kept fraction of every span of ROUND consecutive tiles -- of the whole list where it has fewer --, the
    per-tile counts)"""
    keep = np.asarray(keep).astype(np.int64)
    n = len(keep)
    starts = np.arange(0, n, tile)
    cnt = np.add.reduceat(keep, starts)
    size = np.minimum(tile, n - starts)
    w = min(ROUND, len(starts))
    c, z = np.concatenate([[0], np.cumsum(cnt)]), np.concatenate([[0], np.cumsum(size)])
    return (c[w:] - c[:-w]) / (z[w:] - z[:-w]), cnt


def mixed(keep, tile, what):
    frac, cnt = span_fractions(keep, tile)
    assert 0.3 <= frac.min() and frac.max() <= 0.7, (what, frac.min(), frac.max())
    assert len(np.unique(cnt)) > 1, what
    return float(frac.min()), float(frac.max())


# ------------------------------------------------------------------------------------------------------------ inputs
def stereo_inlier_case():
    """-> (lists, tr [6, 6], ok [6], want): an empty list, the three long ones with one long list under ok = 0 between
    them, and 777 records"""
    def make():
        cal = mi._Cal(inlier_threshold=2.0, **KITTI)
        long_ = [mr.noisy(n, seed, noise=STEREO_NOISE) for seed, n in zip(STEREO_SEEDS, INLIER_LONG)]
        lists = [mr.noisy(0, 8000), long_[0], long_[1], long_[1], long_[2], mr.noisy(777, 8001, noise=STEREO_NOISE)]
        ok = np.array([1, 1, 1, 0, 1, 1], np.int32)
        want = []
        for pm, o in zip(lists, ok):
            f, s = io.inliers(pm, mr.TR, cal, ok=bool(o))
            want.append((f, s, io.near_threshold(s, cal, 1e-9)))
        return lists, np.array([mr.TR] * len(lists), np.float64), ok, want
    return cached("stereo_inliers", make)


def mono_inlier_case():
    """the same shape on flow lists -> (lists, models, ok [6], want flags)"""
    def make():
        long_ = [mp.ground_scene(tp.dtype(), n, seed, noise=FLOW_NOISE) for seed, n in zip(FLOW_SEEDS, INLIER_LONG)]
        short = mp.ground_scene(tp.dtype(), 777, 8209, noise=FLOW_NOISE)
        lists = [long_[0][:0], long_[0], long_[1], long_[1], long_[2], short]
        models = [tp.true_model(short)] + [tp.true_model(pm) for pm in lists[1:]]
        ok = np.array([1, 1, 1, 0, 1, 1], np.int32)
        want = [mo.inliers(pm, m, THR, ok=bool(o))[0] for pm, m, o in zip(lists, models, ok)]
        return lists, models, ok, want
    return cached("mono_inliers", make)


SCENE_SETTINGS = ((0, None), (1, TW))   # (frame, Tw)


def scene_case():
    """-> (lists, ok [6], {setting: want per list}): 0, 65 536, 65 537, the latter again under ok = 0, 131 073 and 300
    records of a standing camera's scene (tr = 0), cut by all three filters"""
    def make():
        long_ = [mr.noisy(n, seed, tr=ZERO, noise=0.3) for seed, n in zip(SCENE_SEEDS, SCENE_LONG)]
        lists = [mr.noisy(0, 8000), long_[0], long_[1], long_[1], long_[2], mr.noisy(300, 8309, tr=ZERO, noise=0.3)]
        ok = np.array([1, 1, 1, 0, 1, 1], np.int32)
        cal = mi._Cal(**KITTI)
        want = {k: [so.stereo(pm, ZERO, cal, so.params(frame=frame, **SCENE_LIMITS), Tw=Tw, ok=bool(o)) for pm, o in zip(lists, ok)]
                for k, (frame, Tw) in enumerate(SCENE_SETTINGS)}
        return lists, ok, want
    return cached("scene", make)


def mono_scene_case(ob, oracle):
    """65 537 flow records under the scene's own pose (handed to both sides) -> (pm, pose dict, want)"""
    def make():
        pm = mp.ground_scene(tp.dtype(), SCENE_LONG[1], 8400)
        t = np.array(mfo.MOTION[3:], np.float64)
        scale = float(np.sqrt((t * t).sum()))
        pose = dict(R=mfo._rot(*mfo.MOTION[:3]).reshape(9), t=t / scale, scale=scale, reason=0)
        want = so.mono(oracle.svd, pm, pose, tp.params(ob), so.params(frame=1, **MONO_LIMITS), Tw=TW)
        return pm, pose, want
    return cached("mono_scene", make)


def landmark_case():
    """One chain of four rows (131 073, 131 073, 65 537 and 300 records) from a carry of 140 000 states, a short chain beside
    it, and the restatement's answers row by row -> dict.  A quarter of every row's records has no point (gaps that run
    into max_missed = 1); gross outliers restart tracks at the gate; prev points past the predecessor on both sides; record
    131 072 of row 1 -- the one record of the third scan round -- is a head, and a record of row 2 continues it."""
    def make():
        rng = np.random.default_rng(8500)
        out = {}
        for name, rows, n_carry, seed in (("long", LANDMARK_ROWS, N_CARRY, 8501), ("short", SHORT_ROWS, 200, 8502)):
            tracks, points = sl.build(rows, seed, n_carry, 1, False, ())
            if name == "long":
                last = rows[1] - 1
                tracks[1]["prev"][last] = -1
                free = np.flatnonzero(tracks[2]["prev"] == -1)
                tracks[2]["prev"][free[free > 40000][0]] = last      # (no other record continues it: its old successor is unlinked)
                dup = np.flatnonzero(tracks[2]["prev"] == last)
                tracks[2]["prev"][dup[1:]] = -1
            points = [p[rng.random(len(p)) < 0.75] for p in points]
            carry = sl.carry_of(n_carry, seed + 10)
            # the states row 0 continues lie 0.1 m from its first observation, so that the gate lets most of them pass
            # (carry_of's lie anywhere in the scene: the gate would restart nearly every track of row 0)
            t0, p0 = tracks[0], points[0]
            q = t0["prev"][p0["src_pos"]]
            at = (q >= 0) & (q < n_carry) & np.isfinite(p0["x"])
            k = (1 + rng.integers(0, 3, int(at.sum()))) * (rng.random(int(at.sum())) < 0.85)
            w = 4.0 * k
            c = carry[q[at]]
            c["sw"] = w; c["n_obs"] = k; c["n_missed"] = 0
            for axis, off in (("x", 0.1), ("y", 0.0), ("z", -0.05)):
                c["sw" + axis] = w * (p0[axis][at].astype(np.float64) + off)
            carry[q[at]] = c
            events = {}
            lms, states = sl.chain_oracle(tracks, points, carry, LP, events)
            out[name] = dict(tracks=tracks, points=points, carry=carry, lms=lms, states=states, events=events)
        return out
    return cached("landmarks", make)


# ------------------------------------------------------------------------------------------------------------ CPU
def test_long_lists_are_not_vacuous(ob, oracle):
    """On the restatements alone: every long list crosses the round boundary it is there for; in every span of 256
    consecutive tiles the kept fraction lies in [0.3, 0.7] and the tile counts differ; the stereo lists hold at most
    0.1 % near-threshold records; the landmark rows hold every event and shape the issue of long lists names.  The
    fractions and the time the inputs took are printed."""
    import time
    t0 = time.time()
    assert [tiles_of(n, INLIER_TILE) for n in INLIER_LONG] == [ROUND, ROUND + 1, 2 * ROUND + 1]
    assert [tiles_of(n, SCENE_TILE) for n in SCENE_LONG] == [ROUND, ROUND + 1, 2 * ROUND + 1]
    lists, _, ok, want = stereo_inlier_case()
    assert [len(pm) for pm in lists] == [0, 262144, 262145, 262145, 524289, 777] and ok.tolist() == [1, 1, 1, 0, 1, 1]
    for i in (1, 2, 4):
        print("stereo inliers", len(lists[i]), mixed(want[i][0], INLIER_TILE, ("stereo", i)))
        assert want[i][2].sum() <= 0.001 * len(lists[i])
    assert want[4][0][-1] == 1
    assert not want[3][0].any() and 0 < want[5][0].sum() < 777
    lists, models, ok, want = mono_inlier_case()
    assert [len(pm) for pm in lists] == [0, 262144, 262145, 262145, 524289, 777]
    for i in (1, 2, 4):
        print("mono inliers", len(lists[i]), mixed(want[i], INLIER_TILE, ("mono", i)))
    assert want[4][-1] == 1 and not want[3].any() and 0 < want[5].sum() < 777
    lists, ok, want = scene_case()
    assert [len(pm) for pm in lists] == [0, 65536, 65537, 65537, 131073, 300]
    for k in range(len(SCENE_SETTINGS)):
        for i in (1, 2, 4):
            print("scene points", k, len(lists[i]), mixed(want[k][i]["keep"], SCENE_TILE, ("scene", k, i)))
            assert len(want[k][i]["points"]) > 0.3 * len(lists[i])
        assert len(want[k][3]["points"]) == 0 and 0 < len(want[k][5]["points"]) < 300
    assert want[0][4]["points"]["src_pos"].max() > 2 * ROUND * SCENE_TILE - 1        # a survivor in the third round
    pm, pose, wm = mono_scene_case(ob, oracle)
    assert len(pm) == 65537 and wm["margin"] >= 1e-6, wm["margin"]
    print("mono scene points", mixed(wm["keep"], SCENE_TILE, "mono scene"))
    lm = landmark_case()
    L = lm["long"]
    assert tuple(len(t) for t in L["tracks"]) == LANDMARK_ROWS
    assert all(L["events"].get(k, 0) >= 100 for k in ("restart", "drop")), L["events"]
    n_pred = [N_CARRY] + [len(t) for t in L["tracks"][:-1]]
    for s, (t, p, lms, st) in enumerate(zip(L["tracks"], L["points"], L["lms"], L["states"])):
        prev = t["prev"]
        assert (prev < -1).any() and (prev >= n_pred[s]).any(), s
        assert len(np.unique(p["src_pos"])) == len(p) and (np.diff(p["src_pos"]) > 0).all()
        if s < 3:
            emitted = np.zeros(len(t), bool); emitted[lms["src_pos"]] = True
            print("landmarks row", s, len(t), len(p), mixed(emitted, SCENE_TILE, ("landmarks", s)))
            head = (prev < 0) | (prev >= n_pred[s])
            ends = np.ones(n_pred[s], bool); ends[prev[~head]] = False       # predecessors nobody continues: a chain ends there
            if s == 1:      # chains start on both sides of record 65 536 and in the third round
                assert head[:65536].any() and head[65536:131072].any() and head[131072], s
            else:           # ... and end on both sides of it (the predecessor of rows 0 and 2 is longer than one round)
                assert ends[:65536].any() and ends[65536:].sum() > 100, s
    assert max(len(p) for p in L["points"]) > 65536                          # more than one round of records carry an observation
    assert (L["points"][1]["src_pos"] >= 65536).sum() > 30000
    assert L["tracks"][1]["prev"][131072] == -1 and (L["tracks"][2]["prev"] == 131072).sum() == 1   # the third round's head is continued
    assert (L["tracks"][3]["prev"] > 65535).any() and (L["tracks"][2]["prev"] > 131071).any()
    assert sum(len(x) for x in lm["short"]["lms"]) > 0
    print(f"inputs and restatements: {time.time() - t0:.1f} s")


# ------------------------------------------------------------------------------------------------------------ GPU
def same_bytes(a, b, what):
    assert len(a) == len(b), what
    for x, y in zip(a, b):
        assert np.asarray(x).tobytes() == np.asarray(y).tobytes(), what


def inlier_result_equal(a, b, k, j, what):
    """list k of result a against list j of result b: flags, count, records, positions"""
    assert a[0][k].tobytes() == b[0][j].tobytes() and a[1][k] == b[1][j], what
    assert a[2][k].tobytes() == b[2][j].tobytes() and a[3][k].tobytes() == b[3][j].tobytes(), what


@pytest.mark.gpu
def test_gpu_stereo_inliers_past_one_round(pkg, gpu):
    """vh_motion_inliers on 262 144, 262 145 and 524 289 records between an empty list, a long list under ok = 0 and one of
    777 records: flags, n_inliers, the compacted records and src_pos are the restatement's (test_motion_inliers.check_against:
    byte for byte outside the records within 1e-9 of the threshold); each long list alone gives the bytes it gives in the
    mixed call; two runs give the same bytes."""
    lists, tr, ok, want = stereo_inlier_case()
    e = pkg.EgoParams.default(**KITTI)
    got = pkg.motion_inliers(e, lists, tr, ok)
    for i, pm in enumerate(lists):
        mi.check_against(pm, want[i], got[0][i], got[1][i], got[2][i], got[3][i], ("mixed", i, len(pm)))
    again = pkg.motion_inliers(e, lists, tr, ok)
    for i in range(len(lists)):
        inlier_result_equal(again, got, i, i, ("rerun", i))
    for i in (1, 2, 4):
        alone = pkg.motion_inliers(e, [lists[i]], tr[[i]], ok[[i]])
        inlier_result_equal(alone, got, 0, i, ("alone", i))


@pytest.mark.gpu
def test_gpu_mono_inliers_past_one_round(pkg, gpu):
    """vh_motion_inliers_mono on the same shape of call, flow lists under their true models: everything byte for byte the
    restatement's, alone as in the mixed call, and from run to run."""
    lists, models, ok, want = mono_inlier_case()
    e = tm.mono_params(pkg)
    marr = mo.as_array(models, pkg.MONO_MODEL_DTYPE)
    got = pkg.motion_inliers_mono(e, lists, marr, ok)
    for i, pm in enumerate(lists):
        tm.check_against(pm, want[i], got[0][i], got[1][i], got[2][i], got[3][i], ("mixed", i, len(pm)))
    again = pkg.motion_inliers_mono(e, lists, marr, ok)
    for i in range(len(lists)):
        inlier_result_equal(again, got, i, i, ("rerun", i))
    for i in (1, 2, 4):
        alone = pkg.motion_inliers_mono(e, [lists[i]], marr[[i]], ok[[i]])
        inlier_result_equal(alone, got, 0, i, ("alone", i))


@pytest.mark.gpu
@pytest.mark.parametrize("setting", range(len(SCENE_SETTINGS)))
def test_gpu_scene_points_past_one_round(setting, pkg, gpu):
    """vh_scene_points_stereo at tr = 0 on 65 536, 65 537 and 131 073 records between lists of 0 and 300 and a long list
    under ok = 0, all three filters on, frame 0 without and frame 1 with a Tw: byte for byte the restatement's, alone as
    in the mixed call, and from run to run."""
    lists, ok, want = scene_case()
    frame, Tw = SCENE_SETTINGS[setting]
    e = pkg.EgoParams.default(**KITTI)
    sp = pkg.SceneParams.default(frame=frame, **SCENE_LIMITS)
    tr = np.zeros((len(lists), 6))
    pts, counts = pkg.scene_points_stereo(e, lists, tr, ok, sp, Tw)
    assert [len(p) for p in pts] == counts.tolist()
    for i in range(len(lists)):
        tsp.compare(pts[i], want[setting][i], ("mixed", setting, i), exact=True)
    same_bytes(pkg.scene_points_stereo(e, lists, tr, ok, sp, Tw)[0], pts, "rerun")
    for i in (1, 2, 4):
        alone = pkg.scene_points_stereo(e, [lists[i]], tr[[i]], ok[[i]], sp, Tw)[0][0]
        assert alone.tobytes() == pts[i].tobytes(), ("alone", setting, i)


@pytest.mark.gpu
def test_gpu_mono_scene_points_past_one_round(pkg, ob, oracle, gpu):
    """vh_scene_points_mono on 65 537 records (frame 1, a Tw, max_err on; the margin of 1e-6 is asserted on the CPU) between
    a short list and a refused one: integers and counts equal, floats within 1 ulp and at most 1 % of them different
    (test_scene_points.compare); alone as in the mixed call."""
    pm, pose, want = mono_scene_case(ob, oracle)
    e = tp.params(pkg)
    sp = pkg.SceneParams.default(frame=1, **MONO_LIMITS)
    short = pm[:300]
    poses = tsp.pose_array(pkg, [pose] * 3)
    pts, counts = pkg.scene_points_mono(e, [short, pm, short], poses, [1, 1, 0], sp, TW)
    d, t = tsp.compare(pts[1], want, "mono 65 537")
    print(f"mono scene points: {t - d} of {t} floats bit-equal to the restatement")
    assert d <= 0.01 * t and counts[2] == 0
    tsp.compare(pts[0], so.mono(oracle.svd, short, pose, tp.params(ob), so.params(frame=1, **MONO_LIMITS), Tw=TW), "mono short")
    alone = pkg.scene_points_mono(e, [pm], poses[:1], [1], sp, TW)[0][0]
    assert alone.tobytes() == pts[1].tobytes()


@pytest.mark.gpu
def test_gpu_landmarks_past_one_round(pkg, gpu):
    """vh_landmarks_update step by step (the long row, the short chain's row and an empty list in one call, each step's
    states feeding the next) and vh_landmarks_chain (three rows in one call from the carry, then the fourth row, an empty
    one and a short one in a second call through the states the first returned): landmarks and states byte for byte
    landmark_oracle's applied list by list, so the chain form equals the update form byte for byte; twice."""
    case = landmark_case()
    L, S = case["long"], case["short"]
    lp = sl.lparams(pkg, LP)
    none_t, none_p = np.zeros(0, lo.TRACK), np.zeros(0, lo.POINT)
    for run in range(2):
        state = [L["carry"], S["carry"], np.zeros(0, lo.STATE)]
        for t in range(4):
            lm, state = pkg.landmarks_update([L["tracks"][t], S["tracks"][t], none_t], [L["points"][t], S["points"][t], none_p], state, lp)
            sl.same(lm, [L["lms"][t], S["lms"][t], np.zeros(0, lo.LANDMARK)], f"update run {run} step {t}")
            sl.same(state, [L["states"][t], S["states"][t], np.zeros(0, lo.STATE)], f"update run {run} step {t} state")
        lm, st = pkg.landmarks_chain(L["tracks"][:3], L["points"][:3], L["carry"], lp)
        sl.same(lm, L["lms"][:3], f"chain run {run}"); sl.same(st, L["states"][:3], f"chain run {run} state")
        tail_t, tail_p = [L["tracks"][3], none_t, S["tracks"][0]], [L["points"][3], none_p, S["points"][0]]
        lm, st2 = pkg.landmarks_chain(tail_t, tail_p, st[2], lp)
        head = lo.update(S["tracks"][0], S["points"][0], None, LP)    # (after an empty row every record starts anew)
        sl.same(lm, [L["lms"][3], np.zeros(0, lo.LANDMARK), head[0]], f"chain tail run {run}")
        sl.same(st2, [L["states"][3], np.zeros(0, lo.STATE), head[1]], f"chain tail run {run} state")
    lm, st = pkg.landmarks_chain(S["tracks"], S["points"], S["carry"], lp)
    sl.same(lm, S["lms"], "short chain"); sl.same(st, S["states"], "short chain state")


# ---- the handle forms at the suite's own 4K configurations
W4K, H4K = 3840, 2160
DIMS4K = [W4K, H4K, 3840]


@pytest.mark.gpu
def test_gpu_4k_flow_mono_inliers_on_a_lone_matcher(pkg, oracle, gpu):
    """The frames and parameters of test_4k_dense_maxima_beyond_the_old_envelope: more than 262 144 flow matches on a lone
    matcher (the list is taken as given: that test holds it to the oracle).  The model is the restatement's model_of on
    every 200th record; the threshold is the median of the restatement's own positive distances, so that about half the
    list is kept.  motionInliersMono's count, getInlierMatches' records and positions -- and the flags they imply: a lone
    matcher has no flag getter -- are byte for byte stateless motion_inliers_mono's on getMatches() and the restatement's."""
    over = {"nms_n": 2, "match_binsize": 25, "match_radius": 60}
    Ip = pkg.synth.frame(W4K, H4K, 0, 0, 1, 4, 9); Ic = pkg.synth.frame(W4K, H4K, 3, 1, 1, 4, 9)
    m = pkg.Matcher(pkg.Params.default(**over), outlier_removal=False)
    m.pushBack(Ip, None, DIMS4K, False)
    m.pushBack(Ic, None, DIMS4K, False)
    m.matchFeatures(pkg.METHOD_FLOW)
    pm = m.getMatches()
    assert len(pm) > 262144
    sub = pm[::200]
    model = mo.model_of(oracle.svd, sub, np.arange(len(sub)))
    assert model["valid"] == 1.0
    # the subset's normalisation serves the whole list: the model is one frame and one F, handed to both sides
    d = np.abs(mo.distances(pm, model))
    pos_d = d[np.isfinite(d) & (d > 0)]
    thr = float(np.median(pos_d)) if len(pos_d) else THR
    want = mo.inliers(pm, model, thr)[0]
    frac, _ = span_fractions(want, INLIER_TILE)
    print(f"4K flow: {len(pm)} matches, threshold {thr:.3e}, kept {want.mean():.3f}, per span {frac.min():.3f} .. {frac.max():.3f}")
    assert 0 < want.sum() < len(pm)
    e = tm.mono_params(pkg, inlier_threshold=thr)
    marr = mo.as_array([model], pkg.MONO_MODEL_DTYPE)
    count = m.motionInliersMono(e, marr)
    out, pos = m.getInlierMatches()
    m.close()
    flags = np.zeros(len(pm), np.uint8); flags[pos] = 1
    tm.check_against(pm, want, flags, count, out, pos, "4K flow handle")
    sf, sn, so_, sp_ = pkg.motion_inliers_mono(e, [pm], marr, [1])
    assert sf[0].tobytes() == flags.tobytes() and sn[0] == count and so_[0].tobytes() == out.tobytes() and sp_[0].tobytes() == pos.tobytes()


HANDLE_LP = lo.params(min_obs=2, max_missed=1, max_dist=2.0, gate_sigma=3.0)
CAL4K = dict(f=1200.0, cu=1920.0, cv=1080.0, base=0.5)
Z4K = CAL4K["f"] * CAL4K["base"] / 14.0     # the synthetic frames: a plane at a disparity of 14 px
TR4K = (0.0, 0.0, 0.0, -5 * Z4K / CAL4K["f"], -1 * Z4K / CAL4K["f"], 0.0)   # ... panning by (5, 1) px per frame


@pytest.mark.gpu
def test_gpu_4k_quad_scene_points_and_landmarks_on_a_lone_matcher(pkg, gpu):
    """The configuration of test_4k_stereo_quad_small_bins with track linking on and three pushes (two steps).  Under the
    synthetic sequence's own motion (zero rotation, the sideways translation that explains a pan of (5, 1) px at a
    disparity of 14) more than 65 536 records are inliers; motionInliers -> scenePoints(Tw) -> landmarks.  Every getter is
    byte for byte the stateless entry on the lists the handle hands out; the stateless inliers are the restatement's
    (check_against), the stateless scene points the restatement's under test_scene_points.compare (tr has zero rotation,
    so sin and cos are exact; the looser rule of a non-zero motion is the one asked for and is not widened), the stateless
    landmarks and states landmark_oracle's byte for byte."""
    p = pkg.Params.default(nms_n=3, match_binsize=25)
    seq = pkg.synth.stereo_sequence(W4K, H4K, 3, disparity=14, seed=5)
    e = pkg.EgoParams.default(inlier_threshold=2.5, **CAL4K)
    cal = mi._Cal(inlier_threshold=2.5, **CAL4K)
    lp = sl.lparams(pkg, HANDLE_LP)
    m = pkg.Matcher(p, outlier_removal=False)
    m.setTrackLinking(True)
    state, n_lm = None, 0
    for t, (left, right) in enumerate(seq):
        m.pushBack(left, right, DIMS4K, False)
        if t == 0:
            continue
        m.matchFeatures(pkg.METHOD_QUAD)
        pm, trk = m.getMatches(), m.getTracks()
        assert len(pm) > 80000 and len(trk) == len(pm)
        f, s = io.inliers(pm, TR4K, cal)
        near = io.near_threshold(s, cal, 1e-9)
        assert f.sum() > 65536 and near.sum() <= 0.001 * len(pm), (f.sum(), near.sum())
        count = m.motionInliers(e, TR4K)
        inl, pos = m.getInlierMatches()
        sf, sn, sout, spos = pkg.motion_inliers(e, [pm], np.array([TR4K]), [1])
        mi.check_against(pm, (f, s, near), sf[0], sn[0], sout[0], spos[0], f"4K quad step {t} stateless")
        assert count == sn[0] and inl.tobytes() == sout[0].tobytes() and pos.tobytes() == spos[0].tobytes()
        Tw = np.eye(4); Tw[:3, 3] = (-TR4K[3] * t, -TR4K[4] * t, 0.0)      # every step's points in the first frame's coordinates
        sp = pkg.SceneParams.default(frame=1, max_depth=60.0)
        pts = m.scenePoints(e, sp, Tw)
        want_pts = pkg.scene_points_stereo(e, [inl], np.array([TR4K]), [1], sp, Tw)[0][0]
        assert len(pts) > 65536 and pts.tobytes() == tsp.mapped(want_pts, pos).tobytes() == m.getScenePoints().tobytes()
        ref = so.stereo(inl, np.array(TR4K), cal, so.params(frame=1, max_depth=60.0), Tw=Tw)
        assert ref["margin"] >= 1e-6
        tsp.compare(want_pts, ref, f"4K quad step {t} scene points")
        lms = m.landmarks(lp)
        ref_lm, ref_state = lo.update(trk, pts, None if state is None else state[0], HANDLE_LP)
        want_lm, state = pkg.landmarks_update([trk], [pts], state, lp)
        assert lms.tobytes() == want_lm[0].tobytes() == m.getLandmarks().tobytes()
        assert want_lm[0].tobytes() == ref_lm.tobytes() and state[0].tobytes() == ref_state.tobytes()
        n_lm += len(lms)
        print(f"4K quad step {t}: {len(pm)} matches, {count} inliers, {len(pts)} points, {len(lms)} landmarks")
    m.close()
    assert n_lm > 65536       # step 2 continues step 1's tracks: more than one round of landmarks is compacted
