"""Landmarks: the scene points of a step fused along the feature tracks -- vh_landmarks_update on
caller-owned lists, vh_group_landmarks / vh_match_landmarks on a handle's tracked lists and scene points.
tests/landmark_oracle.py restates the per-record rule in numpy.

The bound.  The chain of sums of one track is sequential over the steps and independent of every other record; the
library adds, multiplies, divides and takes the square root in IEEE double without contraction, as numpy does.  So every
comparison here is byte for byte -- state_out, the landmarks, the counts -- without a tolerance."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import landmark_oracle as lo
import test_motion_inliers as mi
import test_motion_refit as mr
import test_sequence_recon as sr
from conftest import ROOT

SYMBOLS = ("vh_default_landmark_params", "vh_landmarks_update", "vh_group_landmarks", "vh_match_landmarks", "vh_group_get_landmarks",
           "vh_group_get_landmarks_all", "vh_get_landmarks", "vh_group_landmarks_device")
ptr, expect = mr.ptr, mr.expect
QUAD = sr.QUAD
LENGTHS = (0, 1, 257, 513)       # the tile edges of 256
STEPS = 6
SEED = 4021
SIGMAS = np.array([0.0] + [0.05 * k for k in range(1, 41)], np.float32)   # {0, 0.05 .. 2}
DRIVE = lo.params(min_obs=2, max_missed=1, max_dist=0.5, gate_sigma=3.0)
_CACHE = {}


def lparams(pkg, lp):
    return pkg.LandmarkParams.default(**lp)


def tracks_of(n, prev=None, frame=0, carry=None):
    """n TRACK records: prev as given (default -1), identities carried from `carry` (the predecessor's records) where prev is inside it"""
    t = np.zeros(n, lo.TRACK)
    t["prev"] = -1 if prev is None else prev
    for j in range(n):
        q = int(t["prev"][j])
        if carry is not None and 0 <= q < len(carry):
            t["birth_frame"][j], t["birth_pos"][j], t["age"][j] = carry["birth_frame"][q], carry["birth_pos"][q], carry["age"][q] + 1
        else:
            t["birth_frame"][j], t["birth_pos"][j], t["age"][j] = frame, j, 1
    return t


def points_of(pos, xyz, sigma):
    """POINT records at the record positions pos (increasing)"""
    p = np.zeros(len(pos), lo.POINT)
    p["src_pos"] = pos
    p["x"], p["y"], p["z"] = np.asarray(xyz, np.float64).reshape(-1, 3).T
    p["sigma_z"] = sigma
    p["err"] = 0.25
    p["i1c"] = 1000 + np.asarray(pos)
    p["i1p"] = 2000 + np.asarray(pos)
    return p


def drive():
    """The six steps of the stateless drive: per step the four lists' (tracks, points), and the oracle's answers chained
    through its own states -> (steps, wants, events).  Computed once."""
    if "drive" in _CACHE:
        return _CACHE["drive"]
    rng = np.random.default_rng(SEED)
    steps, world_prev, trk_prev = [], None, None
    for t in range(STEPS):
        tracks, points, worlds = [], [], []
        for s, n in enumerate(LENGTHS):
            n_prev = 0 if trk_prev is None else len(trk_prev[s])
            prev = np.full(n, -1, np.int32)
            if n_prev and n:   # a random partial injection into the previous list; a few deliberately outside it
                k = min(n, n_prev, max(1, int(0.85 * n)))
                prev[rng.permutation(n)[:k]] = rng.permutation(n_prev)[:k]
                wild = rng.permutation(n)[:max(1, n // 100)]
                prev[wild] = n_prev + rng.integers(0, 5, len(wild))
            trk = tracks_of(n, prev, t, None if trk_prev is None else trk_prev[s])
            world = np.stack([rng.uniform(-20, 20, n), rng.uniform(-3, 3, n), rng.uniform(5, 60, n)], 1)
            for j in range(n):
                if 0 <= prev[j] < n_prev:
                    world[j] = world_prev[s][prev[j]]
            seen = np.flatnonzero(rng.random(n) < 0.7)
            sigma = SIGMAS[rng.integers(0, len(SIGMAS), len(seen))]
            xyz = world[seen] + rng.normal(0, 1, (len(seen), 3)) * np.maximum(sigma, 0.02)[:, None] * 0.5
            gross = rng.random(len(seen)) < 0.03
            xyz[gross] += 50.0
            tracks.append(trk); points.append(points_of(seen, xyz, sigma)); worlds.append(world)
        steps.append((tracks, points))
        world_prev, trk_prev = worlds, tracks
    events, wants, state = {}, [], None
    for tracks, points in steps:
        lm, state = lo.update_lists(tracks, points, state, DRIVE, events)
        wants.append((lm, state))
    _CACHE["drive"] = (steps, wants, events)
    return _CACHE["drive"]


def same(got, want, what):
    assert len(got) == len(want), (what, len(got), len(want))
    for s, (g, w) in enumerate(zip(got, want)):
        assert g.dtype == w.dtype and g.tobytes() == w.tobytes(), (what, s, len(g), len(w))


# ------------------------------------------------------------------------------------------------------------ CPU
def test_oracle_constructed_chains():
    """One track seen n times at equal sigma_z: the arithmetic mean to the last bit of the left-to-right sums, sigma =
    s / sqrt(n) to 1 ulp of float; a gate restart; a max_missed drop at exactly max_missed + 1 gaps and not at max_missed."""
    rng = np.random.default_rng(7)
    n, s = 9, np.float32(0.4)
    xyz = rng.normal(0, 1, (n, 3)).astype(np.float32) + np.float32(10)
    lp = lo.params(min_obs=1, max_missed=2, max_dist=0.0, gate_sigma=0.0)
    state, lm = None, None
    for t in range(n):
        trk = tracks_of(1, [0 if t else -1], t, None if t == 0 else trk)
        lm, state = lo.update(trk, points_of([0], xyz[t], s), state, lp)
    w = np.float64(1.0) / (np.float64(s) * np.float64(s))
    sw = sx = sy = sz = np.float64(0)
    for t in range(n):
        sw = sw + w; sx = sx + w * np.float64(xyz[t, 0]); sy = sy + w * np.float64(xyz[t, 1]); sz = sz + w * np.float64(xyz[t, 2])
    assert len(lm) == 1 and lm["n_obs"][0] == n and lm["age"][0] == n and state["n_obs"][0] == n
    assert (lm["x"][0], lm["y"][0], lm["z"][0]) == (np.float32(sx / sw), np.float32(sy / sw), np.float32(sz / sw))
    assert np.allclose([lm["x"][0], lm["y"][0], lm["z"][0]], xyz.astype(np.float64).mean(0), rtol=1e-6)
    want_sigma = np.float32(np.float64(s) / np.sqrt(np.float64(n)))
    assert abs(int(lm["sigma"].view(np.int32)[0]) - int(want_sigma.view(np.int32))) <= 1
    # a gate restart: the third observation lies 5 m off under T = 1 + 2 * 0.5
    lp = lo.params(min_obs=1, max_missed=2, max_dist=1.0, gate_sigma=2.0)
    state, ev = None, {}
    for t, x in enumerate((10.0, 10.1, 15.1, 15.2)):
        lm, state = lo.update(tracks_of(1, [0 if t else -1]), points_of([0], [x, 0, 20], 0.5), state, lp, ev)
        assert lm["n_obs"][0] == (1, 2, 1, 2)[t]
    assert ev == {"restart": 1} and abs(lm["x"][0] - 15.15) < 1e-5
    # the drop: max_missed = 2 survives two gaps and not three
    for gaps, kept in ((2, True), (3, False)):
        lp = lo.params(min_obs=1, max_missed=2)
        ev = {}
        lm, state = lo.update(tracks_of(1), points_of([0], [1, 2, 3], 0.0), None, lp, ev)
        for g in range(gaps):
            lm, state = lo.update(tracks_of(1, [0]), points_of([], np.zeros((0, 3)), 0.0), state, lp, ev)
            assert len(lm) == 0 and state["n_missed"][0] == (g + 1 if g < 2 else 0)
        lm, state = lo.update(tracks_of(1, [0]), points_of([0], [1, 2, 3], 0.0), state, lp, ev)
        assert lm["n_obs"][0] == (2 if kept else 1) and state["n_missed"][0] == 0 and ev == ({} if kept else {"drop": 1})


def test_symbols_layout_and_source_list(pkg, tmp_path):
    """Every new symbol is declared, exported and mirrored; vh_abi_version stays 1; the three structs are 48 / 48 / 24 bytes in
    the C compiler's layout and in the mirrors; the defaults are 2, 3, 0, 0; both new units are in the Makefile's SRCS."""
    header = open(os.path.join(ROOT, "include", "viso_hip.h")).read()
    lib = pkg._lib()
    for name in SYMBOLS:
        assert name + "(" in header and hasattr(C.CDLL(pkg.LIB_PATH), name) and name in pkg.ABI_SYMBOLS, name
    assert '"landmarks"' in header and pkg.abi_version() == 1
    assert callable(pkg.landmarks_update)
    for cls in (pkg.Matcher, pkg.StreamGroup):
        assert "landmarks" in vars(cls) and "getLandmarks" in vars(cls)
    assert all(n in vars(pkg.StreamGroup) for n in ("getLandmarksAll", "landmarksDevice")) and hasattr(pkg.SequenceGroup, "landmarks")
    assert pkg.LANDMARK_DTYPE == lo.LANDMARK and pkg.LANDMARK_STATE_DTYPE == lo.STATE and pkg.TRACK == lo.TRACK
    assert pkg.LANDMARK_DTYPE.itemsize == 48 and pkg.LANDMARK_STATE_DTYPE.itemsize == 48 and C.sizeof(pkg.LandmarkParams) == 24
    lm_f, st_f = lo.LANDMARK.names, ("sw", "swx", "swy", "swz", "n_obs", "n_missed", "reserved")
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "viso_hip.h"\nint main(void) {\n'
                   '  printf("%zu %zu %zu", sizeof(vh_landmark_state), sizeof(vh_landmark), sizeof(vh_landmark_params));\n'
                   + "".join(f'  printf(" %zu", offsetof(vh_landmark, {n}));\n' for n in lm_f)
                   + "".join(f'  printf(" %zu", offsetof(vh_landmark_state, {n}));\n' for n in st_f)
                   + "".join(f'  printf(" %zu", offsetof(vh_landmark_params, {n}));\n' for n in ("min_obs", "max_missed", "max_dist", "gate_sigma"))
                   + '  return 0;\n}\n')
    exe = str(tmp_path / "layout")
    subprocess.check_call(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), str(src), "-o", exe])
    want = [48, 48, 24] + [lo.LANDMARK.fields[n][1] for n in lm_f] + [lo.STATE.fields[n][1] for n in st_f] + [0, 4, 8, 16]
    assert [int(v) for v in subprocess.check_output([exe], timeout=60).decode().split()] == want
    lp = pkg.LandmarkParams(min_obs=9, max_missed=9, max_dist=9, gate_sigma=9)
    lib.vh_default_landmark_params(C.byref(lp))
    assert (lp.min_obs, lp.max_missed, lp.max_dist, lp.gate_sigma) == (2, 3, 0.0, 0.0)
    d = pkg.LandmarkParams.default()
    assert (d.min_obs, d.max_missed, d.max_dist, d.gate_sigma) == (2, 3, 0.0, 0.0)
    srcs = open(os.path.join(pkg.CSRC, "Makefile")).read().split("SRCS", 1)[1].split("ONLY", 1)[0]
    assert "kernels_landmark.hip" in srcs and "engine_landmark.hip" in srcs
    # without a device: nothing to do is VH_OK, argument errors are refused before any device is needed
    n = C.c_int32(7)
    assert lib.vh_landmarks_update(C.byref(lp), 0, 0, None, None, None, None, None, None, None, None, None) == pkg.VH_OK
    off = np.zeros(3, np.int32); counts = np.full(2, 7, np.int32)
    assert lib.vh_landmarks_update(C.byref(lp), 0, 2, None, ptr(off), None, ptr(off), None, None, None, None, ptr(counts)) == pkg.VH_OK
    assert counts.tolist() == [0, 0]
    assert lib.vh_group_landmarks(None, C.byref(lp), C.byref(n)) == pkg.VH_ERR_INVALID_ARG
    assert lib.vh_group_get_landmarks(None, 0, None, 0, C.byref(n)) == pkg.VH_ERR_INVALID_ARG
    assert lib.vh_group_landmarks_device(None, None, None) == pkg.VH_ERR_INVALID_ARG


def test_drive_is_not_vacuous():
    """The oracle alone, on the drive's inputs: at least one gate restart, one max_missed drop, one emitted landmark with
    n_obs >= 4, and a prev outside the predecessor list in every step but the first."""
    steps, wants, events = drive()
    assert events.get("restart", 0) >= 1 and events.get("drop", 0) >= 1, events
    assert max(int(lm["n_obs"].max(initial=0)) for lms, _ in wants for lm in lms) >= 4
    for t in range(1, STEPS):
        assert any((steps[t][0][s]["prev"] >= len(steps[t - 1][0][s])).any() for s in range(len(LENGTHS)))
    assert all(len(p) <= len(t) for tr, pt in steps for t, p in zip(tr, pt))


# ------------------------------------------------------------------------------------------------------------ GPU
@pytest.mark.gpu
def test_gpu_stateless_drive(pkg, gpu):
    """Six steps of four lists (0, 1, 257, 513 records), each step's state_out feeding the next step's prev: state_out, the
    landmarks and the counts byte for byte the oracle's; a second run gives the same bytes; list 2 alone gives the bytes it
    gives among the four."""
    steps, wants, _ = drive()
    lp = lparams(pkg, DRIVE)
    runs = []
    for run in range(2):
        state, got = None, []
        for t, (tracks, points) in enumerate(steps):
            lm, state = pkg.landmarks_update(tracks, points, state, lp)
            same(lm, wants[t][0], f"run {run} step {t} landmarks")
            same(state, wants[t][1], f"run {run} step {t} state")
            got.append((lm, state))
        runs.append(got)
    for t in range(STEPS):
        same(runs[0][t][0], runs[1][t][0], "rerun"); same(runs[0][t][1], runs[1][t][1], "rerun state")
    state = None
    for t, (tracks, points) in enumerate(steps):
        lm, state = pkg.landmarks_update(tracks[2:3], points[2:3], state, lp)
        same(lm, wants[t][0][2:3], f"alone step {t}"); same(state, wants[t][1][2:3], f"alone step {t} state")
    print("landmarks per step:", [[len(x) for x in w[0]] for w in wants])


@pytest.mark.gpu
def test_gpu_parameter_and_input_edges(pkg, gpu):
    """prev = NULL with min_obs = 1: every observed record emitted with n_obs = 1; min_obs = 3: nothing before step 3; both
    gate terms 0: no restart; a list with records and no points: zero landmarks, states carried with n_missed counted; an
    observation with +-inf coordinates zeroes the state.  Each byte for byte the oracle's."""
    steps, _, _ = drive()
    tracks, points = steps[0]
    lp = lo.params(min_obs=1)
    lm, st = pkg.landmarks_update(tracks, points, None, lparams(pkg, lp))
    wl, ws = lo.update_lists(tracks, points, None, lp)
    same(lm, wl, "min_obs 1"); same(st, ws, "min_obs 1 state")
    assert all(len(l) == len(p) and (l["n_obs"] == 1).all() and (l["src_pos"] == p["src_pos"]).all() for l, p in zip(lm, points))
    for name, lp in (("min_obs 3", lo.params(min_obs=3, max_missed=-1)), ("no gate", lo.params(min_obs=2, max_missed=1))):
        ev, state, wstate = {}, None, None
        for t, (tracks, points) in enumerate(steps[:4]):
            lm, state = pkg.landmarks_update(tracks, points, state, lparams(pkg, lp))
            wl, wstate = lo.update_lists(tracks, points, wstate, lp, ev)
            same(lm, wl, f"{name} step {t}"); same(state, wstate, f"{name} step {t} state")
            if name == "min_obs 3" and t < 2:
                assert sum(len(x) for x in lm) == 0
        assert "restart" not in ev and (name != "min_obs 3" or sum(len(x) for x in lm) > 0)
    # records without points: the states are carried, n_missed counted (max_missed = 1: the second gap drops them)
    lp = lo.params(min_obs=1, max_missed=1)
    n = 300
    state = pkg.landmarks_update([tracks_of(n)], [points_of(np.arange(n), np.ones((n, 3)), 0.5)], None, lparams(pkg, lp))[1]
    chain = tracks_of(n, np.arange(n))
    none = points_of([], np.zeros((0, 3)), 0.0)
    for gap in (1, 2):
        lm, state = pkg.landmarks_update([chain], [none], state, lparams(pkg, lp))
        assert len(lm[0]) == 0 and (state[0]["n_missed"] == (1 if gap == 1 else 0)).all() and (state[0]["n_obs"] == (1 if gap == 1 else 0)).all()
    assert state[0].tobytes() == bytes(48 * n)
    # +-inf coordinates zero the state and emit nothing
    xyz = np.ones((n, 3)); xyz[5, 0] = np.inf; xyz[77, 2] = -np.inf; xyz[256, 1] = np.inf
    pts = points_of(np.arange(n), xyz, 0.5)
    first = pkg.landmarks_update([tracks_of(n)], [points_of(np.arange(n), np.ones((n, 3)), 0.5)], None, lparams(pkg, lp))[1]
    lm, state = pkg.landmarks_update([chain], [pts], first, lparams(pkg, lp))
    wl, ws = lo.update_lists([chain], [pts], first, lp)
    same(lm, wl, "inf"); same(state, ws, "inf state")
    assert len(lm[0]) == n - 3 and all(state[0][j].tobytes() == bytes(48) for j in (5, 77, 256))


@pytest.mark.gpu
def test_gpu_validation(pkg, gpu):
    """Non-increasing src_pos, src_pos >= n_rec, min_obs = 0 and prev without prev_offsets: VH_ERR_INVALID_ARG, nothing written."""
    lib = pkg._lib()
    n = 8
    trk = tracks_of(n); roff = np.array([0, n], np.int32)
    good = points_of([1, 3, 6], np.ones((3, 3)), 0.5); poff = np.array([0, 3], np.int32)
    prev = np.zeros(n, lo.STATE); voff = np.array([0, n], np.int32)
    lp = pkg.LandmarkParams.default()

    def call(lp=lp, pts=good, prev=None, voff=None):
        state = np.full(n, 0x5A, np.uint8).repeat(48).view(lo.STATE); out = np.full(n * 48, 0x5A, np.uint8).view(lo.LANDMARK)
        counts = np.full(1, 0x5A5A5A5A, np.int32)
        rc = lib.vh_landmarks_update(C.byref(lp), 0, 1, ptr(trk), ptr(roff), ptr(pts), ptr(poff), ptr(prev), ptr(voff), ptr(state), ptr(out), ptr(counts))
        untouched = state.tobytes() == b"\x5a" * (48 * n) and out.tobytes() == b"\x5a" * (48 * n) and counts[0] == 0x5A5A5A5A
        return rc, untouched

    assert call() == (pkg.VH_OK, False) and call(prev=prev, voff=voff)[0] == pkg.VH_OK
    inv = (pkg.VH_ERR_INVALID_ARG, True)
    assert call(pts=points_of([1, 1, 6], np.ones((3, 3)), 0.5)) == inv
    assert call(pts=points_of([3, 1, 6], np.ones((3, 3)), 0.5)) == inv
    assert call(pts=points_of([1, 3, n], np.ones((3, 3)), 0.5)) == inv
    assert call(pts=points_of([-1, 3, 6], np.ones((3, 3)), 0.5)) == inv
    assert call(lp=pkg.LandmarkParams.default(min_obs=0)) == inv
    assert call(prev=prev) == inv and call(voff=voff) == inv


# ---- the handle form
def pose_of(t):
    """The pose handed to scenePoints as Tw in step t (the same for both sides of every comparison)."""
    Tw = np.eye(4)
    Tw[:3, 3] = (0.4 * t, 0.1 * t, 0.0)
    return Tw


HANDLE_LP = lo.params(min_obs=2, max_missed=1, max_dist=2.0, gate_sigma=3.0)


def handle_step(pkg, g, e, t):
    """matchFeatures .. scenePoints of step t on a group -> (tracks, points) per stream"""
    g.matchFeatures(QUAD)
    g.motionInliers(e, np.array([mi.TR2] * g.S), np.ones(g.S, np.int32))
    g.scenePoints(e, None, pose_of(t))
    return [g.getTracks(s) for s in range(g.S)], [g.getScenePoints(s) for s in range(g.S)]


def group_landmarks(g, lp):
    counts = g.landmarks(lp)
    got = [g.getLandmarks(s) for s in range(g.S)]
    assert [len(x) for x in got] == counts.tolist()
    return got


@pytest.mark.gpu
def test_gpu_handle_form(pkg, gpu):
    """A StreamGroup of S = 2 with track linking on, five steps of push -> quad match -> motionInliers -> scenePoints(Tw) ->
    landmarks: each step byte for byte landmarks_update fed with getTracks, getScenePoints and the stateless chain's own
    previous state; calling twice gives the same bytes; skipping the call in step 3 makes step 4 the prev = None result;
    matching step 4's pair again and calling again gives the bytes from before; a lone Matcher equals stream 0 of an S = 1
    group."""
    dims = sr.dims_of(pkg)
    frames = [sr.frames_of(pkg, 6, seed) for seed in (91, 92)]
    e = mi.hego(pkg, inlier_threshold=2.5)
    lp = lparams(pkg, HANDLE_LP)
    S = 2
    g = pkg.StreamGroup(S, pkg.Params.default())
    g.setTrackLinking(True)
    state, total, deep = None, 0, 0
    for t in range(6):
        g.pushBack(np.stack([f[t][0] for f in frames]), np.stack([f[t][1] for f in frames]), dims)
        if t == 0:
            continue
        tracks, points = handle_step(pkg, g, e, t)
        if t == 3:                                   # no call in step 3: step 4 starts without state
            state = None
            continue
        want, state = pkg.landmarks_update(tracks, points, state, lp)
        got = group_landmarks(g, lp)
        same(got, want, f"step {t}")
        same(group_landmarks(g, lp), want, f"step {t} again")
        out, counts = g.getLandmarksAll(max(1, max(len(x) for x in want)))
        assert all(out[s, :counts[s]].tobytes() == want[s].tobytes() for s in range(S))
        if t >= 4:                                   # the same pair matched again (step 4: no predecessor state; step 5: step 4's,
            tracks2, points2 = handle_step(pkg, g, e, t)   # which is kept): the current state is recomputed, the same bytes
            assert all(a.tobytes() == b.tobytes() for a, b in zip(tracks + points, tracks2 + points2))
            same(group_landmarks(g, lp), want, f"step {t} rematched")
        total += sum(len(x) for x in want)
        deep = max(deep, max(int(x["n_obs"].max(initial=0)) for x in want))
    assert total > 0 and deep >= 2, (total, deep)
    g.close()
    # a lone matcher against stream 0 of a group of one
    g1 = pkg.StreamGroup(1, pkg.Params.default()); g1.setTrackLinking(True)
    m = pkg.Matcher(pkg.Params.default(), outlier_removal=False); m.setTrackLinking(True)
    n_lm = 0
    for t in range(4):
        left, right = frames[0][t]
        g1.pushBack(left[None], right[None], dims); m.pushBack(left, right, dims)
        if t == 0:
            continue
        handle_step(pkg, g1, e, t)
        m.matchFeatures(QUAD); m.motionInliers(e, mi.TR2); m.scenePoints(e, Tw=pose_of(t))
        got = m.landmarks(lp)
        assert got.tobytes() == group_landmarks(g1, lp)[0].tobytes() == m.getLandmarks().tobytes()
        n_lm += len(got)
    assert n_lm > 0
    g1.close(); m.close()


@pytest.mark.gpu
def test_gpu_state_rules_memory_and_failed_allocation(pkg, gpu):
    """VH_ERR_STATE with linking off, before scenePoints and after the next push; VH_ERR_UNSUPPORTED on a SequenceGroup;
    vh_group_device_bytes is unchanged until the first call; a refused allocation is VH_ERR_HIP before any launch, the
    repeated call succeeds with the right bytes and adds exactly the documented block -- 2 x 48 bytes of state, 48 of output
    and 4 of observation index per record slot, 4 per tile of 256 slots, 4 per stream, each array rounded up to 256 --
    once; profile scope "landmarks"."""
    dims = sr.dims_of(pkg)
    frames = [sr.frames_of(pkg, 3, seed) for seed in (85, 86)]
    e = mi.hego(pkg, inlier_threshold=2.5)
    state = pkg.VH_ERR_STATE
    S, MM = 2, 4096
    lp = lparams(pkg, lo.params(min_obs=1))
    off = pkg.StreamGroup(S, pkg.Params.default(), max_matches=MM)         # linking off
    for t in range(2):
        off.pushBack(np.stack([f[t][0] for f in frames]), np.stack([f[t][1] for f in frames]), dims)
    handle_step_no_tracks = lambda g: (g.matchFeatures(QUAD), g.motionInliers(e, np.array([mi.TR2] * S), np.ones(S, np.int32)), g.scenePoints(e))  # noqa: E731
    handle_step_no_tracks(off)
    expect(pkg, state, lambda: off.landmarks(lp))
    off.close()
    sq = pkg.SequenceGroup(4, pkg.Params.default()); sq.setTrackLinking(True)
    expect(pkg, pkg.VH_ERR_UNSUPPORTED, lambda: sq.landmarks(lp))
    sq.close()
    g = pkg.StreamGroup(S, pkg.Params.default(), max_matches=MM)
    g.setTrackLinking(True)
    g.profileEnable(True)
    expect(pkg, state, lambda: g.landmarks(lp))                            # nothing pushed
    for t in range(2):
        g.pushBack(np.stack([f[t][0] for f in frames]), np.stack([f[t][1] for f in frames]), dims)
    g.matchFeatures(QUAD)
    expect(pkg, state, lambda: g.landmarks(lp))                            # no scene points yet
    expect(pkg, state, lambda: g.getLandmarks(0))
    g.motionInliers(e, np.array([mi.TR2] * S), np.ones(S, np.int32))
    g.scenePoints(e)
    expect(pkg, state, lambda: g.landmarksDevice())
    tracks, points = [g.getTracks(s) for s in range(S)], [g.getScenePoints(s) for s in range(S)]
    g.synchronize()
    bytes0 = g.deviceBytes()
    g.debugFailNextAlloc()
    expect(pkg, pkg.VH_ERR_HIP, lambda: g.landmarks(lp))
    g.synchronize()
    assert g.deviceBytes() == bytes0 and g.profileRead("landmarks")[1] == 0
    want = pkg.landmarks_update(tracks, points, None, lp)[0]
    same(group_landmarks(g, lp), want, "the repeated call")
    assert sum(len(x) for x in want) > 0 and all(len(w) == len(p) for w, p in zip(want, points))
    _, stride = g.landmarksDevice()
    up = lambda b: (b + 255) // 256 * 256  # noqa: E731
    block = up(2 * 48 * S * stride) + up(48 * S * stride) + up(4 * S * stride) + up(4 * S * ((stride + 255) // 256)) + up(4 * S)
    assert stride >= MM and g.deviceBytes() == bytes0 + block, (g.deviceBytes() - bytes0, block)
    g.landmarks(lp)
    g.synchronize()
    assert g.deviceBytes() == bytes0 + block and g.profileRead("landmarks")[1] == 2
    g.pushBack(np.stack([f[2][0] for f in frames]), np.stack([f[2][1] for f in frames]), dims)
    expect(pkg, state, lambda: g.landmarks(lp))                            # pushed: the pair the lists belong to is over
    g.matchFeatures(QUAD)
    expect(pkg, state, lambda: g.getLandmarks(0))                          # the landmarks end with the next match
    g.close()
