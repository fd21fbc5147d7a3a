"""Landmarks along the rows of one chain: vh_landmarks_chain on caller-owned lists whose
predecessor is the list before them in the same call, and vh_group_landmarks on a sequence handle with
vh_sequence_set_landmarks on.

The bound.  The expected value of a chain is tests/landmark_oracle.py applied one list at a time, list s - 1's returned
state as list s's prev.  The device walks every track with the state in registers and the same double arithmetic in the
same order, without contraction; so every comparison here is byte for byte -- states, landmarks, counts -- no tolerance.
One care in the inputs: a landmark emitted from sw = 0 (a first observation with sigma_z = +inf: w = 1 / inf = 0) has
0 / 0 coordinates, a NaN whose sign bit is the platform's, not the rule's; so +inf is placed only on records that continue
a state with sw > 0, where it is the rule that is tested: the observation counts, weighs nothing and passes the gate."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import landmark_oracle as lo
import test_motion_inliers as mi
import test_sequence_recon as sr
from conftest import ROOT

SYMBOLS = ("vh_landmarks_chain", "vh_sequence_set_landmarks")
QUAD = sr.QUAD
LENGTHS = (0, 1, 255, 256, 257, 600, 3)            # the tile edges of 256, an empty first list
PERMUTED = (257, 3, 600, 0, 256, 1, 255)           # an empty list mid-chain: every chain ends there
SOLID = (5, 300, 257, 7, 6)                        # no empty list: chain 0 crosses every list
SIGMAS = np.array([0.0, -0.5] + [0.05 * k for k in range(1, 21)], np.float32)   # 0 and negative: w = 1
_CACHE = {}


def ptr(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def expect(pkg, code, fn):
    with pytest.raises(pkg.VisoHipError) as ei:
        fn()
    assert ei.value.code == code, (ei.value.code, code)


def lparams(pkg, lp):
    return pkg.LandmarkParams.default(**lp)


def same(got, want, what):
    assert len(got) == len(want), (what, len(got), len(want))
    for s, (g, w) in enumerate(zip(got, want)):
        assert g.dtype == w.dtype and g.tobytes() == w.tobytes(), (what, s, len(g), len(w))


def chain_oracle(tracks, points, carry, lp, events=None):
    """landmark_oracle.update_lists one list at a time, list s - 1's state as list s's prev -> (landmarks, states)"""
    lms, states, prev = [], [], carry
    for t, p in zip(tracks, points):
        lm, st = lo.update_lists([t], [p], None if prev is None else [prev], lp, events)
        lms.append(lm[0]); states.append(st[0]); prev = st[0]
    return lms, states


def suppressed(tracks, points, states, lms):
    """records that had an observation, kept a state and emitted nothing: min_obs held them back"""
    n = 0
    for p, st, lm in zip(points, states, lms):
        kept = st["n_obs"][p["src_pos"]] > 0
        n += int(kept.sum()) - len(lm)
    return n


def build(lengths, seed, n_carry=0, every=1, special=False, no_points=()):
    """Tracked lists that are the rows of one chain, with their points -> (tracks, points).
    prev: a random partial injection into the list before (list 0: into a carry of n_carry states), each predecessor
    continued at most once; record 0 continues record 0 wherever both exist; a few prev outside the predecessor on both
    sides (< -1 and >= its length).  every: a point for every `every`-th record; no_points: lists without any.  Gross
    outliers (+50 m) restart tracks at the gate.  special: a NaN coordinate in rows = 2 mod 4 and sigma_z = +inf in rows
    = 1 mod 4, the latter only on records that continue an observed one (module docstring)."""
    rng = np.random.default_rng(seed)
    tracks, points, world_prev, n_prev = [], [], None, n_carry
    for s, n in enumerate(lengths):
        prev = np.full(n, -1, np.int32)
        if n and n_prev:
            k = min(n, n_prev, max(1, int(0.8 * n)))
            prev[rng.permutation(n)[:k]] = rng.permutation(n_prev)[:k]
            if n > 1:                                    # record 0 <- record 0, the duplicate (if any) unlinked
                prev[(prev == 0) & (np.arange(n) > 0)] = -1
            prev[0] = 0
        if n >= 3:
            wild = rng.permutation(np.arange(1, n))[:max(2, n // 50)]
            prev[wild[::2]] = n_prev + rng.integers(0, 5, len(wild[::2]))
            prev[wild[1::2]] = -2 - rng.integers(0, 5, len(wild[1::2]))
        inside = (prev >= 0) & (prev < n_prev)
        assert len(np.unique(prev[inside])) == int(inside.sum())
        trk = np.zeros(n, lo.TRACK)
        trk["prev"] = prev; trk["birth_frame"] = s; trk["birth_pos"] = np.arange(n); trk["age"] = 1 + rng.integers(0, 9, n)
        world = np.stack([rng.uniform(-20, 20, n), rng.uniform(-3, 3, n), rng.uniform(5, 60, n)], 1)
        if world_prev is not None:
            world[inside] = world_prev[prev[inside]]
        seen = np.arange(0, n, every) if s not in no_points else np.zeros(0, np.int64)
        if every > 1 and len(seen):                      # ... and not the same records in every row
            seen = np.unique((seen + s) % n)
        sigma = SIGMAS[rng.integers(0, len(SIGMAS), len(seen))].copy()
        xyz = world[seen] + rng.normal(0, 1, (len(seen), 3)) * np.maximum(np.abs(sigma), 0.02)[:, None] * 0.5
        xyz[rng.random(len(seen)) < 0.04] += 50.0
        if special and len(seen):
            if s % 4 == 2:
                xyz[rng.permutation(len(seen))[:max(1, len(seen) // 20)], rng.integers(0, 3)] = np.nan
            if s % 4 == 1:
                sigma[inside[seen]] = np.where(rng.random(int(inside[seen].sum())) < 0.3, np.inf, sigma[inside[seen]])
        p = np.zeros(len(seen), lo.POINT)
        p["src_pos"] = seen; p["x"], p["y"], p["z"] = xyz.T; p["sigma_z"] = sigma; p["err"] = 0.25
        p["i1c"] = 1000 + seen; p["i1p"] = 2000 + seen
        tracks.append(trk); points.append(p)
        world_prev, n_prev = world, n
    return tracks, points


def carry_of(n, seed):
    """n predecessor states: a third empty, the others one to four observations near the origin of the scene"""
    rng = np.random.default_rng(seed)
    c = np.zeros(n, lo.STATE)
    k = rng.integers(0, 5, n) * (rng.random(n) > 0.33)
    w = k * 4.0
    c["sw"] = w; c["swx"] = w * rng.uniform(-20, 20, n); c["swy"] = w * rng.uniform(-3, 3, n); c["swz"] = w * rng.uniform(5, 60, n)
    c["n_obs"] = k; c["n_missed"] = np.where(k > 0, rng.integers(0, 2, n), 0)
    return c


# (name, lengths, n_carry, every, special, no_points, params)
CASES = (
    ("edges", LENGTHS, 0, 1, False, (), lo.params(min_obs=2, max_missed=0, max_dist=0.5, gate_sigma=3.0)),
    ("edges carry", (600, 257, 256, 255, 1, 3), 40, 3, False, (), lo.params(min_obs=1, max_missed=2, max_dist=1.5, gate_sigma=0.0)),
    ("permuted", PERMUTED, 300, 3, False, (5,), lo.params(min_obs=3, max_missed=-1, max_dist=0.0, gate_sigma=3.0)),
    ("permuted gates off", PERMUTED, 0, 1, False, (2,), lo.params(min_obs=1, max_missed=2)),
    ("solid special", SOLID, 9, 1, True, (), lo.params(min_obs=1, max_missed=0, max_dist=0.5, gate_sigma=3.0)),
    ("solid special sigma gate", SOLID, 0, 1, True, (), lo.params(min_obs=3, max_missed=2, max_dist=0.0, gate_sigma=4.0)),
    ("solid special dist gate", SOLID, 3, 1, True, (), lo.params(min_obs=2, max_missed=-1, max_dist=1.0, gate_sigma=0.0)),
    ("solid thirds", SOLID, 0, 3, False, (3,), lo.params(min_obs=2, max_missed=0, max_dist=0.5, gate_sigma=3.0)),
    ("solid thirds kept", SOLID, 5, 3, False, (), lo.params(min_obs=3, max_missed=2, max_dist=2.0, gate_sigma=3.0)),
)


def cases():
    """Every constructed case with the oracle's answer -> [(name, tracks, points, carry, lp, (landmarks, states))], events.
    Computed once and left unchanged."""
    if "cases" not in _CACHE:
        out, events = [], {}
        for i, (name, lengths, n_carry, every, special, none, lp) in enumerate(CASES):
            tracks, points = build(lengths, 500 + i, n_carry, every, special, none)
            # (a carry shorter than list 0's largest prev: build() gave prev up to n_carry + 4)
            carry = carry_of(n_carry, 900 + i) if n_carry else None
            out.append((name, tracks, points, carry, lp, chain_oracle(tracks, points, carry, lp, events)))
        _CACHE["cases"] = (out, events)
    return _CACHE["cases"]


# ------------------------------------------------------------------------------------------------------------ CPU
def test_symbols_source_list_and_host_refusals(pkg):
    """Both symbols are declared, exported and in ABI_SYMBOLS, vh_abi_version stays 1; SequenceGroup.setLandmarks and
    landmarks_chain exist; the new unit is in the Makefile's SRCS; n_sets = 0 is VH_OK, lists without records are VH_OK with
    zero counts, a duplicate prev inside the predecessor list (or inside the carry) is VH_ERR_INVALID_ARG -- all without a
    device."""
    header = open(os.path.join(ROOT, "include", "viso_hip.h")).read()
    lib = pkg._lib()
    for name in SYMBOLS:
        assert name + "(" in header and hasattr(C.CDLL(pkg.LIB_PATH), name) and name in pkg.ABI_SYMBOLS, name
    assert pkg.abi_version() == 1
    assert "setLandmarks" in vars(pkg.SequenceGroup) and callable(pkg.landmarks_chain)
    assert all(hasattr(pkg.SequenceGroup, n) for n in ("landmarks", "getLandmarks", "getLandmarksAll", "landmarksDevice"))
    srcs = open(os.path.join(pkg.CSRC, "Makefile")).read().split("SRCS", 1)[1].split("ONLY", 1)[0]
    assert "kernels_landmark_chain.hip" in srcs and "kernels_landmark.hip" in srcs
    lp = pkg.LandmarkParams.default()
    assert lib.vh_landmarks_chain(C.byref(lp), 0, 0, None, None, None, None, None, 0, None, None, None) == pkg.VH_OK
    off = np.zeros(3, np.int32); counts = np.full(2, 7, np.int32)
    assert lib.vh_landmarks_chain(C.byref(lp), 0, 2, None, ptr(off), None, ptr(off), None, 0, None, None, ptr(counts)) == pkg.VH_OK
    assert counts.tolist() == [0, 0]
    assert lib.vh_sequence_set_landmarks(None, 1) == pkg.VH_ERR_INVALID_ARG

    def call(prev0, prev1, carry=None, lp=lp, n_carry=None):
        trk = np.zeros(6, lo.TRACK); trk["prev"] = list(prev0) + list(prev1)
        roff = np.array([0, 3, 6], np.int32); poff = np.zeros(3, np.int32)
        state = np.full(6 * 48, 0x5A, np.uint8).view(lo.STATE); out = np.full(6 * 48, 0x5A, np.uint8).view(lo.LANDMARK)
        counts = np.full(2, 0x5A5A5A5A, np.int32)
        rc = lib.vh_landmarks_chain(C.byref(lp), 0, 2, ptr(trk), ptr(roff), None, ptr(poff), ptr(carry),
                                    (0 if carry is None else len(carry)) if n_carry is None else n_carry, ptr(state), ptr(out), ptr(counts))
        return rc, state.tobytes() == b"\x5a" * 288 and out.tobytes() == b"\x5a" * 288 and counts[0] == 0x5A5A5A5A

    inv = (pkg.VH_ERR_INVALID_ARG, True)
    assert call((-1, -1, -1), (1, 0, 1)) == inv                    # two records continue record 1
    assert call((2, 2, -1), (0, 1, 2), carry=np.zeros(3, lo.STATE)) == inv   # ... state 2 of the carry
    assert call((-1, -1, -1), (0, 1, 2), lp=pkg.LandmarkParams.default(min_obs=0)) == inv
    assert call((-1, -1, -1), (0, 1, 2), n_carry=-1) == inv and call((-1, -1, -1), (0, 1, 2), n_carry=2) == inv


def test_constructed_chains_are_not_vacuous():
    """The restatement alone on the constructed chains: each of the five events at least once -- a restart at the gate, a
    drop at the gap limit, a state zeroed on a non-finite sum, an emission, a record held back by min_obs -- and the shapes
    the walk has to get right: chains that start in every row, a chain that crosses every list, prev outside the
    predecessor on both sides, a carry shorter than list 0's largest prev."""
    cs, events = cases()
    assert events.get("restart", 0) >= 1 and events.get("drop", 0) >= 1 and events.get("nonfinite", 0) >= 1, events
    assert sum(len(x) for c in cs for x in c[5][0]) > 0
    assert sum(suppressed(c[1], c[2], c[5][1], c[5][0]) for c in cs) > 0
    for name, tracks, points, carry, lp, (lms, states) in cs:
        n_pred = [0 if carry is None else len(carry)] + [len(t) for t in tracks[:-1]]
        for s, t in enumerate(tracks):
            if len(t) >= 3:
                assert (t["prev"] < -1).any() and (t["prev"] >= n_pred[s]).any(), (name, s)
            if len(t) > 1 and s > 0:                           # a head in every row: a chain starts there
                assert ((t["prev"] < 0) | (t["prev"] >= n_pred[s])).any(), (name, s)
        if carry is not None:
            assert tracks[0]["prev"].max() >= len(carry), name
    solid = cs[4]
    assert all(t["prev"][0] == 0 for t in solid[1]) and max(int(x["n_obs"].max(initial=0)) for x in solid[5][0]) >= 3
    assert any(np.isinf(p["sigma_z"]).any() for p in solid[2]) and any(np.isnan(p["x"]).any() or np.isnan(p["y"]).any() or np.isnan(p["z"]).any() for p in solid[2])
    assert all(np.isfinite(x[f]).all() for c in cs for x in c[5][0] for f in ("x", "y", "z", "sigma"))   # (module docstring)


# ------------------------------------------------------------------------------------------------------------ GPU
@pytest.mark.gpu
def test_gpu_constructed_chains(pkg, gpu):
    """Every constructed case: the states, the landmarks and the counts byte for byte the oracle's, and the same bytes on a
    second run."""
    cs, _ = cases()
    for name, tracks, points, carry, lp, (wl, ws) in cs:
        lm, st = pkg.landmarks_chain(tracks, points, carry, lparams(pkg, lp))
        same(st, ws, name + " state"); same(lm, wl, name)
        lm2, st2 = pkg.landmarks_chain(tracks, points, carry, lparams(pkg, lp))
        same(st2, st, name + " rerun state"); same(lm2, lm, name + " rerun")
    print("landmarks per case:", [(c[0], [len(x) for x in c[5][0]]) for c in cs])


@pytest.mark.gpu
def test_gpu_split_call_single_list_and_deep_chain(pkg, gpu):
    """Two calls, the second taking the first's last state as its carry, equal one call over the concatenated lists; one
    list alone equals landmarks_update with the carry as its prev; a chain of 300 lists of 5 records -- deeper than any
    wave -- equals the oracle."""
    cs, _ = cases()
    name, tracks, points, carry, lp, (wl, ws) = cs[8]
    p = lparams(pkg, lp)
    la, sa = pkg.landmarks_chain(tracks[:2], points[:2], carry, p)
    lb, sb = pkg.landmarks_chain(tracks[2:], points[2:], sa[-1], p)
    same(la + lb, wl, "split"); same(sa + sb, ws, "split state")
    name, tracks, points, carry, lp, (wl, ws) = cs[1]
    p = lparams(pkg, lp)
    l1, s1 = pkg.landmarks_chain(tracks[1:2], points[1:2], ws[0], p)
    l2, s2 = pkg.landmarks_update(tracks[1:2], points[1:2], [ws[0]], p)
    same(l1, l2, "one list"); same(s1, s2, "one list state"); same(l1, wl[1:2], "one list oracle")
    assert len(tracks[1]) == 257 and len(l1[0]) > 0
    lp = lo.params(min_obs=2, max_missed=1, max_dist=0.5, gate_sigma=3.0)
    tracks, points = build((5,) * 300, 77, 0, 2)
    wl, ws = chain_oracle(tracks, points, None, lp)
    lm, st = pkg.landmarks_chain(tracks, points, None, lparams(pkg, lp))
    same(st, ws, "deep state"); same(lm, wl, "deep")
    assert all(t["prev"][0] == 0 for t in tracks[1:]) and max(int(x["n_obs"].max(initial=0)) for x in wl) >= 50


# ---- the handle form
HANDLE_LP = lo.params(min_obs=2, max_missed=1, max_dist=2.0, gate_sigma=3.0)
CHUNKS = ((0, 4), (4, 2), (6, 3))     # a short chunk in the middle; row 0 of the first chunk holds no pair
SEED = 91                             # the synthetic sequence of tests/test_landmarks.py's handle test
ROWS = 4
MM = 4096


def pan(t):
    """The left image's pan in frame t (synth.stereo_sequence): it wraps at every fourth frame -- between the chunks here"""
    return (5 * t) % 20, t % 20


def motions(F):
    """One motion per row, the pair frame F + r - 1 -> F + r: test_motion_inliers.TR2 with the pan's own step, so that the
    pair across the wrap has inliers too (TR2 itself where there is no pair)"""
    tr = np.array([mi.TR2] * ROWS)
    for r in range(ROWS):
        if F + r >= 1:
            (x1, y1), (x0, y0) = pan(F + r), pan(F + r - 1)
            tr[r, 3], tr[r, 4] = -(x1 - x0) * 25 / 300.0, -(y1 - y0) * 25 / 300.0
    return tr


def poses(F):
    """One Tw per row, computed from the index of the row's frame F + r: the translation that undoes its pan (0.4 m per 5
    pixels, as tests/test_landmarks.py's pose_of), the same on both sides of every comparison"""
    Tw = np.stack([np.eye(4)] * ROWS)
    for r in range(ROWS):
        x, y = pan(F + r)
        Tw[r, :3, 3] = (0.08 * x, 0.1 * y, 0.0)
    return Tw


def chunk_step(pkg, g, e, F):
    """matchFeatures .. scenePoints of the chunk whose first frame is F -> (tracks, points) per row"""
    g.matchFeatures(QUAD)
    g.motionInliers(e, motions(F), np.ones(ROWS, np.int32))
    g.scenePoints(e, None, poses(F))
    return [g.getTracks(r) for r in range(ROWS)], [g.getScenePoints(r) for r in range(ROWS)]


def rows_landmarks(g, lp):
    counts = g.landmarks(lp)
    got = [g.getLandmarks(r) for r in range(ROWS)]
    assert [len(x) for x in got] == counts.tolist()
    return got


def run_handle(pkg, skip_second=False):
    """The three chunks on a SequenceGroup(4) -> per chunk (got rows, want rows); the checks that need the handle inside"""
    dims = sr.dims_of(pkg)
    frames = sr.frames_of(pkg, 9, SEED)
    e = mi.hego(pkg, inlier_threshold=2.5)
    lp = lparams(pkg, HANDLE_LP)
    g = pkg.SequenceGroup(ROWS, pkg.Params.default(), max_matches=MM)
    g.setTrackLinking(True); g.setLandmarks(True)
    g.profileEnable(True)
    expect(pkg, pkg.VH_ERR_STATE, lambda: g.landmarks(lp))          # nothing pushed
    carry, res, calls = None, [], 0
    for i, (F, n) in enumerate(CHUNKS):
        sr.push(g, frames, F, n, dims)
        if i == 0:
            expect(pkg, pkg.VH_ERR_STATE, lambda: g.setLandmarks(False))   # after the first push
            expect(pkg, pkg.VH_ERR_STATE, lambda: g.landmarks(lp))  # pushed, not matched
        tracks, points = chunk_step(pkg, g, e, F)
        if i == 1 and skip_second:                                   # no call on this chunk: the next one starts without state
            carry = None
            continue
        if i == 0:                                                   # the block: nothing before the first call, all of it by the call
            g.synchronize()
            bytes0 = g.deviceBytes()
            g.debugFailNextAlloc()
            expect(pkg, pkg.VH_ERR_HIP, lambda: g.landmarks(lp))
            g.synchronize()
            assert g.deviceBytes() == bytes0 and g.profileRead("landmarks")[1] == 0
        want, states = pkg.landmarks_chain(tracks[:n], points[:n], carry, lp)
        want += [np.zeros(0, lo.LANDMARK)] * (ROWS - n)
        got = rows_landmarks(g, lp); calls += 1
        same(got, want, f"chunk {i}")
        same(rows_landmarks(g, lp), want, f"chunk {i} again"); calls += 1
        if i == 0:
            _, stride = g.landmarksDevice()
            up = lambda b: (b + 255) // 256 * 256  # noqa: E731
            block = (up(48 * ROWS * stride) + up(48 * stride) + up(48 * ROWS * stride) + up(8 * ROWS * stride)
                     + up(4 * ROWS * ((stride + 255) // 256)) + up(4 * ROWS))
            assert stride >= MM and g.deviceBytes() == bytes0 + block, (g.deviceBytes() - bytes0, block)
            assert len(got[0]) == 0 and len(tracks[0]) == 0          # row 0 of the first chunk is empty
        out, counts = g.getLandmarksAll(max(1, max(len(x) for x in want)))
        assert all(out[r, :counts[r]].tobytes() == want[r].tobytes() for r in range(ROWS))
        d, stride = g.landmarksDevice()
        for r in range(ROWS):
            if len(want[r]):
                assert mi.hip_read(d + r * stride * 48, len(want[r]), lo.LANDMARK).tobytes() == want[r].tobytes()
        if i == 1:                                                   # the chunk matched again: recomputed from the same carry
            tracks2, points2 = chunk_step(pkg, g, e, F)
            assert all(a.tobytes() == b.tobytes() for a, b in zip(tracks + points, tracks2 + points2))
            same(rows_landmarks(g, lp), want, "chunk 1 rematched"); calls += 1
        res.append((i, want))
        carry = states[n - 1]
    g.synchronize()
    assert g.deviceBytes() == bytes0 + block and g.profileRead("landmarks")[1] == calls
    assert g.profileRead("landmark_chain")[1] == calls
    g.close()
    return res


@pytest.mark.gpu
def test_gpu_sequence_handle(pkg, gpu):
    """SequenceGroup(4), track linking and landmarks on, chunks of 4, 2 and 3 frames: every row equals landmarks_chain fed
    with getTracks / getScenePoints of the rows and the previous chunk's last state; a repeated call gives the same bytes;
    after a re-match plus scene points plus landmarks the bytes are equal again and the next chunk still carries;
    getLandmarksAll and landmarksDevice agree with getLandmarks; deviceBytes is unchanged before the first call and grows by
    exactly the documented block, once; a refused allocation is VH_ERR_HIP and the repeated call is right; the setter after
    the first push is refused; a handle without setLandmarks answers VH_ERR_UNSUPPORTED.  The inputs are not vacuous: the
    landmark total is above 0, some landmark has n_obs >= 3, and some landmark in row 0 of chunk 2 has n_obs >= 2 -- a
    state crossed the chunk boundary."""
    res = run_handle(pkg)
    total = sum(len(x) for _, want in res for x in want)
    deep = max(int(x["n_obs"].max(initial=0)) for _, want in res for x in want)
    crossed = int(res[1][1][0]["n_obs"].max(initial=0))
    print("landmarks:", total, "deepest n_obs:", deep, "row 0 of chunk 2:", crossed)
    assert total > 0 and deep >= 3 and crossed >= 2, (total, deep, crossed)
    assert int(res[2][1][0]["n_obs"].max(initial=0)) >= 2            # ... and again behind the re-matched chunk
    lp = lparams(pkg, HANDLE_LP)
    off = pkg.SequenceGroup(ROWS, pkg.Params.default(), max_matches=MM); off.setTrackLinking(True)
    expect(pkg, pkg.VH_ERR_UNSUPPORTED, lambda: off.landmarks(lp))
    off.close()
    plain = pkg.StreamGroup(2, pkg.Params.default())
    assert pkg._lib().vh_sequence_set_landmarks(plain._h, 1) == pkg.VH_ERR_UNSUPPORTED
    plain.close()


@pytest.mark.gpu
def test_gpu_sequence_handle_skipped_chunk(pkg, gpu):
    """No landmarks call on chunk 2: chunk 3 is the carry = None result (run_handle compares it with that).  Every record
    of its row 0 then starts without state, so under min_obs = 2 that row emits nothing, while the rows behind it do."""
    res = run_handle(pkg, skip_second=True)
    assert [i for i, _ in res] == [0, 2] and HANDLE_LP["min_obs"] == 2
    rows = res[1][1]
    assert len(rows[0]) == 0 and sum(len(x) for x in rows[1:]) > 0


@pytest.mark.gpu
def test_child_checking_build(pkg, gpu):
    """The handle test and the constructed chains once more on libviso_hip_check.so (-DVH_CHECK): every successor position a
    walker follows is verified on the device, and no violation is reported."""
    assert os.path.exists(pkg.CHECK_LIB_PATH), "build() makes it"
    env = dict(os.environ, VISO_HIP_LIB=pkg.CHECK_LIB_PATH)
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-q", "-x", "-m", "gpu", "-k",
                        "test_gpu_sequence_handle or test_gpu_constructed_chains"], env=env, capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert " passed" in r.stdout and " skipped" not in r.stdout, r.stdout[-2000:]
    assert "VH_CHECK" not in r.stderr
