"""Reconstruction on a sequence handle and on caller-owned lists: vh_sequence_set_reconstruction,
vh_sequence_reconstruct, vh_sequence_get_recon_tracks, vh_reconstruct_lists against tests/sequence_recon_oracle.py -- the
link rule of tests/track_oracle.py plus reconstruction_oracle.solve_track -- and, where every list's i1c values are
distinct, against the reference's own Reconstruction (reconstruction_oracle.Reconstruction, the golden fixture)."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import recon_cases as rc
import reconstruction_oracle as ro
import sequence_recon_oracle as so
from conftest import GOLDEN, ROOT

SYMBOLS = ("vh_sequence_set_reconstruction", "vh_sequence_reconstruct", "vh_sequence_get_recon_tracks", "vh_reconstruct_lists")
ANGLE_TOL = 1e-9   # degrees: the device's acos is not glibc's (the rule of tests/test_reconstruction.py)
W, H = 320, 160
FLOW, STEREO, QUAD = 0, 1, 2
CAL = (300.0, 160.0, 80.0)
LOOSE = dict(point_type=0, min_track_length=2, max_dist=1e6, min_angle=0.0)   # classification does not hang on the angle


def ptr(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def same(got, want, what=""):
    """Records byte-equal but for the angle, which agrees to ANGLE_TOL."""
    assert len(got) == len(want), (what, len(got), len(want))
    a, b = np.array(got, so.RECON_TRACK), np.array(want, so.RECON_TRACK)
    da = np.abs(a["angle"] - b["angle"])
    assert np.all((da <= ANGLE_TOL) | (np.isnan(a["angle"]) & np.isnan(b["angle"]))), (what, da.max())
    a["angle"] = b["angle"] = 0
    assert a.tobytes() == b.tobytes(), (what, [(x, y) for x, y in zip(a, b) if x.tobytes() != y.tobytes()][:3])


def fixture_lists():
    z = np.load(os.path.join(GOLDEN, "reconstruction_reference.npz"))
    ends = np.cumsum(z["list_counts"])
    lists = [z["matches"][e - n:e] for e, n in zip(ends, z["list_counts"])]
    return [float(v) for v in z["calibration"]], z["Trs"], lists, z["points"]


def first_of_each_i1c(lists):
    """The fixture's lists without the later records of a repeated i1c: where the link rule and the reference agree."""
    out = []
    for pm in lists:
        keep = np.zeros(len(pm), bool)
        keep[np.unique(pm["i1c"], return_index=True)[1]] = True
        out.append(pm[keep])
    return out


def records(pkg, i1p, i1c, px=None):
    pm = np.zeros(len(i1p), pkg.P_MATCH_DTYPE)
    pm["i1p"], pm["i1c"] = i1p, i1c
    if px is not None:
        pm["u1p"], pm["v1p"], pm["u1c"], pm["v1c"] = px
    return pm


def poses_of(n):
    return [rc.pose(0.0, -0.004 * k, 0.0, (0.03 * k, 0.0, 0.5 * k)) for k in range(n)]


def random_chain_lists(pkg, rng, n_lists, max_len, n_index, lengths=None, empty=()):
    """Lists whose records mostly continue a record of the list before (i1p drawn from its i1c), with duplicate i1p and
    i1c, i1p = -1 and indices >= n_index; pixels of static points seen along poses_of, so that tracks solve."""
    poses = poses_of(n_lists + 1)
    out, prev_c = [], np.zeros(0, np.int64)
    for l in range(n_lists):
        n = 0 if l in empty else (lengths[l] if lengths is not None else int(rng.integers(1, max_len + 1)))
        pm = np.zeros(n, pkg.P_MATCH_DTYPE)
        pm["i1c"] = rng.integers(0, n_index + n_index // 8, n)
        pm["i1p"] = rng.integers(-1, n_index + n_index // 8, n)
        if len(prev_c) and n:
            take = rng.random(n) < 0.8
            pm["i1p"][take] = rng.choice(prev_c, int(take.sum()))
        pm["i1p"][rng.random(n) < 0.05] = -1
        for j in range(n):
            Z = rng.uniform(6, 30)
            Pw = (np.linalg.inv(poses[l]) @ np.array([rng.uniform(-0.4, 0.4) * Z, rng.uniform(-0.2, 0.2) * Z, Z, 1.0]))[:3]
            (pm["u1p"][j], pm["v1p"][j]), (pm["u1c"][j], pm["v1c"][j]) = (np.round(rc.project(poses[l + k], Pw)[:2]) for k in (0, 1))
        out.append(pm)
        prev_c = np.array(pm["i1c"], np.int64)
    return out, rc.trs_of(poses)


# ------------------------------------------------------------------------------------------------------------ CPU
def test_symbols_declared_exported_mirrored(pkg):
    header = open(os.path.join(ROOT, "include", "viso_hip.h")).read()
    lib = C.CDLL(pkg.LIB_PATH)
    for name in SYMBOLS:
        assert name + "(" in header, name
        assert hasattr(lib, name), name
        assert name in pkg.ABI_SYMBOLS, name
    assert "VH_RECON_HISTORY 6" in header and pkg.RECON_HISTORY == 6 == so.HISTORY
    for meth in ("setReconstruction", "reconstruct"):
        assert hasattr(pkg.SequenceGroup, meth), meth
    assert callable(pkg.reconstruct_lists)
    for scope in ("recon_store", "recon_tails", "recon_gather", "recon_solve"):
        assert '"%s"' % scope in header, scope


def test_record_layout(pkg, tmp_path):
    want = {"birth_frame": 0, "birth_pos": 8, "frames": 12, "lost_frame": 16, "status": 24, "point": 28, "distance": 40, "angle": 48}
    assert pkg.RECON_TRACK.itemsize == 56 == so.RECON_TRACK.itemsize and pkg.RECON_TRACK == so.RECON_TRACK
    assert {k: pkg.RECON_TRACK.fields[k][1] for k in pkg.RECON_TRACK.names} == want
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include "viso_hip.h"\n'
                   "_Static_assert(sizeof(vh_recon_track) == 56, \"size\");\n"
                   + "".join(f"_Static_assert(offsetof(vh_recon_track, {k}) == {v}, \"{k}\");\n" for k, v in want.items())
                   + "int main(void) { return 0; }\n")
    r = subprocess.run(["gcc", "-std=c11", "-I", os.path.join(ROOT, "include"), "-c", str(src), "-o", str(tmp_path / "layout.o")],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_null_and_argument_errors_need_no_gpu(pkg):
    lib = pkg._lib()
    r = pkg.ReconParams.default()
    n, na = C.c_int32(7), C.c_int32(7)
    out = np.zeros(4, pkg.RECON_TRACK)
    tr = np.zeros((1, 16))
    inv = pkg.VH_ERR_INVALID_ARG
    assert lib.vh_sequence_set_reconstruction(None, C.byref(r), 4) == inv
    assert lib.vh_sequence_reconstruct(None, ptr(tr), C.byref(n), C.byref(na)) == inv
    assert lib.vh_sequence_get_recon_tracks(None, ptr(out), 4, C.byref(n)) == inv
    pm = np.zeros(4, pkg.P_MATCH_DTYPE)
    cnt = np.array([4], np.int32)
    call = lambda *a: lib.vh_reconstruct_lists(*a)  # noqa: E731
    assert call(None, 0, 1, ptr(pm), 4, ptr(cnt), 8, ptr(tr), ptr(out), 4, C.byref(n)) == inv
    assert call(C.byref(r), 0, 1, ptr(pm), 4, ptr(cnt), 8, ptr(tr), ptr(out), 4, None) == inv
    assert call(C.byref(r), 0, -1, ptr(pm), 4, ptr(cnt), 8, ptr(tr), ptr(out), 4, C.byref(n)) == inv
    assert call(C.byref(r), 0, 1, ptr(pm), 4, None, 8, ptr(tr), ptr(out), 4, C.byref(n)) == inv
    assert call(C.byref(r), 0, 1, None, 4, ptr(cnt), 8, ptr(tr), ptr(out), 4, C.byref(n)) == inv
    assert call(C.byref(r), 0, 1, ptr(pm), 4, ptr(cnt), 8, None, ptr(out), 4, C.byref(n)) == inv
    assert call(C.byref(r), 0, 1, ptr(pm), 4, ptr(cnt), 0, ptr(tr), ptr(out), 4, C.byref(n)) == inv
    assert call(C.byref(r), 0, 1, ptr(pm), 2, ptr(cnt), 8, ptr(tr), ptr(out), 4, C.byref(n)) == inv   # count > stride
    assert call(C.byref(r), 0, 1, ptr(pm), 4, ptr(cnt), 8, ptr(tr), None, 4, C.byref(n)) == inv
    assert call(C.byref(r), 0, 1, ptr(pm), 4, ptr(cnt), 8, ptr(tr), ptr(out), -1, C.byref(n)) == inv
    n.value = 7
    assert call(C.byref(r), 0, 0, None, 0, None, 8, None, None, 0, C.byref(n)) == pkg.VH_OK and n.value == 0
    assert len(pkg.reconstruct_lists(r, [], np.zeros((0, 4, 4)), 8)) == 0


def test_oracle_equals_reference_where_i1c_is_distinct(oracle):
    """Every list of the fixture but one repeats an i1c, and the two rules part at the fourth update already (26 of its 314
    lost tracks before it): so the comparison runs on the fixture's lists without the later records of a repeated i1c,
    which keeps 294 of the 314 lost tracks.  Those lists are another drive than the recorded one -- a removed record
    shortens or splits a track: 46 of its 55 points are the fixture's, 9 are not (keeping the LAST record of an i1c
    instead: 51 of 52) -- so the reference here is the restated Reconstruction fed the same lists, which
    tests/test_reconstruction.py pins to the fixture's recorded points on the original lists."""
    cal, Trs, lists, points = fixture_lists()
    assert sum(len(np.unique(pm["i1c"])) < len(pm) for pm in lists) >= 5
    ref_all = ro.Reconstruction(oracle.svd)
    ref_all.setCalibration(*cal)
    for pm, Tr in zip(lists, Trs):
        ref_all.update(pm, Tr, solve=False)
    dl = first_of_each_i1c(lists)
    assert all(len(np.unique(pm["i1c"])) == len(pm) for pm in dl)
    ref = ro.Reconstruction(oracle.svd)
    ref.setCalibration(*cal)
    lost_at = []
    for k, (pm, Tr) in enumerate(zip(dl, Trs)):
        n0 = len(ref.lost_log)
        ref.update(pm, Tr)
        lost_at += [k + 1] * (len(ref.lost_log) - n0)
    assert 2 * len(ref.lost_log) >= len(ref_all.lost_log) > 300
    got = so.whole(oracle.svd, cal, dl, Trs)
    assert got["lost_frame"].tolist() == lost_at
    assert [(int(r["birth_frame"]) - 1, int(r["frames"])) for r in got] == [(f, len(px)) for f, px in ref.lost_log]
    assert len(ref.getPoints()) == len(points) == 55
    assert got[got["status"] == ro.ACCEPTED]["point"].tobytes() == ref.getPoints().tobytes()


def test_oracle_follows_the_link_rule_on_a_duplicated_i1c(pkg, oracle):
    """Two records of list 0 end in feature 3; one record of list 1 continues it.  The link rule continues the LOWER
    position (record 0), the reference the LATER track (record 1): the one difference."""
    poses = poses_of(3)
    Trs = rc.trs_of(poses)
    a = records(pkg, [-1, -1], [3, 3], ([100, 200], [50, 60], [101, 201], [50, 60]))
    b = records(pkg, [3], [5], ([101], [50], [102], [50]))
    got = so.whole(oracle.svd, CAL, [a, b], Trs, **LOOSE)
    assert [(int(r["birth_pos"]), int(r["lost_frame"])) for r in got] == [(1, 2)]      # record 1 is lost, record 0 goes on
    ref = ro.Reconstruction(oracle.svd)
    ref.setCalibration(*CAL)
    for pm, Tr in zip([a, b], Trs):
        ref.update(pm, Tr, solve=False)
    assert [(f, [tuple(map(float, p)) for p in px]) for f, px in ref.lost_log] == [(0, [(100.0, 50.0), (101.0, 50.0)])]  # record 0 is lost


@pytest.fixture(scope="module")
def constructed(pkg, oracle):
    """40 constructed lists and the oracle's whole-drive answer (computed once, shared, left unchanged)."""
    rng = np.random.default_rng(7)
    lists, Trs = random_chain_lists(pkg, rng, 40, 12, 30)
    return lists, Trs, so.whole(oracle.svd, CAL, lists, Trs, n_index=30, **LOOSE)


def test_oracle_chunking_invariance(constructed, oracle):
    lists, Trs, whole = constructed
    assert int(whole["frames"].max()) > 5 and len(whole) > 100
    for T in (1, 7, 16):
        got = np.concatenate(so.run(oracle.svd, CAL, lists, Trs, 64, T, n_index=30, **LOOSE))
        assert got.tobytes() == whole.tobytes(), T


def test_oracle_history_turns_old_tracks_only(constructed, oracle):
    lists, Trs, whole = constructed
    got = np.concatenate(so.run(oracle.svd, CAL, lists, Trs, 3, 7, n_index=30, **LOOSE))
    old = whole["frames"] - 1 > 3
    assert old.any() and not old.all()
    want = whole.copy()
    for k in ("point", "distance", "angle"):
        want[k][old] = 0
    want["status"][old] = so.HISTORY
    assert got.tobytes() == want.tobytes()


# ------------------------------------------------------------------------------------------------------------ GPU
@pytest.mark.gpu
def test_lists_constructed_sizes(pkg, oracle, gpu):
    """List lengths 0, 1, 63, 64, 65 and 257 (part of a wave, one wave, more than one workgroup), an empty list in the middle,
    duplicate i1p and i1c, i1p = -1 and indices >= n_index."""
    rng = np.random.default_rng(13)
    lengths = [1, 63, 64, 65, 257, 257, 0, 65, 64, 63, 1, 257]
    lists, Trs = random_chain_lists(pkg, rng, len(lengths), 0, 200, lengths=lengths, empty=(6,))
    assert any((pm["i1p"] == -1).any() for pm in lists) and any((pm["i1c"] >= 200).any() for pm in lists)
    assert any(len(np.unique(pm["i1c"])) < len(pm) for pm in lists) and any(len(np.unique(pm["i1p"])) < len(pm) for pm in lists)
    want = so.whole(oracle.svd, CAL, lists, Trs, n_index=200, **LOOSE)
    assert (want["lost_frame"] == 7).sum() == 257 and int(want["frames"].max()) >= 4   # the empty list loses every pending track
    r = pkg.ReconParams.default(f=CAL[0], cu=CAL[1], cv=CAL[2], **LOOSE)
    same(pkg.reconstruct_lists(r, lists, Trs, 200), want)
    # the capacity rule of the stateless entry
    n = len(lists)
    stride = max(len(m) for m in lists)
    pm = np.zeros((n, stride), pkg.P_MATCH_DTYPE)
    for l, m in enumerate(lists):
        pm[l, :len(m)] = m
    counts = np.array([len(m) for m in lists], np.int32)
    tr = np.ascontiguousarray(Trs, np.float64).reshape(-1, 16)
    out = np.zeros(5, pkg.RECON_TRACK)
    got = C.c_int32(0)
    rcode = pkg._lib().vh_reconstruct_lists(C.byref(r), 0, n, ptr(pm), stride, ptr(counts), 200, ptr(tr), ptr(out), 5, C.byref(got))
    assert rcode == pkg.VH_ERR_CAPACITY and got.value == len(want)
    same(out, want[:5])


@pytest.mark.gpu
def test_lists_forty_constructed_and_one_long_chain(pkg, oracle, constructed, gpu):
    lists, Trs, whole = constructed
    r = pkg.ReconParams.default(f=CAL[0], cu=CAL[1], cv=CAL[2], **LOOSE)
    same(pkg.reconstruct_lists(r, lists, Trs, 30), whole)
    # one chain through all of 40 lists, lost only because list 40 does not continue it; beside it a track per list
    poses = poses_of(42)
    Pw = np.array([1.5, -0.8, 40.0])
    chain = []
    for l in range(41):
        (u0, v0), (u1, v1) = (np.round(rc.project(poses[l + k], Pw)[:2]) for k in (0, 1))
        if l < 40:
            chain.append(records(pkg, [7, -1], [7, 9], ([u0, 50], [v0, 60], [u1, 51], [v1, 60])))
        else:
            chain.append(records(pkg, [-1], [9], ([50], [60], [51], [60])))
    want = so.whole(oracle.svd, CAL, chain, rc.trs_of(poses), n_index=16, **LOOSE)
    assert int(want["frames"].max()) == 41 and len(want) == 41
    same(pkg.reconstruct_lists(r, chain, rc.trs_of(poses), 16), want)


@pytest.mark.gpu
@pytest.mark.parametrize("point_type", [0, 1, 2])
def test_lists_every_status_value(point_type, pkg, oracle, gpu):
    """The constructed tracks of tests/recon_cases.py, one per outcome, laid into lists: track k keeps feature index k."""
    theta = rc.c_zero_theta(rc.C_ZERO_POINT)
    for _ in range(2):   # the turn of frame 11 from the point as initPoint computes it (as tests/test_reconstruction.py)
        poses = rc.status_poses(theta)
        tab = ro.Tables(rc.F, rc.CU, rc.CV)
        for T in rc.trs_of(poses):
            tab.push(T)
        tracks = rc.status_tracks(poses)
        f, px = tracks["c_zero"]
        theta = rc.c_zero_theta(ro.init_point(tab, oracle.svd, f, f + 2, px))
    names = [nm for nm in tracks if len(tracks[nm][1]) >= 2]   # (a list record spans two frames: no one-frame track)
    n_lists = len(poses)                                       # one list more than pairs: the last pair's tracks are lost in it
    rows = [[] for _ in range(n_lists)]
    for k, nm in enumerate(names):
        f, px = tracks[nm]
        for i in range(len(px) - 1):
            rows[f + i].append((k if i else -1, k, px[i][0], px[i][1], px[i + 1][0], px[i + 1][1]))
    lists = [records(pkg, [r[0] for r in row], [r[1] for r in row], tuple([r[c] for r in row] for c in (2, 3, 4, 5))) for row in rows]
    Trs = np.concatenate([rc.trs_of(poses), np.eye(4)[None]])
    seen = set()
    for min_len in (2, 3):   # (a list record spans two frames: SHORT needs min_track_length = 3)
        kw = dict(point_type=point_type, min_track_length=min_len, max_dist=30.0, min_angle=2.0)
        want = so.whole(oracle.svd, (rc.F, rc.CU, rc.CV), lists, Trs, n_index=32, **kw)
        assert len(want) == len(names)
        seen |= set(want["status"].tolist())
        r = pkg.ReconParams.default(f=rc.F, cu=rc.CU, cv=rc.CV, **kw)
        same(pkg.reconstruct_lists(r, lists, Trs, 32), want)
    assert seen == set(range(6))


@pytest.mark.gpu
def test_lists_reference_fixture(pkg, oracle, gpu):
    """The fixture's lists without the later records of a repeated i1c, the fixture's Trs and calibration: the accepted
    points, in order, are those of the restated reference fed the same lists (not the fixture's recorded `points`: the
    treated lists are another drive, see test_oracle_equals_reference_where_i1c_is_distinct)."""
    cal, Trs, lists, points = fixture_lists()
    dl = first_of_each_i1c(lists)
    assert all(len(np.unique(pm["i1c"])) == len(pm) for pm in dl)
    ref = ro.Reconstruction(oracle.svd)
    ref.setCalibration(*cal)
    for pm, Tr in zip(dl, Trs):
        ref.update(pm, Tr)
    r = pkg.ReconParams.default(f=cal[0], cu=cal[1], cv=cal[2])
    got = pkg.reconstruct_lists(r, dl, Trs, 1 + max(int(pm["i1c"].max()) for pm in dl))
    assert len(ref.getPoints()) == len(points)
    assert got[got["status"] == pkg.RECON_ACCEPTED]["point"].tobytes() == ref.getPoints().tobytes()


def frames_of(pkg, T, seed, w=W, h=H):
    return pkg.synth.stereo_sequence(w, h, T, disparity=6, blur=3, seed=seed)


def dims_of(pkg, w=W, h=H):
    return [w, h, pkg.synth.bytes_per_line(w)]


def push(g, frames, F, n, dims):
    g.pushBack(np.stack([frames[t][0] for t in range(F, F + n)]), np.stack([frames[t][1] for t in range(F, F + n)]), dims)


def rows_of(g, lo, n):
    rec, counts = g.getMatchesAll()
    return [rec[r, :counts[r]].copy() for r in range(lo, n)]


def row_trs(Trs, F, n):
    """One Tr per row of the chunk at F: the motion F+r-1 -> F+r (row 0 of the first chunk holds no pair)."""
    return np.array([Trs[F + r - 1] if F + r >= 1 else np.eye(4) for r in range(n)])


def recon_params(pkg, **kw):
    return pkg.ReconParams.default(f=CAL[0], cu=CAL[1], cv=CAL[2], **dict(LOOSE, **kw))


_DRIVES = {}


def drive40(pkg, oracle, meth):
    """40 synthetic frames: the lists (from a handle without reconstruction), constructed Trs and the oracle's whole-drive
    records, computed once per method and left unchanged."""
    if meth not in _DRIVES:
        frames, dims = frames_of(pkg, 40, 41), dims_of(pkg)
        g = pkg.SequenceGroup(40, pkg.Params.default())
        push(g, frames, 0, 40, dims)
        g.matchFeatures(meth)
        lists = rows_of(g, 1, 40)
        g.close()
        Trs = rc.trs_of(poses_of(40))
        _DRIVES[meth] = (frames, dims, lists, Trs, so.whole(oracle.svd, CAL, lists, Trs, **LOOSE))
    return _DRIVES[meth]


def history_of(whole, Hh):
    want = whole.copy()
    old = want["frames"] - 1 > Hh
    for k in ("point", "distance", "angle"):
        want[k][old] = 0
    want["status"][old] = so.HISTORY
    return want


def run_handle(pkg, frames, dims, meth, T, Hh, Trs, whole, after_next_push=False):
    """The drive through a handle in chunks of T; every chunk's records against the oracle's records lost in its frames.
    -> all records."""
    N = len(frames)
    want = history_of(whole, Hh)
    g = pkg.SequenceGroup(T, pkg.Params.default())
    g.setReconstruction(recon_params(pkg), Hh)
    got_all, lists = [], []
    chunks = [(F, min(T, N - F)) for F in range(0, N, T)]
    for i, (F, n) in enumerate(chunks):
        if not (after_next_push and i):
            push(g, frames, F, n, dims)
        g.matchFeatures(meth)
        lists += rows_of(g, 1 if F == 0 else 0, n)
        if after_next_push and i + 1 < len(chunks):
            push(g, frames, *chunks[i + 1], dims)          # detection of chunk k+1 runs beside reconstruct k
        got = g.reconstruct(row_trs(Trs, F, n))
        lo, hi = max(F, 1), F + n
        same(got, want[(want["lost_frame"] >= lo) & (want["lost_frame"] < hi)], (T, F))
        got_all.append(got)
    g.close()
    return np.concatenate(got_all), lists


@pytest.mark.gpu
@pytest.mark.parametrize("meth", (FLOW, QUAD))
def test_sequence_handle_equals_oracle_and_reference(pkg, oracle, gpu, meth):
    frames, dims, lists, Trs, whole = drive40(pkg, oracle, meth)
    for pm in lists:
        assert len(np.unique(pm["i1c"])) == len(pm) and len(np.unique(pm["i1p"])) == len(pm)
    # properties of the inputs, on the oracle's answer alone
    assert int(whole["frames"].max()) - 1 > 16                   # history crosses a chunk boundary of T = 16; the ring of T = 1 wraps
    assert any(int(f) % 16 == 0 for f in whole["lost_frame"]) and any(int(f) % 7 == 0 for f in whole["lost_frame"])   # lost at a row-0 boundary
    assert len(whole) > 50 and (whole["status"] == ro.ACCEPTED).any()
    ref = ro.Reconstruction(oracle.svd)
    ref.setCalibration(*CAL)
    for pm, Tr in zip(lists, Trs):
        ref.update(pm, Tr, 0, 2, 1e6, 0.0)
    for T in (1, 7, 16):
        got, seen = run_handle(pkg, frames, dims, meth, T, 64, Trs, whole)
        assert all(a.tobytes() == b.tobytes() for a, b in zip(seen, lists)) and len(seen) == len(lists)
        assert got[got["status"] == pkg.RECON_ACCEPTED]["point"].tobytes() == ref.getPoints().tobytes(), T


@pytest.mark.gpu
def test_sequence_handle_short_history(pkg, oracle, gpu):
    frames, dims, lists, Trs, whole = drive40(pkg, oracle, FLOW)
    got, _ = run_handle(pkg, frames, dims, FLOW, 7, 4, Trs, whole)
    n_old = int((whole["frames"] - 1 > 4).sum())
    assert n_old > 0 and int((got["status"] == pkg.RECON_HISTORY).sum()) == n_old


@pytest.mark.gpu
def test_reconstruct_after_the_next_push(pkg, oracle, gpu):
    frames, dims, lists, Trs, whole = drive40(pkg, oracle, FLOW)
    a, _ = run_handle(pkg, frames[:24], dims, FLOW, 7, 64, Trs, whole[whole["lost_frame"] < 24], after_next_push=True)
    assert len(a) > 50


def expect(pkg, code, call):
    with pytest.raises(pkg.VisoHipError) as e:
        call()
    assert e.value.code == code, e.value


@pytest.mark.gpu
def test_call_order_rematch_and_resets(pkg, oracle, gpu):
    """Twice for one chunk and before any match: VH_ERR_STATE.  A rematch before the call replaces the lists.  A chunk
    matched but not reconstructed, a chunk never matched and a dims change start a new Reconstruction, as the oracle's reset()."""
    dims = dims_of(pkg)
    frames = frames_of(pkg, 24, 43)
    Trs = rc.trs_of(poses_of(24))
    g = pkg.SequenceGroup(4, pkg.Params.default())
    g.setReconstruction(recon_params(pkg), 16)
    d = so.Drive(oracle.svd, CAL, 16, **LOOSE)
    expect(pkg, pkg.VH_ERR_STATE, lambda: g.reconstruct(np.zeros((4, 4, 4))))
    push(g, frames, 0, 4, dims)
    expect(pkg, pkg.VH_ERR_STATE, lambda: g.reconstruct(row_trs(Trs, 0, 4)))   # pushed, not matched
    g.matchFeatures(FLOW)
    g.matchFeatures(QUAD)                                                      # the call sees the last lists
    same(g.reconstruct(row_trs(Trs, 0, 4)), d.chunk(1, rows_of(g, 1, 4), Trs[0:3]), "rematch")
    expect(pkg, pkg.VH_ERR_STATE, lambda: g.reconstruct(row_trs(Trs, 0, 4)))   # twice
    total = 0
    for F, what in ((4, "go"), (8, "skip"), (12, "go"), (16, "unmatched"), (20, "go")):
        push(g, frames, F, 4, dims)
        if what == "unmatched":
            d.reset()
            continue
        g.matchFeatures(QUAD)
        if what == "skip":
            d.reset()
            continue
        got = g.reconstruct(row_trs(Trs, F, 4))
        want = d.chunk(F, rows_of(g, 0, 4), Trs[F - 1:F + 3])
        same(got, want, (F, what))
        if F in (12, 20):   # after a break: nothing is lost at the chunk's first frame, every track is born inside it
            assert len(got) and int(got["lost_frame"].min()) == F + 1 and int(got["birth_frame"].min()) == F
            assert (g.getTracks(0)["age"] == 1).all()
        total += len(got)
    assert total > 50
    w2, h2 = 288, 144
    fb = frames_of(pkg, 8, 48, w=w2, h=h2)
    d.reset()
    for F in (0, 4):
        push(g, fb, F, 4, dims_of(pkg, w2, h2))
        g.matchFeatures(QUAD)
        lo = 1 if F == 0 else 0
        same(g.reconstruct(row_trs(Trs, F, 4)), d.chunk(F + lo, rows_of(g, lo, 4), Trs[F + lo - 1:F + 3]), ("dims", F))
    g.close()


@pytest.mark.gpu
def test_switch_rules_and_capacity(pkg, oracle, gpu):
    r = recon_params(pkg)
    dims = dims_of(pkg)
    frames = frames_of(pkg, 6, 45)
    plain = pkg.StreamGroup(2, pkg.Params.default())
    assert pkg._lib().vh_sequence_set_reconstruction(plain._h, C.byref(r), 4) == pkg.VH_ERR_UNSUPPORTED
    plain.close()
    g = pkg.SequenceGroup(6, pkg.Params.default())
    assert pkg._lib().vh_sequence_set_reconstruction(g._h, C.byref(r), 0) == pkg.VH_ERR_INVALID_ARG
    g.setReconstruction(r, 8)
    expect(pkg, pkg.VH_ERR_STATE, lambda: g.setTrackLinking(False))   # linking is on underneath, and stays
    push(g, frames, 0, 6, dims)
    expect(pkg, pkg.VH_ERR_STATE, lambda: g.setReconstruction(r, 8))   # after the first push
    g.matchFeatures(FLOW)
    assert len(g.getTracks(1)) == len(g.getMatches(1)) > 20
    n = C.c_int32(0)
    assert pkg._lib().vh_sequence_get_recon_tracks(g._h, None, 0, C.byref(n)) == pkg.VH_ERR_STATE   # nothing reconstructed yet
    full = g.reconstruct(row_trs(rc.trs_of(poses_of(6)), 0, 6))
    assert len(full) > 10
    part = np.zeros(10, pkg.RECON_TRACK)
    rcode = pkg._lib().vh_sequence_get_recon_tracks(g._h, ptr(part), 10, C.byref(n))
    assert rcode == pkg.VH_ERR_CAPACITY and n.value == len(full) and part.tobytes() == full[:10].tobytes()
    g.close()


@pytest.mark.gpu
def test_switch_off_changes_nothing(pkg, gpu):
    """Linking on, against reconstruction set and cleared again: same lists, tracks and device bytes, no launch in the new
    scopes.  Reconstruction on: same lists and tracks, the ring counted in the device bytes."""
    dims = dims_of(pkg)
    frames = frames_of(pkg, 8, 55)
    Trs = rc.trs_of(poses_of(8))
    scopes = ("recon_store", "recon_tails", "recon_gather", "recon_solve")
    seen = {}
    for name in ("link", "cleared", "on"):
        g = pkg.SequenceGroup(4, pkg.Params.default(), max_features=8192, max_matches=8192)
        if name == "link":
            g.setTrackLinking(True)
        else:
            g.setReconstruction(recon_params(pkg), 8)
            if name == "cleared":
                g.setReconstruction(None)
        g.profileEnable(True)
        out = []
        for F in (0, 4):
            push(g, frames, F, 4, dims)
            g.matchFeatures(QUAD)
            out += [g.getMatches(r).tobytes() for r in range(4)] + [g.getTracks(r).tobytes() for r in range(4)]
            if name == "on":
                g.reconstruct(row_trs(Trs, F, 4))
            else:
                expect(pkg, pkg.VH_ERR_STATE, lambda: g.reconstruct(row_trs(Trs, F, 4)))
        seen[name] = (out, g.deviceBytes(), tuple(g.profileRead(k)[1] for k in scopes))
        g.close()
    assert seen["link"] == seen["cleared"] and seen["link"][2] == (0, 0, 0, 0)
    assert seen["on"][0] == seen["link"][0]
    assert seen["on"][2] == (2, 4, 2, 2)   # (recon_tails: the counting and the appending launch)
    assert seen["on"][1] - seen["link"][1] >= 32 * 8192 * (8 + 4)   # the ring: 32 bytes per record, history + max_frames slots


@pytest.mark.gpu
def test_failed_allocation_inside_the_first_reconstruct(pkg, oracle, gpu):
    dims = dims_of(pkg)
    frames = frames_of(pkg, 5, 57)
    Trs = rc.trs_of(poses_of(5))
    want = None
    for skip in (0, 2, 3, 7, 11):   # the ring, its counters, the first and later gather buffers
        g = pkg.SequenceGroup(5, pkg.Params.default())
        g.setReconstruction(recon_params(pkg), 8)
        push(g, frames, 0, 5, dims)
        g.matchFeatures(FLOW)
        if want is None:
            want = so.whole(oracle.svd, CAL, rows_of(g, 1, 5), Trs, **LOOSE)
            assert len(want) > 20
        g.debugFailAllocAfter(skip)
        expect(pkg, pkg.VH_ERR_HIP, lambda: g.reconstruct(row_trs(Trs, 0, 5)))
        same(g.reconstruct(row_trs(Trs, 0, 5)), want, skip)
        g.close()


@pytest.mark.gpu
def test_child_checking_build(pkg, gpu):
    """The GPU cases of this file once more on libviso_hip_check.so (-DVH_CHECK): every position the new kernels follow is
    verified on the device."""
    assert os.path.exists(pkg.CHECK_LIB_PATH), "build() makes it"
    env = dict(os.environ, VISO_HIP_LIB=pkg.CHECK_LIB_PATH)
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-q", "-x", "-m", "gpu", "-k", "not child"],
                       env=env, capture_output=True, text=True, timeout=900, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert " passed" in r.stdout and " skipped" not in r.stdout, r.stdout[-2000:]
    assert "VH_CHECK" not in r.stderr


@pytest.mark.gpu
def test_child_failure_and_reset_paths_on_poisoned_buffers(gpu):
    """VH_POISON=1: every buffer that is not zero-initialised starts as 0xA5 bytes, so a ring slot or a gather buffer read
    before it was written changes the records."""
    env = dict(os.environ, VH_POISON="1")
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-q", "-x", "-m", "gpu", "-k",
                        "failed_allocation or call_order"],
                       env=env, capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "2 passed" in r.stdout and " skipped" not in r.stdout, r.stdout[-2000:]
