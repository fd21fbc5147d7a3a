"""Reconstruction: vh_reconstruct_tracks, the Reconstruction classes (Python, C++ shim) and the
numpy restatement they are held to (tests/reconstruction_oracle.py), itself pinned to the reference's own class by
tests/golden/reconstruction_reference.npz (tools/gen_golden_reconstruction.py)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import recon_cases as rc
import reconstruction_oracle as ro
from conftest import GOLDEN, ROOT

SYMBOLS = ("vh_default_recon_params", "vh_reconstruct_tracks", "vh_reconstruct_last_kernel_ms")
ANGLE_TOL = 1e-9   # degrees: the device's acos is not glibc's


@pytest.fixture(scope="module")
def fixture():
    z = np.load(os.path.join(GOLDEN, "reconstruction_reference.npz"))
    ends = np.cumsum(z["list_counts"])
    lists = [z["matches"][e - n:e] for e, n in zip(ends, z["list_counts"])]
    return dict(cal=[float(v) for v in z["calibration"]], Trs=z["Trs"], lists=lists, points=z["points"], counts=z["point_counts"])


@pytest.fixture(scope="module")
def restated_drive(fixture, oracle):
    """The restatement run once over the fixture's drive -> (points after every update, the lost tracks in order)."""
    r = ro.Reconstruction(oracle.svd)
    r.setCalibration(*fixture["cal"])
    after = []
    for pm, Tr in zip(fixture["lists"], fixture["Trs"]):
        r.update(pm, Tr)
        after.append(r.getPoints())
    return after, r.lost_log


def _tables(Trs):
    tab = ro.Tables(rc.F, rc.CU, rc.CV)
    for T in Trs:
        tab.push(T)
    return tab


@pytest.fixture(scope="module")
def pool(oracle):
    """257 tracks of 2, 3, 7 and 40 frames and the restatement's answer to each (computed once, shared, left unchanged)."""
    Trs, tracks = rc.pool()
    tab = _tables(Trs)
    want = [ro.solve_track(tab, oracle.svd, f, px) for f, px in tracks]
    return Trs, tracks, want


# ------------------------------------------------------------------------------------------------------------ CPU
def test_recon_symbols_declared_exported_mirrored(pkg):
    header = open(os.path.join(ROOT, "include", "viso_hip.h")).read()
    lib = C.CDLL(pkg.LIB_PATH)
    for name in SYMBOLS:
        assert name + "(" in header, name
        assert hasattr(lib, name), name
        assert name in pkg.ABI_SYMBOLS, name
    for i, name in enumerate(("ACCEPTED", "SHORT", "INFINITY", "TYPE", "NOT_REFINED", "FAR_OR_NARROW")):
        assert f"#define VH_RECON_{name} {i}" in header and getattr(pkg, "RECON_" + name) == i == getattr(ro, name)
    for meth in ("setCalibration", "update", "updateMany", "getPoints"):
        assert hasattr(pkg.Reconstruction, meth), meth
    assert callable(pkg.reconstruct_tracks)
    shim = open(os.path.join(ROOT, "include", "viso_hip_reconstruction.hpp")).read()
    for meth in ("setCalibration", "update", "updateMany", "getPoints", "point3d"):
        assert meth in shim, meth


def test_recon_params_layout_and_defaults(pkg, tmp_path):
    want = {"f": 0, "cu": 8, "cv": 16, "point_type": 24, "min_track_length": 28, "max_dist": 32, "min_angle": 40}
    assert C.sizeof(pkg.ReconParams) == 48 and {n: getattr(pkg.ReconParams, n).offset for n, _ in pkg.ReconParams._fields_} == want
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include "viso_hip.h"\n_Static_assert(sizeof(vh_recon_params) == 48, "size");\n'
                   + "".join(f"_Static_assert(offsetof(vh_recon_params, {k}) == {v}, \"{k}\");\n" for k, v in want.items())
                   + "int main(void) { return 0; }\n")
    r = subprocess.run(["gcc", "-std=c11", "-I", os.path.join(ROOT, "include"), "-c", str(src), "-o", str(tmp_path / "layout.o")],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    p = pkg.ReconParams(f=9, cu=9, cv=9, point_type=9, min_track_length=9, max_dist=9, min_angle=9)
    pkg._lib().vh_default_recon_params(C.byref(p))
    d = pkg.ReconParams.default()
    assert bytes(p) == bytes(d) and (d.f, d.cu, d.cv, d.point_type, d.min_track_length, d.max_dist, d.min_angle) == (1, 0, 0, 1, 2, 30, 2)


def test_recon_argument_errors(pkg):
    """Every rule of the header's error list; none of these calls reaches a device."""
    lib = pkg._lib()
    r = pkg.ReconParams.default()
    Tr = np.tile(np.eye(4).reshape(16), (3, 1))
    first = np.array([0, 1], np.int32); off = np.array([0, 2, 4], np.int32); px = np.zeros((4, 2), np.float32)
    pts = np.zeros((2, 3), np.float32); st = np.zeros(2, np.int32)
    P = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731

    def call(r_=C.byref(r), nf=4, tr=P(Tr), n=2, f=P(first), o=P(off), x=P(px), p=P(pts), s=P(st)):
        return lib.vh_reconstruct_tracks(r_, 0, nf, tr, n, f, o, x, p, s, None)
    bad = pkg.VH_ERR_INVALID_ARG
    assert call(r_=None) == bad and call(tr=None) == bad and call(f=None) == bad and call(o=None) == bad
    assert call(x=None) == bad and call(p=None) == bad and call(s=None) == bad
    assert call(nf=0) == bad and call(n=-1) == bad
    assert call(o=P(np.array([0, 0, 2], np.int32))) == bad       # a track without a frame
    assert call(o=P(np.array([0, 3, 2], np.int32))) == bad       # offsets running backwards
    assert call(o=P(np.array([-1, 2, 4], np.int32))) == bad
    assert call(f=P(np.array([-1, 0], np.int32))) == bad
    assert call(f=P(np.array([0, 3], np.int32))) == bad          # frames 3, 4 of a drive of 4
    assert call(nf=2) == bad                                     # track 1 ends in frame 2
    assert call(n=0) == pkg.VH_OK and call(n=0, f=None, o=None, x=None, p=None, s=None) == pkg.VH_OK   # no launch, no device
    assert call(nf=1, tr=None, n=0) == pkg.VH_OK
    with pytest.raises(ValueError):
        pkg.reconstruct_tracks(r, Tr[:1], first, off, px, n_frames=4)          # three Trs needed
    with pytest.raises(ValueError):
        pkg.reconstruct_tracks(r, Tr, first, off[:2], px)
    with pytest.raises(ValueError):
        pkg.reconstruct_tracks(r, Tr, first, off, px[:3])
    if pkg.device_count() < 1:
        assert call() == pkg.VH_ERR_NO_DEVICE
        assert lib.vh_reconstruct_last_kernel_ms() == -1.0


def test_restatement_reproduces_reference_fixture(fixture, restated_drive):
    """The numpy restatement of the whole class against what the reference's own Reconstruction returned after every
    update of the recorded drive: bit for bit."""
    after, lost = restated_drive
    assert fixture["counts"][-1] >= 40 and len(fixture["lists"]) == 12
    for k, got in enumerate(after):
        assert got.tobytes() == fixture["points"][:fixture["counts"][k]].tobytes(), k
    lengths = {len(px) for _, px in lost}
    assert {2, 3, 7} <= lengths and len(lost) > 250


def test_fixture_holds_the_association_quirks(fixture):
    """Some lists repeat an i1p, some an i1c, and one update is a gap."""
    rep_p = sum(len(np.unique(pm["i1p"])) < len(pm) for pm in fixture["lists"])
    rep_c = sum(len(np.unique(pm["i1c"])) < len(pm) for pm in fixture["lists"])
    assert rep_p >= 5 and rep_c >= 5 and min(len(pm) for pm in fixture["lists"]) <= 5


def _python_lost(pkg, fixture):
    r = pkg.Reconstruction()
    r.setCalibration(*fixture["cal"])
    return [r.associate(pm, k + 1) for k, pm in enumerate(fixture["lists"])]


def test_python_association_equals_restatement(pkg, fixture, restated_drive):
    got = [t for lost in _python_lost(pkg, fixture) for t in lost]
    want = restated_drive[1]
    assert len(got) == len(want)
    for (f, px), (wf, wpx) in zip(got, want):
        assert f == wf and np.array(px, np.float32).tobytes() == np.array(wpx, np.float32).tobytes()


@pytest.mark.parametrize("k", [1, 5, 12])
def test_shim_header_compiles_and_associates(k, pkg, fixture, tmp_path):
    """include/viso_hip_reconstruction.hpp as C++11 with the numeric entry stubbed (tests/cpp/shim_reconstruction.cpp): the
    tracks it hands over, call by call, are the Python class's; the accepted points arrive in track order; updateMany
    makes one call per k updates."""
    exe = str(tmp_path / "shim_reconstruction")
    subprocess.check_call(["g++", "-std=gnu++11", "-O1", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "shim_reconstruction.cpp"), "-o", exe])
    with open(tmp_path / "drive.bin", "wb") as fh:
        fh.write(np.int32(len(fixture["lists"])).tobytes() + np.array(fixture["cal"], np.float64).tobytes())
        for pm, Tr in zip(fixture["lists"], fixture["Trs"]):
            fh.write(np.ascontiguousarray(Tr, np.float64).tobytes() + np.int32(len(pm)).tobytes() + pm.tobytes())
    subprocess.check_call([exe, str(tmp_path / "drive.bin"), str(tmp_path / "out.bin"), str(k)], timeout=60)
    raw = open(tmp_path / "out.bin", "rb").read()
    lost = _python_lost(pkg, fixture)
    groups = [sum(lost[i:i + k], []) for i in range(0, len(lost), k)]
    frames = [min(i + k, len(lost)) + 1 for i in range(0, len(lost), k)]
    pos, want_points = 0, []
    for g, nf in zip(groups, frames):
        if not g:
            continue   # (no lost track: no call)
        got_nf, n = np.frombuffer(raw, np.int32, 2, pos); pos += 8
        assert (got_nf, n) == (nf, len(g))
        first, off, px = rc.flatten([(f, np.array(p, np.float32)) for f, p in g])
        assert np.frombuffer(raw, np.int32, n, pos).tobytes() == first.tobytes(); pos += 4 * n
        assert np.frombuffer(raw, np.int32, n + 1, pos).tobytes() == off.tobytes(); pos += 4 * (n + 1)
        assert np.frombuffer(raw, np.float32, 2 * off[-1], pos).tobytes() == px.tobytes(); pos += 8 * int(off[-1])
        want_points += [(first[t], px[off[t], 0], px[off[t + 1] - 1, 1]) for t in range(0, n, 2)]   # the stub accepts every second track
    end, npts = np.frombuffer(raw, np.int32, 2, pos); pos += 8
    assert end == -1 and npts == len(want_points)
    assert np.frombuffer(raw, np.float32, 3 * npts, pos).tobytes() == np.array(want_points, np.float32).tobytes()


def test_status_cases_cover_every_outcome(oracle):
    """The constructed drive does what its names say, by the restatement alone (the GPU test compares against it)."""
    tab, tracks = _status_drive(oracle)
    info = {}
    got = {name: ro.solve_track(tab, oracle.svd, f, px, 1, info=info if name == "not_converged" else None)[1] for name, (f, px) in tracks.items()}
    assert got == dict(zero_motion=ro.TYPE, infinity=ro.INFINITY, behind=ro.TYPE, below_road=ro.TYPE, road=ro.ACCEPTED, obstacle=ro.ACCEPTED,
                       c_zero=ro.NOT_REFINED, not_converged=ro.NOT_REFINED, far=ro.FAR_OR_NARROW, narrow=ro.FAR_OR_NARROW, short=ro.SHORT)
    assert info["updates"] == 22                                  # still moving after the 22nd update
    f, px = tracks["c_zero"]
    p0, P = ro.init_point(tab, oracle.svd, f, f + 2, px), tab.P_total[f + 1]
    c = P[2][0] * p0[0] + P[2][1] * p0[1] + P[2][2] * p0[2] + P[2][3]
    assert c * c < 1e-10 and ro.update_point(tab, f, px, list(p0)) == ro.FAILED
    _, _, d, a = ro.solve_track(tab, oracle.svd, *tracks["far"])
    assert d >= 30 and ro.solve_track(tab, oracle.svd, *tracks["narrow"])[3] <= 2 < 30
    types = [[ro.point_type(tab, f, f + len(px) - 1, ro.init_point(tab, oracle.svd, f, f + len(px) - 1, px)) for f, px in (tracks[n],)][0]
             for n in ("behind", "below_road", "road", "obstacle")]
    assert types == [-1, 0, 1, 2]


def _status_drive(oracle, with_trs=False):
    theta = rc.c_zero_theta(rc.C_ZERO_POINT)
    for _ in range(2):   # the turn of frame 11 from the point as initPoint computes it
        poses = rc.status_poses(theta)
        Trs = rc.trs_of(poses)
        tab, tracks = _tables(Trs), rc.status_tracks(poses)
        f, px = tracks["c_zero"]
        theta = rc.c_zero_theta(ro.init_point(tab, oracle.svd, f, f + 2, px))
    return (tab, tracks, Trs) if with_trs else (tab, tracks)


# ------------------------------------------------------------------------------------------------------------ GPU
def _compare(got, want, min_angle=2.0):
    """points bit for bit, status equal, distance bit for bit, angle to ANGLE_TOL; a track may skip the status comparison
    only if the restatement's angle is within ANGLE_TOL of min_angle -- and the inputs are chosen so that none is."""
    pts, st, met = got
    skipped = 0
    for t, (wp, ws, wd, wa) in enumerate(want):
        near = ws in (ro.ACCEPTED, ro.FAR_OR_NARROW) and abs(wa - min_angle) <= ANGLE_TOL
        skipped += near
        if not near:
            assert st[t] == ws, (t, st[t], ws)
        assert pts[t].tobytes() == wp.tobytes(), (t, pts[t], wp)
        assert np.float64(met[t, 0]).tobytes() == np.float64(wd).tobytes(), (t, met[t, 0], wd)
        assert abs(met[t, 1] - wa) <= ANGLE_TOL or (np.isnan(met[t, 1]) and np.isnan(wa)), (t, met[t, 1], wa)
    assert skipped == 0 and skipped <= 0.01 * len(want)


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 63, 64, 65, 257])
def test_gpu_kernel_matches_restatement(n, pkg, pool, gpu):
    """vh_reconstruct_tracks on the first n tracks of the pool -- lengths 2, 3, 7 and 40 mixed, tracks from frame 0 and up
    to the last frame, part of a wave, one wave, more than one block -- against the restatement, in input order."""
    Trs, tracks, want = pool
    if n >= 4:
        assert {len(px) for _, px in tracks[:n]} == {2, 3, 7, 40}
        assert any(f == 0 for f, _ in tracks[:n]) and any(f + len(px) == rc.POOL_FRAMES for f, px in tracks[:n])
    first, off, px = rc.flatten(tracks[:n])
    r = pkg.ReconParams.default(f=rc.F, cu=rc.CU, cv=rc.CV)
    _compare(pkg.reconstruct_tracks(r, Trs, first, off, px), want[:n])
    assert pkg.reconstruct_last_kernel_ms() > 0
    if n == 257:
        assert {w[1] for w in want} >= {ro.ACCEPTED, ro.TYPE, ro.FAR_OR_NARROW}
        pts, st, met = pkg.reconstruct_tracks(r, Trs, first, off, px, metrics=False)   # without the optional buffer
        assert met is None and st.tolist() == [w[1] for w in want]


@pytest.mark.gpu
def test_gpu_singular_tr_tables(pkg, oracle, gpu):
    """A singular Tr is not an error: Matrix::inv hands out what its elimination left (src/matrix.cpp:378-387) and every
    later frame's tables are built on it.  Tr 20 with a zero last row (the elimination stops at the fourth pivot) and Tr 33
    with a zero second row (it stops earlier, in the rotation): tracks through the frames behind them are held to the
    restatement's tables like any other."""
    Trs, tracks = rc.pool()
    Trs, tracks = Trs.copy(), tracks[:129]
    Trs[20][3] = 0.0
    Trs[33][1] = 0.0
    tab = _tables(Trs)
    assert np.isfinite(np.array(tab.P_total)).all() and sum(f + len(px) > 34 for f, px in tracks) > 30
    want = [ro.solve_track(tab, oracle.svd, f, px) for f, px in tracks]
    first, off, px = rc.flatten(tracks)
    _compare(pkg.reconstruct_tracks(pkg.ReconParams.default(f=rc.F, cu=rc.CU, cv=rc.CV), Trs, first, off, px), want)


@pytest.mark.gpu
def test_gpu_negative_min_track_length(pkg, pool, gpu):
    """The reference compares pixels.size() >= min_track_length unsigned (src/reconstruction.cpp:131): negative = every track short."""
    Trs, tracks, _ = pool
    first, off, px = rc.flatten(tracks[:8])
    pts, st, met = pkg.reconstruct_tracks(pkg.ReconParams.default(f=rc.F, cu=rc.CU, cv=rc.CV, min_track_length=-1), Trs, first, off, px)
    assert st.tolist() == [ro.SHORT] * 8 and not pts.any() and not met.any()
    assert ro.solve_track(_tables(Trs[:2]), None, 0, tracks[0][1][:2], min_track_length=-1)[1] == ro.SHORT


@pytest.mark.gpu
@pytest.mark.parametrize("point_type", [0, 1, 2])
def test_gpu_every_status_value(point_type, pkg, oracle, gpu):
    """One constructed track per outcome (tests/recon_cases.py: status_tracks), under each point_type."""
    tab, tracks, Trs = _status_drive(oracle, with_trs=True)
    names = list(tracks)
    want = [ro.solve_track(tab, oracle.svd, *tracks[nm], point_type) for nm in names]
    assert {w[1] for w in want} == set(range(6))
    first, off, px = rc.flatten([tracks[nm] for nm in names])
    r = pkg.ReconParams.default(f=rc.F, cu=rc.CU, cv=rc.CV, point_type=point_type)
    _compare(pkg.reconstruct_tracks(r, Trs, first, off, px), want)


@pytest.mark.gpu
def test_gpu_update_reproduces_reference_drive(pkg, fixture, gpu):
    """pkg.Reconstruction.update over the recorded drive: the points after every update are the reference's, bit for bit."""
    r = pkg.Reconstruction()
    r.setCalibration(*fixture["cal"])
    for k, (pm, Tr) in enumerate(zip(fixture["lists"], fixture["Trs"])):
        r.update(pm, Tr)
        assert r.getPoints().tobytes() == fixture["points"][:fixture["counts"][k]].tobytes(), k


@pytest.mark.gpu
@pytest.mark.parametrize("k", [1, 5, 12])
def test_gpu_update_many_equals_single_updates(k, pkg, fixture, gpu):
    r = pkg.Reconstruction()
    r.setCalibration(*fixture["cal"])
    for i in range(0, 12, k):
        r.updateMany(fixture["lists"][i:i + k], fixture["Trs"][i:i + k])
        done = min(i + k, 12)
        assert r.getPoints().tobytes() == fixture["points"][:fixture["counts"][done - 1]].tobytes(), done


@pytest.mark.gpu
def test_gpu_sequence_matches_to_points_end_to_end(pkg, oracle, gpu):
    """The smallest real chain: a SequenceGroup over 6 synthetic frames (flow), its getMatchesAll fed to updateMany with
    constructed Trs; the points are those of the restatement fed the same lists."""
    Wd, Hd, n = 320, 160, 6
    bpl = pkg.synth.bytes_per_line(Wd)
    frames = np.stack([pkg.synth.frame(Wd, Hd, 3 * k, k, 4, 1, 11) for k in range(n)])
    g = pkg.SequenceGroup(n, pkg.Params.default())
    try:
        g.pushBack(frames, None, [Wd, Hd, bpl])
        g.matchFeatures(pkg.METHOD_FLOW)
        rec, counts = g.getMatchesAll()
        lists = [rec[s, :counts[s]].copy() for s in range(1, n)]   # row 0 of a first chunk is empty: 5 pairs
    finally:
        g.close()
    assert len(lists) == 5 and min(len(m) for m in lists) > 50
    poses = [rc.pose(0.0, -0.004 * k, 0.0, (0.03 * k, 0.0, 0.5 * k)) for k in range(n)]
    Trs = rc.trs_of(poses)
    cal = (300.0, 160.0, 80.0)
    r = pkg.Reconstruction()
    r.setCalibration(*cal)
    r.updateMany(lists, Trs, point_type=0, max_dist=1e6, min_angle=0.0)
    want = ro.Reconstruction(oracle.svd)
    want.setCalibration(*cal)
    for pm, Tr in zip(lists, Trs):
        want.update(pm, Tr, 0, 2, 1e6, 0.0)
    assert len(want.lost_log) > 50
    assert r.getPoints().tobytes() == want.getPoints().tobytes()
