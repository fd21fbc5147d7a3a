"""Sequence handles (vh_sequence_*): consecutive frames of ONE camera in the rows of a group.

After a chunk of n frames, pushed when F frames of the sequence came before it, row r < n holds the pair
frame F+r-1 -> frame F+r: its match list and its four feature sets must be byte-equal to those of a lone Matcher
that pushed the same frames one by one.  Row 0 of a sequence's first chunk and the rows >= n of a short chunk are empty.
Integer/byte work: the bar is exact equality everywhere."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

HERE = os.path.dirname(os.path.abspath(__file__))
SYMBOLS = ("vh_sequence_create", "vh_sequence_push_back_device", "vh_sequence_push_back", "vh_sequence_position")
W, H = 320, 160
METHODS = (0, 1, 2)  # flow, stereo, quad


# ------------------------------------------------------------------ CPU
def test_sequence_symbols_declared_exported_mirrored(pkg):
    header = open(os.path.join(ROOT, "include", "viso_hip.h")).read()
    lib = C.CDLL(pkg.LIB_PATH)
    for name in SYMBOLS:
        assert name + "(" in header, name
        assert hasattr(lib, name), name
        assert name in pkg.ABI_SYMBOLS, name
    assert issubclass(pkg.SequenceGroup, pkg.StreamGroup)
    for meth in ("pushBack", "pushBackDevice", "position"):
        assert meth in pkg.SequenceGroup.__dict__, meth


def test_sequence_null_handles_and_pointers_need_no_gpu(pkg):
    lib = pkg._lib()
    p = pkg.Params.default()
    h = C.c_void_p()
    dims = (C.c_int32 * 3)(W, H, pkg.synth.bytes_per_line(W))
    img = np.zeros((H, pkg.synth.bytes_per_line(W)), np.uint8)
    assert lib.vh_sequence_create(None, 0, 8, 0, 0, C.byref(h)) == pkg.VH_ERR_INVALID_ARG
    assert lib.vh_sequence_create(C.byref(p), 0, 8, 0, 0, None) == pkg.VH_ERR_INVALID_ARG
    assert lib.vh_sequence_create(C.byref(p), 0, 0, 0, 0, C.byref(h)) == pkg.VH_ERR_INVALID_ARG
    assert lib.vh_sequence_create(C.byref(pkg.Params.default(nms_n=0)), 0, 8, 0, 0, C.byref(h)) == pkg.VH_ERR_UNSUPPORTED
    assert lib.vh_sequence_push_back(None, img.ctypes.data_as(C.c_void_p), None, img.size, dims, 1) == pkg.VH_ERR_INVALID_ARG
    assert lib.vh_sequence_push_back_device(None, C.c_void_p(4096), None, img.size, dims, 1) == pkg.VH_ERR_INVALID_ARG
    first, n = C.c_int64(-1), C.c_int32(-1)
    assert lib.vh_sequence_position(None, C.byref(first), C.byref(n)) == pkg.VH_ERR_INVALID_ARG


# ------------------------------------------------------------------ GPU
def frames_of(pkg, T, seed, w=W, h=H, disparity=6, blur=3):
    return pkg.synth.stereo_sequence(w, h, T, disparity=disparity, blur=blur, seed=seed)


def lone_run(pkg, p, frames, dims, methods, tr=None, intrinsics=None, stereo=True):
    """A lone Matcher pushed frame by frame -> (matches {(t, method): records}, features {t: [1p, 2p, 1c, 2c]})."""
    m = pkg.Matcher(p, outlier_removal=False)
    if intrinsics is not None:
        m.setIntrinsics(*intrinsics)
    out, feats = {}, {}
    for t, (l, r) in enumerate(frames):
        m.pushBack(l, r if stereo else None, dims)
        if t == 0:
            continue
        feats[t] = [m.getFeatures(k) for k in range(4)]
        for meth in methods:
            m.matchFeatures(meth, None if tr is None else tr[t])
            out[(t, meth)] = m.getMatches()
    m.close()
    return out, feats


def push_chunk(g, frames, t0, n, dims, stereo=True):
    g.pushBack(np.stack([frames[t][0] for t in range(t0, t0 + n)]),
               np.stack([frames[t][1] for t in range(t0, t0 + n)]) if stereo else None, dims)
    assert g.position() == (t0, n)


def check_rows(g, F, n, meth, lone, feats, min_matches=20):
    """Every row of the handle after matching the chunk [F, F + n) with `meth`."""
    nf, nm = g.getCounts()
    for r in range(g.S):
        t = F + r
        if r < n and t >= 1:
            want = lone[(t, meth)]
            assert len(want) >= min_matches, (t, meth, len(want))
            assert nm[r] == len(want) and g.getMatches(r).tobytes() == want.tobytes(), (F, r, meth)
            assert list(nf[r]) == [len(x) for x in feats[t]], (F, r)
            for k in range(4):
                assert np.array_equal(g.getFeatures(r, k), feats[t][k]), (F, r, k)
        else:  # no predecessor (row 0 of the first chunk) or beyond the chunk
            assert nm[r] == 0 and len(g.getMatches(r)) == 0 and not nf[r].any(), (F, r, meth, nm[r], nf[r])
            for k in range(4):
                assert len(g.getFeatures(r, k)) == 0, (F, r, k)


@pytest.mark.gpu
def test_sequence_parity_with_lone_matcher(pkg, ob, oracle, gpu):
    """max_frames = 8, 21 frames pushed as chunks of 8, 8 and 5; flow, stereo and quad on every chunk."""
    p, po = pkg.Params.default(), ob.Params.default()
    dims = [W, H, pkg.synth.bytes_per_line(W)]
    frames = frames_of(pkg, 21, 41)
    lone, feats = lone_run(pkg, p, frames, dims, METHODS)
    g = pkg.SequenceGroup(8, p)
    assert g.position() == (0, 0)
    F = 0
    for n in (8, 8, 5):
        push_chunk(g, frames, F, n, dims)
        for meth in METHODS:
            g.matchFeatures(meth)
            check_rows(g, F, n, meth, lone, feats)
        F += n
    g.close()
    # a subset against the oracle: the pair across the chunk boundaries and one inside a chunk
    for t in (8, 16, 19):
        sets = [oracle.compute_features(po, frames[tt][c], dims)[1] for tt in (t - 1, t) for c in (0, 1)]
        for k in range(4):
            assert np.array_equal(feats[t][k], sets[k]), (t, k)
        for meth in METHODS:
            assert lone[(t, meth)].tobytes() == oracle.matching(po, dims, meth, *sets).tobytes(), (t, meth)


@pytest.mark.gpu
def test_sequence_single_frame_chunks_and_mono(pkg, gpu):
    """Chunks of one frame reproduce the lone matcher, stereo and mono (no right images)."""
    p = pkg.Params.default()
    dims = [W, H, pkg.synth.bytes_per_line(W)]
    frames = frames_of(pkg, 5, 43)
    for stereo, methods in ((True, (2, 1)), (False, (0,))):
        lone, feats = lone_run(pkg, p, frames, dims, methods, stereo=stereo)
        if not stereo:
            assert all(len(f[1]) == len(f[3]) == 0 for f in feats.values())
        g = pkg.SequenceGroup(4, p)
        for t in range(5):
            push_chunk(g, frames, t, 1, dims, stereo)
            for meth in methods:
                g.matchFeatures(meth)
                check_rows(g, t, 1, meth, lone, feats)
        g.close()


@pytest.mark.gpu
def test_sequence_dims_change_restarts(pkg, gpu):
    p = pkg.Params.default()
    dims_a = [W, H, pkg.synth.bytes_per_line(W)]
    w2, h2 = 288, 144
    dims_b = [w2, h2, pkg.synth.bytes_per_line(w2)]
    fa, fb = frames_of(pkg, 4, 47), frames_of(pkg, 6, 48, w=w2, h=h2)
    lone_b, feats_b = lone_run(pkg, p, fb, dims_b, (2,))
    g = pkg.SequenceGroup(4, p)
    push_chunk(g, fa, 0, 4, dims_a)
    g.matchFeatures(2)
    push_chunk(g, fb, 0, 3, dims_b)  # new dims: a new sequence, row 0 without a predecessor
    g.matchFeatures(2)
    check_rows(g, 0, 3, 2, lone_b, feats_b)
    push_chunk(g, fb, 3, 3, dims_b)
    g.matchFeatures(2)
    check_rows(g, 3, 3, 2, lone_b, feats_b)
    g.close()


@pytest.mark.gpu
def test_sequence_mode_mismatch_and_bad_counts(pkg, gpu):
    lib = pkg._lib()
    bpl = pkg.synth.bytes_per_line(W)
    dims = (C.c_int32 * 3)(W, H, bpl)
    imgs = np.zeros((9, H, bpl), np.uint8)
    ptr, stride = imgs.ctypes.data_as(C.c_void_p), H * bpl
    g = pkg.SequenceGroup(8)
    assert lib.vh_group_push_back(g._h, ptr, None, stride, dims, 0) == pkg.VH_ERR_STATE
    assert lib.vh_group_push_back_device(g._h, C.c_void_p(4096), None, stride, dims, 0) == pkg.VH_ERR_STATE
    for n in (0, -1, 9):
        assert lib.vh_sequence_push_back(g._h, ptr, None, stride, dims, n) == pkg.VH_ERR_INVALID_ARG, n
    assert lib.vh_sequence_push_back(g._h, None, None, stride, dims, 2) == pkg.VH_ERR_INVALID_ARG
    assert lib.vh_sequence_position(g._h, None, None) == pkg.VH_ERR_INVALID_ARG
    assert g.position() == (0, 0)
    g.close()
    s = pkg.StreamGroup(3)
    assert lib.vh_sequence_push_back(s._h, ptr, None, stride, dims, 1) == pkg.VH_ERR_STATE
    assert lib.vh_sequence_push_back_device(s._h, C.c_void_p(4096), None, stride, dims, 1) == pkg.VH_ERR_STATE
    first, n = C.c_int64(0), C.c_int32(0)
    assert lib.vh_sequence_position(s._h, C.byref(first), C.byref(n)) == pkg.VH_ERR_STATE
    s.close()


def motion(t):
    """A small forward motion with a little yaw, different for every pair."""
    a = 0.002 * (t % 5)
    tr = np.eye(4)
    tr[0, 0] = tr[2, 2] = np.cos(a)
    tr[0, 2], tr[2, 0] = np.sin(a), -np.sin(a)
    tr[:3, 3] = (0.01 * (t % 3), 0.0, -0.05 * (1 + t % 4))
    return tr


@pytest.mark.gpu
def test_sequence_prior(pkg, gpu):
    """match_features_prior with a Tr_delta per row == Matcher.matchFeatures(2, Tr_delta) pair by pair."""
    intr = (300.0, W / 2.0, H / 2.0, 0.5)
    p = pkg.Params.default(f=intr[0], cu=intr[1], cv=intr[2], base=intr[3])
    dims = [W, H, pkg.synth.bytes_per_line(W)]
    frames = frames_of(pkg, 13, 51)
    tr = {t: motion(t) for t in range(13)}
    lone, feats = lone_run(pkg, p, frames, dims, (2,), tr=tr, intrinsics=intr)
    g = pkg.SequenceGroup(8, p)
    F = 0
    for n in (8, 5):
        push_chunk(g, frames, F, n, dims)
        g.matchFeaturesPrior(2, np.stack([tr[F + r] for r in range(n)]))
        check_rows(g, F, n, 2, lone, feats)
        F += n
    g.close()


def run_child(env_over, sel, timeout=900):
    env = dict(os.environ, **env_over)
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-q", "-x", "-m", "gpu", "-k", sel],
                       env=env, capture_output=True, text=True, timeout=timeout, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert " passed" in r.stdout and " skipped" not in r.stdout, r.stdout[-2000:]
    return r


@pytest.mark.gpu
def test_child_sequence_subbatch_flow_wgs(gpu):
    """The parity case with detection in sub-batches (8 rows as 3 + 3 + 2, 5 as 2 + 2 + 1) and one search workgroup per
    (pass, row)."""
    run_child({"VH_SUBBATCH": "3", "VH_FLOW_WGS": "1"}, "parity_with_lone_matcher or prior")


@pytest.mark.gpu
def test_child_sequence_checking_build(pkg, gpu):
    """The parity case on libviso_hip_check.so (-DVH_CHECK): no index violation on the sequence paths."""
    assert os.path.exists(pkg.CHECK_LIB_PATH), "build() makes it"
    r = run_child({"VISO_HIP_LIB": pkg.CHECK_LIB_PATH, "VH_SUBBATCH": "3"}, "parity_with_lone_matcher or prior or single_frame")
    assert "VH_CHECK" not in r.stderr


@pytest.mark.gpu
def test_sequence_kitti_size(pkg, ob, oracle, gpu):
    """KITTI size, max_frames = 64, two chunks, quad: every row's counts equal the lone matcher's; the records of a sample
    of rows (row 0 of chunk 2 included) equal the oracle's."""
    w, h = 1241, 376
    dims = [w, h, pkg.synth.bytes_per_line(w)]
    p, po = pkg.Params.default(), ob.Params.default()
    base = frames_of(pkg, 20, 1, w=w, h=h, disparity=12, blur=8)  # stereo_sequence's pan repeats every 20 frames
    frames = [base[t % 20] for t in range(128)]
    g = pkg.SequenceGroup(64, p)
    m = pkg.Matcher(p, outlier_removal=False)
    m.pushBack(frames[0][0], frames[0][1], dims)
    got = {}
    for F in (0, 64):
        push_chunk(g, frames, F, 64, dims)
        g.matchFeatures(2)
        nf, nm = g.getCounts()
        for r in range(64):
            t = F + r
            if t == 0:
                assert nm[0] == 0 and not nf[0].any()
                continue
            m.pushBack(frames[t][0], frames[t][1], dims)
            m.matchFeatures(2)
            want = m.getMatches()
            assert nm[r] == len(want) > 1000, (t, nm[r], len(want))
            assert all(nf[r][k] == len(m.getFeatures(k)) for k in range(4)), t
        for r in (0, 1, 63):
            if F + r:
                got[F + r] = g.getMatches(r)
    m.close()
    g.close()
    for t in (64, 1, 127):
        sets = [oracle.compute_features(po, frames[tt][c], dims)[1] for tt in (t - 1, t) for c in (0, 1)]
        assert got[t].tobytes() == oracle.matching(po, dims, 2, *sets).tobytes(), t


@pytest.mark.gpu
def test_sequence_post_chain(pkg, gpu):
    """postBeginDevice / postFinishDevice on a sequence handle after a short chunk: the rows with a pair equal
    remove_outliers_device (+ bucketing) over the lone matcher's lists; the empty rows come out as ok = 0, no error."""
    p = pkg.Params.default()
    dims = [W, H, pkg.synth.bytes_per_line(W)]
    frames = frames_of(pkg, 13, 53)
    lone, _ = lone_run(pkg, p, frames, dims, (2,))
    g = pkg.SequenceGroup(8, p)
    g.postDeviceConfig(1, 2, 16)  # one step per batch: every step is finished right after it begins
    ego = pkg.EgoParams.default(f=300.0, cu=W / 2.0, cv=H / 2.0, base=0.5, ransac_iters=50)
    rng = np.random.default_rng(5)
    F = 0
    for n in (8, 5):
        push_chunk(g, frames, F, n, dims)
        g.matchFeatures(2)
        rand3 = rng.integers(0, 2 ** 31 - 1, (8, ego.ransac_iters, 3)).astype(np.int32)
        g.postBeginDevice(4096, 2, 50.0, 50.0, ego=ego, rand3=rand3, want_lists=True)
        res = g.postFinishDevice(0, want_lists=True)
        assert res["rc"] == pkg.VH_OK
        rows = [r for r in range(n) if F + r >= 1]
        want, _, _ = pkg.remove_outliers_device([lone[(F + r, 2)] for r in rows], max_features=2, bucket_width=50.0,
                                                bucket_height=50.0)
        for r, wl in zip(rows, want):
            assert len(wl) > 5 and res["lists"][r].tobytes() == wl.tobytes(), (F, r)
            assert res["counts"][r] == len(wl)
        for r in range(8):
            if r not in rows:
                assert res["counts"][r] == 0 and not res["ok"][r] and res["n_inliers"][r] == 0, (F, r)
                assert not res["tr"][r].any()
        F += n
    g.close()
