"""Multi-stage matching on sequence handles (vh_sequence_set_multi_stage; DESIGN.md section 6, "Sequence contract").

Row r of a chunk pushed at position F holds the pair F + r - 1 -> F + r: its list, count and sparse list must equal,
byte for byte, those of a lone matcher with vh_set_multi_stage_matching on that was pushed the two frames, and
tests/multistage_oracle.py's answer for the pair directly -- modes 1 (host vote) and 2 (device vote), flow, stereo and
quad, across a chunk boundary, with unused rows, and through every reader of the list."""
import ctypes as C

import numpy as np
import pytest

import multistage_oracle as mo
import track_oracle as to
from test_multistage import scene, images_of, lone_lists, check_not_vacuous
from test_multistage_device import kitti_frames, group_run, KW, KH

W, H = 320, 160
T, N = 4, 7  # max_frames and frames: a chunk of 4 and a chunk of 3
SEED = 5
METHODS = (1, 0, 2)

_cache = {}


def dims_of(pkg, w=W):
    return [w, H if w == W else 169, pkg.synth.bytes_per_line(w)]


def frames(pkg):
    if "fr" not in _cache:
        _cache["fr"] = scene(pkg, N, seed=SEED)
    return _cache["fr"]


def lone(pkg, key, p, fr, dims, methods=(0, 1, 2), on=True):
    """The lone matcher's lists (t, method) and sparse lists (t, method, "sparse"), computed once per configuration."""
    if key not in _cache:
        _cache[key] = lone_lists(pkg, p, fr, dims, methods, on)
    return _cache[key]


def oracle_answers(pkg, ob, oracle):
    if "oracle" not in _cache:
        fr, dims, po = frames(pkg), dims_of(pkg), ob.Params.default(multi_stage=1)
        _cache["oracle"] = {(t, m): mo.multistage(ob, oracle, po, dims, m, images_of(m, fr[t - 1], fr[t])) for t in range(1, N) for m in (0, 1, 2)}
    return _cache["oracle"]


def push(g, fr, F, n, dims):
    g.pushBack(np.stack([fr[t][0] for t in range(F, F + n)]), np.stack([fr[t][1] for t in range(F, F + n)]), dims)


def sequence(pkg, p, mode, max_frames=T):
    g = pkg.SequenceGroup(max_frames, p)
    g.setMultiStage(mode)
    return g


# ------------------------------------------------------------------ CPU: the scenes show something
def test_the_scenes_are_not_vacuous(pkg, ob, oracle):
    """For every method at least one row has a range table different from +-R and at least one row's pass-2 list differs
    from the single-stage list of the same pair (here: every row does)."""
    ans = oracle_answers(pkg, ob, oracle)
    po, dims = ob.Params.default(multi_stage=1), dims_of(pkg)
    R = po.match_radius
    for m in (0, 1, 2):
        narrow = differs = 0
        for t in range(1, N):
            r = ans[(t, m)]
            check_not_vacuous(po, m, r)
            rg = r["ranges"][:, :len(mo.STAGES[m])]
            narrow += bool(((rg[:, :, 0::2] != -R) | (rg[:, :, 1::2] != R)).any())
            differs += oracle.matching(po, dims, m, *r["dense_sets"]).tobytes() != r["dense"].tobytes()
        assert narrow > 0 and differs > 0, (m, narrow, differs)


# ------------------------------------------------------------------ GPU
@pytest.mark.gpu
@pytest.mark.parametrize("mode", (1, 2))
def test_rows_equal_lone_matchers_and_the_oracle(pkg, ob, oracle, gpu, mode):
    fr, dims = frames(pkg), dims_of(pkg)
    p = pkg.Params.default(multi_stage=1)
    want = lone(pkg, "lone", p, fr, dims)
    ans = oracle_answers(pkg, ob, oracle)
    for (t, m), r in ans.items():
        assert want[(t, m)].tobytes() == r["dense"].tobytes() and want[(t, m, "sparse")].tobytes() == r["sparse"].tobytes(), (t, m)
    g = sequence(pkg, p, mode)
    assert len(g.getSparseMatches(0)) == 0
    for F, n in ((0, 4), (4, 3)):
        push(g, fr, F, n, dims)
        for m in METHODS:
            g.matchFeatures(m)
            _, nm = g.getCounts()
            out, cnt = g.getMatchesAll()
            for r in range(T):
                t = F + r
                got, sp = g.getMatches(r), g.getSparseMatches(r)
                if r < n and t >= 1:
                    assert got.tobytes() == ans[(t, m)]["dense"].tobytes(), (mode, t, m, len(got))
                    assert sp.tobytes() == ans[(t, m)]["sparse"].tobytes(), (mode, t, m, len(sp))
                else:  # no pair: empty sparse list, empty list
                    assert len(got) == 0 and len(sp) == 0, (mode, F, r, m)
                assert nm[r] == len(got) and cnt[r] == len(got) and out[r, :cnt[r]].tobytes() == got.tobytes(), (mode, F, r, m)
    # the last call was quad on the chunk (4, 3): the asynchronous download and the host vote read the pass-2 lists
    pout = pkg.pinned_empty((T, 4096), pkg.P_MATCH_DTYPE)
    pcnt = pkg.pinned_empty((T,), np.int32)
    g.downloadMatchesAsync(pout, pcnt)
    g.waitDownload()
    for r in range(3):
        assert pout[r, :pcnt[r]].tobytes() == want[(4 + r, 2)].tobytes(), r
    assert pcnt[3] == 0
    g.removeOutliers()
    for r in range(3):
        assert g.getMatches(r).tobytes() == oracle.remove_outliers(want[(4 + r, 2)])[0].tobytes(), r
    g.close()


@pytest.mark.gpu
def test_refinement_and_half_resolution(pkg, gpu):
    fr, dims = frames(pkg), dims_of(pkg)
    p = pkg.Params.default(multi_stage=1, refinement=2, half_resolution=1, nms_n=1)
    want = lone(pkg, "lone_ref", p, fr, dims)
    g = sequence(pkg, p, 2)
    for F, n in ((0, 4), (4, 3)):
        push(g, fr, F, n, dims)
        for m in METHODS:
            g.matchFeatures(m)
            for r in range(n):
                if F + r >= 1:
                    assert len(want[(F + r, m)]) > 20
                    assert g.getMatches(r).tobytes() == want[(F + r, m)].tobytes(), (F, r, m)
                    assert g.getSparseMatches(r).tobytes() == want[(F + r, m, "sparse")].tobytes(), (F, r, m)
    g.close()


@pytest.mark.gpu
def test_every_pair_crosses_a_chunk_boundary(pkg, gpu):
    """max_frames = 1 at the odd size: row 0 always links to the previous chunk, in both passes."""
    w = 357
    dims = dims_of(pkg, w)
    fr = scene(pkg, 4, w, dims[1], seed=SEED)
    p = pkg.Params.default(multi_stage=1)
    want = lone(pkg, "lone_odd", p, fr, dims)
    for mode in (1, 2):
        g = sequence(pkg, p, mode, 1)
        for t in range(4):
            push(g, fr, t, 1, dims)
            for m in METHODS:
                g.matchFeatures(m)
                if t == 0:
                    assert len(g.getMatches(0)) == 0 and len(g.getSparseMatches(0)) == 0
                    continue
                assert len(want[(t, m)]) > 20
                assert g.getMatches(0).tobytes() == want[(t, m)].tobytes(), (mode, t, m)
                assert g.getSparseMatches(0).tobytes() == want[(t, m, "sparse")].tobytes(), (mode, t, m)
        g.close()


@pytest.mark.gpu
def test_device_post_chain_on_the_handle(pkg, ob, gpu):
    """Mode 2, quad: vote, bucketing and the estimator over the rows equal the same chain over the lone matchers' lists."""
    fr, dims = frames(pkg), dims_of(pkg)
    p = pkg.Params.default(multi_stage=1)
    want = lone(pkg, "lone", p, fr, dims)
    g = sequence(pkg, p, 2)
    g.postDeviceConfig(1, 2, 16)
    ego = pkg.EgoParams.default(f=300.0, cu=W / 2.0, cv=H / 2.0, base=0.5, ransac_iters=50)
    rand3 = np.tile(ob.glibc_rand_after_srand0(50 * 3).reshape(1, 50, 3), (T, 1, 1))
    for F, n in ((0, 4), (4, 3)):
        push(g, fr, F, n, dims)
        g.matchFeatures(2)
        g.postBeginDevice(4096, 2, 50.0, 50.0, ego=ego, rand3=rand3, want_lists=True)
        res = g.postFinishDevice(0, want_lists=True)
        rows = [r for r in range(n) if F + r >= 1]
        lists, _, _ = pkg.remove_outliers_device([want[(F + r, 2)] for r in rows], max_features=2, bucket_width=50.0, bucket_height=50.0)
        tr, ok, inl = pkg.estimate_motion_stereo(ego, lists, rand3[:len(rows)])
        for k, r in enumerate(rows):
            assert len(lists[k]) > 5 and res["lists"][r].tobytes() == lists[k].tobytes(), (F, r)
            assert res["counts"][r] == len(lists[k]) and bool(res["ok"][r]) == bool(ok[k]) and res["n_inliers"][r] == len(inl[k]), (F, r)
            assert np.allclose(res["tr"][r], tr[k], rtol=1e-9, atol=1e-12), (F, r)
        for r in range(T):
            if r not in rows:
                assert res["counts"][r] == 0 and not res["ok"][r], (F, r)
    g.close()


@pytest.mark.gpu
@pytest.mark.parametrize("mode", (1, 2))
def test_tracks_across_the_boundary(pkg, gpu, mode):
    fr, dims = frames(pkg), dims_of(pkg)
    p = pkg.Params.default(multi_stage=1)
    want = lone(pkg, "lone", p, fr, dims)
    cam = to.Camera()
    trk = {}
    for t in range(N):
        cam.push()
        if t:
            trk[t] = cam.match(want[(t, 2)])
    assert (trk[4]["age"] >= 4).any() and (trk[N - 1]["age"] >= N - 1).any()  # ids that survive the boundary
    g = sequence(pkg, p, mode)
    g.setTrackLinking(True)
    for F, n in ((0, 4), (4, 3)):
        push(g, fr, F, n, dims)
        g.matchFeatures(2)
        for r in range(n):
            if F + r >= 1:
                assert g.getMatches(r).tobytes() == want[(F + r, 2)].tobytes(), (F, r)
                assert g.getTracks(r).tobytes() == trk[F + r].tobytes(), (mode, F, r)
    g.close()


@pytest.mark.gpu
def test_an_unmatched_chunk_still_gives_the_predecessor(pkg, gpu):
    """A chunk that is pushed and never matched: row 0 of the next chunk links to its last row, in the sparse pass as in
    the dense one."""
    fr, dims = frames(pkg), dims_of(pkg)
    p = pkg.Params.default(multi_stage=1)
    want = lone(pkg, "lone", p, fr, dims)
    for mode in (1, 2):
        g = sequence(pkg, p, mode)
        push(g, fr, 0, 2, dims)
        g.matchFeatures(0)
        push(g, fr, 2, 3, dims)  # never matched
        push(g, fr, 5, 2, dims)
        for m in (2, 0):
            g.matchFeatures(m)
            for r in range(2):
                assert g.getMatches(r).tobytes() == want[(5 + r, m)].tobytes(), (mode, r, m)
                assert g.getSparseMatches(r).tobytes() == want[(5 + r, m, "sparse")].tobytes(), (mode, r, m)
        g.close()


@pytest.mark.gpu
def test_a_list_the_vote_refuses_gets_the_full_window(pkg, gpu):
    """Mode 2 with the vote's stack cut to one slot (full-size frames, as the group's test): a refused row equals
    single-stage matching and reports the refusal's code; the other rows are voted as ever."""
    lib = pkg._lib()
    S = 4
    dims = [KW, KH, pkg.synth.bytes_per_line(KW)]
    fr = kitti_frames(pkg, S + 1)
    p = pkg.Params.default(multi_stage=1)
    off = group_run(pkg, p, fr, dims, S, "off", steps=2, methods=(0, 2))
    host = group_run(pkg, p, fr, dims, S, "host", steps=2, methods=(0, 2))
    refused = voted = 0
    assert lib.vh_debug_vote_stack_slots(1) == pkg.VH_OK
    try:
        g = sequence(pkg, p, 2, S + 1)
        push(g, fr, 0, S + 1, dims)  # row r = the pair of stream r - 1 of the group runs
        for m in (0, 2):
            g.matchFeatures(m)
            for r in range(1, S + 1):
                n = C.c_int32(-1)
                buf = np.zeros(1 << 15, pkg.P_MATCH_DTYPE)
                rc = lib.vh_group_get_sparse_matches(g._h, r, buf.ctypes.data_as(C.c_void_p), len(buf), C.byref(n))
                dense = g.getMatches(r).tobytes()
                if rc == pkg.VH_OK:
                    voted += 1
                    assert buf[:n.value].tobytes() == host[(1, m, r - 1, "sparse")] and dense == host[(1, m, r - 1, "dense")], (m, r)
                    continue
                assert rc == pkg.VH_ERR_UNSUPPORTED and n.value == 0, (m, r, rc, n.value)
                refused += 1
                assert dense == off[(1, m, r - 1, "dense")], (m, r)
                assert dense != host[(1, m, r - 1, "dense")]
        g.close()
    finally:
        assert lib.vh_debug_vote_stack_slots(0) == pkg.VH_OK
    assert refused > 0, "no list was refused: the fall-back never ran"


@pytest.mark.gpu
@pytest.mark.parametrize("mode", (1, 2))
def test_allocation_failure_in_the_first_match_call(pkg, gpu, mode):
    fr, dims = frames(pkg), dims_of(pkg)
    p = pkg.Params.default(multi_stage=1)
    want = lone(pkg, "lone", p, fr, dims)
    lib = pkg._lib()
    g = sequence(pkg, p, mode)
    push(g, fr, 0, 4, dims)
    before = g.deviceBytes()
    g.debugFailNextAlloc()
    assert lib.vh_group_match_features(g._h, 2) == pkg.VH_ERR_HIP
    for m in (2, 0):
        g.matchFeatures(m)
        for r in range(1, 4):
            assert g.getMatches(r).tobytes() == want[(r, m)].tobytes(), (mode, r, m)
    assert g.deviceBytes() > before  # the range tables (mode 2: and the vote buffer of max_frames lists) are counted
    g.close()


@pytest.mark.gpu
def test_switch_at_zero_is_the_handle_as_it_was(pkg, gpu):
    """Mode 0 (never set, or set and cleared): single-stage lists, the bytes of a multi_stage = 0 handle, no sparse or
    ranged launch; the modes count their sparse sets, and mode 2 its vote buffer."""
    fr, dims = frames(pkg), dims_of(pkg)
    single = lone(pkg, "lone_single", pkg.Params.default(), fr, dims, (0, 2), on=False)
    seen = {}
    for name, ms, modes in (("plain", 0, ()), ("off", 1, ()), ("cleared", 1, (2, 0)), ("host", 1, (1,)), ("device", 1, (2,))):
        g = pkg.SequenceGroup(T, pkg.Params.default(multi_stage=ms))
        for mode in modes:
            g.setMultiStage(mode)
        g.profileEnable(True)
        push(g, fr, 0, 4, dims)
        for m in (0, 2):
            g.matchFeatures(m)
            if name in ("plain", "off", "cleared"):
                for r in range(1, 4):
                    assert g.getMatches(r).tobytes() == single[(r, m)].tobytes(), (name, r, m)
        launches = tuple(g.profileRead(k)[1] for k in ("ranged", "sparse_detect_nms", "sparse_match", "match"))
        seen[name] = (g.deviceBytes(), launches)
        if name in ("plain", "off", "cleared"):
            with pytest.raises(pkg.VisoHipError) as e:
                g.getSparseMatches(0)
            assert e.value.code == pkg.VH_ERR_STATE
        g.close()
    assert seen["plain"] == seen["off"] == seen["cleared"]
    assert seen["off"][1] == (0, 0, 0, 2)
    for name in ("host", "device"):
        assert seen[name][1][0] == 2 and seen[name][1][1] > 0 and seen[name][1][2] == 2 and seen[name][1][3] == 0, seen[name]
    assert seen["device"][0] > seen["host"][0] > seen["off"][0]
