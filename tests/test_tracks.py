"""Feature tracks (vh_set_track_linking / vh_group_get_tracks / vh_link_tracks): the match lists of consecutive frame
pairs linked on the GPU.  Everything is integers: every comparison is byte for byte against tests/track_oracle.py."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import track_oracle as to
from conftest import ROOT

SYMBOLS = ("vh_set_track_linking", "vh_group_set_track_linking", "vh_get_tracks", "vh_group_get_tracks",
           "vh_group_get_tracks_all", "vh_group_tracks_device", "vh_link_tracks", "vh_track_carry_free",
           "vh_group_debug_fail_alloc_after")
W, H = 320, 160
FLOW, STEREO, QUAD = 0, 1, 2


# ------------------------------------------------------------------ CPU
def test_track_symbols_declared_exported_mirrored(pkg):
    header = open(os.path.join(ROOT, "include", "viso_hip.h")).read()
    lib = C.CDLL(pkg.LIB_PATH)
    for name in SYMBOLS:
        assert name + "(" in header, name
        assert hasattr(lib, name), name
        assert name in pkg.ABI_SYMBOLS, name
    for cls, meths in ((pkg.Matcher, ("setTrackLinking", "getTracks")),
                       (pkg.StreamGroup, ("setTrackLinking", "getTracks", "getTracksAll", "tracksDevice"))):
        for meth in meths:
            assert hasattr(cls, meth), (cls, meth)
    assert hasattr(pkg.SequenceGroup, "getTracksAll") and callable(pkg.link_tracks)
    shim = open(os.path.join(ROOT, "include", "viso_hip_matcher.hpp")).read()
    assert "setTrackLinking" in shim and "getTracks" in shim


def test_track_record_layout(pkg, tmp_path):
    """sizeof(vh_track) == 24 and the field offsets, in the header (compiled) and in the numpy mirror."""
    assert pkg.TRACK.itemsize == 24 == to.TRACK.itemsize
    want = {"birth_frame": 0, "birth_pos": 8, "age": 12, "prev": 16, "reserved": 20}
    assert {k: pkg.TRACK.fields[k][1] for k in pkg.TRACK.names} == want
    assert pkg.TRACK == to.TRACK
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include "viso_hip.h"\n'
                   "_Static_assert(sizeof(vh_track) == 24, \"size\");\n"
                   + "".join(f"_Static_assert(offsetof(vh_track, {k}) == {v}, \"{k}\");\n" for k, v in want.items())
                   + "int main(void) { return 0; }\n")
    r = subprocess.run(["gcc", "-std=c11", "-I", os.path.join(ROOT, "include"), "-c", str(src), "-o", str(tmp_path / "layout.o")],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_track_null_handles_and_pointers_need_no_gpu(pkg):
    lib = pkg._lib()
    n = C.c_int32(0)
    buf = np.zeros(4, pkg.TRACK)
    assert lib.vh_set_track_linking(None, 1) == pkg.VH_ERR_INVALID_ARG
    assert lib.vh_group_set_track_linking(None, 1) == pkg.VH_ERR_INVALID_ARG
    assert lib.vh_get_tracks(None, buf.ctypes.data_as(C.c_void_p), 4, C.byref(n)) == pkg.VH_ERR_INVALID_ARG
    assert lib.vh_group_get_tracks(None, 0, buf.ctypes.data_as(C.c_void_p), 4, C.byref(n)) == pkg.VH_ERR_INVALID_ARG
    assert lib.vh_group_get_tracks_all(None, buf.ctypes.data_as(C.c_void_p), 4, C.byref(n)) == pkg.VH_ERR_INVALID_ARG
    p, s = C.c_void_p(), C.c_int64(0)
    assert lib.vh_group_tracks_device(None, C.byref(p), C.byref(s)) == pkg.VH_ERR_INVALID_ARG
    pm = np.zeros(4, pkg.P_MATCH_DTYPE)
    cnt = np.array([4], np.int32)
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    assert lib.vh_link_tracks(0, 1, ptr(pm), 4, None, 8, None, None, ptr(buf)) == pkg.VH_ERR_INVALID_ARG
    assert lib.vh_link_tracks(0, 1, None, 4, ptr(cnt), 8, None, None, ptr(buf)) == pkg.VH_ERR_INVALID_ARG
    assert lib.vh_link_tracks(0, 1, ptr(pm), 4, ptr(cnt), 8, None, None, None) == pkg.VH_ERR_INVALID_ARG
    assert lib.vh_link_tracks(0, 0, ptr(pm), 4, ptr(cnt), 8, None, None, ptr(buf)) == pkg.VH_ERR_INVALID_ARG
    assert lib.vh_link_tracks(0, 1, ptr(pm), 4, ptr(cnt), 0, None, None, ptr(buf)) == pkg.VH_ERR_INVALID_ARG
    assert lib.vh_link_tracks(0, 1, ptr(pm), 2, ptr(cnt), 8, None, None, ptr(buf)) == pkg.VH_ERR_INVALID_ARG  # count > stride
    assert lib.vh_group_debug_fail_alloc_after(None, 0) == pkg.VH_ERR_INVALID_ARG
    lib.vh_track_carry_free(None)


def records(i1p, i1c):
    pm = np.zeros(len(i1p), np.dtype([("i1p", "<i4"), ("i1c", "<i4")]))
    pm["i1p"], pm["i1c"] = i1p, i1c
    return pm


def test_oracle_on_constructed_lists():
    n_index = 10
    a = records([-1, -1, -1, -1], [3, 5, 3, 12])           # stereo-like; feature 3 twice; 12 is outside the table
    b = records([3, 3, 5, 12, -1, 7], [1, 2, 3, 4, 5, 6])  # two claims on feature 3; 12 never links; 7 unknown
    c = records([], [])                                    # an empty list in the middle
    d = records([1, 3], [0, 0])
    (ta, tb, tc, td), carry = to.link([a, b, c, d], n_index)
    assert ta.tolist() == [(0, 0, 1, -1, 0), (0, 1, 1, -1, 0), (0, 2, 1, -1, 0), (0, 3, 1, -1, 0)]
    # j = 0 continues the LOWEST q with i1c == 3 (q = 0); j = 1 loses the contest for q = 0: a new track
    assert tb.tolist() == [(0, 0, 2, 0, 0), (1, 1, 1, -1, 0), (0, 1, 2, 1, 0), (1, 3, 1, -1, 0), (1, 4, 1, -1, 0), (1, 5, 1, -1, 0)]
    assert len(tc) == 0
    assert td.tolist() == [(3, 0, 1, -1, 0), (3, 1, 1, -1, 0)]  # the empty list breaks every chain
    assert carry.next_serial == 4
    te, _ = to.link([records([0, 0], [9, 9])], n_index, carry)
    assert te[0].tolist() == [(3, 0, 2, 0, 0), (4, 1, 1, -1, 0)]


def random_lists(pkg, rng, n_lists, max_len, n_index, empty=(), full=()):
    """Lists with duplicate indices on both sides of a link, i1p = -1 and indices >= n_index."""
    out = []
    for l in range(n_lists):
        n = 0 if l in empty else (max_len if l in full else int(rng.integers(1, max_len + 1)))
        pm = np.zeros(n, pkg.P_MATCH_DTYPE)
        pm["i1c"] = rng.integers(0, n_index + n_index // 8, n)
        pm["i1p"] = rng.integers(-1, n_index + n_index // 8, n)
        pm["i1p"][rng.random(n) < 0.05] = -1
        for k in ("u1p", "v1p", "u1c", "v1c"):
            pm[k] = rng.integers(0, 1000, n)
        out.append(pm)
    return out


def test_oracle_carry_equals_one_long_call(pkg):
    rng = np.random.default_rng(3)
    lists = random_lists(pkg, rng, 9, 60, 40, empty=(4,))
    whole, wc = to.link(lists, 40)
    assert max(int(t["age"].max(initial=0)) for t in whole) >= 3  # (chains exist in these lists)
    for cut in range(1, 9):
        first, carry = to.link(lists[:cut], 40)
        second, c2 = to.link(lists[cut:], 40, carry)
        for x, y in zip(whole, first + second):
            assert x.tobytes() == y.tobytes(), cut
        assert c2.next_serial == wc.next_serial == 9


# ------------------------------------------------------------------ GPU
def frames_of(pkg, T, seed, w=W, h=H, disparity=6, blur=3):
    return pkg.synth.stereo_sequence(w, h, T, disparity=disparity, blur=blur, seed=seed)


def dims_of(pkg, w=W, h=H):
    return [w, h, pkg.synth.bytes_per_line(w)]


def lone_tracked(pkg, p, frames, dims, meth):
    """A lone Matcher with linking on, fed frame by frame -> {t: (matches, tracks)} for the pairs t - 1 -> t."""
    m = pkg.Matcher(p, outlier_removal=False)
    m.setTrackLinking(True)
    out = {}
    for t, (l, r) in enumerate(frames):
        m.pushBack(l, r, dims)
        if t:
            m.matchFeatures(meth)
            out[t] = (m.getMatches(), m.getTracks())
    m.close()
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("meth", (FLOW, QUAD))
def test_sequence_tracks_equal_oracle_and_lone_matcher(pkg, gpu, meth):
    """40 frames through a sequence handle in chunks of T = 1, 7 and 16."""
    p, dims = pkg.Params.default(), dims_of(pkg)
    N = 40
    frames = frames_of(pkg, N, 41)
    lone = lone_tracked(pkg, p, frames, dims, meth)
    cam = to.Camera()
    want = {}
    for t in range(N):
        cam.push()
        if t:
            want[t] = cam.match(lone[t][0])
    # the inputs exercise the feature (properties of the oracle's answer alone)
    ages = np.concatenate([want[t]["age"] for t in want])
    assert ages.max() > 16, ages.max()                      # a track older than the largest chunk
    assert all(len(lone[t][0]) >= 20 for t in lone)
    inside = range(17, 31)                                  # pairs strictly inside the chunk [16, 32) of T = 16
    assert any((want[t]["age"] == 1).any() for t in inside)                                                   # born there
    assert any(len(set(range(len(want[t]))) - set(want[t + 1]["prev"].tolist())) > 0 for t in inside)         # ended there
    for t in want:
        assert lone[t][1].tobytes() == want[t].tobytes(), ("lone", t)
    for T in (1, 7, 16):
        g = pkg.SequenceGroup(T, p)
        g.setTrackLinking(True)
        for F in range(0, N, T):
            n = min(T, N - F)
            g.pushBack(np.stack([frames[t][0] for t in range(F, F + n)]), np.stack([frames[t][1] for t in range(F, F + n)]), dims)
            g.matchFeatures(meth)
            allt, counts = g.getTracksAll()
            for r in range(T):
                t = F + r
                if r < n and t >= 1:
                    assert g.getMatches(r).tobytes() == lone[t][0].tobytes(), (T, t)
                    got = g.getTracks(r)
                    assert got.tobytes() == want[t].tobytes(), (T, t)
                    assert counts[r] == len(got) and allt[r, :counts[r]].tobytes() == got.tobytes(), (T, t)
                else:
                    assert len(g.getTracks(r)) == 0 and counts[r] == 0, (T, F, r)
        g.close()


@pytest.mark.gpu
def test_sequence_rematch_and_unmatched_chunk(pkg, gpu):
    """Matching a chunk again (another method) replaces its lists and keeps the carry; a chunk that is never matched
    breaks the chain; a dims change restarts the serials."""
    p, dims = pkg.Params.default(), dims_of(pkg)
    frames = frames_of(pkg, 20, 43)
    g = pkg.SequenceGroup(4, p)
    g.setTrackLinking(True)

    def chunk(F, n, fr=frames, d=dims):
        g.pushBack(np.stack([fr[t][0] for t in range(F, F + n)]), np.stack([fr[t][1] for t in range(F, F + n)]), d)

    def check(F, n, carry):
        """-> carry of this match call (the oracle's (i1c, tracks) of the last row); rows against a chain from `carry`."""
        pred = carry
        for r in range(n):
            if F + r == 0:
                assert len(g.getTracks(r)) == 0
                continue
            pm = g.getMatches(r)
            assert len(pm) >= 20
            trk = to.link_one(pm, pred, 1 << 24, F + r)
            assert g.getTracks(r).tobytes() == trk.tobytes(), (F, r)
            pred = (np.array(pm["i1c"], np.int64), trk)
        return pred

    chunk(0, 4)
    g.matchFeatures(FLOW)
    check(0, 4, None)
    g.matchFeatures(QUAD)
    c0 = check(0, 4, None)
    chunk(4, 3)
    g.matchFeatures(FLOW)
    check(4, 3, c0)
    g.matchFeatures(STEREO)        # stereo records (i1p = -1) start tracks; the next chunk continues their i1c
    c1 = check(4, 3, c0)
    assert (g.getTracks(0)["age"] == 1).all()
    chunk(7, 4)
    g.matchFeatures(FLOW)
    c2 = check(7, 4, c1)
    assert (g.getTracks(0)["age"] == 2).any()
    chunk(11, 2)                   # never matched
    chunk(13, 4)
    g.matchFeatures(QUAD)
    check(13, 4, None)
    assert (g.getTracks(0)["age"] == 1).all() and (g.getTracks(0)["birth_frame"] == 13).all()
    del c2
    w2, h2 = 288, 144
    fb = frames_of(pkg, 6, 48, w=w2, h=h2)
    chunk(0, 3, fb, dims_of(pkg, w2, h2))
    g.matchFeatures(QUAD)
    cb = check(0, 3, None)
    chunk(3, 3, fb, dims_of(pkg, w2, h2))
    g.matchFeatures(QUAD)
    check(3, 3, cb)
    g.close()


@pytest.mark.gpu
def test_group_streams_do_not_leak(pkg, gpu):
    """3 streams with different seeds over 6 steps: per stream equal to the oracle."""
    p, dims = pkg.Params.default(), dims_of(pkg)
    S, N = 3, 6
    fr = [frames_of(pkg, N, 60 + s) for s in range(S)]
    cams = [to.Camera() for _ in range(S)]
    g = pkg.StreamGroup(S, p)
    g.setTrackLinking(True)
    linked = 0
    for t in range(N):
        g.pushBack(np.stack([fr[s][t][0] for s in range(S)]), np.stack([fr[s][t][1] for s in range(S)]), dims)
        for c in cams:
            c.push()
        if not t:
            continue
        g.matchFeatures(QUAD)
        allt, counts = g.getTracksAll()
        ptr, stride = g.tracksDevice()
        assert ptr and stride >= counts.max()
        for s in range(S):
            pm = g.getMatches(s)
            assert len(pm) >= 20
            want = cams[s].match(pm)
            assert g.getTracks(s).tobytes() == want.tobytes(), (t, s)
            assert allt[s, :counts[s]].tobytes() == want.tobytes()
            linked += int((want["age"] > 1).sum())
    assert linked > 100
    g.close()


@pytest.mark.gpu
def test_breaks_of_a_lone_matcher(pkg, gpu):
    """A step without a match call, replace pushes of A and of B, a dims change, a method change flow -> quad -> stereo."""
    p, dims = pkg.Params.default(), dims_of(pkg)
    fr = frames_of(pkg, 16, 47)
    m = pkg.Matcher(p, outlier_removal=False)
    m.setTrackLinking(True)
    cam = to.Camera()

    def push(t, replace=False, f=fr, d=dims):
        m.pushBack(f[t][0], f[t][1], d, replace)
        cam.push(replace)

    def match(meth, expect_links):
        m.matchFeatures(meth)
        pm = m.getMatches()
        assert len(pm) >= 20
        want = cam.match(pm)
        assert m.getTracks().tobytes() == want.tobytes(), meth
        assert bool((want["age"] > 1).any()) == expect_links, (meth, want["age"].max())
        return want

    push(0); push(1)
    match(FLOW, False)
    push(2)
    match(QUAD, True)          # flow -> quad
    push(3)
    w = match(STEREO, False)   # quad -> stereo: i1p = -1 everywhere
    assert (w["birth_frame"] == 3).all()
    push(4)
    match(FLOW, True)          # stereo -> flow: the stereo list's i1c are continued
    push(5)                    # a step without a match call
    push(6)
    match(QUAD, False)
    push(7)
    match(QUAD, True)
    push(8, replace=True)      # A = frame 7 is overwritten after (6 -> 7) was matched, and not matched again
    push(9)
    w = match(QUAD, False)
    assert (w["birth_frame"] == 8).all()   # (the replace kept the serial of the slot)
    push(10)
    first = match(QUAD, True)
    push(11, replace=True)     # B is replaced, then matched again: the list is replaced, its predecessor stays
    second = match(QUAD, True)
    assert (second["birth_frame"] <= 9).all() and first.tobytes() != second.tobytes()
    match(FLOW, True)          # the same pair once more with another method
    push(12)
    match(FLOW, True)
    w2, h2 = 288, 144
    fb = frames_of(pkg, 4, 48, w=w2, h=h2)
    cam.restart()
    push(0, f=fb, d=dims_of(pkg, w2, h2)); push(1, f=fb, d=dims_of(pkg, w2, h2))
    w = match(QUAD, False)
    assert (w["birth_frame"] == 1).all()
    push(2, f=fb, d=dims_of(pkg, w2, h2))
    match(QUAD, True)
    m.close()


@pytest.mark.gpu
def test_many_match_calls_on_one_pair(pkg, gpu):
    """More match calls than the tables' epoch counter holds: the predecessor survives the counter coming round."""
    p, dims = pkg.Params.default(), dims_of(pkg)
    fr = frames_of(pkg, 4, 49)
    m = pkg.Matcher(p, outlier_removal=False)
    m.setTrackLinking(True)
    cam = to.Camera()
    for t in range(3):
        m.pushBack(fr[t][0], fr[t][1], dims)
        cam.push()
        if t:
            m.matchFeatures(QUAD)
            want = cam.match(m.getMatches())
    for k in range(300):
        m.matchFeatures(FLOW if k % 50 == 49 else QUAD)
        if k % 50 >= 48 or k in (250, 251, 252, 253, 254, 255, 256):
            want = cam.match(m.getMatches())
            assert (want["age"] == 2).any()
            assert m.getTracks().tobytes() == want.tobytes(), k
    m.pushBack(fr[3][0], fr[3][1], dims)
    cam.push()
    m.matchFeatures(QUAD)
    want = cam.match(m.getMatches())
    assert (want["age"] == 3).any() and m.getTracks().tobytes() == want.tobytes()
    m.close()


@pytest.mark.gpu
def test_refinement_and_multi_stage(pkg, gpu):
    """refinement = 2 drops records after the circle check: positions are those of the emitted list.  Multi-stage on:
    the tracked list is the dense list of pass 2."""
    dims = dims_of(pkg)
    fr = frames_of(pkg, 6, 51, blur=4)
    plain = None
    for name, p in (("plain", pkg.Params.default()), ("refine", pkg.Params.default(refinement=2)), ("multi", pkg.Params.default(multi_stage=1))):
        m = pkg.Matcher(p, outlier_removal=False)
        if name == "multi":
            m.setMultiStageMatching(True)
        m.setTrackLinking(True)
        cam = to.Camera()
        counts = []
        for t in range(6):
            m.pushBack(fr[t][0], fr[t][1], dims)
            cam.push()
            if t:
                m.matchFeatures(QUAD)
                pm = m.getMatches()
                want = cam.match(pm)
                assert len(pm) >= 20 and m.getTracks().tobytes() == want.tobytes(), (name, t)
                counts.append(len(pm))
        assert (want["age"] >= 3).any(), name
        if name == "plain":
            plain = counts
        elif name == "refine":
            assert any(c < q for c, q in zip(counts, plain)), (counts, plain)  # (records were dropped on these frames)
        m.close()


@pytest.mark.gpu
def test_link_tracks_stateless(pkg, gpu):
    """64 constructed lists of up to 65 535 records, duplicate and out-of-range indices, split through the carry."""
    rng = np.random.default_rng(11)
    n_index = 50000
    lists = random_lists(pkg, rng, 64, 65535, n_index, empty=(20, 21, 63), full=(5, 6))
    want, _ = to.link(lists, n_index)
    assert max(int(t["age"].max(initial=0)) for t in want) >= 5
    whole, _ = pkg.link_tracks(lists, n_index)
    for l in range(64):
        assert whole[l].tobytes() == want[l].tobytes(), l
    for cut in (1, 21, 40):
        a, carry = pkg.link_tracks(lists[:cut], n_index)
        b, carry2 = pkg.link_tracks(lists[cut:], n_index, carry)
        for l, t in enumerate(a + b):
            assert t.tobytes() == want[l].tobytes(), (cut, l)
        # a carry is not consumed: the same continuation again
        b2, _ = pkg.link_tracks(lists[cut:cut + 2], n_index, carry)
        assert b2[0].tobytes() == want[cut].tobytes() and b2[1].tobytes() == want[cut + 1].tobytes()
    # the carry of a call that ended with an empty list: the next list starts new tracks at the next serial
    c, _ = pkg.link_tracks([lists[0]], n_index, carry2)
    assert (c[0]["age"] == 1).all() and (c[0]["birth_frame"] == 64).all()


@pytest.mark.gpu
def test_link_tracks_on_voted_lists(pkg, gpu):
    """The use the stateless entry exists for: lists the handle never sees again (after the vote) are linked by it."""
    p, dims = pkg.Params.default(), dims_of(pkg)
    fr = frames_of(pkg, 6, 53)
    m = pkg.Matcher(p)  # matchFeatures ends with removeOutliers
    lists = []
    for t in range(6):
        m.pushBack(fr[t][0], fr[t][1], dims)
        if t:
            m.matchFeatures(QUAD)
            lists.append(m.getMatches())
    n_index = max(int(x["i1c"].max()) for x in lists) + 1
    m.close()
    want, _ = to.link(lists, n_index)
    got, _ = pkg.link_tracks(lists, n_index)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(got, want))
    assert max(int(t["age"].max()) for t in want) == 5


@pytest.mark.gpu
def test_switch_off_changes_nothing(pkg, gpu):
    """Off (never set, or set and cleared): same match lists, same device bytes, no track_* launch, getters VH_ERR_STATE."""
    p, dims = pkg.Params.default(), dims_of(pkg)
    S = 3
    fr = frames_of(pkg, 5, 55)
    seen = {}
    for name, toggle in (("plain", ()), ("cleared", (True, False)), ("on", (True,))):
        g = pkg.StreamGroup(S, p)
        for on in toggle:
            g.setTrackLinking(on)
        g.profileEnable(True)
        lists = []
        for t in range(3):
            g.pushBack(np.stack([fr[s + t][0] for s in range(S)]), np.stack([fr[s + t][1] for s in range(S)]), dims)
            if t:
                for meth in (FLOW, QUAD):
                    g.matchFeatures(meth)
                    lists += [g.getMatches(s).tobytes() for s in range(S)]
        launches = tuple(g.profileRead(k)[1] for k in ("track_scatter", "track_link", "track_rank", "track_carry", "emit_matches"))
        seen[name] = (lists, g.deviceBytes(), launches)
        if name != "on":
            for call in (lambda: g.getTracks(0), g.getTracksAll, g.tracksDevice):
                with pytest.raises(pkg.VisoHipError) as e:
                    call()
                assert e.value.code == pkg.VH_ERR_STATE
        else:
            assert len(g.getTracks(0)) == len(g.getMatches(0))
        with pytest.raises(pkg.VisoHipError) as e:
            g.setTrackLinking(True)   # after the first push
        assert e.value.code == pkg.VH_ERR_STATE
        g.close()
    assert seen["plain"] == seen["cleared"]
    assert seen["plain"][2] == (0, 0, 0, 0, 4)
    assert seen["on"][0] == seen["plain"][0]
    assert seen["on"][2] == (4, 4, 4, 0, 4)
    m = pkg.Matcher(p)
    mcap = len(m.getMatches())  # (nothing matched)
    assert mcap == 0
    with pytest.raises(pkg.VisoHipError) as e:
        m.getTracks()
    assert e.value.code == pkg.VH_ERR_STATE
    m.close()
    # memory with the switch on: two tables of 4 * cap bytes per row (+ the second list's), 24 * mcap per list, the counts
    g = pkg.StreamGroup(S, p, max_features=4096, max_matches=2048)
    g.setTrackLinking(True)
    for t in range(2):
        g.pushBack(np.stack([fr[s + t][0] for s in range(S)]), np.stack([fr[s + t][1] for s in range(S)]), dims)
    before = g.deviceBytes()
    g.matchFeatures(QUAD)
    assert g.deviceBytes() - before == 2 * S * 4096 * 4 + S * 4096 * 4 + 2 * S * 2048 * 24 + 2 * S * 4
    g.close()


@pytest.mark.gpu
def test_failed_allocation_leaves_the_handle_usable(pkg, gpu):
    p, dims = pkg.Params.default(), dims_of(pkg)
    fr = frames_of(pkg, 5, 57)
    m = pkg.StreamGroup(1, p)
    m.setTrackLinking(True)
    cam = to.Camera()
    for t in range(2):
        m.pushBack(fr[t][0][None], fr[t][1][None], dims)
        cam.push()
    m.debugFailNextAlloc()
    with pytest.raises(pkg.VisoHipError) as e:
        m.matchFeatures(QUAD)       # the track buffers cannot be had: nothing is matched
    assert e.value.code == pkg.VH_ERR_HIP
    with pytest.raises(pkg.VisoHipError) as e:
        m.getTracks(0)
    assert e.value.code == pkg.VH_ERR_STATE
    m.pushBack(fr[2][0][None], fr[2][1][None], dims)
    cam.push()                      # (the pair 0 -> 1 has no tracked list)
    m.matchFeatures(QUAD)
    want = cam.match(m.getMatches(0))
    assert (want["age"] == 1).all() and (want["birth_frame"] == 2).all()
    assert m.getTracks(0).tobytes() == want.tobytes()
    m.pushBack(fr[3][0][None], fr[3][1][None], dims)
    cam.push()
    m.debugFailNextAlloc()
    with pytest.raises(pkg.VisoHipError):
        m.matchFeatures(FLOW)       # the flow method's pixel mask cannot be had: the pair 2 -> 3 stays without a list
    m.matchFeatures(QUAD)
    want = cam.match(m.getMatches(0))
    assert (want["age"] == 2).any() and m.getTracks(0).tobytes() == want.tobytes()
    m.pushBack(fr[4][0][None], fr[4][1][None], dims)
    cam.push()
    m.matchFeatures(FLOW)
    want = cam.match(m.getMatches(0))
    assert (want["age"] == 3).any() and m.getTracks(0).tobytes() == want.tobytes()
    m.close()


@pytest.mark.gpu
def test_failure_between_allocation_and_clearing(pkg, gpu):
    """A match call that allocates the track tables (or the flow method's pixel mask) and then fails before their
    clearing is queued: the next call still clears them.  (Decisive with VH_POISON=1, where fresh buffers hold 0xA5:
    test_child_failure_paths_on_poisoned_buffers.)"""
    dims = dims_of(pkg)
    fr = frames_of(pkg, 4, 61)

    def clean_lists(p, meth, multi):
        m = pkg.StreamGroup(1, p)
        if multi:
            m.setMultiStageMatching(True)
        out = {}
        for t in range(4):
            m.pushBack(fr[t][0][None], fr[t][1][None], dims)
            if t:
                m.matchFeatures(meth)
                out[t] = m.getMatches(0)
        m.close()
        return out

    # multi-stage + linking, quad: the four track buffers are allocated, then the range table's allocation fails;
    # linking alone, flow: the pixel mask is allocated, then the first track buffer's allocation fails
    for name, p, meth, multi, skip in (("ranges", pkg.Params.default(multi_stage=1), QUAD, True, 4),
                                       ("mask", pkg.Params.default(), FLOW, False, 1)):
        want_pm = clean_lists(p, meth, multi)
        m = pkg.StreamGroup(1, p)
        if multi:
            m.setMultiStageMatching(True)
        m.setTrackLinking(True)
        cam = to.Camera()
        for t in range(4):
            m.pushBack(fr[t][0][None], fr[t][1][None], dims)
            cam.push()
            if not t:
                continue
            if t == 1:
                before = m.deviceBytes()
                m.debugFailAllocAfter(skip)
                with pytest.raises(pkg.VisoHipError) as e:
                    m.matchFeatures(meth)
                assert e.value.code == pkg.VH_ERR_HIP, name
                assert m.deviceBytes() > before, name   # (buffers were allocated by the failed call)
            m.matchFeatures(meth)
            pm = m.getMatches(0)
            assert len(pm) >= 20 and pm.tobytes() == want_pm[t].tobytes(), (name, t)
            want = cam.match(pm)
            assert m.getTracks(0).tobytes() == want.tobytes(), (name, t)
        assert (want["age"] == 3).any(), name
        m.close()


@pytest.mark.gpu
def test_child_failure_paths_on_poisoned_buffers(gpu):
    """The failure paths with VH_POISON=1: every buffer that is not zero-initialised at allocation starts as 0xA5 bytes, so
    a table or mask that is used without having been cleared changes the lists and the tracks."""
    env = dict(os.environ, VH_POISON="1")
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-q", "-x", "-m", "gpu", "-k",
                        "between_allocation or failed_allocation_leaves"],
                       env=env, capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "2 passed" in r.stdout and " skipped" not in r.stdout, r.stdout[-2000:]


@pytest.mark.gpu
def test_match_capacity_beyond_the_position_field(pkg, gpu):
    """max_matches above 2^24 - 1 does not fit a table entry: the match call says so instead of linking wrongly."""
    dims = dims_of(pkg)
    fr = frames_of(pkg, 2, 63)
    for on, code in ((True, pkg.VH_ERR_UNSUPPORTED), (False, pkg.VH_OK)):
        m = pkg.StreamGroup(1, pkg.Params.default(), max_matches=1 << 24)
        m.setTrackLinking(on)
        for t in range(2):
            m.pushBack(fr[t][0][None], fr[t][1][None], dims)
        assert pkg._lib().vh_group_match_features(m._h, QUAD) == code, on
        m.close()


@pytest.mark.gpu
def test_capacity_rules_of_the_getters(pkg, gpu):
    p, dims = pkg.Params.default(), dims_of(pkg)
    fr = frames_of(pkg, 2, 59)
    m = pkg.Matcher(p, outlier_removal=False)
    m.setTrackLinking(True)
    for t in range(2):
        m.pushBack(fr[t][0], fr[t][1], dims)
    m.matchFeatures(QUAD)
    full = m.getTracks()
    n = C.c_int32(0)
    part = np.zeros(10, pkg.TRACK)
    rc = pkg._lib().vh_get_tracks(m._h, part.ctypes.data_as(C.c_void_p), 10, C.byref(n))
    assert rc == pkg.VH_ERR_CAPACITY and n.value == len(full) > 10 and part.tobytes() == full[:10].tobytes()
    m.close()


@pytest.mark.gpu
def test_child_tracks_checking_build(pkg, gpu):
    """The GPU cases of this file once more on libviso_hip_check.so (-DVH_CHECK): every index the track kernels follow is
    verified on the device."""
    assert os.path.exists(pkg.CHECK_LIB_PATH), "build() makes it"
    env = dict(os.environ, VISO_HIP_LIB=pkg.CHECK_LIB_PATH)
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-q", "-x", "-m", "gpu", "-k", "not child"],
                       env=env, capture_output=True, text=True, timeout=900, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert " passed" in r.stdout and " skipped" not in r.stdout, r.stdout[-2000:]
    assert "VH_CHECK" not in r.stderr
