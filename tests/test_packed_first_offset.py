"""The packed-list stateless entries on lists that do not begin at record 0.  They share one staging path -- the records
go up to the slots [offsets[0], offsets[n]) of the device block, and every slice output comes back from the slots of the
same numbers -- so one mistake there would be every entry's.  Each entry runs twice on the same four lists of 0, 1, 65 and
1 025 records (the empty list first, so two offsets coincide; 65 crosses a wave; 1 025 crosses VH_INLIER_TILE, four
VH_SCENE_TILEs and two VH_MONO_POSE_TILEs): packed from record 0, and behind offsets[0] = 3 with three records in front that
belong to no list.  The per-list outputs must be the same bytes, the slices of the slice outputs too, and what lies in
front of offsets[0] and behind each list's written count must still be the pattern the arrays were filled with."""
import ctypes as C

import numpy as np
import pytest

import egomotion_scene as es
import mono_pose_oracle as mp
from test_stateless_validation import PACKED_ARRAYS, PACKED_ENTRIES, ptr

pytestmark = pytest.mark.gpu

LENGTHS = (0, 1, 65, 1025)
FRONT = 3
PATTERN = 0xA7
# the slice outputs and the per-list count that says how much of a list's slice is written (None: all of it)
SLICES = {"flags": None, "inlier_pm": "n_inliers", "src_pos": "n_inliers", "points": "counts"}


@pytest.fixture(scope="module")
def scenes(pkg):
    """stereo and mono lists, their inputs, and the offsets of both runs -- built once, never changed"""
    n = len(LENGTHS)
    total = sum(LENGTHS)
    ego = pkg.EgoParams.default(ransac_iters=50)
    mono = pkg.MonoParams.default(ransac_iters=50)
    quad, tr = es.scene(pkg.P_MATCH_DTYPE, total, 7)
    flow = mp.ground_scene(pkg.P_MATCH_DTYPE, total, 11)
    cuts = np.concatenate([[0], np.cumsum(LENGTHS)]).astype(np.int32)
    # one model and one pose for every list: the estimator's on the longest list, so that the short lists are exercised too
    longest = flow[cuts[3]:cuts[4]]
    rand8 = np.random.default_rng(3).integers(0, 2**31 - 1, (1, mono.ransac_iters, 8)).astype(np.int32)
    _, ok, _, model = pkg.estimate_motion_mono(mono, [longest], rand8, model=True)
    assert ok[0] and model[0]["valid"] == 1.0
    _, ok, pose = pkg.pose_mono(mono, [longest], model, [1])
    assert ok[0]
    front = np.zeros(FRONT, pkg.P_MATCH_DTYPE)
    for name in front.dtype.names:
        front[name] = 12345                       # records of no list: a kernel that read them would not get the lists' results
    inputs = {"tr": np.tile(tr, (n, 1)), "ok": np.ones(n, np.int32), "model": np.repeat(model, n), "pose": np.repeat(pose, n),
              "Tw": np.tile(np.eye(4).ravel(), (n, 1))}
    return dict(ego=ego, mono=mono, n=n, total=total, cuts=cuts, front=front, inputs=inputs, lists={"ego": quad, "mono": flow})


def run(pkg, scenes, name, first):
    """-> {output: bytes as uint8 [elements][bytes of one]} of one call with the lists behind offsets[0] = first"""
    params, extra, args = PACKED_ENTRIES[name]
    n, end = scenes["n"], first + scenes["total"]
    pm = np.concatenate([scenes["front"][:first], scenes["lists"][params]])
    off = (scenes["cuts"] + first).astype(np.int32)
    sp = pkg.SceneParams.default(frame=0)
    given = {a: np.ascontiguousarray(scenes["inputs"][a]) for a, kind in args if kind == "in" or a == "Tw"}   # (alive through the call)
    bufs = {a: np.full((end if a in SLICES else n, PACKED_ARRAYS[a][0]), PATTERN, np.uint8) for a, _ in args if a not in given}
    tail = [ptr(given[a]) if a in given else ptr(bufs[a]) for a, _ in args]
    head = [C.byref(scenes[params])] + [C.byref(sp) for _ in extra]
    rc = getattr(pkg._lib(), name)(*head, 0, n, ptr(pm), ptr(off), *tail)
    assert rc == pkg.VH_OK, (name, first, rc)
    return bufs, off


@pytest.mark.parametrize("name", sorted(PACKED_ENTRIES))
def test_lists_behind_first_offset(name, pkg, scenes):
    at0, off0 = run(pkg, scenes, name, 0)
    at3, off3 = run(pkg, scenes, name, FRONT)
    n = scenes["n"]
    written = 0
    for a in at0:
        if a not in SLICES:
            assert at0[a].tobytes() == at3[a].tobytes(), (name, a)          # per-list outputs: the same bytes
            assert not (at0[a] == PATTERN).all(axis=1).any(), (name, a)       # ... and every one of them written
            continue
        counts = None if SLICES[a] is None else at0[SLICES[a]].copy().view(np.int32).ravel()
        assert (at3[a][:FRONT] == PATTERN).all(), (name, a, "in front of offsets[0]")
        for s in range(n):
            length = int(off0[s + 1] - off0[s])
            k = length if counts is None else int(counts[s])
            assert 0 <= k <= length, (name, a, s, k)
            written += k
            assert at0[a][off0[s]:off0[s] + k].tobytes() == at3[a][off3[s]:off3[s] + k].tobytes(), (name, a, s)
            for got, off in ((at0[a], off0), (at3[a], off3)):
                assert (got[off[s] + k:off[s + 1]] == PATTERN).all(), (name, a, s, "behind the written count")
    if any(a in SLICES for a in at0):
        assert written > 1000, (name, "the lists must leave something to compare")
