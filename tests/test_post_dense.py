"""Dense inliers and the motion refit as stages of the device post chain:
vh_group_post_device_dense / vh_group_post_finish_device_dense.  Everything the chain delivers is held to code that
existed before it -- the getters (the dense lists of every step, fetched before postBeginDevice), the stateless entries
(remove_outliers_device, motion_inliers, refit_motion, estimate_motion_mono, motion_inliers_mono) and the numpy
restatements (tests/inlier_oracle.py, refit_oracle.py, mono_inlier_oracle.py) -- never to its own output.

Frames: 240 x 120 synthetic stereo, the smallest of the sizes tried whose voted quad list (about 1 770 records) is longer
than VH_INLIER_TILE = 1 024, so that a list spans two tiles, the second partly filled (asserted).  S = 3: stream 1 sees
constant images (an empty list, ok = 0), stream 2 is textured on its left 45 % only (a list shorter than one tile).
Shape of the ring: 2 steps per batch, 2 batches, six steps -- the ring comes round, and one finish closes a half-full
batch.

Bounds.  flags against inlier_oracle: equal except records whose sum lies within 1e-9 relative of the threshold, at most
0.1 % of a list (the device's sin / cos, section 4.10).  tr_refit against refit_oracle: rtol 1e-9, atol 1e-12, ok and
n_updates exact (section 4.12).  Mono flags against mono_inlier_oracle: exact (section 4.11).  All else byte for byte."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import inlier_oracle as io
import mono_inlier_oracle as moo
import refit_oracle as ro
from conftest import ROOT

SYMBOLS = ("vh_group_post_device_dense", "vh_group_post_finish_device_dense")
W, H, S, T = 240, 120, 3, 7
FLOW, QUAD = 0, 2
TILE = 1024                       # VH_INLIER_TILE
CAL = dict(f=225.0, cu=120.0, cv=60.0, base=0.5)
RTOL, ATOL = 1e-9, 1e-12          # tests/test_egomotion.py:94, DESIGN.md section 4.12
BAND, BAND_SHARE = 1e-9, 1e-3
CAP = 4096
FIELDS = ("voted_counts", "inlier_counts", "tr_refit", "ok_refit", "n_updates", "model", "voted_pm", "flags", "inlier_pm", "src_pos")
# begin (b) and finish (f, age) in the order a caller two steps ahead would issue them; ("f", 5, 0) closes a half-full batch
SCHEDULE = (("b", 1), ("b", 2), ("b", 3), ("f", 1, 2), ("b", 4), ("f", 2, 2), ("b", 5), ("f", 3, 2), ("f", 4, 1), ("f", 5, 0),
            ("b", 6), ("f", 6, 0))


class Cal:
    def __init__(self, **kw):
        self.__dict__.update(kw)


def ptr(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def expect(pkg, code, call):
    with pytest.raises(pkg.VisoHipError) as e:
        call()
    assert e.value.code == code, e.value


def dims_of(pkg):
    return [W, H, pkg.synth.bytes_per_line(W)]


_FRAMES = {}


def frames_of(pkg):
    """[stream][t] -> (left, right)"""
    if "f" not in _FRAMES:
        fr = [pkg.synth.stereo_sequence(W, H, T, disparity=6, blur=3, seed=seed) for seed in (71, 72, 73)]
        fr[1] = [(np.full_like(a, 90), np.full_like(b, 90)) for a, b in fr[1]]
        half = []
        for a, b in fr[2]:
            a, b = a.copy(), b.copy()
            a[:, int(0.45 * W):] = 90; b[:, int(0.45 * W):] = 90
            half.append((a, b))
        fr[2] = half
        _FRAMES["f"] = fr
    return _FRAMES["f"]


def ego_of(pkg):
    """inlier_threshold 2.5, as the handle tests of test_motion_refit.py: the synthetic frames move by whole pixels, so a
    wrong match is off by whole pixels and its sum of squares is an integer -- under the default threshold of 2.0 a record
    that is off by 2 px in one coordinate has the sum 4.0 = threshold^2 up to rounding, and one such record in a list of
    640 is more than the 0.1 % the band may hold.  6.25 is no sum of integer squares."""
    return pkg.EgoParams.default(ransac_iters=50, inlier_threshold=2.5, **CAL)


def mono_of(pkg):
    return pkg.MonoParams.default(ransac_iters=50, f=CAL["f"], cu=CAL["cu"], cv=CAL["cv"], height=1.0)


def draws(k):
    return np.random.default_rng(11).integers(0, 2 ** 31 - 1, (T, S, 50, k)).astype(np.int32)


def push(g, fr, t, dims):
    g.pushBack(np.stack([f[t][0] for f in fr]), np.stack([f[t][1] for f in fr]), dims)


def run_group(pkg, mode, mono=False, dense=("counts", "lists")):
    """The six steps of SCHEDULE on a fresh group -> {t: (the step's dense lists as the getters gave them, finish dict)}"""
    fr, dims = frames_of(pkg), dims_of(pkg)
    g = pkg.StreamGroup(S, pkg.Params.default())
    g.postDeviceConfig(2, 2, 16)
    g.postDeviceDense(mode)
    e, m = ego_of(pkg), mono_of(pkg)
    rnd = draws(8 if mono else 3)
    push(g, fr, 0, dims)
    lists, out = {}, {}
    for op in SCHEDULE:
        if op[0] == "b":
            t = op[1]
            push(g, fr, t, dims)
            g.matchFeatures(FLOW if mono else QUAD)
            lists[t] = [g.getMatches(s) for s in range(S)]
            if mono:
                g.postBeginDevice(CAP, 2, 50.0, 50.0, mono=m, rand8=rnd[t], want_lists=True)
            else:
                g.postBeginDevice(CAP, 2, 50.0, 50.0, ego=e, rand3=rnd[t], want_lists=True)
        else:
            _, t, age = op
            out[t] = (lists[t], g.postFinishDevice(age, want_lists=True, list_cap=CAP, dense=dense if mode else None))
    g.close()
    return out


_RUNS = {}


def stereo_run(pkg, mode):
    if mode not in _RUNS:
        _RUNS[mode] = run_group(pkg, mode)
    return _RUNS[mode]


def same_base(a, b, what):
    """tr, ok, n_inliers, bucketed lists and counts of two finish dicts, bit for bit"""
    assert a["tr"].tobytes() == b["tr"].tobytes() and np.array_equal(a["ok"], b["ok"]), what
    assert np.array_equal(a["n_inliers"], b["n_inliers"]) and np.array_equal(a["counts"], b["counts"]) and a["rc"] == b["rc"], what
    assert [x.tobytes() for x in a["lists"]] == [x.tobytes() for x in b["lists"]], what


def check_stereo_step(pkg, mode, lists, res, what, streams=None):
    """One step of a quad + stereo chain in `mode` against the stateless entries and the restatements, for `streams`."""
    n = len(lists)
    streams = range(n) if streams is None else streams
    e = ego_of(pkg)
    cal = Cal(inlier_threshold=e.inlier_threshold, reweighting=e.reweighting, **CAL)
    voted_w, _, _ = pkg.remove_outliers_device(lists, lanes_per_wave=16)
    tr, ok = res["tr"], res["ok"].astype(np.int32)
    fl1, n1, in1, pos1 = pkg.motion_inliers(e, voted_w, tr, ok)
    want = (fl1, n1, in1, pos1)
    tr_cls, ok_cls = tr, ok
    if mode >= 2:
        tr_r, ok_r, nu_r = pkg.refit_motion(e, in1, tr, ok)
        if mode == 3:
            want = pkg.motion_inliers(e, voted_w, tr_r, ok_r.astype(np.int32))
            tr_cls, ok_cls = tr_r, ok_r.astype(np.int32)
    for s in streams:
        w = (what, s)
        assert res["voted"][s].tobytes() == voted_w[s].tobytes() and res["voted_counts"][s] == len(voted_w[s]), w
        assert res["flags"][s].tobytes() == want[0][s].tobytes() and res["inlier_counts"][s] == want[1][s], w
        assert res["inliers"][s].tobytes() == want[2][s].tobytes() and res["src_pos"][s].tobytes() == want[3][s].tobytes(), w
        fl_o, sums = io.inliers(voted_w[s], tr_cls[s], cal, ok=bool(ok_cls[s]))
        band = io.near_threshold(sums, cal, BAND)
        print(f"{what} stream {s}: voted {len(voted_w[s])}, inliers {int(want[1][s])}, within the band {int(band.sum())}")
        assert band.sum() <= BAND_SHARE * max(len(sums), 1), (w, int(band.sum()), len(sums))
        assert np.array_equal(res["flags"][s][~band], fl_o[~band]), w
        if mode >= 2:
            assert res["tr_refit"][s].tobytes() == tr_r[s].tobytes() and res["ok_refit"][s] == ok_r[s] and res["n_updates"][s] == nu_r[s], w
            tr_o, ok_o, nu_o, _ = ro.refit(in1[s], tr[s], cal, ok=bool(ok[s]))
            assert bool(ok_o) == bool(res["ok_refit"][s]) and nu_o == res["n_updates"][s], (w, ok_o, nu_o, res["n_updates"][s])
            assert np.allclose(res["tr_refit"][s], tr_o, rtol=RTOL, atol=ATOL), (w, res["tr_refit"][s], tr_o)
            assert (res["n_updates"][s] >= 1) == bool(ok[s] and n1[s] >= 6), w
        else:
            assert "tr_refit" not in res
    return voted_w, n1


# ------------------------------------------------------------------------------------------------------------ CPU
def test_symbols_struct_layout_and_argument_errors(pkg, tmp_path):
    """The two symbols are declared, exported and mirrored; vh_post_dense is ten pointers, 80 bytes, member k at offset
    8 k, in the header's order -- the C compiler's layout equals the ctypes mirror's; a mode outside 0..3 and a null
    handle are VH_ERR_INVALID_ARG."""
    header = open(os.path.join(ROOT, "include", "viso_hip.h")).read()
    lib = pkg._lib()
    for name in SYMBOLS:
        assert name + "(" in header and hasattr(C.CDLL(pkg.LIB_PATH), name) and name in pkg.ABI_SYMBOLS, name
    assert "postDeviceDense" in vars(pkg.StreamGroup) and hasattr(pkg.SequenceGroup, "postDeviceDense")
    assert tuple(n for n, _ in pkg.PostDense._fields_) == FIELDS
    assert C.sizeof(pkg.PostDense) == 80
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "viso_hip.h"\nint main(void) {\n  printf("%zu", sizeof(vh_post_dense));\n'
                   + "".join(f'  printf(" %zu", offsetof(vh_post_dense, {n}));\n' for n in FIELDS) + '  return 0;\n}\n')
    exe = str(tmp_path / "layout")
    subprocess.check_call(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), str(src), "-o", exe])
    got = [int(v) for v in subprocess.check_output([exe], timeout=60).decode().split()]
    assert got == [C.sizeof(pkg.PostDense)] + [getattr(pkg.PostDense, n).offset for n in FIELDS] == [80] + [8 * k for k in range(10)]
    inv = pkg.VH_ERR_INVALID_ARG
    for mode in (-1, 4, 7):
        assert lib.vh_group_post_device_dense(None, mode) == inv
    assert lib.vh_group_post_device_dense(None, 1) == inv
    d = pkg.PostDense()
    cnt = np.zeros(3, np.int32)
    assert lib.vh_group_post_finish_device_dense(None, 0, None, None, None, None, 0, ptr(cnt), C.byref(d)) == inv
    assert lib.vh_group_post_finish_device_dense(None, 0, None, None, None, None, 0, ptr(cnt), None) == inv


# ------------------------------------------------------------------------------------------------------------ GPU
@pytest.mark.gpu
@pytest.mark.parametrize("mode", [1, 2, 3])
def test_gpu_quad_stereo_chain(mode, pkg, gpu):
    """Case 1: modes 1, 2, 3 over six steps -- the voted lists, both classifications and the refit against the stateless
    entries byte for byte and against the restatements; the plain results bit for bit those of a mode-0 group."""
    off = stereo_run(pkg, 0)
    on = stereo_run(pkg, mode)
    longest, started = 0, 0
    for t in range(1, T):
        lists, res = on[t]
        assert [x.tobytes() for x in lists] == [x.tobytes() for x in off[t][0]]
        same_base(res, off[t][1], (mode, t))
        assert res["rc"] == pkg.VH_OK
        voted, n1 = check_stereo_step(pkg, mode, lists, res, f"mode {mode} step {t}")
        longest = max(longest, max(len(v) for v in voted))
        assert len(voted[1]) == 0 and not res["ok"][1] and res["voted_counts"][1] == 0 and res["inlier_counts"][1] == 0
        assert 6 < len(voted[2]) < TILE
        if mode >= 2:
            assert not res["ok_refit"][1] and res["n_updates"][1] == 0 and not res["tr_refit"][1].any()
            started += int((res["n_updates"] >= 1).sum())
        assert res["ok"][0] and n1[0] > TILE          # the inliers of a list span two tiles as well
    assert TILE < longest < 2 * TILE, longest           # two tiles, the second partly filled
    assert mode == 1 or started >= 6


@pytest.mark.gpu
def test_gpu_flow_mono_chain(pkg, gpu):
    """Case 2: flow lists, the monocular estimator, mode 1 -- the model is the one estimate_motion_mono gives on the
    returned bucketed lists with the same draws, bit for bit; flags, counts, records and positions equal the stateless
    motion_inliers_mono and the restatement exactly."""
    m = mono_of(pkg)
    rnd = draws(8)
    on = run_group(pkg, 1, mono=True)
    off = run_group(pkg, 0, mono=True)
    valid = 0
    for t in range(1, T):
        lists, res = on[t]
        same_base(res, off[t][1], ("mono", t))
        model_w = pkg.estimate_motion_mono(m, res["lists"], rnd[t], model=True)[3]
        assert res["model"].tobytes() == model_w.tobytes(), t
        voted_w, _, _ = pkg.remove_outliers_device(lists, lanes_per_wave=16)
        ok = res["ok"].astype(np.int32)
        want = pkg.motion_inliers_mono(m, voted_w, res["model"], ok)
        for s in range(S):
            w = ("mono", t, s)
            assert res["voted"][s].tobytes() == voted_w[s].tobytes() and res["voted_counts"][s] == len(voted_w[s]), w
            assert res["flags"][s].tobytes() == want[0][s].tobytes() and res["inlier_counts"][s] == want[1][s], w
            assert res["inliers"][s].tobytes() == want[2][s].tobytes() and res["src_pos"][s].tobytes() == want[3][s].tobytes(), w
            fl_o, _ = moo.inliers(voted_w[s], moo.from_array(res["model"][s]), m.inlier_threshold, ok=bool(ok[s]))
            assert np.array_equal(res["flags"][s], fl_o), w
            print(f"mono step {t} stream {s}: voted {len(voted_w[s])}, ok {bool(ok[s])}, valid {res['model'][s]['valid']}, inliers {int(want[1][s])}")
        assert len(voted_w[0]) > TILE and res["model"][1]["valid"] == 0 and not res["ok"][1]
        valid += int(res["model"]["valid"].sum())
        assert "tr_refit" not in res
    assert valid >= 6


def one_step(pkg, cap_begin, mode=3, t=2):
    """Steps 1 .. t on a fresh group with one step per batch, the last one begun with slots of cap_begin records
    -> (g, the step's lists)"""
    fr, dims = frames_of(pkg), dims_of(pkg)
    g = pkg.StreamGroup(S, pkg.Params.default())
    g.postDeviceConfig(1, 2, 16)
    g.postDeviceDense(mode)
    for k in range(t + 1):
        push(g, fr, k, dims)
    g.matchFeatures(QUAD)
    lists = [g.getMatches(s) for s in range(S)]
    g.postBeginDevice(cap_begin, 2, 50.0, 50.0, ego=ego_of(pkg), rand3=draws(3)[t], want_lists=True)
    return g, lists


def check_refused(res, s):
    assert res["voted_counts"][s] == -1 and res["inlier_counts"][s] == -1 and res["counts"][s] == -1, s
    assert not res["ok_refit"][s] and res["n_updates"][s] == 0 and not res["tr_refit"][s].any() and not res["ok"][s], s
    assert len(res["voted"][s]) == len(res["flags"][s]) == len(res["inliers"][s]) == len(res["src_pos"][s]) == 0, s


@pytest.mark.gpu
def test_gpu_refused_lists(pkg, gpu):
    """Case 3: slots between two streams' list lengths truncate the longer list -- that stream reports the -1 / zero
    markers, the others are delivered as in case 1 (the same frames and draws), the call returns VH_ERR_CAPACITY; the
    same with the sweep's flip stack shrunk to four slots (VH_ERR_UNSUPPORTED); and an output array shorter than a
    delivered list gives -1 counts for that stream alone."""
    full_lists, full = stereo_run(pkg, 3)[2]
    n0, n2 = len(full_lists[0]), len(full_lists[2])
    cap = (n0 + n2) // 2
    assert 6 < n2 < cap < n0
    g, lists = one_step(pkg, cap)
    res = g.postFinishDevice(0, want_lists=True, list_cap=CAP, strict=False, dense=("counts", "lists"))
    g.close()
    assert res["rc"] == pkg.VH_ERR_CAPACITY
    check_refused(res, 0)
    check_stereo_step(pkg, 3, lists, res, "truncated", streams=(1, 2))
    for key in ("voted", "flags", "inliers", "src_pos"):
        assert res[key][2].tobytes() == full[key][2].tobytes() and len(res[key][1]) == 0, key
    assert res["tr_refit"][2].tobytes() == full["tr_refit"][2].tobytes() and res["tr"][2].tobytes() == full["tr"][2].tobytes()
    # the flip stack
    lib = pkg._lib()
    assert lib.vh_debug_vote_stack_slots(4) == pkg.VH_OK
    try:
        g, lists = one_step(pkg, CAP)
        res = g.postFinishDevice(0, want_lists=True, list_cap=CAP, strict=False, dense=("counts", "lists"))
        g.close()
    finally:
        assert lib.vh_debug_vote_stack_slots(0) == pkg.VH_OK
    assert res["rc"] == pkg.VH_ERR_UNSUPPORTED
    refused = [s for s in range(S) if res["voted_counts"][s] < 0]
    assert refused and 1 not in refused, refused
    for s in refused:
        check_refused(res, s)
    for s in set(range(S)) - set(refused):
        for key in ("voted", "flags", "inliers", "src_pos"):
            assert res[key][s].tobytes() == full[key][s].tobytes(), (key, s)
        assert res["tr_refit"][s].tobytes() == full["tr_refit"][s].tobytes()
    # output arrays shorter than stream 0's list, longer than stream 2's
    g, lists = one_step(pkg, CAP)
    res = g.postFinishDevice(0, list_cap=cap, strict=False, dense=("counts", "lists"))
    g.close()
    assert res["rc"] == pkg.VH_ERR_CAPACITY and res["voted_counts"][0] == -1 and res["inlier_counts"][0] == -1
    assert res["ok_refit"][0] == full["ok_refit"][0] and res["tr_refit"].tobytes() == full["tr_refit"].tobytes()
    for key in ("voted", "flags", "inliers", "src_pos"):
        assert res[key][2].tobytes() == full[key][2].tobytes() and len(res[key][0]) == 0, key


@pytest.mark.gpu
def test_gpu_rules_and_failed_allocation(pkg, gpu):
    """Case 4: the mode cannot change while steps are in flight; mode 2 with the mono estimator and mode 1 without an
    estimator are VH_ERR_INVALID_ARG; asking for tr_refit in mode 1 is VH_ERR_STATE and leaves the step to be finished;
    the plain postFinishDevice in mode 3 returns the mode-0 dict; a refused allocation in the begin call is VH_ERR_HIP,
    leaves the bytes as they were, and the repeated call gives what an undisturbed one gives."""
    fr, dims = frames_of(pkg), dims_of(pkg)
    e, m = ego_of(pkg), mono_of(pkg)
    r3, r8 = draws(3), draws(8)
    inv, state = pkg.VH_ERR_INVALID_ARG, pkg.VH_ERR_STATE
    g = pkg.StreamGroup(S, pkg.Params.default())
    g.postDeviceConfig(2, 2, 16)
    for mode in (-1, 4):
        expect(pkg, inv, lambda: g.postDeviceDense(mode))
    g.postDeviceDense(2)
    for t in range(3):
        push(g, fr, t, dims)
    g.matchFeatures(QUAD)
    expect(pkg, inv, lambda: g.postBeginDevice(CAP, 2, 50.0, 50.0, mono=m, rand8=r8[2]))
    g.postDeviceDense(1)
    expect(pkg, inv, lambda: g.postBeginDevice(CAP, 2, 50.0, 50.0))
    g.debugFailNextAlloc()
    expect(pkg, pkg.VH_ERR_HIP, lambda: g.postBeginDevice(CAP, 2, 50.0, 50.0, ego=e, rand3=r3[2], want_lists=True))
    bytes1 = g.deviceBytes()                              # the batch's own blocks exist, the refused dense block does not
    lists = [g.getMatches(s) for s in range(S)]
    g.postBeginDevice(CAP, 2, 50.0, 50.0, ego=e, rand3=r3[2], want_lists=True)   # the repeated call
    assert 53 * CAP * 2 * S <= g.deviceBytes() - bytes1 < 56 * CAP * 2 * S   # 53 bytes per record slot of 2 x 3 lists and little else
    expect(pkg, state, lambda: g.postDeviceDense(3))      # a step is in flight
    expect(pkg, state, lambda: g.postFinishDevice(0, want_lists=True, list_cap=CAP, dense=("counts", "refit")))
    res = g.postFinishDevice(0, want_lists=True, list_cap=CAP, dense=("counts", "lists"))   # the step is still there
    check_stereo_step(pkg, 1, lists, res, "after the refused calls")
    want = stereo_run(pkg, 1)[2][1]
    same_base(res, want, "repeated begin")
    assert [x.tobytes() for x in res["flags"]] == [x.tobytes() for x in want["flags"]]
    g.postDeviceDense(3)                                  # nothing in flight any more
    g.matchFeatures(QUAD)
    g.postBeginDevice(CAP, 2, 50.0, 50.0, ego=e, rand3=r3[2], want_lists=True)
    plain = g.postFinishDevice(0, want_lists=True, list_cap=CAP)
    assert sorted(plain) == ["counts", "lists", "n_inliers", "ok", "rc", "tr"]
    same_base(plain, stereo_run(pkg, 0)[2][1], "plain finish in mode 3")
    g.close()


@pytest.mark.gpu
def test_gpu_off_state(pkg, gpu):
    """Case 5: a group that never calls postDeviceDense and one that sets mode 0 hold the same bytes, give the same
    results and record no inlier_* / motion_refit / post_dense_gate scope; a mode-3 group records them and holds more."""
    fr, dims = frames_of(pkg), dims_of(pkg)
    seen = {}
    for name, mode in (("never", None), ("zero", 0), ("three", 3)):
        g = pkg.StreamGroup(S, pkg.Params.default())
        g.profileEnable(True)
        g.postDeviceConfig(1, 2, 16)
        if mode is not None:
            g.postDeviceDense(mode)
        for t in range(3):
            push(g, fr, t, dims)
        g.matchFeatures(QUAD)
        g.postBeginDevice(CAP, 2, 50.0, 50.0, ego=ego_of(pkg), rand3=draws(3)[2], want_lists=True)
        res = g.postFinishDevice(0, want_lists=True, list_cap=CAP)
        g.synchronize()
        scopes = {k: g.profileRead(k)[1] for k in ("inlier_flag", "inlier_flag_mono", "inlier_compact", "motion_refit", "post_dense_gate")}
        seen[name] = (g.deviceBytes(), res, scopes)
        g.close()
    assert seen["never"][0] == seen["zero"][0] < seen["three"][0]
    same_base(seen["never"][1], seen["zero"][1], "off"); same_base(seen["never"][1], seen["three"][1], "mode 3, plain finish")
    same_base(seen["never"][1], stereo_run(pkg, 0)[2][1], "one step per batch against two")
    assert not any(seen["never"][2].values()) and not any(seen["zero"][2].values()), seen
    assert seen["three"][2] == {"inlier_flag": 2, "inlier_flag_mono": 0, "inlier_compact": 2, "motion_refit": 1, "post_dense_gate": 1}


@pytest.mark.gpu
def test_gpu_sequence_handle(pkg, gpu):
    """Case 6: a sequence handle, chunks of 4 and 2 frames, mode 3: the rows with a pair are held to the stateless
    entries as in case 1, the rows without one come out empty with ok = 0."""
    dims = dims_of(pkg)
    fr = frames_of(pkg)[0]
    g = pkg.SequenceGroup(4, pkg.Params.default())
    g.postDeviceConfig(1, 2, 16)
    g.postDeviceDense(3)
    e = ego_of(pkg)
    rnd = np.random.default_rng(12).integers(0, 2 ** 31 - 1, (2, 4, 50, 3)).astype(np.int32)
    F, started = 0, 0
    for k, n in enumerate((4, 2)):
        g.pushBack(np.stack([fr[t][0] for t in range(F, F + n)]), np.stack([fr[t][1] for t in range(F, F + n)]), dims)
        g.matchFeatures(QUAD)
        rec, counts = g.getMatchesAll()
        lists = [rec[r, :counts[r]].copy() for r in range(4)]
        g.postBeginDevice(CAP, 2, 50.0, 50.0, ego=e, rand3=rnd[k], want_lists=True)
        res = g.postFinishDevice(0, want_lists=True, list_cap=CAP, dense=("counts", "lists"))
        assert res["rc"] == pkg.VH_OK
        check_stereo_step(pkg, 3, lists, res, f"sequence chunk {k}")
        rows = [r for r in range(n) if F + r >= 1]
        for r in range(4):
            if r in rows:
                assert res["voted_counts"][r] > TILE and res["ok"][r], (k, r)
            else:
                assert res["voted_counts"][r] == 0 and res["inlier_counts"][r] == 0 and not res["ok_refit"][r] and res["n_updates"][r] == 0, (k, r)
        started += int((res["n_updates"] >= 1).sum())
        F += n
    assert started >= 4
    g.close()


@pytest.mark.gpu
def test_child_checking_build(pkg, gpu):
    """Case 7: cases 1 and 2 once more on libviso_hip_check.so (-DVH_CHECK)."""
    assert os.path.exists(pkg.CHECK_LIB_PATH), "build() makes it"
    env = dict(os.environ, VISO_HIP_LIB=pkg.CHECK_LIB_PATH)
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-q", "-x", "-m", "gpu", "-k", "quad_stereo_chain or flow_mono_chain"],
                       env=env, capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "4 passed" in r.stdout and " skipped" not in r.stdout, r.stdout[-2000:]
    assert "VH_CHECK" not in r.stderr
