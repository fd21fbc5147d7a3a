"""The covariance, the mono refit and the mono pose as stages of the device post chain:
vh_group_post_device_tail / vh_group_post_finish_device_tail / vh_group_post_device_shape.  Everything the tail delivers
is held to code that existed before it: the voted and inlier lists the chain hands out through vh_post_dense are fed to
the stateless entries (motion_covariance, refit_model_mono, motion_inliers_mono, pose_mono), whose bytes the tail must
repeat -- the kernels are the same and the order of their sums is fixed by N -- and to the restatements of
tests/cov_oracle.py, mono_refit_oracle.py, mono_pose_oracle.py and mono_refine_oracle.py under those files' own bounds.

Frames, streams and the ring follow tests/test_post_dense.py: 240 x 120, S = 3 with an empty and a short stream, 2 steps
x 2 batches over six steps -- with pixel noise and the sub-pixel fit, and for the mono cases two planes instead of one
(frames_of, mono_frames_of and params_of say why, with the figures measured without them).  Those frames give voted lists
of about 1 770 records, four LDS tiles of 512 in the pose's rank / vote kernels; the noise costs matches, and the lists
here are shorter: voted lists longer than one classification tile of 1 024 (asserted in the sequence case), inlier lists
of 320 .. 1 300 records (measured on an MI355X), so the rank / vote kernels make up to three trips, not four.  The paths
a fourth trip would take are those of the second and third: the loop over tiles, a partly filled last tile.

The restatements are run on steps 2 and 5 of the six (they take a second per list); the stateless entries on all of them.
A deviation of the stateless kernels from the restatements that showed on the lists of steps 1, 3, 4 or 6 alone would
not be seen here: those steps rest on byte equality with the stateless entries, which their own test files hold to the
restatements.

The conditions that keep the cases from passing vacuously are asserted on what the stateless entries return.
"""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import cov_oracle as co
import mono_inlier_oracle as moo
import mono_pose_oracle as mp
import mono_refine_oracle as mq
import mono_refit_oracle as mr
import test_mono_pose_refined as tq   # its yardstick: D_REF, differences
import test_mono_refit as tr_         # its yardstick: MARGIN, yardstick()
import test_motion_cov as tc          # its yardstick: MARGIN, yardstick()
import test_post_dense as pd
from conftest import ROOT

SYMBOLS = ("vh_group_post_device_tail", "vh_group_post_device_shape", "vh_group_post_finish_device_tail")
FIELDS = ("cov", "ssr", "ok_cov", "model_refit", "ok_model", "w", "tr_pose", "ok_pose", "pose", "refine")
S, T, CAP = pd.S, pd.T, pd.CAP
FLOW, QUAD = pd.FLOW, pd.QUAD
COV, REFIT, POSE, REFINE = 1, 2, 4, 8
TAIL_SCOPES = ("motion_cov", "mono_refit", "mono_pose_head", "mono_pose_tri", "mono_pose_front", "mono_pose_rank", "mono_pose_vote",
               "mono_pose_finish", "mono_pose_refine")
ORACLE_STEPS = (2, 5)             # the steps the restatements are run on
Cal, ptr, expect = pd.Cal, pd.ptr, pd.expect


NOISE = 3                         # grey levels, uniform, independent per frame and camera
_FRAMES = {}


def frames_of(pkg):
    """The frames of test_post_dense.py with pixel noise.  Those frames are exact integer pans of one canvas: every correct
    match is exact, the residuals of a fitted motion and the smallest singular values of the epipolar moment matrix are
    rounding noise (measured on them: ssr 9.7e-25 over 1 778 inliers), and a relative bound on them holds for no
    implementation.  With noise and Params.refinement = 2 the positions jitter by a fraction of a pixel, as real ones do."""
    if "f" not in _FRAMES:
        rng = np.random.default_rng(2024)
        noisy = lambda a: np.clip(a.astype(np.int32) + rng.integers(-NOISE, NOISE + 1, a.shape), 0, 255).astype(np.uint8)
        fr = [[(noisy(a), noisy(b)) for a, b in stream] for stream in pd.frames_of(pkg)]
        fr[1] = pd.frames_of(pkg)[1]   # the constant stream stays constant: an empty list
        for stream in fr:              # (the padding columns stay zero)
            for a, b in stream:
                a[:, pd.W:] = 0; b[:, pd.W:] = 0
        _FRAMES["f"] = fr
    return _FRAMES["f"]


def mono_frames_of(pkg):
    """The mono cases' frames: TWO fronto-parallel planes under one sideways translation -- the upper half of every image
    pans by (5, 1) px per frame over one canvas, the lower half by (10, 2) px over another (a plane at half the depth) --
    with the pixel noise of frames_of.  The frames of test_post_dense.py show one plane, and the epipolar geometry of a
    planar scene is degenerate: the 9 x 9 moment matrix has three small singular values, F is not determined by the data
    and two correct implementations differ in it (measured on them: F 2.4e-02 from the wider restatement against a bound
    of 9.3e-11).  With x' = x + d e for two values of d, x^T F x = 0 and e^T F x = 0 for every x: F = [e]x alone.
    Streams as there: stream 1 constant, stream 2 a short list -- textured on 45 % of its width, here the left 22 % and the
    right 23 %, both planes in each, so that its field of view is as wide as stream 0's."""
    if "m" not in _FRAMES:
        W, H = pd.W, pd.H
        rng = np.random.default_rng(2025)
        noisy = lambda a: np.clip(a.astype(np.int32) + rng.integers(-NOISE, NOISE + 1, a.shape), 0, 255).astype(np.uint8)
        bpl = pkg.synth.bytes_per_line(W)
        fr = []
        for seed in (71, 72, 73):
            far, near = (pkg.synth.canvas(W + 64, H + 32, 3, sd) for sd in (seed, seed + 100))   # (H + 96, W + 128)
            stream = []
            for t in range(T):
                img = np.zeros((H, bpl), np.uint8)
                img[:H // 2, :W] = far[32 + t:32 + t + H // 2, 32 + 5 * t:32 + 5 * t + W]
                img[H // 2:, :W] = near[32 + 2 * t + H // 2:32 + 2 * t + H, 32 + 10 * t:32 + 10 * t + W]
                img[:, :W] = noisy(img[:, :W])
                stream.append((img, img.copy()))
            fr.append(stream)
        fr[1] = pd.frames_of(pkg)[1]
        for a, b in fr[2]:   # (a narrow field of view conditions t badly: measured 27 x D_REF['t'] on the left 45 % alone)
            a[:, int(0.22 * W):int(0.77 * W)] = 90; b[:, int(0.22 * W):int(0.77 * W)] = 90
        _FRAMES["m"] = fr
    return _FRAMES["m"]


def params_of(pkg):
    """refinement = 2, the sub-pixel fit: under 1 (whole pixels) a record is exact or off by a pixel or more, the mono
    estimator's threshold of 1e-5 keeps the exact ones alone, and their residuals are rounding noise again (measured:
    w deviates 0.18, the refined pose's ssr 4.5, relative, on the short stream)."""
    return pkg.Params.default(refinement=2)


def mono_of(pkg):
    """The mono parameters of test_post_dense.py (height 1, pitch 0) with the motion threshold opened: the synthetic frames
    pan by (5, 1) px, so the points triangulate some 45 baselines away and their median L1 distance lies near the default
    threshold of 100 -- the pose would be refused for too little motion on some steps and not on others."""
    m = pd.mono_of(pkg)
    m.motion_threshold = 1000.0
    return m


def run_group(pkg, mode, mask, mono=False, schedule=pd.SCHEDULE, group=None, steps=(2, 2)):
    """The six steps of pd.SCHEDULE on a fresh group with the tail `mask` -> {t: (the step's dense lists, finish dict)}"""
    fr, dims = mono_frames_of(pkg) if mono else frames_of(pkg), pd.dims_of(pkg)
    g = group or pkg.StreamGroup(S, params_of(pkg))
    g.postDeviceConfig(steps[0], steps[1], 16)
    g.postDeviceDense(mode)
    g.postDeviceTail(mask)
    e, m = pd.ego_of(pkg), mono_of(pkg)
    rnd = pd.draws(8 if mono else 3)
    pd.push(g, fr, 0, dims)
    lists, out = {}, {}
    for op in schedule:
        if op[0] == "b":
            t = op[1]
            pd.push(g, fr, t, dims)
            g.matchFeatures(FLOW if mono else QUAD)
            lists[t] = [g.getMatches(s) for s in range(S)]
            if mono:
                g.postBeginDevice(CAP, 2, 50.0, 50.0, mono=m, rand8=rnd[t], want_lists=True)
            else:
                g.postBeginDevice(CAP, 2, 50.0, 50.0, ego=e, rand3=rnd[t], want_lists=True)
        else:
            _, t, age = op
            out[t] = (lists[t], g.postFinishDevice(age, want_lists=True, list_cap=CAP, dense=("counts", "lists") if mode else None,
                                                   tail=() if mask else None))
    if group is None:
        g.close()
    return out


_RUNS = {}


def run_of(pkg, mode, mask, mono):
    key = (mode, mask, mono)
    if key not in _RUNS:
        _RUNS[key] = run_group(pkg, mode, mask, mono)
    return _RUNS[key]


def same_dense(a, b, what):
    """every vh_post_dense output of two finish dicts, bit for bit"""
    for k in ("voted_counts", "inlier_counts", "tr_refit", "ok_refit", "n_updates", "model"):
        assert (k in a) == (k in b), (what, k)
        if k in a:
            assert np.asarray(a[k]).tobytes() == np.asarray(b[k]).tobytes(), (what, k)
    for k in ("voted", "flags", "inliers", "src_pos"):
        assert [x.tobytes() for x in a[k]] == [x.tobytes() for x in b[k]], (what, k)


# ------------------------------------------------------------------------------------------------------------ CPU
def test_symbols_struct_layout_and_argument_errors(pkg, tmp_path):
    """The three symbols are declared, exported and mirrored; vh_post_tail is 88 bytes with pointer k at offset 8 + 8 k in the
    header's order -- the C compiler's layout equals the ctypes mirror's; a null handle is VH_ERR_INVALID_ARG under any mask;
    unknown bits and bit 8 without bit 4 are refused for the mask's sake, before the handle is looked at: the message of
    vh_last_error says so (no handle exists without a GPU, so the code alone cannot tell the two causes apart)."""
    header = open(os.path.join(ROOT, "include", "viso_hip.h")).read()
    lib = pkg._lib()
    for name in SYMBOLS:
        assert name + "(" in header and hasattr(C.CDLL(pkg.LIB_PATH), name) and name in pkg.ABI_SYMBOLS, name
    for name in ("postDeviceTail", "postDeviceShape"):
        assert name in vars(pkg.StreamGroup) and hasattr(pkg.SequenceGroup, name), name
    assert (pkg.POST_TAIL_COV, pkg.POST_TAIL_MONO_REFIT, pkg.POST_TAIL_MONO_POSE, pkg.POST_TAIL_MONO_REFINE) == (COV, REFIT, POSE, REFINE)
    for name, bit in (("COV", 1), ("MONO_REFIT", 2), ("MONO_POSE", 4), ("MONO_REFINE", 8)):
        assert f"#define VH_POST_TAIL_{name} {bit}u" in header, name
    assert tuple(n for n, _ in pkg.PostTail._fields_) == ("size", "reserved") + FIELDS
    assert C.sizeof(pkg.PostTail) == 88 and pkg.abi_version() == 1
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "viso_hip.h"\nint main(void) {\n  printf("%zu", sizeof(vh_post_tail));\n'
                   + "".join(f'  printf(" %zu", offsetof(vh_post_tail, {n}));\n' for n in ("size", "reserved") + FIELDS) + '  return 0;\n}\n')
    exe = str(tmp_path / "layout")
    subprocess.check_call(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), str(src), "-o", exe])
    got = [int(v) for v in subprocess.check_output([exe], timeout=60).decode().split()]
    assert got == [C.sizeof(pkg.PostTail)] + [getattr(pkg.PostTail, n).offset for n in ("size", "reserved") + FIELDS]
    assert got == [88, 0, 4] + [8 + 8 * k for k in range(10)]
    inv = pkg.VH_ERR_INVALID_ARG
    for mask in (0, 1, 4, 6, 12, 14, 15):
        assert lib.vh_group_post_device_tail(None, mask) == inv, mask
    for mask in (16, 8, 9, 10, 1 << 31, 32 | 4):
        lib.vh_error_string(0)   # (any call in between: the message is the last failing call's)
        assert lib.vh_group_post_device_tail(None, mask) == inv, mask
        assert b"VH_POST_TAIL" in lib.vh_last_error(), (mask, lib.vh_last_error())
    a, b = C.c_int32(0), C.c_int32(0)
    assert lib.vh_group_post_device_shape(None, C.byref(a), C.byref(b)) == inv
    t = pkg.PostTail(size=88)
    cnt = np.zeros(3, np.int32)
    assert lib.vh_group_post_finish_device_tail(None, 0, None, None, None, None, 0, ptr(cnt), None, C.byref(t)) == inv
    assert lib.vh_group_post_finish_device_tail(None, 0, None, None, None, None, 0, ptr(cnt), None, None) == inv


# ------------------------------------------------------------------------------------------------------------ GPU
def cov_pairing(mode, res):
    """-> (tr, ok) the covariance of a step in `mode` belongs to (section 4.19: the batch's final motion)"""
    if mode == 1:
        return res["tr"], res["ok"].astype(np.int32)
    return res["tr_refit"], res["ok_refit"].astype(np.int32)


@pytest.mark.gpu
@pytest.mark.parametrize("mode", [1, 2, 3])
def test_gpu_stereo_covariance(mode, pkg, gpu):
    """Case 1: modes 1, 2, 3 with COV over six steps -- cov, ssr, ok_cov byte-equal to motion_covariance on the returned
    inlier lists under the mode's pairing, within 16 d_ref / 16 d_ssr of cov_oracle's wider form; everything else bit for
    bit what a mask-0 group returns."""
    off = run_of(pkg, mode, 0, False)
    on = run_of(pkg, mode, COV, False)
    e = pd.ego_of(pkg)
    cal = Cal(reweighting=e.reweighting, **pd.CAL)
    d_ref, d_ssr = tc.yardstick()
    accepted = 0
    for t in range(1, T):
        lists, res = on[t]
        pd.same_base(res, off[t][1], (mode, t))
        same_dense(res, off[t][1], (mode, t))
        assert res["rc"] == pkg.VH_OK
        tr, ok = cov_pairing(mode, res)
        cov_w, ssr_w, ok_w = pkg.motion_covariance(e, res["inliers"], tr, ok)
        accepted += int(np.sum(ok_w))
        assert res["cov"].tobytes() == np.asarray(cov_w).tobytes() and res["ssr"].tobytes() == np.asarray(ssr_w).tobytes(), (mode, t)
        assert np.array_equal(res["ok_cov"], np.asarray(ok_w, bool)), (mode, t)
        assert not res["ok_cov"][1] and not res["cov"][1].any() and res["ssr"][1] == 0          # the empty stream
        if t not in ORACLE_STEPS:
            continue
        for s in range(S):
            ext = co.covariance_ext(res["inliers"][s], tr[s], cal, ok=bool(ok[s]))
            assert bool(ext[2]) == bool(res["ok_cov"][s]), (mode, t, s)
            if ext[2]:
                dc, ds = co.deviation(res["cov"][s], ext[0]), co.deviation_ssr(res["ssr"][s], ext[1])
                print(f"mode {mode} step {t} stream {s}: N {len(res['inliers'][s])}  ssr {res['ssr'][s]:.3e} (wider form {float(ext[1]):.3e})  cov {dc:.3e} (bound {tc.MARGIN * d_ref:.3e})  "
                      f"ssr {ds:.3e} (bound {tc.MARGIN * d_ssr:.3e})")
                assert dc <= tc.MARGIN * d_ref and ds <= tc.MARGIN * d_ssr, (mode, t, s, dc, ds)
    assert accepted >= 1, "no list of the stateless entry has ok_cov = 1"


def check_pose(pkg, oracle, m, inliers, model, ok_in, res, refine, what, restate):
    """tr_pose / ok_pose / pose (and refine) of one step against stateless pose_mono on the final inlier lists under the
    model they were classified under, and (restate) against the restatements -> (accepted poses, converged refinements)
    as the stateless entry has them."""
    want = pkg.pose_mono(m, inliers, model, ok_in, refine=refine)
    plain = pkg.pose_mono(m, inliers, model, ok_in) if refine else want
    assert res["tr_pose"].tobytes() == want[0].tobytes() and np.array_equal(res["ok_pose"], np.asarray(want[1], bool)), what
    assert res["pose"].tobytes() == want[2].tobytes(), what
    if refine:
        assert res["refine"].tobytes() == want[3].tobytes(), what
        for s in range(S):
            if want[3][s]["status"] != 0:      # a refused refinement is not a refused pose: the plain one, byte for byte
                assert res["tr_pose"][s].tobytes() == plain[0][s].tobytes() and res["pose"][s].tobytes() == plain[2][s].tobytes(), (what, s)
                assert bool(res["ok_pose"][s]) == bool(plain[1][s]), (what, s)
    else:
        assert "refine" not in res
    for s in range(S if restate else 0):
        w = (what, s)
        pm, mod, ok = inliers[s], moo.from_array(model[s]), bool(ok_in[s])
        pose, tr = res["pose"][s], res["tr_pose"][s]
        if refine:
            exp, ref = mq.refine(oracle.svd, pm, mod, m, ok=ok)
            rec = res["refine"][s]
            assert rec["status"] == ref["status"] and rec["n_updates"] == ref["n_updates"], (w, rec["status"], rec["n_updates"], ref["status"], ref["n_updates"])
            if ref["status"] == 0:
                _, ref_ld = mq.refine(oracle.svd, pm, mod, m, ok=ok, ft=tq.LD, with_tail=False)
                d = tq.differences(dict(R=pose["R"], t=pose["t"], B=rec["B"], cov=rec["cov"], ssr=rec["ssr"]), ref_ld)
                print(what, s, {q: f"{v:.2e}" for q, v in d.items()}, "in units of d_ref:", {q: f"{d[q] / tq.D_REF[q]:.1f}" for q in tq.D_REF})
                for q in tq.D_REF:
                    assert d[q] <= 16 * tq.D_REF[q], (w, q, d[q], tq.D_REF[q])
        else:
            exp = mp.pose(oracle.svd, pm, mod, m, ok=ok)
            assert pose["R"].tobytes() == np.asarray(exp["R"], np.float64).tobytes() and pose["t"].tobytes() == np.asarray(exp["t"], np.float64).tobytes(), w
            assert np.float64(pose["median"]).tobytes() == np.float64(exp["median"]).tobytes(), (w, pose["median"], exp["median"])
        print(f"{what} stream {s}: N {len(pm)}, reason {pose['reason']} (restated {exp['reason']}), n_front {pose['n_front']}, vote margin {exp['margin']}")
        assert bool(res["ok_pose"][s]) == exp["ok"] and pose["reason"] == exp["reason"], (w, pose["reason"], exp["reason"])
        assert pose["candidate"] == exp["candidate"] and pose["n_front"] == exp["n_front"] and pose["reserved_"] == 0, w
        assert np.array_equal(pose["chirality"], exp["chirality"]), (w, pose["chirality"], exp["chirality"])
        for got, ref_ in ((tr, exp["tr"]), (pose["scale"], exp["scale"]), (pose["plane"], exp["plane"])):
            assert np.allclose(got, ref_, rtol=1e-9, atol=1e-12), (w, got, ref_)
    conv = int(np.sum((want[3]["status"] == 0) & (want[3]["n_updates"] >= 1))) if refine else 0
    return int(np.sum((np.asarray(want[1]) != 0) & (want[2]["reason"] == 0))), conv


@pytest.mark.gpu
@pytest.mark.parametrize("mask", [REFIT, POSE, REFIT | POSE, POSE | REFINE, REFIT | POSE | REFINE], ids=["refit", "pose", "refit_pose", "refined", "all"])
def test_gpu_mono_tail(mask, pkg, oracle, gpu):
    """Cases 2, 3, 4: flow lists, the mono estimator, mode 1 with the refit, the pose, the refined pose and their
    combinations over six steps.  The refit is refit_model_mono's on the first classification's inliers (a mask-0 run of
    the same steps) under the returned estimator model, the classification handed out is motion_inliers_mono's under the
    refitted model, the pose is pose_mono's on the final inlier lists under the model they were classified under."""
    m = mono_of(pkg)
    off = run_of(pkg, 1, 0, True)
    on = run_of(pkg, 1, mask, True)
    d_ref, d_w, _ = tr_.yardstick(oracle)
    refitted = moved = poses = converged = 0
    for t in range(1, T):
        lists, res = on[t]
        base = off[t][1]
        what = f"mask {mask} step {t}"
        pd.same_base(res, base, what)
        assert res["rc"] == pkg.VH_OK and res["model"].tobytes() == base["model"].tobytes(), what   # d->model stays the estimator's
        assert [x.tobytes() for x in res["voted"]] == [x.tobytes() for x in base["voted"]], what
        ok = res["ok"].astype(np.int32)
        model_cls, ok_cls = res["model"], ok
        if mask & REFIT:
            model_w, ok_w, w_w = pkg.refit_model_mono(m, base["inliers"], res["model"], ok)
            assert res["model_refit"].tobytes() == model_w.tobytes() and res["w"].tobytes() == np.asarray(w_w).tobytes(), what
            assert np.array_equal(res["ok_model"], np.asarray(ok_w, bool)), what
            ok_cls, model_cls = np.asarray(ok_w, np.int32), res["model_refit"]
            fl, n_in, rec, pos = pkg.motion_inliers_mono(m, res["voted"], model_cls, ok_cls)
            for s in range(S):
                assert res["flags"][s].tobytes() == fl[s].tobytes() and res["inlier_counts"][s] == n_in[s], (what, s)
                assert res["inliers"][s].tobytes() == rec[s].tobytes() and res["src_pos"][s].tobytes() == pos[s].tobytes(), (what, s)
                if ok_w[s]:
                    refitted += 1
                    moved += int(fl[s].tobytes() != base["flags"][s].tobytes())
            assert not res["ok_model"][1] and res["model_refit"][1].tobytes() == bytes(128) and not res["w"][1].any()
            for s in range(S if t in ORACLE_STEPS else 0):
                ext = mr.refit_ext(base["inliers"][s], moo.from_array(res["model"][s]), bool(ok[s]))
                assert bool(ext[1]) == bool(res["ok_model"][s]), (what, s)
                if ext[1]:
                    dF, dw = mr.deviation_F(res["model_refit"][s]["F"], ext[3]), mr.deviation_w(res["w"][s], ext[4])
                    print(f"{what} stream {s}: N {len(base['inliers'][s])}  F {dF:.3e} (bound {tr_.MARGIN * d_ref:.3e})  w {dw:.3e} (bound {tr_.MARGIN * d_w:.3e})")
                    assert dF <= tr_.MARGIN * d_ref and dw <= tr_.MARGIN * d_w, (what, s, dF, dw)
        else:
            same_dense(res, base, what)
            assert "model_refit" not in res
        if mask & POSE:
            p, c = check_pose(pkg, oracle, m, res["inliers"], model_cls, ok_cls, res, bool(mask & REFINE), what, t in ORACLE_STEPS)
            poses += p; converged += c
            assert not res["ok_pose"][1] and res["pose"][1]["reason"] == 1 and not res["tr_pose"][1].any()
        else:
            assert "pose" not in res
    print(f"mask {mask}: lists refitted {refitted}, of them with other flags {moved}; poses accepted {poses}, refinements converged {converged}")
    if mask & REFIT:
        assert refitted >= 1 and moved >= 1
    if mask & POSE:
        assert poses >= 1
    if mask & REFINE:
        assert converged >= 1


def begin_one(pkg, g, t, mono, cap=CAP):
    """push frames 0 .. t on a fresh pair history, match, begin step t"""
    fr, dims = mono_frames_of(pkg) if mono else frames_of(pkg), pd.dims_of(pkg)
    for k in range(t + 1):
        pd.push(g, fr, k, dims)
    g.matchFeatures(FLOW if mono else QUAD)
    if mono:
        g.postBeginDevice(cap, 2, 50.0, 50.0, mono=mono_of(pkg), rand8=pd.draws(8)[t], want_lists=True)
    else:
        g.postBeginDevice(cap, 2, 50.0, 50.0, ego=pd.ego_of(pkg), rand3=pd.draws(3)[t], want_lists=True)


@pytest.mark.gpu
def test_gpu_rules_and_failed_allocation(pkg, gpu):
    """Case 5, the refusals: unknown bits and REFINE without POSE; every begin-time combination; an output the step's mask
    did not produce is VH_ERR_STATE and leaves the step to be finished; the mask cannot change while a step is in flight;
    a bad size; a refused allocation of the tail's block leaves the begin call repeatable; the shape is the configured one."""
    fr, dims = frames_of(pkg), pd.dims_of(pkg)
    e, m = pd.ego_of(pkg), mono_of(pkg)
    r3, r8 = pd.draws(3), pd.draws(8)
    inv, state = pkg.VH_ERR_INVALID_ARG, pkg.VH_ERR_STATE
    g = pkg.StreamGroup(S, params_of(pkg))
    g.postDeviceConfig(2, 2, 16)
    assert g.postDeviceShape() == (2, 2)
    for mask in (16, 8, 9, 32 | 1):
        expect(pkg, inv, lambda: g.postDeviceTail(mask))
    for t in range(3):
        pd.push(g, fr, t, dims)
    g.matchFeatures(QUAD)
    stereo = lambda: g.postBeginDevice(CAP, 2, 50.0, 50.0, ego=e, rand3=r3[2], want_lists=True)
    mono = lambda: g.postBeginDevice(CAP, 2, 50.0, 50.0, mono=m, rand8=r8[2], want_lists=True)
    none = lambda: g.postBeginDevice(CAP, 2, 50.0, 50.0)
    g.postDeviceTail(COV)
    expect(pkg, inv, stereo)                               # dense mode 0
    g.postDeviceDense(1)
    expect(pkg, inv, mono); expect(pkg, inv, none)         # COV with the mono estimator / with none
    for mask in (REFIT, POSE, POSE | REFINE, COV | REFIT):
        g.postDeviceTail(mask)
        expect(pkg, inv, stereo); expect(pkg, inv, none)   # the mono bits with the stereo estimator / with none
    g.postDeviceTail(POSE)
    g.postDeviceDense(2)
    expect(pkg, inv, mono)                                 # mode 2 refuses the mono estimator as it always did
    g.postDeviceDense(1)
    g.postDeviceTail(COV)
    bytes0 = g.deviceBytes()
    g.debugFailAllocAfter(1)                               # the dense block succeeds, the tail's is refused
    expect(pkg, pkg.VH_ERR_HIP, stereo)
    bytes1 = g.deviceBytes()
    stereo()                                               # the repeated call
    assert g.postDeviceShape() == (2, 2)
    grown = g.deviceBytes() - bytes1
    assert bytes1 > bytes0 and 300 * 2 * S <= grown <= (300 + 3 * 256) * 2 * S + 256, (bytes0, bytes1, grown)
    expect(pkg, state, lambda: g.postDeviceTail(0))        # a step is in flight
    expect(pkg, state, lambda: g.postDeviceTail(COV | POSE))
    for name in ("mono_refit", "pose", "refine"):
        expect(pkg, state, lambda: g.postFinishDevice(0, want_lists=True, list_cap=CAP, dense=("counts", "lists"), tail=(name,)))
    lib = pkg._lib()
    cnt = np.zeros(S, np.int32); tr = np.zeros((S, 6)); ok = np.zeros(S, np.int32); ni = np.zeros(S, np.int32); ssr = np.zeros(S)
    for size in (0, 4, 12, 20):
        t = pkg.PostTail(size=size, ssr=ssr.ctypes.data)
        assert lib.vh_group_post_finish_device_tail(g._h, 0, ptr(tr), ptr(ok), ptr(ni), None, 0, ptr(cnt), None, C.byref(t)) == inv, size
    res = g.postFinishDevice(0, want_lists=True, list_cap=CAP, dense=("counts", "lists"), tail=())    # the step is still there
    want = run_of(pkg, 1, COV, False)[2][1]
    pd.same_base(res, want, "after the refused calls")
    assert res["cov"].tobytes() == want["cov"].tobytes() and res["ssr"].tobytes() == want["ssr"].tobytes() and np.array_equal(res["ok_cov"], want["ok_cov"])
    # a struct that ends before a member: the member is not read (size 16: cov alone)
    g.matchFeatures(QUAD)
    stereo()
    cov = np.zeros((S, 36))
    t = pkg.PostTail(size=16, cov=cov.ctypes.data, refine=1)   # (refine lies beyond the size: a non-null garbage pointer must not matter)
    assert lib.vh_group_post_finish_device_tail(g._h, 0, ptr(tr), ptr(ok), ptr(ni), None, 0, ptr(cnt), None, C.byref(t)) == pkg.VH_OK
    assert cov.tobytes() == want["cov"].tobytes()
    # the older entries under a mask: the mask-0 results
    g.matchFeatures(QUAD)
    stereo()
    plain = g.postFinishDevice(0, want_lists=True, list_cap=CAP)
    assert sorted(plain) == ["counts", "lists", "n_inliers", "ok", "rc", "tr"]
    pd.same_base(plain, run_of(pkg, 0, 0, False)[2][1], "plain finish under a mask")
    g.close()


@pytest.mark.gpu
def test_gpu_off_state(pkg, gpu):
    """Case 5, the off state: a group that never calls postDeviceTail and one that sets mask 0 hold the same bytes, give
    the same results and record none of the tail's scopes; a group with the mono mask 2|4|8 records each once (the
    classification twice) and holds more."""
    seen = {}
    for name, mask in (("never", None), ("zero", 0), ("all", REFIT | POSE | REFINE)):
        g = pkg.StreamGroup(S, params_of(pkg))
        g.profileEnable(True)
        g.postDeviceConfig(1, 2, 16)
        g.postDeviceDense(1)
        if mask is not None:
            g.postDeviceTail(mask)
        begin_one(pkg, g, 2, True)
        assert g.postDeviceShape() == (1, 2)
        res = g.postFinishDevice(0, want_lists=True, list_cap=CAP, dense=("counts", "lists"))
        g.synchronize()
        scopes = {k: g.profileRead(k)[1] for k in TAIL_SCOPES + ("inlier_flag_mono", "inlier_compact")}
        seen[name] = (g.deviceBytes(), res, scopes)
        g.close()
    assert seen["never"][0] == seen["zero"][0] < seen["all"][0]
    pd.same_base(seen["never"][1], seen["zero"][1], "off"); same_dense(seen["never"][1], seen["zero"][1], "off")
    pd.same_base(seen["never"][1], seen["all"][1], "mask 14, dense finish")
    pd.same_base(seen["never"][1], run_of(pkg, 1, 0, True)[2][1], "one step per batch against two")
    for name in ("never", "zero"):
        assert not any(seen[name][2][k] for k in TAIL_SCOPES) and seen[name][2]["inlier_flag_mono"] == 1, seen[name][2]
    assert seen["all"][2] == dict({k: 1 for k in TAIL_SCOPES if k != "motion_cov"}, motion_cov=0, inlier_flag_mono=2, inlier_compact=2)
    # 16 bytes per record slot for the pose, and per list the records of section 4.19 (each array rounded up to 256 bytes)
    extra = seen["all"][0] - seen["zero"][0]
    assert 16 * CAP * S <= extra <= 16 * CAP * S + (148 + 972 + 288) * S + 12 * 256, extra


@pytest.mark.gpu
def test_gpu_refused_list(pkg, gpu):
    """Case 5, a list the vote refused (the sweep's flip stack shrunk to four slots, as case 3 of test_post_dense.py): zero
    tail records with ok = 0 for that stream, the other streams as an undisturbed run has them, the refusal's code."""
    lib = pkg._lib()
    for mono, mask in ((False, COV), (True, REFIT | POSE | REFINE)):
        full = run_of(pkg, 3 if not mono else 1, mask, mono)[2][1]
        assert lib.vh_debug_vote_stack_slots(4) == pkg.VH_OK
        try:
            g = pkg.StreamGroup(S, params_of(pkg))
            g.postDeviceConfig(1, 2, 16)
            g.postDeviceDense(1 if mono else 3)
            g.postDeviceTail(mask)
            begin_one(pkg, g, 2, mono)
            res = g.postFinishDevice(0, want_lists=True, list_cap=CAP, strict=False, dense=("counts", "lists"), tail=())
            g.close()
        finally:
            assert lib.vh_debug_vote_stack_slots(0) == pkg.VH_OK
        assert res["rc"] == pkg.VH_ERR_UNSUPPORTED
        refused = [s for s in range(S) if res["voted_counts"][s] < 0]
        assert refused and 1 not in refused, refused
        keys = [k for k in FIELDS if k in res]
        assert keys == [k for k in FIELDS if k in full] and keys
        for k in keys:
            for s in range(S):
                if s in refused:
                    assert not np.asarray(res[k][s]).tobytes().strip(b"\0"), (k, s)
                else:
                    assert np.asarray(res[k][s]).tobytes() == np.asarray(full[k][s]).tobytes(), (k, s)


@pytest.mark.gpu
def test_gpu_sequence_handle(pkg, gpu):
    """Case 6: a sequence handle, chunks of 4 and 2 frames, the mono mask 2|4|8: every row is byte-equal to the group form of
    its pair (a group of one stream stepped over the same frames with the row's draws); the rows without a pair come out
    empty with ok = 0."""
    mask = REFIT | POSE | REFINE
    dims = pd.dims_of(pkg)
    fr = mono_frames_of(pkg)[0]
    m = mono_of(pkg)
    rnd = np.random.default_rng(12).integers(0, 2 ** 31 - 1, (2, 4, 50, 8)).astype(np.int32)
    g = pkg.SequenceGroup(4, params_of(pkg))
    one = pkg.StreamGroup(1, params_of(pkg))
    for h in (g, one):
        h.postDeviceConfig(1, 2, 16)
        h.postDeviceDense(1)
        h.postDeviceTail(mask)
    one.pushBack(fr[0][0][None], fr[0][1][None], dims)
    F, pairs = 0, 0
    for k, n in enumerate((4, 2)):
        g.pushBack(np.stack([fr[t][0] for t in range(F, F + n)]), np.stack([fr[t][1] for t in range(F, F + n)]), dims)
        g.matchFeatures(FLOW)
        g.postBeginDevice(CAP, 2, 50.0, 50.0, mono=m, rand8=rnd[k], want_lists=True)
        res = g.postFinishDevice(0, want_lists=True, list_cap=CAP, dense=("counts", "lists"), tail=())
        assert res["rc"] == pkg.VH_OK
        for r in range(4):
            if r >= n or F + r < 1:
                assert res["voted_counts"][r] == 0 and not res["ok_model"][r] and not res["ok_pose"][r] and res["refine"][r]["status"] == 1, (k, r)
                assert res["model_refit"][r].tobytes() == bytes(128) and not res["tr_pose"][r].any(), (k, r)
                continue
            one.pushBack(fr[F + r][0][None], fr[F + r][1][None], dims)
            one.matchFeatures(FLOW)
            one.postBeginDevice(CAP, 2, 50.0, 50.0, mono=m, rand8=rnd[k][r:r + 1], want_lists=True)
            want = one.postFinishDevice(0, want_lists=True, list_cap=CAP, dense=("counts", "lists"), tail=())
            pairs += 1
            assert res["voted_counts"][r] == want["voted_counts"][0] > pd.TILE and res["tr"][r].tobytes() == want["tr"][0].tobytes(), (k, r)
            for key in tuple(k_ for k_ in FIELDS if k_ in res) + ("model", "inlier_counts"):
                assert np.asarray(res[key][r]).tobytes() == np.asarray(want[key][0]).tobytes(), (k, r, key)
            for key in ("voted", "flags", "inliers", "src_pos"):
                assert res[key][r].tobytes() == want[key][0].tobytes(), (k, r, key)
        F += n
    assert pairs == 5
    g.close(); one.close()


@pytest.mark.gpu
def test_child_checking_build(pkg, gpu):
    """Case 7: cases 1 and 3 once more on libviso_hip_check.so (-DVH_CHECK)."""
    assert os.path.exists(pkg.CHECK_LIB_PATH), "build() makes it"
    env = dict(os.environ, VISO_HIP_LIB=pkg.CHECK_LIB_PATH)
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-q", "-x", "-m", "gpu", "-k",
                        "stereo_covariance or mono_tail and (pose or refit_pose)"],
                       env=env, capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "5 passed" in r.stdout and " skipped" not in r.stdout, r.stdout[-2000:]
    assert "VH_CHECK" not in r.stderr
