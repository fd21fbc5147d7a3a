"""Multi-stage matching (vh_set_multi_stage_matching): sparse pass, prior ranges, ranged
dense search.

The GPU's lists must equal tests/multistage_oracle.py's restatement of the contract byte for byte (float fields bit for
bit): the stateless vh_match_ranged, a lone matcher with the switch on, groups, the asynchronous download, the device
post chain and the estimator; with the switch off a multi_stage = 1 handle returns today's single-stage lists."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import multistage_oracle as mo
import refine_oracle as ro
from conftest import ROOT

W, H = 320, 160
F32 = np.float32
NEW_SYMBOLS = ("vh_set_multi_stage_matching", "vh_group_set_multi_stage_matching", "vh_get_sparse_matches",
               "vh_group_get_sparse_matches", "vh_prior_statistics", "vh_match_ranged")
NEED = {0: (0, 2), 1: (2, 3), 2: (0, 1, 2, 3)}


# ------------------------------------------------------------------ scenes and the conditions they must meet
def scene(pkg, T=2, w=W, h=H, seed=7, disparity=6, blur=3, blank=0.55):
    """Stereo frames whose right-hand part is featureless: some statistics bins see no sparse match at all."""
    out = []
    for l, r in pkg.synth.stereo_sequence(w, h, T, disparity=disparity, blur=blur, seed=seed):
        l, r = l.copy(), r.copy()
        l[:, int(w * blank):] = 90
        r[:, int(w * blank):] = 90
        out.append((l, r))
    return out


def images_of(method, prev, cur):
    imgs = (prev[0], prev[1], cur[0], cur[1])
    return [imgs[k] if k in NEED[method] else None for k in range(4)]


def check_not_vacuous(po, method, r):
    """The conditions of the issue, asserted on the oracle's output: the voted sparse list is non-empty, at least one
    statistics bin is narrower than +-R and at least one is empty, the pass-2 list is non-empty."""
    R = po.match_radius
    nst = len(mo.STAGES[method])
    rg = r["ranges"][:, :nst]
    assert len(r["sparse"]) > 0 and len(r["dense"]) > 0
    assert ((rg[:, :, 1] - rg[:, :, 0]) < 2 * R).any(), "no bin narrower than +-R"
    assert ((rg[:, :, 0::2] == -R) & (rg[:, :, 1::2] == R)).all(axis=(1, 2)).any(), "no empty bin"


# ------------------------------------------------------------------ CPU
def test_symbols_declared_exported_mirrored(pkg):
    header = open(os.path.join(ROOT, "include", "viso_hip.h")).read()
    lib = C.CDLL(pkg.LIB_PATH)
    for name in NEW_SYMBOLS:
        assert name + "(" in header, name
        assert hasattr(lib, name), name
        assert name in pkg.ABI_SYMBOLS, name
    assert callable(pkg.prior_statistics) and callable(pkg.match_ranged)
    assert callable(pkg.Matcher.setMultiStageMatching) and callable(pkg.StreamGroup.setMultiStageMatching)
    assert callable(pkg.Matcher.getSparseMatches) and callable(pkg.StreamGroup.getSparseMatches)
    shim = open(os.path.join(ROOT, "include", "viso_hip_matcher.hpp")).read()
    assert "setMultiStageMatching" in shim and "vh_set_multi_stage_matching" in shim


def test_null_and_bad_arguments_need_no_gpu(pkg):
    lib = pkg._lib()
    p = pkg.Params.default(multi_stage=1)
    dims = (C.c_int32 * 3)(W, H, W)
    pm = np.zeros(3, pkg.P_MATCH_DTYPE)
    P = pm.ctypes.data_as(C.c_void_p)
    rg = np.zeros((7 * 4, 4, 4), F32)
    Rp = rg.ctypes.data_as(C.c_void_p)
    n = C.c_int32(0)
    assert lib.vh_set_multi_stage_matching(None, 1) == pkg.VH_ERR_INVALID_ARG
    assert lib.vh_group_set_multi_stage_matching(None, 0) == pkg.VH_ERR_INVALID_ARG
    assert lib.vh_get_sparse_matches(None, None, 0, C.byref(n)) == pkg.VH_ERR_INVALID_ARG
    assert lib.vh_group_get_sparse_matches(None, 0, None, 0, C.byref(n)) == pkg.VH_ERR_INVALID_ARG
    assert lib.vh_prior_statistics(None, dims, 0, P, 3, Rp) == pkg.VH_ERR_INVALID_ARG
    assert lib.vh_prior_statistics(C.byref(p), None, 0, P, 3, Rp) == pkg.VH_ERR_INVALID_ARG
    assert lib.vh_prior_statistics(C.byref(p), dims, 0, None, 3, Rp) == pkg.VH_ERR_INVALID_ARG
    assert lib.vh_prior_statistics(C.byref(p), dims, 0, P, -1, Rp) == pkg.VH_ERR_INVALID_ARG
    assert lib.vh_prior_statistics(C.byref(p), dims, 3, P, 3, Rp) == pkg.VH_ERR_INVALID_ARG
    assert lib.vh_prior_statistics(C.byref(p), dims, 0, P, 3, None) == pkg.VH_ERR_INVALID_ARG
    assert lib.vh_prior_statistics(C.byref(pkg.Params.default(match_binsize=0)), dims, 0, P, 3, Rp) == pkg.VH_ERR_UNSUPPORTED
    assert lib.vh_prior_statistics(C.byref(p), (C.c_int32 * 3)(0, H, W), 0, P, 3, Rp) == pkg.VH_ERR_INVALID_ARG
    bad = pm.copy()
    bad["u1p"][1] = np.nan
    assert lib.vh_prior_statistics(C.byref(p), dims, 0, bad.ctypes.data_as(C.c_void_p), 3, Rp) == pkg.VH_ERR_INVALID_ARG
    assert lib.vh_prior_statistics(C.byref(p), dims, 0, None, 0, Rp) == pkg.VH_OK  # no records: every bin +-R
    assert (rg[:, :, 0::2] == -200).all() and (rg[:, :, 1::2] == 200).all()
    f = np.zeros((4, 12), np.int32)
    Fp = f.ctypes.data_as(C.c_void_p)
    args = (Fp, 0, Fp, 0, Fp, 0, Fp, 0)
    assert lib.vh_match_ranged(None, 0, dims, 0, *args, Rp, P, 3, C.byref(n)) == pkg.VH_ERR_INVALID_ARG
    assert lib.vh_match_ranged(C.byref(p), 0, None, 0, *args, Rp, P, 3, C.byref(n)) == pkg.VH_ERR_INVALID_ARG
    assert lib.vh_match_ranged(C.byref(p), 0, dims, 0, *args, None, P, 3, C.byref(n)) == pkg.VH_ERR_INVALID_ARG
    assert lib.vh_match_ranged(C.byref(p), 0, dims, 0, *args, Rp, P, 3, None) == pkg.VH_ERR_INVALID_ARG
    assert lib.vh_match_ranged(C.byref(p), 0, dims, 3, *args, Rp, P, 3, C.byref(n)) == pkg.VH_ERR_INVALID_ARG
    assert lib.vh_match_ranged(C.byref(pkg.Params.default(nms_n=0)), 0, dims, 0, *args, Rp, P, 3, C.byref(n)) == pkg.VH_ERR_UNSUPPORTED


def test_oracle_with_full_ranges_equals_the_pinned_matching(pkg, ob, oracle):
    """With every range at +-R use_prior changes nothing: the restatement equals oracle.matching byte for byte."""
    for seed, kw in ((7, {}), (3, dict(match_binsize=30, match_radius=60)), (9, dict(half_resolution=1, nms_n=1))):
        po = ob.Params.default(**kw)
        dims = [W, H, pkg.synth.bytes_per_line(W)]
        fr = scene(pkg, 2, seed=seed)
        sets = [oracle.compute_features(po, I, dims)[1] for I in (fr[0][0], fr[0][1], fr[1][0], fr[1][1])]
        for method in (0, 1, 2):
            use = [sets[k] if k in NEED[method] else None for k in range(4)]
            want = oracle.matching(po, dims, method, *use)
            got = mo.ranged_matching(po, dims, method, *use, mo.full_ranges(po, dims))
            assert len(want) > 50 and got.tobytes() == want.tobytes(), (kw, method)
        # an empty candidate set: no matches, as the pinned oracle
        assert len(mo.ranged_matching(po, dims, 0, None, None, sets[2], None, mo.full_ranges(po, dims))) == 0


def record(pkg, **kw):
    m = np.zeros(1, pkg.P_MATCH_DTYPE)
    for f in ("u1p", "v1p", "u2p", "v2p", "u1c", "v1c", "u2c", "v2c"):
        m[f] = -1
    for k, v in kw.items():
        m[k] = v
    return m


def test_statistics_on_hand_made_lists(pkg, ob):
    po = ob.Params.default()  # binsize 50, radius 200
    dims = [320, 160, 320]    # 7 x 4 bins
    ubn = 7
    R = 200
    # one flow observation in bin (3, 1): d = 0 -> 20 wide; its 3 x 3 neighbourhood sees it, nothing else does
    one = record(pkg, u1c=170, v1c=70, u1p=175, v1p=68)
    rg = mo.statistics(po, dims, 0, one)
    assert rg.shape == (28, 4, 4)
    for vb in range(4):
        for ub in range(7):
            got = rg[vb * ubn + ub]
            if 2 <= ub <= 4 and 0 <= vb <= 2:
                assert got[0].tolist() == [-5, 15, -12, 8] and got[1].tolist() == [-15, 5, -8, 12], (ub, vb)
            else:
                assert got[0].tolist() == [-R, R, -R, R] and got[1].tolist() == [-R, R, -R, R], (ub, vb)  # empty: unwidened
            assert got[2].tolist() == [-R, R, -R, R] and got[3].tolist() == [-R, R, -R, R]                # flow has two stages
    # d = 7 -> widened by ceil(13 / 2) = 7 on both sides (21 wide); d >= 20 untouched
    two = np.concatenate([one, record(pkg, u1c=160, v1c=60, u1p=172, v1p=88)])  # du = 5, 12; dv = -2, 28
    rg = mo.statistics(po, dims, 0, two)[1 * ubn + 3]
    assert rg[0].tolist() == [5 - 7, 12 + 7, -2, 28] and rg[1].tolist() == [-12 - 7, -5 + 7, -28, 2]
    assert rg[0][1] - rg[0][0] == 21
    # spreading is clamped at the borders: a match in the corner bin (0, 0) reaches bins (0..1, 0..1) only
    corner = record(pkg, u1c=10, v1c=10, u1p=10, v1p=10)
    rg = mo.statistics(po, dims, 0, corner)
    hit = {b for b in range(28) if rg[b, 0, 0] != -R}
    assert hit == {0, 1, ubn, ubn + 1}
    far = record(pkg, u1c=319, v1c=159, u1p=300, v1p=150)  # the last bins hold the remainder of the image
    hit = {b for b in range(28) if mo.statistics(po, dims, 0, far)[b, 0, 0] != -R}
    assert hit == {2 * ubn + 5, 2 * ubn + 6, 3 * ubn + 5, 3 * ubn + 6}
    # stereo: v-ranges [-10, 10]; reference point (u1c, v1c)
    st = record(pkg, u1c=170, v1c=70, u2c=160, v2c=70)
    rg = mo.statistics(po, dims, 1, st)[1 * ubn + 3]
    assert rg[0].tolist() == [-20, 0, -10, 10] and rg[1].tolist() == [0, 20, -10, 10]
    # quad: the reference point is (u1p, v1p), not (u1c, v1c)
    q = record(pkg, u1p=20, v1p=20, u2p=12, v2p=20, u1c=300, v1c=150, u2c=290, v2c=151)
    rg = mo.statistics(po, dims, 2, q)
    hit = {b for b in range(28) if rg[b, 0, 0] != -R}
    assert hit == {0, 1, ubn, ubn + 1}
    assert rg[0, 0].tolist() == [-18, 2, -10, 10]                     # 1p -> 2p: du = -8
    assert rg[0, 1].tolist() == [278 - 10, 278 + 10, 131 - 10, 131 + 10]  # 2p -> 2c
    assert rg[0, 2].tolist() == [0, 20, -10, 10]                      # 2c -> 1c: du = 10
    assert rg[0, 3].tolist() == [-280 - 10, -280 + 10, -130 - 10, -130 + 10]  # 1c -> 1p


def test_prior_statistics_equals_the_numpy_statistics(pkg, ob, oracle):
    """vh_prior_statistics runs on the host: exactly the restatement, on real voted sparse lists and on random ones."""
    dims = [W, H, pkg.synth.bytes_per_line(W)]
    fr = scene(pkg, 2, seed=7)
    for kw in ({}, dict(match_binsize=30, match_radius=60), dict(match_binsize=64, match_radius=37)):
        p, po = pkg.Params.default(multi_stage=1, **kw), ob.Params.default(multi_stage=1, **kw)
        for method in (0, 1, 2):
            r = mo.multistage(ob, oracle, po, dims, method, images_of(method, fr[0], fr[1]))
            assert len(r["sparse"]) > 20
            got = pkg.prior_statistics(p, dims, method, r["sparse"])
            assert got.tobytes() == r["ranges"].tobytes(), (kw, method)
    rng = np.random.default_rng(5)
    p, po = pkg.Params.default(), ob.Params.default()
    for method in (0, 1, 2):
        pm = np.zeros(40, pkg.P_MATCH_DTYPE)
        for f in ("u1p", "u2p", "u1c", "u2c"):
            pm[f] = rng.integers(0, W, 40)
        for f in ("v1p", "v2p", "v1c", "v2c"):
            pm[f] = rng.integers(0, H, 40)
        assert pkg.prior_statistics(p, dims, method, pm).tobytes() == mo.statistics(po, dims, method, pm).tobytes(), method


# ------------------------------------------------------------------ GPU
CONFIGS = (
    (7, {}),
    (3, dict(match_binsize=30, match_radius=60)),
    (5, dict(nms_n=3, match_binsize=64, match_radius=37)),
    (9, dict(half_resolution=1, nms_n=1)),
)


@pytest.mark.gpu
def test_match_ranged_against_the_oracle(pkg, ob, oracle, gpu):
    """Ranges from real sparse lists and random integer ranges (empty windows included), methods 0/1/2."""
    dims = [W, H, pkg.synth.bytes_per_line(W)]
    rng = np.random.default_rng(23)
    differs = 0
    shared = 0
    for seed, kw in CONFIGS:
        p, po = pkg.Params.default(multi_stage=1, **kw), ob.Params.default(multi_stage=1, **kw)
        fr = scene(pkg, 2, seed=seed)
        for method in (0, 1, 2):
            r = mo.multistage(ob, oracle, po, dims, method, images_of(method, fr[0], fr[1]))
            check_not_vacuous(po, method, r)
            got = pkg.match_ranged(p, dims, method, r["ranges"], *r["dense_sets"])
            assert got.tobytes() == r["dense"].tobytes(), (kw, method, len(got), len(r["dense"]))
            single = oracle.matching(po, dims, method, *r["dense_sets"])
            differs += got.tobytes() != single.tobytes()
            # with full ranges: today's list
            assert pkg.match_ranged(p, dims, method, mo.full_ranges(po, dims), *r["dense_sets"]).tobytes() == single.tobytes()
            # random integer ranges, a part of them empty (min > max): min_ind = 0 must come out as in the reference
            # (the learned ranges moved and resized at random -- windows that miss the true displacement by a few
            #  pixels --, every eighth window emptied, a few bins with windows nowhere near the motion)
            nb = len(r["ranges"])
            rnd = r["ranges"].copy()
            rnd[:, :, 0::2] += rng.integers(-9, 6, (nb, 4, 2)).astype(F32)
            rnd[:, :, 1::2] += rng.integers(-6, 9, (nb, 4, 2)).astype(F32)
            empty = rng.random((nb, 4, 2)) < 0.125
            rnd[:, :, 1::2] = np.where(empty, rnd[:, :, 0::2] - rng.integers(1, 5, (nb, 4, 2)).astype(F32), rnd[:, :, 1::2])
            wild = rng.random(nb) < 0.1
            rnd[wild] = rng.integers(-40, 40, (int(wild.sum()), 4, 4)).astype(F32)
            assert (rnd[:, :, 1::2] < rnd[:, :, 0::2]).any() and (rnd == np.round(rnd)).all()
            trace = {}
            want = mo.ranged_matching(po, dims, method, *r["dense_sets"], rnd, trace)
            shared += sum(len(v) > 1 for v in trace.values())
            got = pkg.match_ranged(p, dims, method, rnd, *r["dense_sets"])
            assert len(want) > 0 and got.tobytes() == want.tobytes(), (kw, method, len(got), len(want))
    assert differs > 0, "the ranged lists never differ from the single-stage ones: the scenes show nothing"
    assert shared > 0, "no query was reached by two drivers from different statistics bins"


def expected_lists(ob, oracle, po, dims, method, prev, cur, refinement=0):
    r = mo.multistage(ob, oracle, po, dims, method, images_of(method, prev, cur))
    check_not_vacuous(po, method, r)
    dense = r["dense"]
    if refinement:
        dense = ro.refine(dense, method, refinement, dims, (prev[0], prev[1], cur[0], cur[1]), oracle.filters)
    return r, dense


@pytest.mark.gpu
def test_lone_matcher_with_the_switch_on(pkg, ob, oracle, gpu):
    """Several pushes, a replace and a change of dims; the sparse getter against pass 1; refinement 1 and 2."""
    for refinement, kw in ((0, {}), (1, dict(nms_n=3)), (2, dict(half_resolution=1, nms_n=1)), (0, dict(match_binsize=30, match_radius=60))):
        p = pkg.Params.default(multi_stage=1, refinement=refinement, **kw)
        po = ob.Params.default(multi_stage=1, refinement=refinement, **kw)
        m = pkg.Matcher(p, outlier_removal=False)
        m.setMultiStageMatching(True)
        assert len(m.getSparseMatches()) == 0
        for (w, h) in ((W, H), (W + 37, H + 9)):
            dims = [w, h, pkg.synth.bytes_per_line(w)]
            fr = scene(pkg, 4, w, h, seed=w + refinement)
            pairs = []
            for t in range(4):
                m.pushBack(fr[t][0], fr[t][1], dims, replace=(t == 2))
                if t == 0:
                    continue
                prev = fr[0] if t <= 2 else fr[2]  # t = 2 replaced frame 1 by frame 2
                for method in (1, 0, 2):
                    m.matchFeatures(method)
                    r, want = expected_lists(ob, oracle, po, dims, method, prev, fr[t], refinement)
                    got = m.getMatches()
                    assert got.tobytes() == want.tobytes(), (refinement, kw, w, t, method, len(got), len(want))
                    assert m.getSparseMatches().tobytes() == r["sparse"].tobytes(), (refinement, kw, w, t, method)
                pairs.append(t)
            assert pairs == [1, 2, 3]
        # removeOutliers afterwards works on the pass-2 list
        m.removeOutliers()
        assert m.getMatches().tobytes() == oracle.remove_outliers(want)[0].tobytes()
        m.close()


def lone_lists(pkg, p, frames, dims, methods, on):
    m = pkg.Matcher(p, outlier_removal=False)
    if on:
        m.setMultiStageMatching(True)
    out = {}
    for t, (l, r) in enumerate(frames):
        m.pushBack(l, r, dims)
        if t == 0:
            continue
        for meth in methods:
            m.matchFeatures(meth)
            out[(t, meth)] = m.getMatches()
            if on:
                out[(t, meth, "sparse")] = m.getSparseMatches()
    m.close()
    return out


@pytest.mark.gpu
def test_group_equals_lone_matchers_and_every_reader_sees_pass_two(pkg, ob, oracle, gpu):
    dims = [W, H, pkg.synth.bytes_per_line(W)]
    T = 7
    fr = scene(pkg, T, seed=21)
    p = pkg.Params.default(multi_stage=1)
    po = ob.Params.default(multi_stage=1)
    lone = lone_lists(pkg, p, fr, dims, (0, 1, 2), True)
    r, want = expected_lists(ob, oracle, po, dims, 2, fr[0], fr[1])
    assert lone[(1, 2)].tobytes() == want.tobytes()
    for S in (2, 5):  # a small group runs on one stream, a larger one on three
        g = pkg.StreamGroup(S, p)
        g.setMultiStageMatching(True)
        base = None
        for step in range(3):
            L = np.stack([fr[s + step][0] for s in range(S)]); R = np.stack([fr[s + step][1] for s in range(S)])
            g.pushBack(L, R, dims)
            if step == 0:
                continue
            for meth in (0, 1, 2):
                g.matchFeatures(meth)
                for s in range(S):
                    assert g.getMatches(s).tobytes() == lone[(s + step, meth)].tobytes(), (S, step, s, meth)
                    assert g.getSparseMatches(s).tobytes() == lone[(s + step, meth, "sparse")].tobytes(), (S, step, s, meth)
        # the last step was quad: counts, the one-wait getter, the download, the estimator and the post chain
        step = 2
        lists = [lone[(s + step, 2)] for s in range(S)]
        nf, nm = g.getCounts()
        assert nm.tolist() == [len(x) for x in lists]
        out, cnt = g.getMatchesAll()
        for s in range(S):
            assert out[s, :cnt[s]].tobytes() == lists[s].tobytes()
        pout = pkg.pinned_empty((S, 4096), pkg.P_MATCH_DTYPE)
        pcnt = pkg.pinned_empty((S,), np.int32)
        g.downloadMatchesAsync(pout, pcnt)
        g.waitDownload()
        for s in range(S):
            assert pcnt[s] == len(lists[s]) and pout[s, :pcnt[s]].tobytes() == lists[s].tobytes(), s
        ego = pkg.EgoParams.default(f=300.0, cu=W / 2, cv=H / 2, base=0.5, ransac_iters=50)
        rand3 = np.tile(ob.glibc_rand_after_srand0(50 * 3).reshape(1, 50, 3), (S, 1, 1))
        tr, ok, ninl = g.estimateMotion(ego, rand3)
        tr2, ok2, inl2 = pkg.estimate_motion_stereo(ego, lists, rand3)
        assert ok.tolist() == ok2.tolist() and ninl.tolist() == [len(x) for x in inl2]
        assert np.allclose(tr, tr2, rtol=1e-9, atol=1e-12)
        g.postDeviceConfig(1, 2, 16)
        g.postBeginDevice(4096, 2, 50.0, 50.0, want_lists=True)
        res = g.postFinishDevice(0, want_lists=True, estimator=False)
        bucketed, _, _ = pkg.remove_outliers_device(lists, max_features=2, bucket_width=50.0, bucket_height=50.0)
        for s in range(S):
            assert len(bucketed[s]) > 5 and res["lists"][s].tobytes() == bucketed[s].tobytes(), s
        assert g.deviceBytes() > 0
        g.close()


@pytest.mark.gpu
def test_switch_off_is_todays_single_stage_matching(pkg, ob, oracle, gpu):
    """A multi_stage = 1 handle without the switch (or with it set and cleared again): single-stage lists, no sparse
    kernels launched, no more memory than a multi_stage = 0 handle."""
    dims = [W, H, pkg.synth.bytes_per_line(W)]
    S = 3
    fr = scene(pkg, 4, seed=5)
    seen = {}
    changed = 0
    for name, ms, toggle in (("plain", 0, None), ("off", 1, None), ("cleared", 1, (True, False)), ("on", 1, (True,))):
        g = pkg.StreamGroup(S, pkg.Params.default(multi_stage=ms))
        for on in toggle or ():
            g.setMultiStageMatching(on)
        g.profileEnable(True)
        for t in range(2):
            g.pushBack(np.stack([fr[s + t][0] for s in range(S)]), np.stack([fr[s + t][1] for s in range(S)]), dims)
        for meth in (0, 2):
            g.matchFeatures(meth)
            for s in range(S):
                sets = [oracle.compute_features(ob.Params.default(), I, dims)[1] for I in (fr[s][0], fr[s][1], fr[s + 1][0], fr[s + 1][1])]
                use = [sets[k] if k in NEED[meth] else None for k in range(4)]
                single = oracle.matching(ob.Params.default(), dims, meth, *use)
                if name == "on":
                    changed += g.getMatches(s).tobytes() != single.tobytes()
                else:
                    assert g.getMatches(s).tobytes() == single.tobytes(), (name, meth, s)
        launches = (g.profileRead("ranged")[1], g.profileRead("sparse_detect_nms")[1], g.profileRead("match")[1])
        seen[name] = (g.deviceBytes(), launches)
        if name != "on":
            with pytest.raises(pkg.VisoHipError) as e:
                g.getSparseMatches(0)
            assert e.value.code == pkg.VH_ERR_STATE
        g.close()
    assert seen["plain"] == seen["off"] == seen["cleared"]
    assert changed > 0  # (the switch does something on these frames)
    assert seen["off"][1] == (0, 0, 2)
    assert seen["on"][1][0] == 2 and seen["on"][1][1] > 0 and seen["on"][1][2] == 0
    assert seen["on"][0] > seen["off"][0]  # the sparse sets and the range tables are counted


@pytest.mark.gpu
def test_state_and_envelope_errors(pkg, gpu):
    lib = pkg._lib()
    dims = [W, H, pkg.synth.bytes_per_line(W)]
    fr = scene(pkg, 2, seed=5)
    m = pkg.Matcher(pkg.Params.default(multi_stage=0))
    assert lib.vh_set_multi_stage_matching(m._h, 1) == pkg.VH_ERR_INVALID_ARG  # needs p.multi_stage = 1
    assert lib.vh_set_multi_stage_matching(m._h, 0) == pkg.VH_OK
    m.close()
    m = pkg.Matcher(pkg.Params.default(multi_stage=1), outlier_removal=False)
    m.setIntrinsics(300.0, W / 2, H / 2, 0.5)
    m.setMultiStageMatching(True)
    m.setMultiStageMatching(True)  # idempotent
    for l, r in fr:
        m.pushBack(l, r, dims)
    assert lib.vh_set_multi_stage_matching(m._h, 0) == pkg.VH_ERR_STATE  # before the first push only
    assert lib.vh_set_multi_stage_matching(m._h, 1) == pkg.VH_ERR_STATE
    tr = np.eye(4).reshape(16)
    assert lib.vh_match_features(m._h, 2, tr.ctypes.data_as(C.c_void_p)) == pkg.VH_ERR_UNSUPPORTED
    assert lib.vh_match_features(m._h, 0, tr.ctypes.data_as(C.c_void_p)) == pkg.VH_ERR_UNSUPPORTED
    m.matchFeatures(2)
    assert len(m.getMatches()) > 50
    m.close()
    m = pkg.Matcher(pkg.Params.default(multi_stage=1))
    m.pushBack(fr[0][0], fr[0][1], dims)
    assert lib.vh_set_multi_stage_matching(m._h, 1) == pkg.VH_ERR_STATE
    m.close()
    g = pkg.SequenceGroup(4, pkg.Params.default(multi_stage=1))
    assert lib.vh_group_set_multi_stage_matching(g._h, 1) == pkg.VH_ERR_UNSUPPORTED  # said so in the header
    g.close()
    rg = np.zeros((7 * 4, 4, 4), F32)
    rg[3, 1, 2] = np.inf
    with pytest.raises(pkg.VisoHipError) as e:
        pkg.match_ranged(pkg.Params.default(), dims, 0, rg, None, None, None, None)
    assert e.value.code == pkg.VH_ERR_INVALID_ARG


@pytest.mark.gpu
def test_child_multistage_checking_build(pkg, gpu):
    """The stateless, lone and group cases on libviso_hip_check.so (-DVH_CHECK), detection in sub-batches."""
    assert os.path.exists(pkg.CHECK_LIB_PATH), "build() makes it"
    env = dict(os.environ, VISO_HIP_LIB=pkg.CHECK_LIB_PATH, VH_SUBBATCH="3")
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-q", "-x", "-m", "gpu", "-k",
                        "match_ranged or lone_matcher or group_equals"], env=env, capture_output=True, text=True, timeout=900, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "3 passed" in r.stdout and " skipped" not in r.stdout, r.stdout[-2000:]
    assert "VH_CHECK" not in r.stderr
