"""Match refinement (vh_params.refinement = 1 pixel, 2 sub-pixel).

The GPU's refined lists must equal tests/refine_oracle.py's restatement of the contract byte for byte (float fields
bit for bit) on every path that hands out a match list: the stateless vh_refine_matches, a lone matcher, groups,
sequence handles, the asynchronous download and the device post chain."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import refine_oracle as ro
from conftest import ROOT

W, H = 320, 160
F32 = np.float32


# ------------------------------------------------------------------ CPU
def test_refine_symbol_declared_exported_mirrored(pkg):
    header = open(os.path.join(ROOT, "include", "viso_hip.h")).read()
    assert "vh_refine_matches(" in header
    assert hasattr(C.CDLL(pkg.LIB_PATH), "vh_refine_matches")
    assert "vh_refine_matches" in pkg.ABI_SYMBOLS
    assert callable(pkg.refine_matches)


def test_refine_null_and_bad_arguments_need_no_gpu(pkg):
    lib = pkg._lib()
    bpl = pkg.synth.bytes_per_line(W)
    dims = (C.c_int32 * 3)(W, H, bpl)
    img = np.zeros((H, bpl), np.uint8)
    I = img.ctypes.data_as(C.c_void_p)
    pm = np.zeros(3, pkg.P_MATCH_DTYPE)
    P = pm.ctypes.data_as(C.c_void_p)
    n = C.c_int32(-7)
    p1 = pkg.Params.default(refinement=1)
    assert lib.vh_refine_matches(None, 0, 2, dims, I, I, I, I, P, 3, C.byref(n)) == pkg.VH_ERR_INVALID_ARG
    assert lib.vh_refine_matches(C.byref(p1), 0, 2, None, I, I, I, I, P, 3, C.byref(n)) == pkg.VH_ERR_INVALID_ARG
    assert lib.vh_refine_matches(C.byref(p1), 0, 2, dims, I, I, I, I, P, 3, None) == pkg.VH_ERR_INVALID_ARG
    assert lib.vh_refine_matches(C.byref(p1), 0, 2, dims, I, I, I, I, None, 3, C.byref(n)) == pkg.VH_ERR_INVALID_ARG
    assert lib.vh_refine_matches(C.byref(p1), 0, 2, dims, I, I, I, I, P, -1, C.byref(n)) == pkg.VH_ERR_INVALID_ARG
    assert lib.vh_refine_matches(C.byref(p1), 0, 3, dims, I, I, I, I, P, 3, C.byref(n)) == pkg.VH_ERR_INVALID_ARG
    assert lib.vh_refine_matches(C.byref(p1), 0, 2, dims, I, None, I, I, P, 3, C.byref(n)) == pkg.VH_ERR_INVALID_ARG  # quad reads 2p
    assert lib.vh_refine_matches(C.byref(p1), 0, 0, dims, None, None, I, None, P, 3, C.byref(n)) == pkg.VH_ERR_INVALID_ARG  # flow reads 1p
    assert lib.vh_refine_matches(C.byref(p1), 0, 1, dims, None, None, None, I, P, 3, C.byref(n)) == pkg.VH_ERR_INVALID_ARG  # stereo reads 1c
    bad = (C.c_int32 * 3)(W, H, W - 1)
    assert lib.vh_refine_matches(C.byref(p1), 0, 2, bad, I, I, I, I, P, 3, C.byref(n)) == pkg.VH_ERR_INVALID_ARG
    assert lib.vh_refine_matches(C.byref(pkg.Params.default(nms_n=0)), 0, 2, dims, I, I, I, I, P, 3, C.byref(n)) == pkg.VH_ERR_UNSUPPORTED
    # refinement <= 0 or no records: nothing changes, nothing is launched (no device needed)
    before = pm.tobytes()
    for r in (0, -3):
        n.value = -7
        assert lib.vh_refine_matches(C.byref(pkg.Params.default(refinement=r)), 0, 2, dims, I, I, I, I, P, 3, C.byref(n)) == pkg.VH_OK
        assert n.value == 3 and pm.tobytes() == before
    n.value = -7
    assert lib.vh_refine_matches(C.byref(p1), 0, 0, dims, I, None, I, None, None, 0, C.byref(n)) == pkg.VH_OK and n.value == 0


def test_solve_restatement_matches_numpy():
    rng = np.random.default_rng(3)
    for _ in range(50):
        A = rng.normal(size=(6, 6)) + 6 * np.eye(6)
        b = rng.normal(size=6)
        assert np.allclose(ro.solve(A.tolist(), b.tolist()), np.linalg.solve(A, b), rtol=0, atol=1e-12)
    AtA = ro.mat_t_mul(ro.DESIGN, ro.DESIGN)
    b = rng.integers(0, 4000, 6).astype(float)
    assert np.allclose(ro.solve(AtA, b.tolist()), np.linalg.solve(np.array(AtA), b), rtol=0, atol=1e-12)


def test_paraboloid_minimum_recovered():
    """Costs sampled from an exact paraboloid with cross term: the fit returns its minimum (float rounding only)."""
    for x0, y0 in ((0.3, -0.2), (-0.45, 0.4), (0.0, 0.1), (0.12, -0.33)):
        # f = a (x - x0)^2 + b (y - y0)^2 + c (x - x0)(y - y0) + 100
        a, b, c = 30.0, 20.0, 7.0
        c9 = [a * (x - x0) ** 2 + b * (y - y0) ** 2 + c * (x - x0) * (y - y0) + 100 for y in (-1, 0, 1) for x in (-1, 0, 1)]
        ddu, ddv = ro.parabolic_offset(c9)
        assert abs(float(ddu) - x0) < 1e-6 and abs(float(ddv) - y0) < 1e-6, (x0, y0, ddu, ddv)


def test_degenerate_and_border_cases_are_dropped():
    flat = [5.0] * 9
    assert ro.parabolic_offset(flat) is None  # divisor 0
    no_cross = [(x * x + y * y) * 10.0 for y in (-1, 0, 1) for x in (-1, 0, 1)]
    assert ro.parabolic_offset(no_cross) is None  # cross term exactly 0: stock libviso2's second test
    far = [200.0 * (x - 1.3) ** 2 + 50 * y * y + 3 * x * y for y in (-1, 0, 1) for x in (-1, 0, 1)]
    assert ro.parabolic_offset(far) is None  # |ddu| >= 1
    # bounds: anchor and target inside, on the float values
    D = np.zeros((H, W, 16), np.int32)
    dims = (W, H, W)
    assert ro.refine_hop(dims, D, D, F32(3.9), F32(50), F32(50), F32(50), False) == (F32(50), F32(50))  # pixel: left
    assert ro.refine_hop(dims, D, D, F32(3.9), F32(50), F32(50), F32(50), True) is None                  # sub-pixel: dropped
    assert ro.refine_hop(dims, D, D, F32(50), F32(50), F32(W - 5 - 3 + 0.5), F32(50), True) is None
    assert ro.refine_hop(dims, D, D, F32(50), F32(50), F32(W - 5 - 2), F32(50), False) == (F32(W - 9), F32(48))  # flat: the first
    # a flat window: the first minimum is (0, 0) -> a border minimum, dropped in sub-pixel mode
    assert ro.refine_hop(dims, D, D, F32(50), F32(50), F32(60), F32(60), True) is None


# ------------------------------------------------------------------ GPU
def scene(pkg, T=3, w=W, h=H, seed=7, disparity=6, blur=3):
    return pkg.synth.stereo_sequence(w, h, T, disparity=disparity, blur=blur, seed=seed)


def expected(oracle, po, dims, method, prev, cur, refinement):
    """Oracle features and matching of the pair, then the restatement's refinement at full resolution."""
    imgs = (prev[0], prev[1], cur[0], cur[1])
    sets = [oracle.compute_features(po, I, dims)[1] for I in imgs]
    raw = oracle.matching(po, dims, method, *sets)
    return ro.refine(raw, method, refinement, dims, imgs, oracle.filters), raw


def random_records(pkg, rng, n, w, h):
    pm = np.zeros(n, pkg.P_MATCH_DTYPE)
    for f in ("u1p", "u2p", "u1c", "u2c"):
        pm[f] = rng.uniform(0, w, n).astype(np.float32)
    for f in ("v1p", "v2p", "v1c", "v2c"):
        pm[f] = rng.uniform(0, h, n).astype(np.float32)
    half = n // 2  # integer coordinates as the matcher produces them, some right at the bounds
    for f in ("u1p", "u2p", "u1c", "u2c", "v1p", "v2p", "v1c", "v2c"):
        pm[f][:half] = np.floor(pm[f][:half])
    edge = [4, 5, 6, 7, w - 5, w - 6, w - 7, w - 8]
    for k, e in enumerate(edge):
        pm["u2c"][k] = e; pm["u1p"][k] = e; pm["u2p"][k] = e; pm["u1c"][k + 8] = e
    pm["i1p"], pm["i2p"], pm["i1c"], pm["i2c"] = np.arange(n), np.arange(n) + 1, np.arange(n) + 2, np.arange(n) + 3
    return pm


@pytest.mark.gpu
def test_refine_matches_stateless_crafted_and_random(pkg, ob, oracle, gpu):
    bpl = pkg.synth.bytes_per_line(W)
    dims = [W, H, bpl]
    fr = scene(pkg)
    imgs = (fr[0][0], fr[0][1], fr[1][0], fr[1][1])
    rng = np.random.default_rng(11)
    pm = random_records(pkg, rng, 600, W, H)
    # ties and flat patches: a constant image gives flat planes everywhere
    flat = np.full((H, bpl), 77, np.uint8)
    stats = {}  # the branches the device was compared on (refine_oracle.refine_hop)
    for method in (0, 1, 2):
        for refinement in (1, 2, 5):
            p = pkg.Params.default(refinement=refinement)
            need = {0: (0, 2), 1: (2, 3), 2: (0, 1, 2, 3)}[method]
            args = [imgs[k] if k in need else None for k in range(4)]
            got = pkg.refine_matches(p, dims, method, pm, *args)
            want = ro.refine(pm, method, refinement, dims, args, oracle.filters, stats)
            # (random positions rarely pass three sub-pixel fits in a row: quad keeps few of them)
            assert len(want) > (5 if refinement == 2 else 20) and got.tobytes() == want.tobytes(), (method, refinement, len(got), len(want))
            fl = [flat if k in need else None for k in range(4)]
            got = pkg.refine_matches(p, dims, method, pm, *fl)
            want = ro.refine(pm, method, refinement, dims, fl, oracle.filters, stats)
            assert got.tobytes() == want.tobytes(), ("flat", method, refinement)
    # real matches of the pair: sub-pixel moves most of them off the integer grid
    raw = oracle.matching(ob.Params.default(), dims, 2, *[oracle.compute_features(ob.Params.default(), I, dims)[1] for I in imgs])
    got = pkg.refine_matches(pkg.Params.default(refinement=2), dims, 2, raw, *imgs)
    want = ro.refine(raw, 2, 2, dims, imgs, oracle.filters, stats)
    assert got.tobytes() == want.tobytes() and len(got) > 50
    # every branch of a hop met the device: moved, outside the bounds, a border minimum, a degenerate fit (divisor or cross
    # term below 1e-8) and a fit whose minimum lies a pixel or more away
    for branch in ("moved", "outside", "border", "degenerate", "far"):
        assert stats.get(branch, 0) > 0, (branch, stats)
    assert np.mean(got["u2c"] != np.floor(got["u2c"])) > 0.3


@pytest.mark.gpu
def test_stateless_entries_ignore_refinement(pkg, ob, oracle, gpu):
    """vh_match has no images: its lists stay unrefined whatever refinement says (byte-equal for 0, 1 and 2, and equal to
    the oracle's matching); vh_compute_features and vh_match_all do not depend on the field either."""
    dims = [W, H, pkg.synth.bytes_per_line(W)]
    fr = scene(pkg, 2, seed=17)
    imgs = (fr[0][0], fr[0][1], fr[1][0], fr[1][1])
    po = ob.Params.default()
    sets = [oracle.compute_features(po, I, dims)[1] for I in imgs]
    for method in (0, 1, 2):
        want = oracle.matching(po, dims, method, *sets)
        assert len(want) > 50
        for refinement in (0, 1, 2):
            got = pkg.match(pkg.Params.default(refinement=refinement), dims, method, *sets)
            assert got.tobytes() == want.tobytes(), (method, refinement)
    p2 = pkg.Params.default(refinement=2, multi_stage=1)
    for I, s in zip(imgs, sets):
        m1, m2 = pkg.compute_features(p2, I, dims)
        assert np.array_equal(m2, s)
    best = pkg.match_all(pkg.Params.default(refinement=2), dims, sets[2], sets[0])
    assert np.array_equal(best, oracle.match_all(po, dims, sets[2], sets[0]))


def lone_lists(pkg, p, frames, dims, methods, replace_at=None, stereo=True):
    m = pkg.Matcher(p, outlier_removal=False)
    out = {}
    for t, (l, r) in enumerate(frames):
        m.pushBack(l, r if stereo else None, dims, replace=(t == replace_at))
        if t == 0:
            continue
        for meth in methods:
            m.matchFeatures(meth)
            out[(t, meth)] = m.getMatches()
    m.close()
    return out


@pytest.mark.gpu
def test_lone_matcher_methods_modes_half_resolution(pkg, ob, oracle, gpu):
    """Methods 0/1/2 x refinement 1/2 x half_resolution 0/1 with nms_n 1-3; a replace and a change of dims."""
    cases = [(1, 0, 1), (2, 0, 2), (1, 1, 3), (2, 1, 2), (2, 0, 1), (1, 1, 2)]
    for refinement, half, nms_n in cases:
        p = pkg.Params.default(refinement=refinement, half_resolution=half, nms_n=nms_n)
        po = ob.Params.default(refinement=refinement, half_resolution=half, nms_n=nms_n)
        for (w, h) in ((W, H), (W + 37, H + 9)):
            dims = [w, h, pkg.synth.bytes_per_line(w)]
            fr = scene(pkg, 3, w, h, seed=w + nms_n)
            lists = lone_lists(pkg, p, [fr[0], fr[1], fr[2]], dims, (0, 1, 2), replace_at=2)
            for meth in (0, 1, 2):
                for t, prev in ((1, fr[0]), (2, fr[0])):  # t = 2 replaced frame 1 by frame 2
                    want, raw = expected(oracle, po, dims, meth, prev, fr[t], refinement)
                    got = lists[(t, meth)]
                    assert len(raw) > 10 and got.tobytes() == want.tobytes(), (refinement, half, nms_n, w, meth, t, len(got), len(want))
        # refinement 2 drops some of them, 1 none
        if refinement == 1:
            assert len(want) == len(raw)


@pytest.mark.gpu
def test_groups_and_sequence_rows_equal_lone_matcher(pkg, gpu):
    dims = [W, H, pkg.synth.bytes_per_line(W)]
    T = 8
    fr = scene(pkg, T, seed=21)
    for refinement in (1, 2):
        p = pkg.Params.default(refinement=refinement)
        lone = lone_lists(pkg, p, fr, dims, (0, 1, 2))
        for S in (5, 7):
            g = pkg.StreamGroup(S, p)
            for t in range(2):
                L = np.stack([fr[(s + t) % T][0] for s in range(S)]); R = np.stack([fr[(s + t) % T][1] for s in range(S)])
                g.pushBack(L, R, dims)
            for meth in (0, 1, 2):
                g.matchFeatures(meth)
                for s in range(S):
                    t = (s + 1) % T
                    if t == 0:
                        continue
                    assert g.getMatches(s).tobytes() == lone[(t, meth)].tobytes(), (refinement, S, s, meth)
            g.close()
        g = pkg.SequenceGroup(4, p)
        F = 0
        for n in (4, 4):
            g.pushBack(np.stack([fr[F + r][0] for r in range(n)]), np.stack([fr[F + r][1] for r in range(n)]), dims)
            for meth in (0, 1, 2):
                g.matchFeatures(meth)
                for r in range(n):
                    if F + r >= 1:
                        assert g.getMatches(r).tobytes() == lone[(F + r, meth)].tobytes(), (refinement, F, r, meth)
            F += n
        g.close()


@pytest.mark.gpu
def test_param_txt_configuration_kitti(pkg, ob, oracle, gpu):
    """multi_stage = 1, half_resolution = 1, refinement = 1 at 1241 x 376, quad and flow."""
    w, h = 1241, 376
    dims = [w, h, pkg.synth.bytes_per_line(w)]
    kw = dict(multi_stage=1, half_resolution=1, refinement=1)
    p, po = pkg.Params.default(**kw), ob.Params.default(**kw)
    fr = scene(pkg, 2, w, h, seed=1, disparity=12, blur=8)
    lists = lone_lists(pkg, p, fr, dims, (2, 0))
    for meth in (2, 0):
        want, raw = expected(oracle, po, dims, meth, fr[0], fr[1], 1)
        got = lists[(1, meth)]
        assert len(got) > 100 and got.tobytes() == want.tobytes(), meth
        assert (got["u1c"] % 2 == 0).all() and not (got["u1p"] % 2 == 0).all()  # the anchor stays, the hops leave the grid


@pytest.mark.gpu
def test_download_async_and_device_post_chain(pkg, ob, oracle, gpu):
    dims = [W, H, pkg.synth.bytes_per_line(W)]
    S = 4
    fr = scene(pkg, 5, seed=33)
    p = pkg.Params.default(refinement=2)
    lone = lone_lists(pkg, p, fr, dims, (2,))
    g = pkg.StreamGroup(S, p)
    g.postDeviceConfig(1, 2, 16)
    out = pkg.pinned_empty((S, 4096), pkg.P_MATCH_DTYPE)
    cnt = pkg.pinned_empty((S,), np.int32)
    for t in range(2):
        g.pushBack(np.stack([fr[s + t][0] for s in range(S)]), np.stack([fr[s + t][1] for s in range(S)]), dims)
    g.matchFeatures(2)
    g.downloadMatchesAsync(out, cnt)
    g.waitDownload()
    for s in range(S):
        want = lone[(s + 1, 2)]
        assert cnt[s] == len(want) and out[s, :cnt[s]].tobytes() == want.tobytes(), s
    g.postBeginDevice(4096, 2, 50.0, 50.0, want_lists=True)
    res = g.postFinishDevice(0, want_lists=True, estimator=False)
    refined = [lone[(s + 1, 2)] for s in range(S)]
    voted, _, _ = pkg.remove_outliers_device(refined)  # the device vote alone
    bucketed, _, _ = pkg.remove_outliers_device(refined, max_features=2, bucket_width=50.0, bucket_height=50.0)
    for s in range(S):
        want, _ = oracle.remove_outliers(refined[s])
        assert len(want) > 10 and voted[s].tobytes() == want.tobytes(), s
        assert res["lists"][s].tobytes() == bucketed[s].tobytes() and res["counts"][s] == len(bucketed[s]), s
    g.close()


@pytest.mark.gpu
def test_refinement_zero_unchanged_and_not_launched(pkg, ob, oracle, gpu):
    dims = [W, H, pkg.synth.bytes_per_line(W)]
    S = 3
    fr = scene(pkg, 4, seed=5)
    for refinement, launches in ((0, 0), (2, 2)):
        g = pkg.StreamGroup(S, pkg.Params.default(refinement=refinement))
        g.profileEnable(True)
        for t in range(2):
            g.pushBack(np.stack([fr[s + t][0] for s in range(S)]), np.stack([fr[s + t][1] for s in range(S)]), dims)
        g.matchFeatures(2)
        for s in range(S):
            want, raw = expected(oracle, ob.Params.default(), dims, 2, fr[s], fr[s + 1], refinement)
            assert g.getMatches(s).tobytes() == want.tobytes(), (refinement, s)
        assert g.profileRead("refine_planes")[1] == launches and g.profileRead("refine")[1] == launches // 2, refinement
        bytes_ = g.deviceBytes()
        g.close()
        if refinement == 0:
            base = bytes_
        else:
            assert bytes_ > base


def run_child(env_over, sel, timeout=600):
    env = dict(os.environ, **env_over)
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-q", "-x", "-m", "gpu", "-k", sel],
                       env=env, capture_output=True, text=True, timeout=timeout, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert " passed" in r.stdout and " skipped" not in r.stdout, r.stdout[-2000:]
    return r


@pytest.mark.gpu
def test_child_refinement_checking_build(pkg, gpu):
    """The group, sequence and stateless cases on libviso_hip_check.so (-DVH_CHECK), detection in sub-batches."""
    assert os.path.exists(pkg.CHECK_LIB_PATH), "build() makes it"
    r = run_child({"VISO_HIP_LIB": pkg.CHECK_LIB_PATH, "VH_SUBBATCH": "3"}, "groups_and_sequence or stateless")
    assert "VH_CHECK" not in r.stderr


@pytest.mark.gpu
def test_failed_first_push_leaves_nothing_behind(pkg, ob, oracle, gpu):
    """A first pushBack whose k-th device allocation fails (engine.hip: ensure / allocate, the staging blocks of push_host)
    releases everything it made: deviceBytes() is 0 right after, and the handle then computes what an undisturbed one
    does, in the same memory.  320 x 160, S = 2 (serial: the host-mapped match block is on the path), refinement = 1 and
    half_resolution = 1 so that their blocks are too; skip = 0, the middle, and the last allocation of the push."""
    kw = dict(refinement=1, half_resolution=1)
    p, po = pkg.Params.default(**kw), ob.Params.default(**kw)
    dims = [W, H, pkg.synth.bytes_per_line(W)]
    S = 2
    fr = [pkg.synth.stereo_sequence(W, H, 3, disparity=6, blur=4, seed=31 + s) for s in range(S)]
    push = lambda g, t: g.pushBack(np.stack([fr[s][t][0] for s in range(S)]), np.stack([fr[s][t][1] for s in range(S)]), dims)

    def finish(g):  # two more pushes and a quad match -> the lists and the memory held
        for t in (1, 2):
            push(g, t)
        g.matchFeatures(pkg.METHOD_QUAD)
        out = [g.getMatches(s) for s in range(S)], g.deviceBytes()
        g.close()
        return out

    g = pkg.StreamGroup(S, p)
    push(g, 0)
    clean, clean_bytes = finish(g)
    assert all(len(pm) >= 20 for pm in clean), [len(pm) for pm in clean]
    want, raw = expected(oracle, po, dims, pkg.METHOD_QUAD, fr[0][1], fr[0][2], 1)
    assert clean[0].tobytes() == want.tobytes()

    n_alloc = None  # allocations of a first push: the smallest skip at which it succeeds
    for skip in range(64):
        g = pkg.StreamGroup(S, p)
        g.debugFailAllocAfter(skip)
        try:
            push(g, 0)
            n_alloc = skip
        except pkg.VisoHipError as e:
            assert e.code == pkg.VH_ERR_HIP, skip
        g.close()
        if n_alloc is not None:
            break
    assert n_alloc is not None and n_alloc >= 3, n_alloc
    for skip in (0, n_alloc // 2, n_alloc - 1):
        g = pkg.StreamGroup(S, p)
        g.debugFailAllocAfter(skip)
        with pytest.raises(pkg.VisoHipError) as e:
            push(g, 0)
        assert e.value.code == pkg.VH_ERR_HIP and g.deviceBytes() == 0, skip
        push(g, 0)
        got, got_bytes = finish(g)
        assert got_bytes == clean_bytes, (skip, got_bytes, clean_bytes)
        for s in range(S):
            assert got[s].tobytes() == clean[s].tobytes(), (skip, s)


@pytest.mark.gpu
def test_child_failed_first_push_on_poisoned_buffers(gpu):
    """The same with VH_POISON=1: buffers that are not zero-initialised at allocation start as 0xA5 bytes."""
    run_child({"VH_POISON": "1"}, "failed_first_push_leaves")
