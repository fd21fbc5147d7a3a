"""The mono model refit: vh_refit_model_mono, vh_group_refit_model_mono,
vh_match_refit_model_mono -- fundamentalMatrix (reference src/viso_mono.cpp:235-266) over every record of whole lists, in
the normalised frame of the model the lists were classified under.  The contract is restated in tests/mono_refit_oracle.py.

The GPU bound.  d_ref / d_w are the largest deviations of `refit` (double, sequential sum, the pinned Matrix::svd) from
`refit_ext` (numpy.longdouble, a cyclic Jacobi) over LISTS: || F - F_ext ||_F and max |w - w_ext| / |w_ext| over w[8], w[7].
The device is held to 16 d_ref / 16 d_w against `refit_ext`: it adds in another order (a tree fixed by the list's length,
whose error bound is no worse than the sequential sum's), the margin covers that.  Measured on the CPU
(test_restatement_against_wider_arithmetic prints them): d_ref = 5.8e-12, d_w = 6.3e-10.
The input condition: (w[7] - w[8]) / w[0] of M over LISTS is 8.32e-07 at its smallest; GAP_FLOOR
holds the scenes to it, the tolerance is not loosened to admit a worse scene."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import mono_inlier_oracle as mo
import mono_refit_oracle as mr
import test_mono_inliers as tm    # its helpers: hmono, rand8_of, check_against
import test_motion_inliers as ti  # its helpers: the stereo scene of the handle tests
import test_sequence_recon as sr  # its helpers: the synthetic frames, expect()
from conftest import ROOT

SYMBOLS = ("vh_refit_model_mono", "vh_group_refit_model_mono", "vh_match_refit_model_mono")
SCOPE = "mono_refit"
FLOW, QUAD, STEREO = sr.FLOW, sr.QUAD, sr.STEREO
MARGIN = 16.0
GAP_FLOOR = 8.3e-7
# the floor of :76, the wave and workgroup edges, several trips per lane
LENGTHS = (0, 9, 10, 63, 64, 65, 255, 256, 257, 1027, 4099)
ptr, expect = sr.ptr, sr.expect
_CACHE = {}


def dtype():
    return ti._parity_dtype()


@pytest.fixture(autouse=True)
def entries(pkg):
    """Every test here is about the refit's entries, the restatement's own included (it is their yardstick): without them
    in the library's ABI none of it passes."""
    assert all(name in pkg.ABI_SYMBOLS and hasattr(pkg._lib(), name) for name in SYMBOLS)


def lists():
    """A list per length (seed = position) with the model it comes with, the garbage-model list (ok_in = 0) and the list
    with a NaN record -> dict name -> (pm, model, ok_in)."""
    if "lists" not in _CACHE:
        out = {}
        for k, n in enumerate(LENGTHS):
            pm = mr.flow_scene(dtype(), n, 100 + k)
            model = mr.start_model(pm, tilt=0.05) if n >= 10 else dict(c=np.array([600.0, 180.0, 590.0, 185.0]), s=np.array([0.004, 0.0041]),
                                                                         F=mr.normalised_F(mr.true_F(), [600, 180, 590, 185], [0.004, 0.0041]), valid=1.0)
            out[n] = (pm, model, 1)
        pm = mr.flow_scene(dtype(), 64, 200)
        out["ok0"] = (pm, dict(c=np.full(4, np.nan), s=np.full(2, np.inf), F=np.full(9, np.nan), valid=0.0), 0)
        pm = mr.flow_scene(dtype(), 255, 201)
        model = mr.start_model(pm, tilt=0.05)
        pm["v1c"][131] = np.nan
        out["nan"] = (pm, model, 1)
        _CACHE["lists"] = out
    return _CACHE["lists"]


def expectation(oracle):
    """name -> (refit, refit_ext) of every list, computed once."""
    if "want" not in _CACHE:
        _CACHE["want"] = {k: (mr.refit(oracle.svd, pm, m, ok), mr.refit_ext(pm, m, ok)) for k, (pm, m, ok) in lists().items()}
    return _CACHE["want"]


def yardstick(oracle):
    """-> (d_ref, d_w, the smallest gap) over LISTS"""
    if "d" not in _CACHE:
        d_ref = d_w = 0.0
        gap = np.inf
        for k, (dbl, ext) in expectation(oracle).items():
            if not dbl[1]:
                continue
            assert ext[1], k
            d_ref = max(d_ref, mr.deviation_F(dbl[0]["F"], ext[3])); d_w = max(d_w, mr.deviation_w(dbl[2], ext[4]))
            pm, m, _ = lists()[k]
            gap = min(gap, mr.gap(oracle.svd(mr.moments(mr.rows(pm, m)))[1]))
        _CACHE["d"] = (d_ref, d_w, gap)
    return _CACHE["d"]


# ------------------------------------------------------------------------------------------------------------ CPU
def test_symbols_declared_exported_mirrored_and_argument_errors(pkg):
    """Every new symbol is declared, exported and mirrored; vh_abi_version stays 1; n_sets = 0 and lists without records are
    VH_OK without a device; null and negative arguments are VH_ERR_INVALID_ARG."""
    header = open(os.path.join(ROOT, "include", "viso_hip.h")).read()
    lib = pkg._lib()
    for name in SYMBOLS:
        assert name + "(" in header and hasattr(C.CDLL(pkg.LIB_PATH), name) and name in pkg.ABI_SYMBOLS, name
    assert pkg.abi_version() == 1
    assert callable(pkg.refit_model_mono) and "refitModelMono" in vars(pkg.Matcher)
    assert "refitModelMono" in vars(pkg.StreamGroup) and hasattr(pkg.SequenceGroup, "refitModelMono")
    e = tm.mono_params(pkg)
    pm = np.zeros(12, pkg.P_MATCH_DTYPE)
    off = np.array([0, 12], np.int32)
    model = np.zeros(1, pkg.MONO_MODEL_DTYPE); ok = np.ones(1, np.int32)
    mout = np.zeros(1, pkg.MONO_MODEL_DTYPE); okout = np.full(1, 7, np.int32); w = np.full((1, 2), 7.0)
    inv = pkg.VH_ERR_INVALID_ARG
    call = lib.vh_refit_model_mono
    assert call(C.byref(e), 0, 0, None, None, None, None, None, None, None) == pkg.VH_OK
    empty = np.array([3, 3, 3], np.int32)
    m2 = np.zeros(2, pkg.MONO_MODEL_DTYPE); m2["valid"] = 5; ok2 = np.full(2, 7, np.int32); w2 = np.full((2, 2), 7.0)
    assert call(C.byref(e), 0, 2, None, ptr(empty), ptr(np.zeros(2, pkg.MONO_MODEL_DTYPE)), ptr(np.ones(2, np.int32)), ptr(m2), ptr(ok2), ptr(w2)) == pkg.VH_OK
    assert ok2.tolist() == [0, 0] and not w2.any() and m2.tobytes() == bytes(256)
    assert pkg.refit_model_mono(e, [], [], [])[1].shape == (0,)
    good = [C.byref(e), 0, 1, ptr(pm), ptr(off), ptr(model), ptr(ok), ptr(mout), ptr(okout), ptr(w)]
    for k in (0, 3, 4, 5, 6, 7, 8, 9):
        assert call(*[None if j == k else a for j, a in enumerate(good)]) == inv, k
    assert call(C.byref(e), 0, -1, *good[3:]) == inv
    assert call(*good[:4], ptr(np.array([12, 0], np.int32)), *good[5:]) == inv
    assert call(*good[:4], ptr(np.array([-1, 3], np.int32)), *good[5:]) == inv
    n = np.zeros(1, np.int32)
    assert lib.vh_group_refit_model_mono(None, C.byref(e), 0, ptr(mout), ptr(okout), ptr(w), ptr(n)) == inv
    assert lib.vh_match_refit_model_mono(None, C.byref(e), 0, ptr(mout), ptr(okout), ptr(w), ptr(n)) == inv


def test_restatement_recovers_the_true_F_without_noise(oracle):
    """Noise-free flow of a general 3-d scene under a known R, t: the refit's F, denormalised, is the true F up to scale, and
    w[8] / w[0] is at rounding level.  The bounds: the coordinates are floats, off by up to 2^-14 pixels (half an ulp
    below 2048) = 1.2e-4 * s ~ 3e-7 in the normalised frame, so a row's residual under the true F is ~ 1e-6 and w[8] / w[0]
    ~ 1e-12 or less: bound 1e-11.  For the direction, with f0 the true F in the normalised frame and r0 = f0^T M f0:
    r0 >= w[8] cos^2 + w[7] sin^2, so sin^2 <= (r0 - w[8]) / (w[7] - w[8]); the rank-2 step moves f by no more than its
    distance to the nearest rank-2 matrix, which is no farther than f0: twice that bound."""
    for n, seed in ((500, 1), (2000, 2), (10, 3)):
        pm = mr.flow_scene(dtype(), n, seed, noise=0.0)
        m0 = mr.start_model(pm, tilt=0.05)
        got, ok, w = mr.refit(oracle.svd, pm, m0)
        ext = mr.refit_ext(pm, m0)
        assert ok and ext[1]
        M = mr.moments(mr.rows(pm, m0))
        W = oracle.svd(M)[1]
        f0 = mr.normalised_F(mr.true_F(), m0["c"], m0["s"])
        bound = 2 * np.sqrt(max(f0 @ M @ f0 - W[8], 0.0) / (W[7] - W[8])) + 1e-12
        s_norm, s_pix = mr.sin_angle(got["F"], f0), mr.sin_angle(mr.denormalise(got), mr.true_F())
        print(f"n = {n}: sin(normalised) {s_norm:.3e} (bound {bound:.3e})  sin(pixel) {s_pix:.3e}  w8/w0 {W[8] / W[0]:.3e}")
        assert s_norm <= bound and mr.sin_angle(ext[0]["F"], f0) <= bound
        # (the denormalisation is a fixed linear map of the nine entries: it stretches an angle by its condition number at most)
        kappa = np.linalg.cond(np.kron(mr.T_of(m0["c"][2], m0["c"][3], m0["s"][1]).T, mr.T_of(m0["c"][0], m0["c"][1], m0["s"][0]).T))
        assert s_pix <= kappa * bound and s_pix <= s_norm * kappa
        assert W[8] / W[0] <= 1e-11 and w[0] == W[8] and w[1] == W[7]
        assert got["c"].tobytes() == np.asarray(m0["c"]).tobytes() and got["s"].tobytes() == np.asarray(m0["s"]).tobytes()
        assert np.dot(got["F"], m0["F"]) > 0 and np.dot(ext[0]["F"], m0["F"]) > 0      # the sign rule


def test_restatement_improves_on_the_bucketed_model(ob, oracle):
    """0.3 pixel noise, 2 000 records: the estimator's model of a bucketed list of 200 of them (the pinned estimator's inlier
    set, the refit of :80), the whole list classified under it, the refit over all those inliers -- its F is closer to the true
    one than the model it started from (measured: sin 4.9e-3 after 1.46e-2 before, a ratio of 2.98, over 1 910 dense inliers where the estimator had 183; asserted: closer)."""
    pm = mr.flow_scene(dtype(), 2000, 11)
    rng = np.random.default_rng(12)
    few = pm[np.sort(rng.permutation(2000)[:200])]
    start, ok, inl = tm.restated_model(ob, oracle, few)
    assert start["valid"] == 1.0 and len(inl) >= 10
    flags, _ = mo.inliers(pm, start, tm.THR)
    assert flags.sum() > 4 * len(inl)
    got, ok, w = mr.refit(oracle.svd, pm[flags == 1], start)
    assert ok
    f0 = mr.normalised_F(mr.true_F(), start["c"], start["s"])
    before, after = mr.sin_angle(start["F"], f0), mr.sin_angle(got["F"], f0)
    print(f"bucketed inliers {len(inl)}, dense inliers {int(flags.sum())}: sin before {before:.3e}, after {after:.3e}, ratio {before / after:.2f}")
    assert after < before


def test_restatement_against_wider_arithmetic(oracle):
    """`refit` against `refit_ext` over LISTS: d_ref and d_w are finite (printed: the yardstick of the GPU tests); the refused
    lists are refused by both; every scene holds the input condition."""
    d_ref, d_w, gap = yardstick(oracle)
    print(f"d_ref = {d_ref:.3e}  d_w = {d_w:.3e}  smallest (w7 - w8) / w0 = {gap:.3e}  (np.longdouble wider than double: {mr.EXTENDED})")
    assert np.isfinite(d_ref) and np.isfinite(d_w) and 0 < d_ref < 1e-9 and 0 < d_w < 1e-7
    assert gap >= GAP_FLOOR
    want = expectation(oracle)
    for k in (0, 9, "ok0", "nan"):
        for res in want[k]:
            assert not res[1] and res[0]["valid"] == 0.0 and not np.asarray(res[0]["F"]).any() and not res[2].any(), k
    assert all(want[n][0][1] and want[n][1][1] for n in LENGTHS[2:])


def test_device_functions_on_the_host_equal_the_restatement(tmp_path):
    """csrc/vh_mono.h (mono_normalise, mono_row9: the rows mono_refit_kernel and mono_final_a_kernel form) compiled for the
    host with -ffp-contract=off: the N x 9 system of every list is the restatement's, byte for byte."""
    exe = str(tmp_path / "mono_refit_check")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", os.path.join(ROOT, "tests", "cpp", "mono_refit_check.cpp"), "-lm", "-o", exe])
    dt = np.dtype([("c", "<f8", (4,)), ("s", "<f8", (2,)), ("F", "<f8", (9,)), ("valid", "<f8")])
    for k, (pm, model, _) in lists().items():
        fin, fout = str(tmp_path / f"in{k}"), str(tmp_path / f"out{k}")
        with open(fin, "wb") as fh:
            fh.write(mo.as_array([model], dt).tobytes()); fh.write(np.int64(len(pm)).tobytes()); fh.write(pm.tobytes())
        subprocess.check_call([exe, fin, fout], timeout=60)
        assert np.fromfile(fout, np.float64).tobytes() == mr.rows(pm, model).tobytes(), k


# ------------------------------------------------------------------------------------------------------------ GPU
def same_result(a, b, k):
    return a[0][k].tobytes() == b[0][k].tobytes() and a[1][k] == b[1][k] and a[2][k].tobytes() == b[2][k].tobytes()


def check_list(pkg, oracle, name, model, ok, w, what):
    """One list's device result against the contract: ok exact, c and s copied bit for bit, F and w within 16 d_ref / 16 d_w
    of the long double form; the zero record where refused."""
    pm, m_in, _ = lists()[name]
    dbl, ext = expectation(oracle)[name]
    d_ref, d_w, _ = yardstick(oracle)
    assert bool(ok) == dbl[1] == ext[1], what
    if not ok:
        assert model.tobytes() == bytes(128) and not w.any(), what
        return 0.0
    assert model["c"].tobytes() == np.asarray(m_in["c"], np.float64).tobytes() and model["s"].tobytes() == np.asarray(m_in["s"], np.float64).tobytes(), what
    assert model["valid"] == 1.0, what
    dF, dw = mr.deviation_F(model["F"], ext[3]), mr.deviation_w(w, ext[4])
    print(f"{what}: F {dF:.3e} (bound {MARGIN * d_ref:.3e})  w {dw:.3e} (bound {MARGIN * d_w:.3e})")
    assert dF <= MARGIN * d_ref and dw <= MARGIN * d_w, (what, dF, dw, d_ref, d_w)
    return max(dF / (MARGIN * d_ref), dw / (MARGIN * d_w))


def call_stateless(pkg, names):
    e = tm.mono_params(pkg)
    L = lists()
    return pkg.refit_model_mono(e, [L[k][0] for k in names], mo.as_array([L[k][1] for k in names], pkg.MONO_MODEL_DTYPE), [L[k][2] for k in names])


GROUPS = ((0, 9, 1027, "ok0", 65), (4099, "nan", 10, 63, 256), (257, 64, 255, 4099, 10))


@pytest.mark.gpu
def test_gpu_stateless(pkg, oracle, gpu):
    """vh_refit_model_mono on lists of 0 .. 4 099 records, one list per call and five lists of mixed length per call, one with
    ok_in = 0 and a NaN model, one with a NaN record: ok_out, F and w within 16 d_ref / 16 d_w of the long double form,
    c and s copied bit for bit, the same bytes alone and among other lists and from two runs.
    Measured on an MI355X: the largest deviation is 0.092 of the bound (F, at N = 10)."""
    alone = {}
    worst = 0.0
    for k in lists():
        res = call_stateless(pkg, [k])
        assert same_result(res, call_stateless(pkg, [k]), 0), k
        worst = max(worst, check_list(pkg, oracle, k, res[0][0], res[1][0], res[2][0], f"alone {k}"))
        alone[k] = res
    for names in GROUPS:
        res = call_stateless(pkg, names)
        again = call_stateless(pkg, names)
        for j, k in enumerate(names):
            assert same_result(res, again, j), (names, k)
            assert res[0][j].tobytes() == alone[k][0][0].tobytes() and res[1][j] == alone[k][1][0] and res[2][j].tobytes() == alone[k][2][0].tobytes(), (names, k)
    print(f"largest deviation / bound = {worst:.3f}")
    # the parameters are not read by the refit
    e2 = pkg.MonoParams.default(ransac_iters=1, inlier_threshold=9.0, motion_threshold=1.0, height=9.0, pitch=0.3, f=2.0, cu=3.0, cv=4.0)
    pm, m, ok = lists()[257]
    assert same_result(pkg.refit_model_mono(e2, [pm], mo.as_array([m], pkg.MONO_MODEL_DTYPE), [ok]), alone[257], 0)


@pytest.mark.gpu
def test_gpu_sign_rule_and_quad_records(pkg, oracle, gpu):
    """-F as the incoming model gives the negated F, bytes equal apart from the sign, the same w; the refined F has a positive
    dot product with the F it refines; quad records of the same flow give the bytes of the flow records."""
    e = tm.mono_params(pkg)
    for n in (10, 257, 1027):
        pm, m, ok = lists()[n]
        neg = dict(m, F=-np.asarray(m["F"]))
        a = pkg.refit_model_mono(e, [pm], mo.as_array([m], pkg.MONO_MODEL_DTYPE), [ok])
        b = pkg.refit_model_mono(e, [pm], mo.as_array([neg], pkg.MONO_MODEL_DTYPE), [ok])
        assert a[1][0] and b[1][0] and np.dot(a[0][0]["F"], m["F"]) > 0
        assert (-b[0][0]["F"]).tobytes() == a[0][0]["F"].tobytes() and a[2].tobytes() == b[2].tobytes(), n
        assert a[0][0]["c"].tobytes() == b[0][0]["c"].tobytes() and a[0][0]["s"].tobytes() == b[0][0]["s"].tobytes()
    k = LENGTHS.index(1027)
    flow, quad = mr.flow_scene(dtype(), 1027, 100 + k), mr.flow_scene(dtype(), 1027, 100 + k, quad=True)
    assert flow.tobytes() == lists()[1027][0].tobytes() and (quad["u2c"] != -1).all()
    assert all(flow[c].tobytes() == quad[c].tobytes() for c in ("u1p", "v1p", "u1c", "v1c"))
    marr = mo.as_array([lists()[1027][1]], pkg.MONO_MODEL_DTYPE)
    assert same_result(pkg.refit_model_mono(e, [flow], marr, [1]), pkg.refit_model_mono(e, [quad], marr, [1]), 0)


def check_reclassified(pkg, g_lists, e, model, ok, counts, got, what):
    """The classification a reclassifying refit left: flags, records and positions byte-equal to vh_motion_inliers_mono under
    the returned model, and to the restatement exactly.  got: per list (flags, records, positions)."""
    flags, ninl, outs, poss = pkg.motion_inliers_mono(e, g_lists, model, ok)
    for s, pm in enumerate(g_lists):
        f, out, pos = got[s]
        assert f.tobytes() == flags[s].tobytes() and out.tobytes() == outs[s].tobytes() and np.array_equal(pos, poss[s]) and counts[s] == ninl[s], (what, s)
        want = mo.inliers(pm, mo.from_array(model[s]), e.inlier_threshold, ok=bool(ok[s]))[0]
        tm.check_against(pm, want, f, counts[s], out, pos, (what, s))


def refit_path(pkg, ob, g, what, rows=None):
    """estimateMotionMono(model=True) -> motionInliersMono -> refitModelMono on a group's current lists."""
    e = tm.hmono(pkg, inlier_threshold=3e-5)
    S = g.S
    _, _, ninl, models = g.estimateMotionMono(e, tm.rand8_of(ob, e, S), model=True)
    ok0 = models["valid"].astype(np.int32)
    rec, n = g.getMatchesAll()
    full = [rec[s, :n[s]] for s in range(S)]
    c0 = g.motionInliersMono(e, models, ok0)
    inl0 = [g.getInlierMatches(s) for s in range(S)]
    # reclassify = False: the stateless refit of the lists the getter returns, the classification untouched
    m1, ok1, w1, c1 = g.refitModelMono(e, reclassify=False)
    want = pkg.refit_model_mono(e, [x[0] for x in inl0], models, ok0)
    assert m1.tobytes() == want[0].tobytes() and np.array_equal(ok1, want[1]) and w1.tobytes() == want[2].tobytes(), what
    assert np.array_equal(c1, c0), what
    for s in range(S):
        out, pos = g.getInlierMatches(s)
        assert out.tobytes() == inl0[s][0].tobytes() and np.array_equal(pos, inl0[s][1]), (what, s)
        assert ok1[s] == (ok0[s] == 1 and c0[s] >= 10), (what, s, ok0, c0)
    assert ok1.any(), (what, ok0, c0)
    # reclassify = True: the same refit, then the lists under its result
    m2, ok2, w2, c2 = g.refitModelMono(e, reclassify=True)
    assert m2.tobytes() == m1.tobytes() and np.array_equal(ok2, ok1) and w2.tobytes() == w1.tobytes(), what
    check_reclassified(pkg, full, e, m2, ok2.astype(np.int32), c2, [(g.getInlierFlags(s),) + g.getInlierMatches(s) for s in range(S)], what)
    # a second call: nothing goes up, the refined model is the one the classification was made under
    inl2 = [g.getInlierMatches(s)[0] for s in range(S)]
    m3, ok3, w3, c3 = g.refitModelMono(e, reclassify=False)
    want = pkg.refit_model_mono(e, inl2, m2, ok2.astype(np.int32))
    assert m3.tobytes() == want[0].tobytes() and np.array_equal(ok3, want[1]) and w3.tobytes() == want[2].tobytes() and np.array_equal(c3, c2), what
    if rows is not None:   # a sequence handle: rows without a pair hold nothing
        assert all(n[r] == 0 and not ok1[r] and c2[r] == 0 and m1[r].tobytes() == bytes(128) for r in range(S) if r not in rows), (what, n, rows)
    return ok1


@pytest.mark.gpu
@pytest.mark.parametrize("method", [FLOW, QUAD])
def test_gpu_group_of_three(method, pkg, ob, gpu):
    """A plain group of S = 3 (one stream of constant images: empty lists) on flow and on quad lists."""
    dims = sr.dims_of(pkg)
    frames = [sr.frames_of(pkg, 3, seed) for seed in (81, 82, 83)]
    frames[1] = [(np.full_like(a, 90), np.full_like(b, 90)) for a, b in frames[1]]
    g = pkg.StreamGroup(3, pkg.Params.default())
    for t in range(3):
        g.pushBack(np.stack([f[t][0] for f in frames]), np.stack([f[t][1] for f in frames]) if method == QUAD else None, dims)
        if t == 0:
            continue
        g.matchFeatures(method)
        ok = refit_path(pkg, ob, g, f"group m{method} t{t}")
        assert not ok[1]
    g.close()


@pytest.mark.gpu
def test_gpu_sequence_handle_and_lone_matcher(pkg, ob, gpu):
    """A sequence handle across one chunk boundary (chunks of 4 and 2 frames: row 0 of the first and rows 2, 3 of the second
    hold no pair), and a lone matcher."""
    dims = sr.dims_of(pkg)
    frames = sr.frames_of(pkg, 6, 84)
    g = pkg.SequenceGroup(4, pkg.Params.default())
    g.pushBack(np.stack([frames[t][0] for t in range(4)]), None, dims)
    g.matchFeatures(FLOW)
    refit_path(pkg, ob, g, "sequence chunk 0", rows=(1, 2, 3))
    g.pushBack(np.stack([frames[t][0] for t in range(4, 6)]), None, dims)
    g.matchFeatures(FLOW)
    refit_path(pkg, ob, g, "sequence chunk 1", rows=(0, 1))
    g.close()
    m = pkg.Matcher(pkg.Params.default(), outlier_removal=False)
    for left, _ in frames[:2]:
        m.pushBack(left, None, dims)
    m.matchFeatures(FLOW)
    pm = m.getMatches()
    e = tm.hmono(pkg, inlier_threshold=3e-5)
    models = pkg.estimate_motion_mono(e, [pm], tm.rand8_of(ob, e, 1), model=True)[3]
    assert models["valid"][0] == 1.0
    c0 = m.motionInliersMono(e, models)
    inl0 = m.getInlierMatches()[0]
    m1, ok1, w1, c1 = m.refitModelMono(e)
    want = pkg.refit_model_mono(e, [inl0], models, [1])
    assert ok1 and c1 == c0 and m1.tobytes() == want[0].tobytes() and w1.tobytes() == want[2][0].tobytes()
    m2, ok2, w2, c2 = m.refitModelMono(e, reclassify=True)
    assert m2.tobytes() == m1.tobytes() and ok2
    flags, ninl, outs, poss = pkg.motion_inliers_mono(e, [pm], m2, [1])
    out, pos = m.getInlierMatches()
    assert c2 == ninl[0] and out.tobytes() == outs[0].tobytes() and np.array_equal(pos, poss[0])
    tm.check_against(pm, mo.inliers(pm, mo.from_array(m2[0]), e.inlier_threshold)[0], flags[0], c2, out, pos, "lone matcher")
    m3, ok3, w3, c3 = m.refitModelMono(e)
    want = pkg.refit_model_mono(e, [out], m2, [1])
    assert m3.tobytes() == want[0].tobytes() and ok3 == want[1][0] and w3.tobytes() == want[2][0].tobytes() and c3 == c2
    m.close()


def block_bounds(S):
    """The refit's block: 128 + 16 + 4 bytes per stream, each of the three arrays rounded up to 256 bytes at most."""
    return 148 * S, 148 * S + 3 * 255


@pytest.mark.gpu
def test_gpu_state_rules_off_state_and_failed_allocation(pkg, ob, gpu):
    """VH_ERR_STATE before a classification, after a stereo classification and after a push; a handle that never calls the
    entry holds the bytes of one that only classifies and has no mono_refit launch; a refused allocation is VH_ERR_HIP before
    any launch, leaves the bytes as they were, and the repeated call gives what the stateless form gives."""
    dims = sr.dims_of(pkg)
    frames = [sr.frames_of(pkg, 3, seed) for seed in (85, 86)]
    e = tm.hmono(pkg, inlier_threshold=3e-5)
    ego = ti.hego(pkg, inlier_threshold=2.5)
    state = pkg.VH_ERR_STATE
    seen = {}
    for name in ("off", "on"):
        g = pkg.StreamGroup(2, pkg.Params.default())
        g.profileEnable(True)
        expect(pkg, state, lambda: g.refitModelMono(e))                  # nothing pushed
        for t in range(2):
            g.pushBack(np.stack([f[t][0] for f in frames]), np.stack([f[t][1] for f in frames]), dims)
        g.matchFeatures(QUAD)
        expect(pkg, state, lambda: g.refitModelMono(e))                  # not classified yet
        g.motionInliers(ego, np.array([ti.TR2] * 2), np.ones(2, np.int32))
        expect(pkg, state, lambda: g.refitModelMono(e))                  # the current result is a stereo classification
        _, _, _, models = g.estimateMotionMono(e, tm.rand8_of(ob, e, 2), model=True)
        ok0 = models["valid"].astype(np.int32)
        g.motionInliersMono(e, models, ok0)
        expect(pkg, state, lambda: g.refitMotion(ego))                   # the stereo refit on a mono classification: as before
        bytes0 = g.deviceBytes()
        if name == "on":
            inl = [g.getInlierMatches(s)[0] for s in range(2)]
            want = pkg.refit_model_mono(e, inl, models, ok0)
            g.debugFailNextAlloc()
            expect(pkg, pkg.VH_ERR_HIP, lambda: g.refitModelMono(e, reclassify=True))
            assert g.deviceBytes() == bytes0 and g.profileRead(SCOPE)[1] == 0
            assert all(g.getInlierMatches(s)[0].tobytes() == inl[s].tobytes() for s in range(2))   # the handle is as it was
            m1, ok1, w1, _ = g.refitModelMono(e)                         # the repeated call
            assert m1.tobytes() == want[0].tobytes() and np.array_equal(ok1, want[1]) and w1.tobytes() == want[2].tobytes() and ok1.any()
            lo, hi = block_bounds(2)
            assert lo <= g.deviceBytes() - bytes0 <= hi, (g.deviceBytes() - bytes0, lo, hi)
            bytes1 = g.deviceBytes()
            g.refitModelMono(e, reclassify=True); g.refitModelMono(e)
            assert g.deviceBytes() == bytes1                             # one block, allocated once
        g.synchronize()
        seen[name] = (bytes0, g.profileRead(SCOPE)[1])
        g.pushBack(np.stack([f[2][0] for f in frames]), np.stack([f[2][1] for f in frames]), dims)
        expect(pkg, state, lambda: g.refitModelMono(e))                  # pushed: the pair the lists belong to is over
        g.close()
    assert seen["off"][0] == seen["on"][0] and seen["off"][1] == 0 and seen["on"][1] == 3
