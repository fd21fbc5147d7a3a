"""Mono motion inliers: the model the mono estimator exports (vh_estimate_motion_mono_model,
vh_group_estimate_motion_mono_model) and VisualOdometryMono::getInlier (reference src/viso_mono.cpp:268-315) on whole flow
and quad lists under such a model -- vh_motion_inliers_mono on caller-owned lists, vh_group_motion_inliers_mono /
vh_match_inliers_mono on the device-resident lists of a handle.  tests/mono_inlier_oracle.py is the restatement; the CPU
part ties it to the scene and to the host-compiled device functions, the GPU part holds the kernels to it byte for byte:
the test uses no transcendental function, so no record is excepted."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import mono_inlier_oracle as mo
import test_motion_inliers as ti   # its helpers: hip_read, the handle scenes
import test_sequence_recon as sr   # its helpers: the synthetic frames, expect()
from conftest import ROOT
from egomotion_scene import rot

SYMBOLS = ("vh_estimate_motion_mono_model", "vh_group_estimate_motion_mono_model", "vh_motion_inliers_mono",
           "vh_group_motion_inliers_mono", "vh_match_inliers_mono")
SCOPES = ("inlier_flag_mono", "inlier_compact")
FLOW, QUAD, STEREO = sr.FLOW, sr.QUAD, sr.STEREO
TILE = 1024                      # VH_INLIER_TILE
MONO_KITTI = dict(f=645.24, cu=635.96, cv=194.13, height=1.65)
TR = (0.002, -0.01, 0.001, 0.02, -0.005, -0.9)
THR = 0.00001                    # VisualOdometryMono::parameters' inlier_threshold
ptr, expect, hip_read = sr.ptr, sr.expect, ti.hip_read


def p_match_dtype():
    return ti._parity_dtype()


def projected(n, seed, tr=TR, outliers=0.2, ground=0.45, cal=MONO_KITTI):
    """n flow records (right-camera fields -1): exact projections of 3-d points before and after the motion tr, rounded
    to float, a share `ground` of them on the road plane; exactly round(outliers * n) records have their current position
    displaced by 15 .. 40 pixels in a random direction.  -> (p_match[n], displaced mask)"""
    rng = np.random.default_rng(seed)
    f, cu, cv, height = cal["f"], cal["cu"], cal["cv"], cal["height"]
    R, t = rot(*tr[:3]), np.array(tr[3:])
    out = np.zeros(n, p_match_dtype())
    for name in out.dtype.names:
        out[name] = -1
    bad = np.zeros(n, bool)
    bad[rng.permutation(n)[:int(round(outliers * n))]] = True
    k = 0
    while k < n:
        Z = rng.uniform(4, 50)
        if rng.random() < ground:
            X, Y = rng.uniform(-0.8, 0.8) * Z * 0.6, height
        else:
            X, Y = rng.uniform(-1, 1) * Z * 0.9, rng.uniform(-0.28, 0.02) * Z
        P = np.array([X, Y, Z]); Q = R @ P + t
        if Q[2] < 2:
            continue
        vals = np.array([f * P[0] / P[2] + cu, f * P[1] / P[2] + cv, f * Q[0] / Q[2] + cu, f * Q[1] / Q[2] + cv])
        if bad[k]:
            a, r = rng.uniform(0, 2 * np.pi), rng.uniform(15, 40)
            vals[2:] += r * np.array([np.cos(a), np.sin(a)])
        rec = out[k]
        rec["u1p"], rec["v1p"], rec["u1c"], rec["v1c"] = vals.astype(np.float32)
        rec["i1p"] = rec["i1c"] = k
        k += 1
    return out, bad


def mono_params(mod, **kw):
    return mod.MonoParams.default(**{**dict(ransac_iters=100, **MONO_KITTI), **kw})


def restated_model(ob, oracle, pm, **kw):
    """The model of a list: normalise(pm) + fundamentalMatrix on the pinned estimator's inlier set.  -> (model, ok, inliers)"""
    e = mono_params(ob, **kw)
    if len(pm) < 10:
        return dict(mo.ZERO_MODEL), False, np.zeros(0, np.int32)
    ok, _, inl = oracle.estimate_motion_mono(e, pm, oracle.draw_samples_n(len(pm), 8, e.ransac_iters))
    return mo.model_of(oracle.svd, pm, inl), ok, inl


# ------------------------------------------------------------------------------------------------------------ CPU
def test_symbols_declared_exported_mirrored_and_argument_errors(pkg):
    """Every new symbol is declared, exported and mirrored; vh_mono_model is 16 doubles; n_sets = 0 and lists without
    records are VH_OK without a device; null and negative arguments are VH_ERR_INVALID_ARG."""
    header = open(os.path.join(ROOT, "include", "viso_hip.h")).read()
    lib = pkg._lib()
    for name in SYMBOLS:
        assert name + "(" in header and hasattr(C.CDLL(pkg.LIB_PATH), name) and name in pkg.ABI_SYMBOLS, name
    assert "typedef struct vh_mono_model" in header and C.sizeof(pkg.MonoModel) == 128 == pkg.MONO_MODEL_DTYPE.itemsize
    assert [n for n, _ in pkg.MonoModel._fields_] == list(pkg.MONO_MODEL_DTYPE.names) == ["c", "s", "F", "valid"]
    assert pkg.abi_version() == 1
    assert callable(pkg.motion_inliers_mono) and "motionInliersMono" in vars(pkg.Matcher)
    assert "motionInliersMono" in vars(pkg.StreamGroup) and hasattr(pkg.SequenceGroup, "motionInliersMono")
    e = mono_params(pkg)
    pm = np.zeros(12, pkg.P_MATCH_DTYPE)
    off = np.array([0, 12], np.int32)
    model = np.zeros(1, pkg.MONO_MODEL_DTYPE); ok = np.ones(1, np.int32); fl = np.zeros(12, np.uint8); cnt = np.full(1, 7, np.int32)
    inv = pkg.VH_ERR_INVALID_ARG
    call = lambda *a: lib.vh_motion_inliers_mono(*a, None, None)  # noqa: E731
    assert call(C.byref(e), 0, 0, None, None, None, None, None, None) == pkg.VH_OK
    empty = np.array([3, 3, 3], np.int32); cnt2 = np.full(2, 7, np.int32)
    assert call(C.byref(e), 0, 2, None, ptr(empty), ptr(np.zeros(2, pkg.MONO_MODEL_DTYPE)), ptr(np.ones(2, np.int32)), None, ptr(cnt2)) == pkg.VH_OK
    assert cnt2.tolist() == [0, 0]
    good = [C.byref(e), 0, 1, ptr(pm), ptr(off), ptr(model), ptr(ok), ptr(fl), ptr(cnt)]
    for k in (0, 3, 4, 5, 6, 7, 8):
        assert call(*[None if j == k else a for j, a in enumerate(good)]) == inv, k
    assert call(C.byref(e), 0, -1, *good[3:]) == inv
    assert call(*good[:4], ptr(np.array([12, 0], np.int32)), *good[5:]) == inv
    assert call(*good[:4], ptr(np.array([-1, 3], np.int32)), *good[5:]) == inv
    n = C.c_int32(0)
    assert lib.vh_group_motion_inliers_mono(None, C.byref(e), ptr(model), ptr(ok), ptr(cnt)) == inv
    assert lib.vh_match_inliers_mono(None, C.byref(e), ptr(model), 1, C.byref(n)) == inv
    # the estimator entries: the plain entries' argument rules, and the model must be given
    r8 = np.zeros((1, e.ransac_iters, 8), np.int32); tr = np.zeros((1, 6)); ninl = np.zeros(1, np.int32)
    est = [C.byref(e), 0, 1, ptr(pm), ptr(off), ptr(r8), ptr(tr), ptr(ok), ptr(ninl), None, ptr(model)]
    for k in (0, 3, 4, 5, 6, 7, 8, 10):
        assert lib.vh_estimate_motion_mono_model(*[None if j == k else a for j, a in enumerate(est)]) == inv, k
    assert lib.vh_estimate_motion_mono_model(est[0], 0, 0, *est[3:]) == inv
    assert lib.vh_group_estimate_motion_mono_model(None, C.byref(e), ptr(r8), ptr(tr), ptr(ok), ptr(ninl), ptr(model)) == inv


MEANING_CASES = [(60, 1, 0.10), (150, 22, 0.30), (300, 29, 0.20), (40, 4, 0.25)]   # (n, seed, outliers); the seeds: see the test


@pytest.mark.parametrize("n,seed,outliers", MEANING_CASES)
def test_restatement_flags_the_true_correspondences(n, seed, outliers, ob, oracle):
    """On exact projections with 10-30 % gross outliers the restatement, under the model built from the pinned estimator's
    inlier set, flags every true correspondence and no displaced one.  Premise, asserted here: every true record's distance
    is below a tenth of the threshold and every displaced record's above ten times it (a displacement along the epipolar
    line would not be; the seeds are those for which none is)."""
    pm, bad = projected(n, seed, outliers=outliers)
    assert 0.1 * n - 1 <= bad.sum() <= 0.3 * n + 1
    model, ok, inl = restated_model(ob, oracle, pm)
    assert ok and model["valid"] == 1.0
    flags, d = mo.inliers(pm, model, THR)
    assert np.abs(d[~bad]).max() < THR / 10 and np.abs(d[bad]).min() > THR * 10, (np.abs(d[~bad]).max(), np.abs(d[bad]).min())
    assert np.array_equal(flags.astype(bool), ~bad)
    assert np.array_equal(np.flatnonzero(~bad), inl)   # ... and it is the set the estimator refitted on


def test_restatement_edges(ob, oracle):
    """F = 0: no inliers (0/0).  NaN and infinite coordinates are outliers, never errors.  ok = 0: no inliers.  A list of
    one record is classified like any other.  F and -F give equal flags and equal distances."""
    pm, bad = projected(80, 3)
    model, ok, _ = restated_model(ob, oracle, pm)
    flags, d = mo.inliers(pm, model, THR)
    assert ok and 0 < flags.sum() < len(pm)
    zero = dict(model, F=np.zeros(9))
    f0, d0 = mo.inliers(pm, zero, THR)
    assert f0.sum() == 0 and np.isnan(d0).all()
    q = pm.copy()
    good = np.flatnonzero(flags)[:8]
    for j, name in enumerate(("u1p", "v1p", "u1c", "v1c")):
        q[name][good[2 * j]] = np.nan; q[name][good[2 * j + 1]] = np.inf if j % 2 else -np.inf
    fq, dq = mo.inliers(q, model, THR)
    assert fq[good].sum() == 0 and not np.isfinite(dq[good]).any()
    rest = np.setdiff1d(np.arange(len(pm)), good)
    assert np.array_equal(fq[rest], flags[rest])
    assert mo.inliers(pm, model, THR, ok=False)[0].sum() == 0
    for i in (int(np.flatnonzero(flags)[0]), int(np.flatnonzero(flags == 0)[0])):
        assert mo.inliers(pm[i:i + 1], model, THR)[0][0] == flags[i]
    fn, dn = mo.inliers(pm, dict(model, F=-model["F"]), THR)
    assert fn.tobytes() == flags.tobytes() and dn.tobytes() == d.tobytes()


LENGTHS = (0, 1, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 3 * TILE + 1)
EXTRA = (777, 2049, 11, 130, 500)
_PARITY = {}


def parity_lists(ob, oracle):
    """The 17 lists of the stateless parity test with their models and ok flags, built once: one per length of LENGTHS and
    five more.  Models restated from the pinned estimator's inlier set, and hand-made ones: F = 0, a rank-1 F, huge scales,
    -F, NaN (under ok = 0, where the model is not read).  -> (lists, models [17 dicts], ok [17])"""
    if not _PARITY:
        base, _ = projected(400, 50)
        base_model = restated_model(ob, oracle, base)[0]
        assert base_model["valid"] == 1.0
        poison = dict(c=np.full(4, np.nan), s=np.full(2, np.nan), F=np.full(9, np.nan), valid=np.nan)
        lists, models, oks = [], [], []
        for k, n in enumerate(LENGTHS + EXTRA):
            pm, _ = projected(n, 100 + k, outliers=0.0 if n == 63 else 0.25)
            model, ok = (restated_model(ob, oracle, pm)[0] if n >= 40 else base_model), 1
            assert model["valid"] == 1.0, n
            if n == 64:        # no inlier: every current position far away
                pm["v1c"] += 50
            if n in (65, 11):  # ok = 0: the model is not read
                model, ok = poison, 0
            if n == 255:
                model = dict(model, F=np.zeros(9))
            if n == 256:       # NaN and infinities in every field that is read, one record each
                for j, name in enumerate(("u1p", "v1p", "u1c", "v1c")):
                    pm[name][3 * j] = np.nan; pm[name][3 * j + 1] = np.inf; pm[name][3 * j + 2] = -np.inf
            if n == 257:       # rank 1: F = a b^T
                model = dict(model, F=np.outer([0.3, -0.5, 0.01], [0.7, 0.2, -0.004]).reshape(9))
            if n == 1023:      # huge scales, finite floats: distances of the order of 1e60
                model = dict(model, s=model["s"] * 1e30)
            if n == 130:       # scales that carry every coordinate past the floats: inf coordinates, NaN distances
                model = dict(model, s=np.array([1e300, 1e300]))
            if n == 500:
                model = dict(model, F=-model["F"])
            lists.append(pm); models.append(model); oks.append(ok)
        _PARITY["v"] = (lists, models, np.array(oks, np.int32))
    return _PARITY["v"]


def parity_expectation(ob, oracle):
    """(flags, distances) of every parity list under THR, once."""
    if "want" not in _PARITY:
        lists, models, oks = parity_lists(ob, oracle)
        _PARITY["want"] = [mo.inliers(pm, m, THR, ok=bool(ok)) for pm, m, ok in zip(lists, models, oks)]
    return _PARITY["want"]


def test_parity_inputs_hold_their_premises(ob, oracle):
    """Every edge the GPU parity test names is in the lists."""
    lists, models, oks = parity_lists(ob, oracle)
    want = parity_expectation(ob, oracle)
    assert tuple(len(pm) for pm in lists[:len(LENGTHS)]) == LENGTHS and len(lists) == 17 and 0 < oks.sum() < 17
    by_len = {len(pm): w for pm, w in zip(lists, want)}
    assert by_len[63][0].all() and not by_len[64][0].any() and not by_len[65][0].any() and not by_len[11][0].any()
    assert not by_len[255][0].any() and np.isnan(by_len[255][1]).all()                       # F = 0
    f, d = by_len[256]
    assert not f[:12].any() and not np.isfinite(d[:12]).any() and f[12:].sum() > 100
    assert np.isfinite(by_len[257][1]).all()                                                    # rank 1
    f, d = by_len[1023]
    assert np.isfinite(d).all() and np.abs(d).min() > 1e50 and not f.any()                    # huge scales, finite floats
    assert not by_len[130][0].any() and not np.isfinite(by_len[130][1]).any()
    for n in (1024, 1025, 3 * TILE + 1, 777, 2049, 500):
        assert 0.6 * n < by_len[n][0].sum() < 0.9 * n, n
    assert by_len[1][0].tolist() == [1]


def test_device_functions_on_the_host_equal_the_restatement(tmp_path, ob, oracle):
    """csrc/vh_mono.h (mono_center, mono_scale, sampson_inlier: what inlier_flag_mono_kernel runs per record) compiled for the
    host with -ffp-contract=off: the flags of every parity list are the restatement's, byte for byte."""
    exe = str(tmp_path / "mono_inlier_check")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", os.path.join(ROOT, "tests", "cpp", "mono_inlier_check.cpp"), "-lm", "-o", exe])
    lists, models, oks = parity_lists(ob, oracle)
    want = parity_expectation(ob, oracle)
    dt = np.dtype([("c", "<f8", (4,)), ("s", "<f8", (2,)), ("F", "<f8", (9,)), ("valid", "<f8")])
    for k, (pm, model) in enumerate(zip(lists, models)):
        fin, fout = str(tmp_path / f"in{k}"), str(tmp_path / f"out{k}")
        with open(fin, "wb") as fh:
            fh.write(mo.as_array([model], dt).tobytes()); fh.write(np.float64(THR).tobytes())
            fh.write(np.int64(len(pm)).tobytes()); fh.write(pm.tobytes())
        subprocess.check_call([exe, fin, fout], timeout=60)
        got = np.fromfile(fout, np.uint8)
        assert got.tobytes() == mo.inliers(pm, model, THR)[0].tobytes(), (k, len(pm))
        if oks[k]:
            assert got.tobytes() == want[k][0].tobytes()


# ------------------------------------------------------------------------------------------------------------ GPU
def check_against(pm, want_flags, flags, count, out, pos, what):
    """Device results of one list against the restatement: everything byte-equal."""
    assert len(flags) == len(pm) and flags.dtype == np.uint8, what
    assert flags.tobytes() == want_flags.tobytes(), (what, np.flatnonzero(flags != want_flags)[:5])
    assert count == want_flags.sum() == len(out) == len(pos), what
    assert np.array_equal(pos, np.flatnonzero(want_flags)), what
    assert out.tobytes() == pm[pos].tobytes(), what


def run_stateless_parity(pkg, ob, oracle):
    lists, models, oks = parity_lists(ob, oracle)
    want = parity_expectation(ob, oracle)
    e = mono_params(pkg)
    marr = mo.as_array(models, pkg.MONO_MODEL_DTYPE)
    for sel in (list(range(17)), [8], [12, 3], list(range(16, -1, -1))):
        args = ([lists[i] for i in sel], marr[sel], oks[sel])
        flags, ninl, outs, poss = pkg.motion_inliers_mono(e, *args)
        again = pkg.motion_inliers_mono(e, *args)
        for k, i in enumerate(sel):
            check_against(lists[i], want[i][0], flags[k], ninl[k], outs[k], poss[k], (sel, i))
            assert flags[k].tobytes() == again[0][k].tobytes() and outs[k].tobytes() == again[2][k].tobytes()
            assert poss[k].tobytes() == again[3][k].tobytes() and ninl[k] == again[1][k]
    # only inlier_threshold of the parameters is read
    e2 = pkg.MonoParams.default(ransac_iters=1, inlier_threshold=THR, motion_threshold=1.0, height=9.0, pitch=0.3, f=2.0, cu=3.0, cv=4.0)
    assert pkg.motion_inliers_mono(e2, [lists[12]], marr[[12]], oks[[12]])[0][0].tobytes() == want[12][0].tobytes()


@pytest.mark.gpu
def test_gpu_stateless_parity(pkg, ob, oracle, gpu):
    """vh_motion_inliers_mono: flags, counts, compacted records and positions byte-equal to the restatement on lists of
    0 .. 3 * tile + 1 records, 1, 2 and 17 lists per call with mixed ok, restated and hand-made models (F = 0, rank 1, huge
    scales, -F), NaN and infinite coordinates, a list of inliers only and one without any; twice, byte-equal from run to run."""
    run_stateless_parity(pkg, ob, oracle)


@pytest.mark.gpu
def test_child_checking_build(pkg, gpu):
    """The parity and strict-compare cases once more on libviso_hip_check.so (-DVH_CHECK): every device-side index
    invariant verified."""
    import sys
    assert os.path.exists(pkg.CHECK_LIB_PATH), "build() makes it"
    env = dict(os.environ, VISO_HIP_LIB=pkg.CHECK_LIB_PATH)
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-q", "-x", "-m", "gpu", "-k", "stateless_parity or strict_compare"],
                       env=env, capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "4 passed" in r.stdout and " skipped" not in r.stdout, r.stdout[-2000:]
    assert "VH_CHECK" not in r.stderr


@pytest.mark.gpu
@pytest.mark.parametrize("which", ["small", "middle", "large"])
def test_gpu_strict_compare_at_the_threshold(which, pkg, ob, oracle, gpu):
    """inlier_threshold set to exactly a record's restated distance: the record is an outlier; with the next double above
    it, an inlier -- for a distance of the order of float rounding, one near the default threshold's decade and one of a
    displaced record."""
    lists, models, _ = parity_lists(ob, oracle)
    pm, model = lists[9], models[9]                      # 1024 records, a restated model
    d = np.abs(mo.inliers(pm, model, THR)[1])
    order = np.argsort(d)
    pos = d[order] > 0
    i = int({"small": order[pos][len(order[pos]) // 8], "middle": order[np.searchsorted(d[order], 1e-9)], "large": order[-5]}[which])
    assert d[i] > 0 and np.isfinite(d[i])
    marr = mo.as_array([model], pkg.MONO_MODEL_DTYPE)
    for thr, want_i in ((d[i], 0), (np.nextafter(d[i], np.inf), 1)):
        want = mo.inliers(pm, model, thr)[0]
        assert want[i] == want_i
        flags, ninl, outs, poss = pkg.motion_inliers_mono(mono_params(pkg, inlier_threshold=float(thr)), [pm], marr, np.ones(1))
        check_against(pm, want, flags[0], ninl[0], outs[0], poss[0], (which, thr))
        assert flags[0][i] == want_i


def same_model(got, want, what):
    """c, s, valid bit for bit; F bit for bit up to one common sign (the Sampson test is the same for F and -F)."""
    assert got["valid"] == want["valid"] and got["c"].tobytes() == np.asarray(want["c"], np.float64).tobytes(), (what, got, want)
    assert got["s"].tobytes() == np.asarray(want["s"], np.float64).tobytes(), (what, got, want)
    F, G = np.asarray(want["F"], np.float64), got["F"]
    assert G.tobytes() == F.tobytes() or G.tobytes() == (-F).tobytes(), (what, G, F)
    return G.tobytes() == F.tobytes()


@pytest.mark.gpu
def test_gpu_model_output(pkg, ob, oracle, gpu):
    """vh_estimate_motion_mono_model on lists of 9 records (valid = 0, zeros), 10 records, 400 and 700 exact projections with
    few outliers (700: the winner's inlier count is past the 640 rows the refit holds in LDS) and a list that fails after
    the refit (median depth above motion_threshold: ok = 0, valid = 1): c, s, F equal the restatement bit for bit, and
    tr / ok / n_inliers / inliers equal the plain entry's bit for bit."""
    lists = [projected(9, 60, outliers=0.0)[0], projected(10, 61, outliers=0.0)[0], projected(400, 62, outliers=0.05)[0],
             projected(700, 63, outliers=0.04)[0]]
    signs = []
    for kw, sel in (({}, [0, 1, 2, 3]), ({"motion_threshold": 1e-3}, [2])):
        e = mono_params(pkg, **kw)
        r8 = np.stack([ob.glibc_rand_after_srand0(8 * e.ransac_iters).reshape(e.ransac_iters, 8)] * len(sel))
        pms = [lists[i] for i in sel]
        tr, ok, inl, models = pkg.estimate_motion_mono(e, pms, r8, model=True)
        tr0, ok0, inl0 = pkg.estimate_motion_mono(e, pms, r8)
        assert tr.tobytes() == tr0.tobytes() and ok.tobytes() == ok0.tobytes()
        assert all(a.tobytes() == b.tobytes() for a, b in zip(inl, inl0))
        for k, pm in enumerate(pms):
            want, ok_w, inl_w = restated_model(ob, oracle, pm, **kw)
            assert ok[k] == ok_w and np.array_equal(inl[k], inl_w), (kw, len(pm))
            signs.append(same_model(mo.from_array(models[k]), want, (kw, len(pm))))
            if len(pm) == 9:
                assert models[k].tobytes() == bytes(128)
            if len(pm) >= 400:
                assert models[k]["valid"] == 1.0 and len(inl_w) > (640 if len(pm) == 700 else 300)
                assert bool(ok[k]) == (not kw)             # the small motion_threshold fails the list after the refit
                # the dense classification under the exported model is the estimator's inlier set on its own list
                flags = pkg.motion_inliers_mono(e, [pm], models[[k]], np.ones(1))[0][0]
                assert np.array_equal(np.flatnonzero(flags), mo.inliers(pm, want, THR)[0].nonzero()[0])
    assert all(signs), signs   # the refit's F has the restatement's sign on these lists


HCAL = dict(f=300.0, cu=160.0, cv=80.0, height=1.0)


def hmono(pkg, **kw):
    return pkg.MonoParams.default(**{**dict(ransac_iters=50, **HCAL), **kw})


def rand8_of(ob, e, S):
    r = ob.glibc_rand_after_srand0(8 * e.ransac_iters).reshape(e.ransac_iters, 8)
    return np.stack([r] * S)


def hand_models(pkg, g):
    """A model per stream that the flow of the synthetic frames (a pan of (5, 1) pixels) does not fit everywhere: the
    normalisation of the stream's own list and F = the essential matrix of a sideways translation with a small roll --
    records far from the image centre disagree."""
    rec, n = g.getMatchesAll()
    out = []
    for s in range(g.S):
        nrm = mo.normalise(rec[s, :n[s]])
        if nrm is None:
            out.append(dict(mo.ZERO_MODEL, valid=1.0, s=np.ones(2)))
            continue
        a = 0.004 + 0.001 * s
        out.append(dict(c=nrm[0], s=nrm[1], F=np.array([0, 0, 0.2, 0, 0, -1.0, -0.2 + a, 1.0, 0.0]), valid=1.0))
    return out


def check_handle(pkg, g, e, models, ok, what):
    """One classification of the handle's current lists under (models, ok): the flags are the restatement's on the lists
    getMatchesAll returns; the inlier matches are list[flags] with their positions; the per-stream form, the _all form and
    the device arrays agree.  -> counts"""
    rec, n = g.getMatchesAll()
    counts = g.motionInliersMono(e, mo.as_array(models, pkg.MONO_MODEL_DTYPE), ok)
    cap = max(int(n.max(initial=0)), 1)
    arec, apos, acnt = g.getInlierMatchesAll(cap)
    d_flags, d_pm, d_pos, stride = g.inliersDevice()
    assert np.array_equal(acnt, counts) and stride >= cap
    for s in range(g.S):
        pm = rec[s, :n[s]]
        want = mo.inliers(pm, models[s], e.inlier_threshold, ok=bool(ok[s]))[0]
        flags = g.getInlierFlags(s)
        out, pos = g.getInlierMatches(s)
        check_against(pm, want, flags, counts[s], out, pos, (what, s))
        assert arec[s, :acnt[s]].tobytes() == out.tobytes() and np.array_equal(apos[s, :acnt[s]], pos), (what, s)
        assert hip_read(d_flags + s * stride, n[s], np.uint8).tobytes() == flags.tobytes(), (what, s)
        assert hip_read(d_pm + s * stride * 48, counts[s], pkg.P_MATCH_DTYPE).tobytes() == out.tobytes(), (what, s)
        assert np.array_equal(hip_read(d_pos + s * stride * 4, counts[s], np.int32), pos), (what, s)
    return counts


def classify_twice(pkg, ob, g, what, rows=None):
    """Models from the estimator on the same lists, then hand-made ones with every ok set: the second call replaces the
    result.  Rows without a pair get a NaN model, which must not be read."""
    e = hmono(pkg)
    tr, ok, ninl, models = g.estimateMotionMono(e, rand8_of(ob, e, g.S), model=True)
    plain = g.estimateMotionMono(e, rand8_of(ob, e, g.S))
    assert tr.tobytes() == plain[0].tobytes() and np.array_equal(ok, plain[1]) and np.array_equal(ninl, plain[2]), what
    _, n = g.getMatchesAll()
    est = [mo.from_array(m) for m in models]
    valid = np.array([m["valid"] for m in est])
    assert np.array_equal(valid == 1.0, ninl >= 10), (what, valid, ninl)
    for s in range(g.S):
        if n[s] == 0:
            est[s] = dict(c=np.full(4, np.nan), s=np.full(2, np.nan), F=np.full(9, np.nan), valid=0.0)
    c1 = check_handle(pkg, g, e, est, valid.astype(np.int32), what + " estimated")
    assert all(c1[s] >= 10 for s in range(g.S) if valid[s]), (what, c1, ninl)   # (the refit F, not the winning hypothesis': the counts need not be equal)
    e2 = hmono(pkg, inlier_threshold=3e-5)
    c2 = check_handle(pkg, g, e2, hand_models(pkg, g), np.ones(g.S, np.int32), what + " given")
    if rows is not None:   # a sequence handle: rows without a pair hold nothing
        assert all(n[r] == 0 and c1[r] == 0 and c2[r] == 0 for r in range(g.S) if r not in rows), (what, n, rows)
        assert all(n[r] > 100 for r in rows), (what, n)
    assert 0 < c2.sum() < n.sum(), (what, c2, n)
    return c1, c2


@pytest.mark.gpu
@pytest.mark.parametrize("method,refinement,multi", [(FLOW, 0, False), (QUAD, 0, False), (FLOW, 2, False), (QUAD, 2, False), (FLOW, 0, True)])
def test_gpu_group_of_three(method, refinement, multi, pkg, ob, gpu):
    """A group of S = 3 (one stream of constant images: empty lists) on flow and on quad lists, refinement 0 and 2,
    multi-stage matching on; at the end the lists are replaced by vh_group_remove_outliers and classified once more."""
    dims = sr.dims_of(pkg)
    frames = [sr.frames_of(pkg, 3, seed) for seed in (71, 72, 73)]
    frames[1] = [(np.full_like(a, 90), np.full_like(b, 90)) for a, b in frames[1]]
    g = pkg.StreamGroup(3, pkg.Params.default(refinement=refinement, multi_stage=1 if multi else 0))
    if multi:
        g.setMultiStageMatching(True)
    for t in range(3):
        g.pushBack(np.stack([f[t][0] for f in frames]), np.stack([f[t][1] for f in frames]) if method == QUAD else None, dims)
        if t == 0:
            continue
        g.matchFeatures(method)
        c1, c2 = classify_twice(pkg, ob, g, f"group m{method} r{refinement} m{multi} t{t}")
        assert c1[1] == 0 and c2[1] == 0
    before = g.getMatchesAll()[1]
    g.removeOutliers(2)
    assert (g.getMatchesAll()[1] <= before).all()
    e2 = hmono(pkg, inlier_threshold=3e-5)
    c3 = check_handle(pkg, g, e2, hand_models(pkg, g), np.ones(3, np.int32), "group, voted lists")
    assert 0 < c3.sum() < g.getMatchesAll()[1].sum()
    g.close()


@pytest.mark.gpu
def test_gpu_sequence_handle_and_lone_matcher(pkg, ob, gpu):
    """A sequence handle with chunks of 4 and 2 frames (row 0 of the first chunk and rows 2, 3 of the second hold no pair:
    count 0, their model -- NaN here -- is not read), and a lone matcher with and without removeOutliers."""
    dims = sr.dims_of(pkg)
    frames = sr.frames_of(pkg, 6, 74)
    g = pkg.SequenceGroup(4, pkg.Params.default())
    g.pushBack(np.stack([frames[t][0] for t in range(4)]), None, dims)
    g.matchFeatures(FLOW)
    classify_twice(pkg, ob, g, "sequence chunk 0", rows=(1, 2, 3))
    g.pushBack(np.stack([frames[t][0] for t in range(4, 6)]), None, dims)
    g.matchFeatures(FLOW)
    classify_twice(pkg, ob, g, "sequence chunk 1", rows=(0, 1))
    g.close()
    for removal in (True, False):   # matchFeatures ends with removeOutliers on the host, or leaves the device list as it is
        m = pkg.Matcher(pkg.Params.default(), outlier_removal=removal)
        for left, _ in frames[:2]:
            m.pushBack(left, None, dims)
        m.matchFeatures(FLOW)
        pm = m.getMatches()
        e = hmono(pkg, inlier_threshold=3e-5)
        nrm = mo.normalise(pm)
        model = dict(c=nrm[0], s=nrm[1], F=np.array([0, 0, 0.2, 0, 0, -1.0, -0.196, 1.0, 0.0]), valid=1.0)
        f, _ = mo.inliers(pm, model, e.inlier_threshold)
        assert 0 < f.sum() < len(pm)
        marr = mo.as_array([model], pkg.MONO_MODEL_DTYPE)
        assert m.motionInliersMono(e, marr) == f.sum()
        out, pos = m.getInlierMatches()
        assert np.array_equal(pos, np.flatnonzero(f)) and out.tobytes() == pm[f == 1].tobytes()
        assert m.motionInliersMono(e, marr, ok=False) == 0 and len(m.getInlierMatches()[0]) == 0
        m.close()


def model_bytes(S):
    return 128 * S


@pytest.mark.gpu
def test_gpu_state_rules_capacity_and_failed_allocation(pkg, ob, gpu):
    """VH_ERR_STATE before any push, before any match and on stereo lists; the stereo classifier on flow lists is still
    VH_ERR_STATE; mono after stereo on the same quad lists replaces the result and the other way round; the getters after
    the next match call; the capacity rule; a refused allocation of the main block and of the model block is VH_ERR_HIP,
    leaves the device bytes as they were, and the repeated call gives what an undisturbed one gives with the bytes the
    formula says."""
    lib = pkg._lib()
    dims = sr.dims_of(pkg)
    frames = sr.frames_of(pkg, 3, 75)
    e = hmono(pkg, inlier_threshold=3e-5)
    ego = ti.hego(pkg, inlier_threshold=2.5)
    tr = np.array([ti.TR2]); ok = np.ones(1, np.int32)
    g = pkg.StreamGroup(1, pkg.Params.default())
    getters = (lambda: g.getInlierFlags(0), lambda: g.getInlierMatches(0), lambda: g.getInlierMatchesAll(8), g.inliersDevice)
    state = pkg.VH_ERR_STATE
    anym = np.zeros(1, pkg.MONO_MODEL_DTYPE)
    expect(pkg, state, lambda: g.motionInliersMono(e, anym, ok))      # nothing pushed
    g.pushBack(frames[0][0][None], frames[0][1][None], dims)
    expect(pkg, state, lambda: g.motionInliersMono(e, anym, ok))      # nothing matched
    g.pushBack(frames[1][0][None], frames[1][1][None], dims)
    g.matchFeatures(STEREO)
    expect(pkg, state, lambda: g.motionInliersMono(e, anym, ok))      # stereo lists carry no flow
    g.matchFeatures(FLOW)
    expect(pkg, state, lambda: g.motionInliers(ego, tr, ok))          # the stereo test on flow lists: as before
    for call in getters:
        expect(pkg, state, call)                                      # not classified yet
    pm = g.getMatches(0)
    model = hand_models(pkg, g)
    marr = mo.as_array(model, pkg.MONO_MODEL_DTYPE)
    f, _ = mo.inliers(pm, model[0], e.inlier_threshold)
    assert 1 < f.sum() < len(pm)
    bytes0 = g.deviceBytes()
    g.debugFailNextAlloc()                                            # the main block
    expect(pkg, pkg.VH_ERR_HIP, lambda: g.motionInliersMono(e, marr, ok))
    assert g.deviceBytes() == bytes0
    g.debugFailAllocAfter(1)                                          # the model block, after the main block succeeded
    expect(pkg, pkg.VH_ERR_HIP, lambda: g.motionInliersMono(e, marr, ok))
    assert g.deviceBytes() == bytes0
    for call in getters:
        expect(pkg, state, call)
    assert g.motionInliersMono(e, marr, ok)[0] == f.sum()             # the repeated call
    stride = g.inliersDevice()[3]
    tiles = (stride + TILE - 1) // TILE
    grown = g.deviceBytes() - bytes0
    assert 53 * stride + 4 * tiles + 56 + model_bytes(1) <= grown <= 53 * stride + 4 * tiles + 56 + 7 * 255 + model_bytes(1), (grown, stride)
    assert g.getInlierFlags(0).tobytes() == f.tobytes()
    out, pos = g.getInlierMatches(0)
    assert out.tobytes() == pm[f == 1].tobytes() and np.array_equal(pos, np.flatnonzero(f))
    # capacity rule: the full number, the first cap elements, VH_ERR_CAPACITY
    n = C.c_int32(0)
    k = int(f.sum())
    buf = np.zeros(k, pkg.P_MATCH_DTYPE); bpos = np.full(k, -7, np.int32); bfl = np.full(len(pm), 9, np.uint8)
    assert lib.vh_group_get_inlier_matches(g._h, 0, ptr(buf), ptr(bpos), k - 1, C.byref(n)) == pkg.VH_ERR_CAPACITY
    assert n.value == k and buf[:k - 1].tobytes() == out[:k - 1].tobytes() and bpos[k - 1] == -7 and np.array_equal(bpos[:k - 1], pos[:k - 1])
    assert lib.vh_group_get_inlier_flags(g._h, 0, ptr(bfl), len(pm) - 1, C.byref(n)) == pkg.VH_ERR_CAPACITY
    assert n.value == len(pm) and bfl[:-1].tobytes() == f[:-1].tobytes() and bfl[-1] == 9
    # the next match call ends the classification; quad lists take both tests, each replacing the other's result
    g.matchFeatures(QUAD)
    for call in getters:
        expect(pkg, state, call)
    pm = g.getMatches(0)
    model = hand_models(pkg, g); marr = mo.as_array(model, pkg.MONO_MODEL_DTYPE)
    fm, _ = mo.inliers(pm, model[0], e.inlier_threshold)
    fs, ss = ti.io.inliers(pm, ti.TR2, ti._Cal(inlier_threshold=2.5, **ti.HCAL))
    assert not ti.io.near_threshold(ss, ti._Cal(inlier_threshold=2.5, **ti.HCAL), 1e-9).any() and fm.tobytes() != fs.tobytes()
    bytes1 = g.deviceBytes()
    for _ in range(2):
        assert g.motionInliers(ego, tr, ok)[0] == fs.sum() and g.getInlierFlags(0).tobytes() == fs.tobytes()
        assert g.motionInliersMono(e, marr, ok)[0] == fm.sum() and g.getInlierFlags(0).tobytes() == fm.tobytes()
        out, pos = g.getInlierMatches(0)
        assert out.tobytes() == pm[fm == 1].tobytes() and np.array_equal(pos, np.flatnonzero(fm))
    assert g.deviceBytes() == bytes1                                  # one result, one set of blocks
    g.pushBack(frames[2][0][None], frames[2][1][None], dims)
    expect(pkg, state, lambda: g.motionInliersMono(e, marr, ok))      # pushed, not matched
    g.close()
    # a handle whose first classification is the stereo one allocates what it always did: no model block
    g = pkg.StreamGroup(1, pkg.Params.default())
    for t in range(2):
        g.pushBack(frames[t][0][None], frames[t][1][None], dims)
    g.matchFeatures(QUAD)
    b0 = g.deviceBytes()
    g.motionInliers(ego, tr, ok)
    b1 = g.deviceBytes()
    stride = g.inliersDevice()[3]
    assert 53 * stride + 4 * ((stride + TILE - 1) // TILE) + 56 <= b1 - b0 <= 53 * stride + 4 * ((stride + TILE - 1) // TILE) + 56 + 7 * 255
    g.motionInliersMono(e, mo.as_array(hand_models(pkg, g), pkg.MONO_MODEL_DTYPE), ok)
    assert g.deviceBytes() - b1 == model_bytes(1)
    g.close()


@pytest.mark.gpu
def test_gpu_unused_means_untouched(pkg, ob, gpu):
    """A handle that runs the estimator without a model and never classifies holds the bytes it held before this feature
    existed -- those of a handle that only matches plus the plain estimator's blocks (its scratch, tr, ok / n_inliers and
    the random draws, by the formulas of csrc/kernels_mono.hip and Group::estimate_motion_mono), and so those of a handle
    that also asks for the models less their 128 bytes per stream -- and has no inlier_flag_mono launch; its results equal
    those of the handle that uses the feature."""
    dims = sr.dims_of(pkg)
    frames = [sr.frames_of(pkg, 3, seed) for seed in (76, 77)]
    e = hmono(pkg)
    seen = {}
    for name in ("match", "off", "model", "on"):
        g = pkg.StreamGroup(2, pkg.Params.default())
        g.profileEnable(True)
        res = []
        for t in range(3):
            g.pushBack(np.stack([f[t][0] for f in frames]), None, dims)
            if t == 0:
                continue
            g.matchFeatures(FLOW)
            if name == "match":
                continue
            r = g.estimateMotionMono(e, rand8_of(ob, e, 2), model=name != "off")
            res.append((r[0].tobytes(), r[1].tobytes(), r[2].tobytes()))
            if name == "on":
                g.motionInliersMono(e, r[3], r[3]["valid"].astype(np.int32))
                stride = g.inliersDevice()[3]
        g.synchronize()
        seen[name] = (res, g.deviceBytes(), [g.profileRead(k)[1] for k in SCOPES])
        g.close()
    assert seen["off"][0] == seen["model"][0] == seen["on"][0]
    assert seen["off"][2] == [0, 0] and seen["model"][2] == [0, 0] and seen["on"][2] == [2, 2]
    assert seen["model"][1] - seen["off"][1] == model_bytes(2)
    S, cap, it = 2, stride, e.ransac_iters
    per_list = (236 * cap + 1024 + 8 + 15) // 16 * 16                     # mono_per_list(cap)
    queue = 16 + (S * it * 4 + 15) // 16 * 16                             # mono_queue_bytes
    estimator = (S * per_list + queue + S * it * 72) + 48 * S + 8 * S + 4 * S * it * 8   # scratch | tr | ok, n_inliers | rand8
    assert seen["off"][1] - seen["match"][1] == estimator, (seen["off"][1], seen["match"][1], estimator)
    slots, tiles = 2 * stride, 2 * ((stride + TILE - 1) // TILE)
    grown = seen["on"][1] - seen["model"][1]
    low = 53 * slots + 4 * tiles + 56 * 2 + model_bytes(2)
    assert low <= grown <= low + 7 * 255, (grown, slots, tiles)
