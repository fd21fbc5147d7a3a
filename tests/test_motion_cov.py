"""Motion covariance: cov = ssr / (4N - 6) * (J^T J)^-1 of a stereo motion over whole quad lists
-- vh_motion_covariance on caller-owned lists, vh_group_motion_covariance / vh_match_motion_covariance on the compacted
inlier lists of a handle's stereo classification.  tests/cov_oracle.py is the restatement, in double (`covariance`) and
in a wider arithmetic (`covariance_ext`).

The GPU bound.  d_ref / d_ssr are the largest deviations of `covariance` from `covariance_ext` over SCENES (the lists of
the GPU parity tests, with and without reweighting, at a rotation and at tr = 0), in the measure
max_mn |dcov_mn| / sqrt(cov_mm cov_nn), resp. |dssr| / ssr: the double restatement's own error.  The device must lie
within 16 d_ref / 16 d_ssr of `covariance_ext`: it adds in another order (a tree, whose error bound is no worse than the
sequential sum's) and its sin / cos may differ from libm's by an ulp or two; a wrong term or dof misses by many orders.
Measured on the CPU (test_restatement_against_wider_arithmetic prints them): d_ref = 9.4e-14, d_ssr = 9.4e-14."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import cov_oracle as co
import refit_oracle as ro
import test_motion_inliers as mi
import test_motion_refit as mr
import test_post_dense as pd
import test_sequence_recon as sr
from conftest import ROOT
from egomotion_scene import EXACT, KITTI, two_motion_scene

SYMBOLS = ("vh_motion_covariance", "vh_group_motion_covariance", "vh_match_motion_covariance")
W = 256                          # VH_REFIT_THREADS
QUAD, FLOW = sr.QUAD, sr.FLOW
Cal, ptr, expect, noisy, P_MATCH = mr.Cal, mr.ptr, mr.expect, mr.noisy, mr.P_MATCH
TR = np.array(mr.TR) + 1e-4 * np.array([1, -1, 1, -1, 1, -1])   # near the scenes' motion, as a fitted motion is
MARGIN = 16

# ------------------------------------------------------------------------------------------------------------ lists
LENGTHS = (5, 6, 63, 64, 65, W - 1, W, W + 1, 4 * W + 1)
_CACHE = {}


def lists():
    if "lists" not in _CACHE:
        _CACHE["lists"] = [noisy(n, 900 + k) for k, n in enumerate(LENGTHS)]
    return _CACHE["lists"]


#: (reweighting, tr) of the parity tests
SETTINGS = ((0, TR), (1, TR), (0, np.zeros(6)), (1, np.zeros(6)))


def expectation(k):
    """SETTINGS[k] on every list, once -> [(double (cov, ssr, ok), wider (cov, ssr, ok))]"""
    if ("want", k) not in _CACHE:
        rw, tr = SETTINGS[k]
        cal = Cal(reweighting=rw, **KITTI)
        _CACHE["want", k] = [(co.covariance(pm, tr, cal), co.covariance_ext(pm, tr, cal)) for pm in lists()]
    return _CACHE["want", k]


def yardstick():
    """-> (d_ref, d_ssr) over SCENES = every list under every setting"""
    if "d" not in _CACHE:
        d_ref = d_ssr = 0.0
        for k in range(len(SETTINGS)):
            for (cov, ssr, ok), (cov_x, ssr_x, ok_x) in expectation(k):
                assert ok == ok_x
                if ok:
                    d_ref = max(d_ref, co.deviation(cov, cov_x)); d_ssr = max(d_ssr, co.deviation_ssr(ssr, ssr_x))
        _CACHE["d"] = (d_ref, d_ssr)
    return _CACHE["d"]


def rank_deficient():
    """300 identical records under the power-of-two intrinsics EXACT at tr = 0 (test_motion_refit.identical_list): every
    entry of A is an exact sum in any order and the elimination meets a pivot of exactly 0."""
    return mr.identical_list()


def host_cov(exe, tmp, pm, tr, cal, lanes):
    """tests/cpp/cov_check.cpp on one list -> (cov [6, 6], ssr, ok, same)"""
    fin, fout = str(tmp / "in"), str(tmp / "out")
    with open(fin, "wb") as fh:
        fh.write(np.array([cal.f, cal.cu, cal.cv, cal.base, cal.reweighting, *tr], np.float64).tobytes())
        fh.write(np.int64(len(pm)).tobytes()); fh.write(np.int64(lanes).tobytes()); fh.write(pm.tobytes())
    subprocess.check_call([exe, fin, fout], timeout=60)
    raw = open(fout, "rb").read()
    tail = np.frombuffer(raw[37 * 8:], np.int32)
    return np.frombuffer(raw[:288], np.float64).reshape(6, 6), float(np.frombuffer(raw[288:296], np.float64)[0]), int(tail[0]), int(tail[1])


# ------------------------------------------------------------------------------------------------------------ CPU
def test_symbols_declared_exported_mirrored_and_argument_errors(pkg):
    """The three symbols are declared, exported and mirrored, the Python wrappers exist; n_sets = 0 and lists without
    records are VH_OK without a device and zero the outputs; null and negative arguments are VH_ERR_INVALID_ARG."""
    header = open(os.path.join(ROOT, "include", "viso_hip.h")).read()
    lib = pkg._lib()
    for name in SYMBOLS:
        assert name + "(" in header and hasattr(C.CDLL(pkg.LIB_PATH), name) and name in pkg.ABI_SYMBOLS, name
    assert callable(pkg.motion_covariance) and "motionCovariance" in vars(pkg.Matcher) and "motionCovariance" in vars(pkg.StreamGroup)
    assert hasattr(pkg.SequenceGroup, "motionCovariance")
    e = pkg.EgoParams.default(**KITTI)
    pm = np.zeros(8, pkg.P_MATCH_DTYPE)
    off = np.array([0, 8], np.int32)
    tr = np.zeros((1, 6)); ok = np.ones(1, np.int32)
    cov = np.full((2, 36), 7.0); ssr = np.full(2, 7.0); oko = np.full(2, 7, np.int32)
    call = lib.vh_motion_covariance
    assert call(C.byref(e), 0, 0, None, None, None, None, None, None, None) == pkg.VH_OK
    empty = np.array([3, 3, 3], np.int32)
    assert call(C.byref(e), 0, 2, None, ptr(empty), ptr(np.zeros((2, 6))), ptr(np.ones(2, np.int32)), ptr(cov), ptr(ssr), ptr(oko)) == pkg.VH_OK
    assert not cov.any() and not ssr.any() and not oko.any()
    inv = pkg.VH_ERR_INVALID_ARG
    good = [C.byref(e), 0, 1, ptr(pm), ptr(off), ptr(tr), ptr(ok), ptr(cov), ptr(ssr), ptr(oko)]
    for k in (0, 3, 4, 5, 6, 7, 8, 9):
        args = list(good); args[k] = None
        assert call(*args) == inv, k
    args = list(good); args[2] = -1
    assert call(*args) == inv
    for bad in ([8, 0], [-1, 7]):
        args = list(good); args[4] = ptr(np.array(bad, np.int32))
        assert call(*args) == inv
    n = C.c_int32(0)
    assert lib.vh_group_motion_covariance(None, C.byref(e), None, None, ptr(cov), ptr(ssr), ptr(oko), ptr(oko)) == inv
    assert lib.vh_match_motion_covariance(None, C.byref(e), None, None, ptr(cov), ptr(ssr), C.byref(n), C.byref(n)) == inv


def test_restatement_against_wider_arithmetic():
    """`covariance` against `covariance_ext` over SCENES: d_ref and d_ssr are finite (printed: the yardstick of the GPU
    bound); both forms agree on ok everywhere, N = 5 is refused, cov is exactly symmetric; rows_in in float64 is
    refit_oracle.rows byte for byte; the fsum / Fraction form of covariance_ext agrees with the long double form."""
    d_ref, d_ssr = yardstick()
    print(f"d_ref = {d_ref:.3e}  d_ssr = {d_ssr:.3e}  (np.longdouble wider than double: {co.EXTENDED})")
    assert np.isfinite(d_ref) and np.isfinite(d_ssr)
    for k, (rw, tr) in enumerate(SETTINGS):
        for pm, ((cov, ssr, ok), _) in zip(lists(), expectation(k)):
            assert ok == (len(pm) >= 6) and np.array_equal(cov, cov.T)
            assert ok or (not cov.any() and ssr == 0.0)
    cal = Cal(reweighting=1, **KITTI)
    pm = lists()[4]
    J, res, _ = ro.rows(pm, list(TR), cal)
    J2, res2 = co.rows_in(pm, TR, cal, np.float64)
    assert J.tobytes() == J2.tobytes() and res.tobytes() == res2.tobytes()
    # (the fsum / Fraction form sums exactly, but its terms are float64: a residual is a difference of values near 600 px
    # that leaves about 0.3 px, 2e-13 relative per term before averaging -- 1e-12 is room for that, not a measured figure)
    a, b = co.covariance_ext(pm, TR, cal, extended=False), co.covariance_ext(pm, TR, cal)
    assert a[2] and b[2] and co.deviation(a[0], b[0]) <= 1e-12 and co.deviation_ssr(a[1], b[1]) <= 1e-12
    assert not co.covariance(pm, TR, cal, ok=False)[2]


def test_refusal_inputs_hold_their_premises():
    """On the restatement alone: the rank-deficient list is refused by the elimination (both forms); a list with a NaN
    record ends in the non-finite rule."""
    for rw in (0, 1):
        cal = Cal(reweighting=rw, **EXACT)
        J, res, _ = ro.rows(rank_deficient(), [0.0] * 6, cal)
        A, _ = ro.normal_equations(J, res)
        assert not co.matrix_solve(A, [[float(i == j) for j in range(6)] for i in range(6)])
        assert not co.covariance(rank_deficient(), np.zeros(6), cal)[2] and not co.covariance_ext(rank_deficient(), np.zeros(6), cal)[2]
        pm, start = mr.nan_list()
        for got in (co.covariance(pm, start, Cal(reweighting=rw, **KITTI)), co.covariance_ext(pm, start, Cal(reweighting=rw, **KITTI))):
            assert not got[2] and not got[0].any() and got[1] == 0.0


def test_shared_header_on_the_host_equals_the_restatement(tmp_path):
    """csrc/vh_ego.h (ego_accumulate<true>) and vh_gauss_jordan.h (vh_gauss_jordan_mem) compiled for the host with
    -ffp-contract=off: summed record after record, cov, ssr and ok are `covariance`'s byte for byte on every list and
    setting, the rank-deficient list and the NaN list; every column of the inverse is the single right-hand side form's
    bit for bit; summed in the kernel's shape, ok is the same and cov / ssr lie within the GPU bound of covariance_ext
    (the device differs from this form only by its sin and cos).  The largest ratio to the bound is printed."""
    exe = str(tmp_path / "cov_check")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", os.path.join(ROOT, "tests", "cpp", "cov_check.cpp"), "-lm", "-o", exe])
    d_ref, d_ssr = yardstick()
    worst = 0.0
    for k, (rw, tr) in enumerate(SETTINGS):
        cal = Cal(reweighting=rw, **KITTI)
        cases = [(pm, tr, cal, want, ext) for pm, (want, ext) in zip(lists(), expectation(k))]
        pm, start = mr.nan_list()
        cases.append((pm, start, cal, co.covariance(pm, start, cal), None))
        ecal = Cal(reweighting=rw, **EXACT)
        cases.append((rank_deficient(), np.zeros(6), ecal, co.covariance(rank_deficient(), np.zeros(6), ecal), None))
        for pm, t, c, (cov_w, ssr_w, ok_w), ext in cases:
            cov_s, ssr_s, ok_s, same = host_cov(exe, tmp_path, pm, t, c, 0)
            assert ok_s == int(ok_w) and same == 1, (k, len(pm))
            assert cov_s.tobytes() == cov_w.tobytes() and ssr_s == ssr_w, (k, len(pm))
            cov_k, ssr_k, ok_k, same = host_cov(exe, tmp_path, pm, t, c, W)
            assert ok_k == ok_s and same == 1 and np.array_equal(cov_k, cov_k.T), (k, len(pm))
            if ok_k and ext is not None:
                ratio = max(co.deviation(cov_k, ext[0]) / (MARGIN * d_ref), co.deviation_ssr(ssr_k, ext[1]) / (MARGIN * d_ssr))
                worst = max(worst, ratio)
                assert ratio <= 1.0, (k, len(pm), ratio)
    print(f"kernel-shaped sums against covariance_ext, largest share of the GPU bound: {worst:.3f}")


def test_covariance_predicts_the_scatter_of_the_estimate():
    """Monte Carlo on the restatement alone.  A fixed scene of 400 exact records under a true motion, no reweighting;
    K = 400 trials with independent Gaussian noise of 0.3 px on the four current coordinates; refit_oracle.refit finds each
    trial's minimum and `covariance` runs at it.  Per parameter, sample variance of the estimates / mean predicted
    variance lies in 1 +- 5 sqrt(2 / (K - 1)) = 1 +- 0.35: five standard deviations of a variance estimate.
    (K = 400 and sigma = 0.3 as first set: neither was changed.)"""
    K, sigma = 400, 0.3
    base = np.ascontiguousarray(two_motion_scene(P_MATCH, 400, 0, 77)[0])
    cal = Cal(reweighting=0, **KITTI)
    rng = np.random.default_rng(5)
    est, pred = [], []
    for _ in range(K):
        pm = base.copy()
        for name in ("u1c", "v1c", "u2c", "v2c"):
            pm[name] = (base[name].astype(np.float64) + rng.normal(0, sigma, len(pm))).astype(np.float32)
        tr, ok, _, _ = ro.refit(pm, np.array(mr.TR), cal)
        cov, ssr, ok2 = co.covariance(pm, tr, cal)
        assert ok and ok2
        est.append(tr); pred.append(np.diag(cov))
    ratio = np.var(np.array(est), axis=0, ddof=1) / np.mean(np.array(pred), axis=0)
    bound = 5 * np.sqrt(2 / (K - 1))
    print("sample variance / predicted variance per parameter:", np.round(ratio, 3), f"bound 1 +- {bound:.3f}")
    assert (np.abs(ratio - 1) <= bound).all(), ratio


# ------------------------------------------------------------------------------------------------------------ GPU
def check_cov(got, ext, n, what):
    """got = (cov, ssr, ok) of one list against covariance_ext's: ok exact, cov / ssr within MARGIN x the yardstick."""
    d_ref, d_ssr = yardstick()
    cov, ssr, ok = got
    assert bool(ok) == bool(ext[2]) == (n >= 6), (what, ok, ext[2])
    assert np.array_equal(cov, cov.T), what
    if not ok:
        assert not cov.any() and ssr == 0.0, what
        return
    dc, ds = co.deviation(cov, ext[0]), co.deviation_ssr(ssr, ext[1])
    print(f"{what}: cov {dc:.3e} (bound {MARGIN * d_ref:.3e})  ssr {ds:.3e} (bound {MARGIN * d_ssr:.3e})")
    assert dc <= MARGIN * d_ref and ds <= MARGIN * d_ssr, (what, dc, ds, d_ref, d_ssr)


@pytest.mark.gpu
@pytest.mark.parametrize("k", range(len(SETTINGS)))
def test_gpu_stateless_parity(k, pkg, gpu):
    """vh_motion_covariance on lists of 5 (refused), 6, 63, 64, 65, 255, 256, 257 and 1 025 records, with and without
    reweighting, at a rotation and at tr = 0: ok exact, cov and ssr within 16 d_ref / 16 d_ssr of covariance_ext, cov
    exactly symmetric; then one call holding an empty list and a list with ok = 0 whose tr is NaN between two long ones."""
    rw, tr = SETTINGS[k]
    e = pkg.EgoParams.default(reweighting=rw, **KITTI)
    ls = lists()
    cov, ssr, ok = pkg.motion_covariance(e, ls, np.tile(tr, (len(ls), 1)), np.ones(len(ls)))
    for i, (pm, (_, ext)) in enumerate(zip(ls, expectation(k))):
        check_cov((cov[i], ssr[i], ok[i]), ext, len(pm), (k, len(pm)))
    mixed = [ls[8], ls[8][:0], ls[7], ls[8]]
    trs = np.tile(tr, (4, 1)); trs[2] = np.nan
    cov2, ssr2, ok2 = pkg.motion_covariance(e, mixed, trs, [1, 1, 0, 1])
    assert list(ok2) == [True, False, False, True] and not cov2[1:3].any() and not ssr2[1:3].any()
    for i in (0, 3):
        assert cov2[i].tobytes() == cov[8].tobytes() and ssr2[i] == ssr[8]
    # inlier_threshold and ransac_iters are not read
    e2 = pkg.EgoParams.default(reweighting=rw, inlier_threshold=0.1, ransac_iters=1, **KITTI)
    assert pkg.motion_covariance(e2, [ls[8]], tr[None], [1])[0].tobytes() == cov[8].tobytes()


@pytest.mark.gpu
@pytest.mark.parametrize("rw", [0, 1])
def test_gpu_refusals(rw, pkg, gpu):
    """A list holding a NaN record: ok_out = 0 and zeros, VH_OK from the call.  A rank-deficient list: the ok_out the
    double restatement gives (it refuses, test_refusal_inputs_hold_their_premises)."""
    pm, start = mr.nan_list()
    cov, ssr, ok = pkg.motion_covariance(pkg.EgoParams.default(reweighting=rw, **KITTI), [pm], start[None], [1])
    assert not ok[0] and not cov.any() and ssr[0] == 0.0
    want = co.covariance(rank_deficient(), np.zeros(6), Cal(reweighting=rw, **EXACT))
    cov, ssr, ok = pkg.motion_covariance(pkg.EgoParams.default(reweighting=rw, **EXACT), [rank_deficient()], np.zeros((1, 6)), [1])
    assert bool(ok[0]) == want[2] and not want[2] and not cov.any() and ssr[0] == 0.0


@pytest.mark.gpu
def test_gpu_determinism_and_independence(pkg, gpu):
    """Two runs give the same bytes; a list gives the same bytes alone, among others in either order, and when its records
    are handed over at another offset."""
    e = pkg.EgoParams.default(**KITTI)
    ls = lists()
    alone = {}
    for sel in (list(range(9)), [8], [3, 8], list(range(8, -1, -1))):
        args = ([ls[i] for i in sel], np.tile(TR, (len(sel), 1)), np.ones(len(sel)))
        got, again = pkg.motion_covariance(e, *args), pkg.motion_covariance(e, *args)
        for a, b in zip(got, again):
            assert a.tobytes() == b.tobytes(), sel
        for j, i in enumerate(sel):
            one = (got[0][j].tobytes(), got[1][j].tobytes(), bool(got[2][j]))
            assert alone.setdefault(i, one) == one, (sel, i)
    # the same records behind 37 others that belong to no list (offsets[0] = 37)
    pm = np.concatenate([noisy(37, 5), ls[8]]).astype(pkg.P_MATCH_DTYPE)
    off = np.array([37, 37 + len(ls[8])], np.int32)
    cov = np.zeros((1, 36)); ssr = np.zeros(1); ok = np.zeros(1, np.int32)
    rc = pkg._lib().vh_motion_covariance(C.byref(e), 0, 1, ptr(pm), ptr(off), ptr(np.ascontiguousarray(TR[None])), ptr(np.ones(1, np.int32)),
                                         ptr(cov), ptr(ssr), ptr(ok))
    assert rc == pkg.VH_OK and (cov.tobytes(), ssr.tobytes(), bool(ok[0])) == alone[8]


@pytest.mark.gpu
def test_child_checking_build(pkg, gpu):
    """The stateless cases and the handle cases once more on libviso_hip_check.so (-DVH_CHECK)."""
    assert os.path.exists(pkg.CHECK_LIB_PATH), "build() makes it"
    env = dict(os.environ, VISO_HIP_LIB=pkg.CHECK_LIB_PATH)
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-q", "-x", "-m", "gpu", "-k",
                        "stateless_parity or group_of_three or state_rules"], env=env, capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "6 passed" in r.stdout and " skipped" not in r.stdout, r.stdout[-2000:]
    assert "VH_CHECK" not in r.stderr


def same_bytes(got, want, what):
    assert got[0].tobytes() == want[0].tobytes() and got[1].tobytes() == want[1].tobytes() and np.array_equal(got[2], want[2]), (what, got, want)


def check_handle_cov(pkg, ob, g, e, what, rows=None):
    """estimateMotion, motionInliers, then motionCovariance in its three uses, each byte-equal to the stateless entry on
    getInlierMatches under the motion in question; counts are the lists' lengths; rows without a pair have ok = 0."""
    S = g.S
    tr0, ok0, _ = g.estimateMotion(e, mi.rand3_of(ob, e, S))
    ok0 = ok0.astype(np.int32)
    counts = g.motionInliers(e, tr0, ok0)
    inl = [g.getInlierMatches(s)[0] for s in range(S)]
    got = g.motionCovariance(e)
    same_bytes(got, pkg.motion_covariance(e, inl, tr0, ok0), what)
    assert np.array_equal(got[3], counts), what
    if rows is not None:
        assert all(not got[2][r] and not got[0][r].any() for r in range(S) if r not in rows), (what, got[2])
    for s in range(S):
        assert bool(got[2][s]) <= bool(ok0[s] and counts[s] >= 6), (what, s)
    # reclassify = False: the refit's motion belongs to the lists it was fitted on -- handed over by the caller
    tr1, ok1, _, c1 = g.refitMotion(e)
    got1 = g.motionCovariance(e, tr=tr1, ok=ok1)
    same_bytes(got1, pkg.motion_covariance(e, inl, tr1, ok1), what)
    same_bytes(g.motionCovariance(e), got, what)                       # the classification's own motion is untouched
    # reclassify = True: the refined motion and its inliers, nothing uploaded
    tr2, ok2, _, c2 = g.refitMotion(e, reclassify=True)
    inl2 = [g.getInlierMatches(s)[0] for s in range(S)]
    got2 = g.motionCovariance(e)
    same_bytes(got2, pkg.motion_covariance(e, inl2, tr2, ok2), what)
    assert np.array_equal(got2[3], c2), what
    return got, got2, counts


@pytest.mark.gpu
def test_gpu_group_of_three(pkg, ob, gpu):
    """A group of S = 3 on 240 x 120 frames, one stream of constant images (empty lists) and one half-empty stream."""
    fr, dims = pd.frames_of(pkg), pd.dims_of(pkg)
    e = pd.ego_of(pkg)
    g = pkg.StreamGroup(pd.S, pkg.Params.default())
    accepted = 0
    for t in range(3):
        pd.push(g, fr, t, dims)
        if t == 0:
            continue
        g.matchFeatures(QUAD)
        got, got2, counts = check_handle_cov(pkg, ob, g, e, f"group t{t}")
        assert not got[2][1] and counts[1] == 0 and not got[0][1].any()
        accepted += int(got[2].sum()) + int(got2[2].sum())
    assert accepted >= 2
    g.close()


@pytest.mark.gpu
def test_gpu_sequence_handle_and_lone_matcher(pkg, ob, gpu):
    """A sequence handle with chunks of 4 and 2 frames (rows without a pair: ok_out = 0), and a lone matcher."""
    dims = sr.dims_of(pkg)
    frames = sr.frames_of(pkg, 6, 74)
    e = mi.hego(pkg, inlier_threshold=2.5)
    g = pkg.SequenceGroup(4, pkg.Params.default())
    sr.push(g, frames, 0, 4, dims)
    g.matchFeatures(QUAD)
    check_handle_cov(pkg, ob, g, e, "sequence chunk 0", rows=(1, 2, 3))
    sr.push(g, frames, 4, 2, dims)
    g.matchFeatures(QUAD)
    check_handle_cov(pkg, ob, g, e, "sequence chunk 1", rows=(0, 1))
    g.close()
    m = pkg.Matcher(pkg.Params.default(), outlier_removal=True)
    for left, right in frames[:2]:
        m.pushBack(left, right, dims)
    m.matchFeatures(QUAD)
    n = m.motionInliers(e, mi.TR2)
    inl = m.getInlierMatches()[0]
    assert n == len(inl) > 6
    cov, ssr, ok, cnt = m.motionCovariance(e)
    want = pkg.motion_covariance(e, [inl], np.array([mi.TR2]), [1])
    assert cov.tobytes() == want[0][0].tobytes() and ssr == want[1][0] and ok == bool(want[2][0]) and cnt == n
    tr1, ok1, _, _ = m.refitMotion(e)
    cov1, ssr1, okc1, _ = m.motionCovariance(e, tr=tr1, ok=ok1)
    want = pkg.motion_covariance(e, [inl], tr1[None], [ok1])
    assert cov1.tobytes() == want[0][0].tobytes() and ssr1 == want[1][0] and okc1 == bool(want[2][0])
    m.close()


@pytest.mark.gpu
def test_gpu_state_rules_failed_allocation_and_off_state(pkg, ob, gpu):
    """VH_ERR_STATE before a classification, after a mono classification, after the next match and push; tr without ok
    (and ok without tr) is VH_ERR_INVALID_ARG; a refused allocation is VH_ERR_HIP, leaves the bytes and the
    classification as they were, and the repeated call gives what a fresh handle gives; a handle that never calls the
    feature holds the parent's bytes and has no motion_cov launch, and motionInliers / refitMotion return what the
    stateless entries return."""
    dims = sr.dims_of(pkg)
    frames = sr.frames_of(pkg, 3, 75)
    e = mi.hego(pkg, inlier_threshold=2.5)
    tr = np.array([mi.TR2]); ok = np.ones(1, np.int32)
    state = pkg.VH_ERR_STATE
    g = pkg.StreamGroup(1, pkg.Params.default())
    g.profileEnable(True)
    cov = lambda: g.motionCovariance(e)  # noqa: E731
    expect(pkg, state, cov)                                           # nothing pushed
    g.pushBack(frames[0][0][None], frames[0][1][None], dims)
    g.pushBack(frames[1][0][None], frames[1][1][None], dims)
    g.matchFeatures(QUAD)
    expect(pkg, state, cov)                                           # not classified yet
    model = np.zeros(1, pkg.MONO_MODEL_DTYPE)
    mono = pkg.MonoParams.default(f=mi.HCAL["f"], cu=mi.HCAL["cu"], cv=mi.HCAL["cv"])
    g.motionInliersMono(mono, model, np.zeros(1, np.int32))
    expect(pkg, state, cov)                                           # a mono classification
    n0 = g.motionInliers(e, tr, ok)[0]
    flags0 = g.getInlierFlags(0).tobytes()
    inl = g.getInlierMatches(0)[0]
    expect(pkg, pkg.VH_ERR_INVALID_ARG, lambda: g.motionCovariance(e, tr=tr))
    expect(pkg, pkg.VH_ERR_INVALID_ARG, lambda: g.motionCovariance(e, ok=ok))
    # the off state: what the parent's handle holds and returns
    refit = g.refitMotion(e)
    want = pkg.refit_motion(e, [inl], tr, ok)
    assert refit[0].tobytes() == want[0].tobytes() and np.array_equal(refit[1], want[1]) and np.array_equal(refit[2], want[2]) and refit[3][0] == n0
    assert n0 == pkg.motion_inliers(e, [g.getMatches(0)], tr, ok)[1][0]
    g.synchronize()
    bytes0 = g.deviceBytes()
    assert g.profileRead("motion_cov")[1] == 0
    g.debugFailNextAlloc()
    expect(pkg, pkg.VH_ERR_HIP, cov)
    assert g.deviceBytes() == bytes0 and g.getInlierFlags(0).tobytes() == flags0
    g.synchronize()
    assert g.profileRead("motion_cov")[1] == 0                        # refused before any launch
    got = g.motionCovariance(e)                                       # the repeated call
    same_bytes(got, pkg.motion_covariance(e, [inl], tr, ok), "repeated")
    assert got[3][0] == n0 and g.deviceBytes() == bytes0 + 6 * 256     # five arrays rounded up to 256 bytes each; cov [36] takes 512
    g.synchronize()
    assert g.profileRead("motion_cov")[1] == 1
    g.matchFeatures(QUAD)
    expect(pkg, state, cov)                                           # the next match ends the classification
    g.motionInliers(e, tr, ok)
    g.pushBack(frames[2][0][None], frames[2][1][None], dims)
    expect(pkg, state, cov)                                           # pushed, not matched
    g.close()
    # a fresh handle that takes the same steps and never asks for the covariance: the same bytes, no launch
    h = pkg.StreamGroup(1, pkg.Params.default())
    h.profileEnable(True)
    h.pushBack(frames[0][0][None], frames[0][1][None], dims)
    h.pushBack(frames[1][0][None], frames[1][1][None], dims)
    h.matchFeatures(QUAD)
    h.motionInliersMono(mono, model, np.zeros(1, np.int32))
    h.motionInliers(e, tr, ok)
    again = h.refitMotion(e)
    h.synchronize()
    assert h.deviceBytes() == bytes0 and h.profileRead("motion_cov")[1] == 0
    assert again[0].tobytes() == refit[0].tobytes()
    h.close()
