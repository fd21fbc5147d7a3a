"""Motion refit: the reference's final optimisation (src/viso_stereo.cpp:126-139, updateParameters
with eps 1e-8 until it converges) on whole quad lists -- vh_refit_motion on caller-owned lists, vh_group_refit_motion /
vh_match_refit_motion on the compacted inlier lists of a handle's stereo classification.  tests/refit_oracle.py is the
restatement; the CPU part ties it to the pinned estimateMotion bit for bit and to the shared header compiled for the host
byte for byte, the GPU part holds the kernel to it: ok and n_updates exactly, tr within the bound worked out below.

The bound on tr.  The project's own is rtol 1e-9, atol 1e-12 (tests/test_egomotion.py).  The kernel sums the normal
equations in another order than the restatement; tests/cpp/refit_check.cpp restates that order on the host, and over all
parity lists (6 .. 9 000 records, reweighting 0 and 1) the two orders differ by at most 2.7e-15 absolute in tr (measured
on the CPU, asserted below to stay under a tenth of the project's bound) -- so the project's bound is used, the factor of
at least ten being the room for the device's sin and cos."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import refit_oracle as ro
import test_motion_inliers as mi
import test_sequence_recon as sr
from conftest import ROOT
from egomotion_scene import EXACT, KITTI, bad_disparity, rot, scene

SYMBOLS = ("vh_refit_motion", "vh_group_refit_motion", "vh_match_refit_motion")
W = 256                          # VH_REFIT_THREADS
FLOW, QUAD = sr.FLOW, sr.QUAD
TR = (0.004, -0.012, 0.002, 0.03, -0.01, -0.85)
RTOL, ATOL = 1e-9, 1e-12         # tests/test_egomotion.py:94
P_MATCH = np.dtype([(n, "<f4" if n[0] in "uv" else "<i4") for n in
                    ("u1p", "v1p", "i1p", "u2p", "v2p", "i2p", "u1c", "v1c", "i1c", "u2c", "v2c", "i2c")])   # Matcher::p_match


class Cal:
    """Calibration and parameters as the restatements read them: attributes by keyword."""
    def __init__(self, **kw):
        self.__dict__.update(kw)


def ptr(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def expect(pkg, code, call):
    with pytest.raises(pkg.VisoHipError) as e:
        call()
    assert e.value.code == code, e.value


def noisy(n, seed, tr=TR, noise=0.3, cal=KITTI):
    """n records: projections of 3-d points before and after the motion tr with uniform +-noise px on every coordinate."""
    rng = np.random.default_rng(seed)
    f, cu, cv, base = cal["f"], cal["cu"], cal["cv"], cal["base"]
    R, t = rot(*tr[:3]), np.array(tr[3:])
    Z = rng.uniform(4, 60, n)
    P = np.stack([rng.uniform(-1, 1, n) * Z * 0.9, rng.uniform(-0.3, 0.25, n) * Z, Z], 1)
    Q = P @ R.T + t
    Q[:, 2] = np.maximum(Q[:, 2], 2.0)
    vals = np.stack([f * P[:, 0] / P[:, 2] + cu, f * P[:, 1] / P[:, 2] + cv, f * (P[:, 0] - base) / P[:, 2] + cu, f * P[:, 1] / P[:, 2] + cv,
                     f * Q[:, 0] / Q[:, 2] + cu, f * Q[:, 1] / Q[:, 2] + cv, f * (Q[:, 0] - base) / Q[:, 2] + cu, f * Q[:, 1] / Q[:, 2] + cv], 1)
    vals += rng.uniform(-noise, noise, vals.shape)
    out = np.zeros(n, P_MATCH)
    for k, name in enumerate(("u1p", "v1p", "u2p", "v2p", "u1c", "v1c", "u2c", "v2c")):
        out[name] = vals[:, k].astype(np.float32)
    out["i1p"] = out["i2p"] = out["i1c"] = out["i2c"] = np.arange(n)
    return out


# ------------------------------------------------------------------------------------------------------------ lists
LENGTHS = (0, 5, 6, 7, 63, 64, 65, W - 1, W, W + 1, 2 * W + 1, 3073, 9000, 777, 130, 40, 1000)
#: seed of each list, chosen on the CPU so that test_parity_inputs_hold_their_premises holds
SEEDS = (300, 301, 625, 303, 304, 356, 306, 307, 308, 326, 344, 311, 312, 313, 314, 349, 316)
OK_IN = np.array([1, 1, 1, 1, 1, 1, 0, 1, 1, 1, 1, 1, 1, 1, 0, 1, 1], np.int32)
_PARITY = {}


def parity_lists(oracle, ob):
    """The 17 lists of the stateless parity test, built once, with their starts: zero motion (several updates), the
    estimator's tr (estimateMotion restated in C on the first 300 records, 50 samples) and the scene's motion perturbed
    by 1e-3, in turn.  -> (lists, starts [17, 6], ok_in [17])"""
    if "lists" not in _PARITY:
        lists, starts = [], []
        for k, (n, seed) in enumerate(zip(LENGTHS, SEEDS)):
            pm = noisy(n, seed)
            if k % 3 == 0 or n < 6:
                start = np.zeros(6)
            elif k % 3 == 1:
                head = np.ascontiguousarray(pm[:300]).view(ob.P_MATCH_DTYPE)
                e = ob.EgoParams.default(ransac_iters=50, **KITTI)
                ok, start, _ = oracle.estimate_motion_stereo(e, head, oracle.draw_samples(len(head), 50))
                assert ok, (n, seed)
            else:
                start = np.array(TR) + 1e-3 * np.random.default_rng(seed).uniform(-1, 1, 6)
            lists.append(pm); starts.append(start)
        _PARITY["lists"] = (lists, np.array(starts, np.float64), OK_IN)
    return _PARITY["lists"]


def parity_expectation(oracle, ob, rw):
    """The restatement's (tr, ok, n_updates, steps) of every parity list under reweighting rw, once."""
    if ("want", rw) not in _PARITY:
        lists, starts, oks = parity_lists(oracle, ob)
        cal = Cal(reweighting=rw, **KITTI)
        _PARITY["want", rw] = [ro.refit(pm, tr, cal, ok=bool(ok)) for pm, tr, ok in zip(lists, starts, oks)]
    return _PARITY["want", rw]


#: a list of 300 copies of one record under the power-of-two intrinsics EXACT and a zero start: every entry of the normal
#: equations is an exact sum in any order, and the elimination meets a pivot of exactly 0 in the first update (found by
#: a search over such records with the restatement; asserted in test_parity_inputs_hold_their_premises)
def identical_list():
    pm = np.zeros(300, P_MATCH)
    pm["u1p"] = 326; pm["u2p"] = 322; pm["v1p"] = pm["v2p"] = 128
    pm["u1c"] = 256; pm["u2c"] = 252; pm["v1c"] = pm["v2c"] = 129
    return pm


def nan_list():
    pm = noisy(500, 330)
    pm["u1c"][123] = np.nan
    return pm, np.array(TR) + 1e-3


def cap_list():
    """40 records with zero or negative disparity throughout (egomotion_scene.REFIT_FAIL_SEEDS): from a zero start under
    reweighting 1 the steps shrink by about a fifth per update and are still 3e-6 at the 102nd -- the cap, found by running
    the restatement over those scenes on the CPU; asserted in test_parity_inputs_hold_their_premises."""
    return bad_disparity(scene(P_MATCH, 40, 30, outliers=0.5)[0], 1.1, 30)[0]


def within_bound(got, want):
    return np.allclose(got, want, rtol=RTOL, atol=ATOL)


def host_refit(exe, tmp, pm, tr, cal, lanes):
    """tests/cpp/refit_check.cpp on one list -> (tr [6], ok, n_updates)"""
    fin, fout = str(tmp / "in"), str(tmp / "out")
    with open(fin, "wb") as fh:
        fh.write(np.array([cal.f, cal.cu, cal.cv, cal.base, cal.reweighting, *tr], np.float64).tobytes())
        fh.write(np.int64(len(pm)).tobytes()); fh.write(np.int64(lanes).tobytes()); fh.write(pm.tobytes())
    subprocess.check_call([exe, fin, fout], timeout=60)
    raw = open(fout, "rb").read()
    tail = np.frombuffer(raw[48:], np.int32)
    return np.frombuffer(raw[:48], np.float64), int(tail[0]), int(tail[1])


# ------------------------------------------------------------------------------------------------------------ CPU
def test_symbols_declared_exported_mirrored_and_argument_errors(pkg):
    """The three symbols are declared, exported and mirrored, the Python wrappers exist; n_sets = 0 and lists without
    records are VH_OK without a device; null and negative arguments are VH_ERR_INVALID_ARG."""
    header = open(os.path.join(ROOT, "include", "viso_hip.h")).read()
    lib = pkg._lib()
    for name in SYMBOLS:
        assert name + "(" in header and hasattr(C.CDLL(pkg.LIB_PATH), name) and name in pkg.ABI_SYMBOLS, name
    assert "int32_t vh_refit_motion(const vh_ego_params *e, int32_t device, int32_t n_sets, const vh_p_match *pm, const int32_t *offsets," in header
    assert "int32_t vh_group_refit_motion(vh_group *g, const vh_ego_params *e, int32_t reclassify, double *tr_out, int32_t *ok_out," in header
    assert "int32_t vh_match_refit_motion(vh_matcher *m, const vh_ego_params *e, int32_t reclassify, double *tr_out, int32_t *ok_out," in header
    assert callable(pkg.refit_motion) and "refitMotion" in vars(pkg.Matcher) and "refitMotion" in vars(pkg.StreamGroup)
    assert hasattr(pkg.SequenceGroup, "refitMotion")
    e = pkg.EgoParams.default(**KITTI)
    pm = np.zeros(8, pkg.P_MATCH_DTYPE)
    off = np.array([0, 8], np.int32)
    tr = np.zeros((1, 6)); ok = np.ones(1, np.int32)
    tro = np.full((2, 6), 7.0); oko = np.full(2, 7, np.int32); nu = np.full(2, 7, np.int32)
    call = lib.vh_refit_motion
    assert call(C.byref(e), 0, 0, None, None, None, None, None, None, None) == pkg.VH_OK
    empty = np.array([3, 3, 3], np.int32)
    assert call(C.byref(e), 0, 2, None, ptr(empty), ptr(np.zeros((2, 6))), ptr(np.ones(2, np.int32)), ptr(tro), ptr(oko), ptr(nu)) == pkg.VH_OK
    assert not tro.any() and not oko.any() and not nu.any()
    inv = pkg.VH_ERR_INVALID_ARG
    good = [C.byref(e), 0, 1, ptr(pm), ptr(off), ptr(tr), ptr(ok), ptr(tro), ptr(oko), ptr(nu)]
    for k in (0, 3, 4, 5, 6, 7, 8, 9):
        args = list(good); args[k] = None
        assert call(*args) == inv, k
    args = list(good); args[2] = -1
    assert call(*args) == inv
    for bad in ([8, 0], [-1, 7]):
        args = list(good); args[4] = ptr(np.array(bad, np.int32))
        assert call(*args) == inv
    n = C.c_int32(0)
    assert lib.vh_group_refit_motion(None, C.byref(e), 0, ptr(tro), ptr(oko), ptr(nu), ptr(nu)) == inv
    assert lib.vh_match_refit_motion(None, C.byref(e), 0, ptr(tro), C.byref(n), C.byref(n), C.byref(n)) == inv


@pytest.mark.parametrize("n,seed,noise", [(60, 2, 0.3), (250, 6, 0.3), (400, 1, 0.0)])
def test_restatement_is_the_pinned_estimate_motion(n, seed, noise, ob, oracle):
    """estimateMotion built from update_parameters (eps 1e-6, at most 22 updates per sample), inlier_oracle and refit on
    the winner's inliers equals vo_estimate_motion_stereo with the same samples bit for bit -- tr, ok and the inlier set --
    with 1 and 50 samples, reweighting 0 and 1."""
    pm, _ = scene(ob.P_MATCH_DTYPE, n, seed, noise=noise)
    for rw in (0, 1):
        for iters in (1, 50):
            e = ob.EgoParams.default(reweighting=rw, ransac_iters=iters, **KITTI)
            cal = Cal(reweighting=rw, inlier_threshold=e.inlier_threshold, **KITTI)
            samples = oracle.draw_samples(n, iters)
            ok_o, tr_o, inl_o = oracle.estimate_motion_stereo(e, pm, samples)
            ok_r, tr_r, inl_r = ro.estimate_motion(pm, samples, cal)
            assert ok_r == ok_o and np.array_equal(inl_r, inl_o), (rw, iters)
            assert np.asarray(tr_r, np.float64).tobytes() == tr_o.tobytes(), (rw, iters, tr_r, tr_o)
            assert ok_o or iters == 1


def test_parity_inputs_hold_their_premises(ob, oracle):
    """Asserted on the restatement alone: every list that is expected to converge does, its last step is at most 5e-9 and
    the step before it at least 2e-8 (so a rounding difference cannot change n_updates); zero starts take several
    updates; the identical list is refused by the first solve; the NaN list converges to NaN in one update; the cap list
    is still updating, by steps a hundred times eps, at the 102nd update."""
    lists, starts, oks = parity_lists(oracle, ob)
    assert tuple(len(pm) for pm in lists) == LENGTHS and len(lists) == 17 and 0 < oks.sum() < 17
    for rw in (0, 1):
        for k, (pm, (tr, ok, nupd, steps)) in enumerate(zip(lists, parity_expectation(oracle, ob, rw))):
            if len(pm) < 6 or not oks[k]:
                assert not ok and nupd == 0 and not np.any(tr)
                continue
            assert ok and 1 <= nupd <= 20 and steps[-1] <= 5e-9, (rw, k, steps)
            assert nupd == 1 or steps[-2] >= 2e-8, (rw, k, steps)
            if not starts[k].any():
                assert nupd >= 4, (rw, k, steps)
        tr, ok, nupd, _ = ro.refit(identical_list(), np.zeros(6), Cal(reweighting=rw, **EXACT))
        assert not ok and nupd == 1 and not np.any(tr)
        pm, start = nan_list()
        tr, ok, nupd, _ = ro.refit(pm, start, Cal(reweighting=rw, **KITTI))
        assert ok and nupd == 1 and np.isnan(tr).all()
    tr, ok, nupd, steps = ro.refit(cap_list(), np.zeros(6), Cal(reweighting=1, **KITTI))
    assert not ok and nupd == 102 and not np.any(tr) and min(steps) > 1e-6


def test_shared_header_on_the_host_equals_the_restatement(tmp_path, ob, oracle):
    """csrc/vh_ego.h (ego_observe, ego_rot, ego_accumulate, ego_solve) and vh_gauss_jordan.h compiled for the host with
    -ffp-contract=off: summed record after record, tr, ok and n_updates are the restatement's byte for byte on every
    parity list, the identical list and the NaN list; summed in refit_kernel's shape (lane stride, butterfly, waves in
    ascending order), ok and n_updates are the same and tr differs by less than a tenth of the project's bound -- which is
    why the GPU tests use the project's bound.  The largest difference is printed."""
    exe = str(tmp_path / "refit_check")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", os.path.join(ROOT, "tests", "cpp", "refit_check.cpp"), "-lm", "-o", exe])
    lists, starts, oks = parity_lists(oracle, ob)
    worst = 0.0
    for rw in (0, 1):
        cal = Cal(reweighting=rw, **KITTI)
        cases = [(pm, tr, cal, want) for pm, tr, ok, want in zip(lists, starts, oks, parity_expectation(oracle, ob, rw)) if ok]
        pm, start = nan_list()
        cases.append((pm, start, cal, ro.refit(pm, start, cal)))
        ecal = Cal(reweighting=rw, **EXACT)
        cases.append((identical_list(), np.zeros(6), ecal, ro.refit(identical_list(), np.zeros(6), ecal)))
        if rw:
            cases.append((cap_list(), np.zeros(6), cal, ro.refit(cap_list(), np.zeros(6), cal)))
        for pm, start, c, (tr_w, ok_w, n_w, _) in cases:
            tr_s, ok_s, n_s = host_refit(exe, tmp_path, pm, start, c, 0)
            assert (ok_s, n_s) == (int(ok_w), n_w) and tr_s.tobytes() == np.asarray(tr_w, np.float64).tobytes(), (rw, len(pm))
            tr_k, ok_k, n_k = host_refit(exe, tmp_path, pm, start, c, W)
            assert (ok_k, n_k) == (ok_s, n_s), (rw, len(pm))
            assert np.array_equal(np.isnan(tr_k), np.isnan(tr_s))
            if not np.isnan(tr_s).any():
                diff = np.abs(tr_k - tr_s)
                worst = max(worst, float(diff.max()))
                assert (diff <= 0.1 * (ATOL + RTOL * np.abs(tr_s))).all(), (rw, len(pm), diff)
    print(f"sequential against kernel-shaped sums, largest |tr difference| over the parity lists: {worst:.3e}")


def test_refit_makes_sense():
    """+-0.3 px noise, a start 1e-3 off in every component: the sum of squared weighted residuals does not grow, tr ends
    closer to the scene's motion than it started, and refitting the result takes one update.  (Dense lists: with a few
    hundred records the noise alone moves the optimum further from the scene's motion than the start is.)"""
    for n, seed, rw in ((9000, 340, 1), (20000, 341, 0)):
        pm = noisy(n, seed)
        cal = Cal(reweighting=rw, **KITTI)
        start = np.array(TR) + 1e-3 * np.random.default_rng(seed).choice([-1.0, 1.0], 6)
        tr, ok, nupd, _ = ro.refit(pm, start, cal)
        assert ok and nupd >= 2
        assert ro.cost(pm, tr, cal) <= ro.cost(pm, start, cal) * (1 + 1e-12)
        assert np.linalg.norm(tr - np.array(TR)) < np.linalg.norm(start - np.array(TR))
        tr2, ok2, nupd2, _ = ro.refit(pm, tr, cal)
        assert ok2 and nupd2 == 1 and within_bound(tr2, tr)


# ------------------------------------------------------------------------------------------------------------ GPU
def check_refit(got, want, what):
    tr, ok, nupd = got
    tr_w, ok_w, n_w, steps = want
    assert bool(ok) == bool(ok_w) and int(nupd) == n_w, (what, ok, nupd, ok_w, n_w, steps)
    assert np.array_equal(np.isnan(tr), np.isnan(tr_w)), (what, tr, tr_w)
    if not np.isnan(tr_w).any():
        assert within_bound(tr, tr_w), (what, tr, tr_w, np.abs(tr - tr_w).max())


def run_stateless_parity(pkg, ob, oracle, rw):
    lists, starts, oks = parity_lists(oracle, ob)
    want = parity_expectation(oracle, ob, rw)
    e = pkg.EgoParams.default(reweighting=rw, **KITTI)
    alone = {}
    for sel in (list(range(17)), [12], [3, 9], list(range(16, -1, -1))):
        args = ([lists[i] for i in sel], starts[sel], oks[sel])
        got = pkg.refit_motion(e, *args)
        again = pkg.refit_motion(e, *args)
        for a, b in zip(got, again):
            assert a.tobytes() == b.tobytes(), sel                     # from run to run
        for k, i in enumerate(sel):
            check_refit((got[0][k], got[1][k], got[2][k]), want[i], (rw, sel, i))
            one = (got[0][k].tobytes(), bool(got[1][k]), int(got[2][k]))
            assert alone.setdefault(i, one) == one, (rw, sel, i)       # alone, in a pair, among 17 in either order
    # inlier_threshold and ransac_iters are not read
    e2 = pkg.EgoParams.default(reweighting=rw, inlier_threshold=0.1, ransac_iters=1, **KITTI)
    assert pkg.refit_motion(e2, [lists[12]], starts[[12]], oks[[12]])[0].tobytes() == alone[12][0]


@pytest.mark.gpu
@pytest.mark.parametrize("rw", [0, 1])
def test_gpu_stateless_parity(rw, pkg, ob, oracle, gpu):
    """vh_refit_motion: ok and n_updates are the restatement's, tr within the project's bound, on lists of 0 .. 9 000
    records around every edge of the workgroup (6, 64, W, 2 W + 1), 1, 2 and 17 lists per call with mixed ok_in, starts at
    zero motion, at the estimator's tr and at a perturbed tr; byte-equal from run to run and whatever else the call holds."""
    run_stateless_parity(pkg, ob, oracle, rw)


@pytest.mark.gpu
@pytest.mark.parametrize("rw", [0, 1])
def test_gpu_identical_records_and_nan(rw, pkg, gpu):
    """A list of identical records: the first solve refuses, ok = 0, n_updates = 1, tr = 0.  A list with one NaN record:
    ok, n_updates and the NaN pattern of tr are the restatement's.  A list that is still updating at the 102nd update."""
    e = pkg.EgoParams.default(reweighting=rw, **EXACT)
    got = pkg.refit_motion(e, [identical_list()], np.zeros((1, 6)), np.ones(1))
    check_refit((got[0][0], got[1][0], got[2][0]), ro.refit(identical_list(), np.zeros(6), Cal(reweighting=rw, **EXACT)), "identical")
    assert not got[1][0] and got[2][0] == 1 and not got[0].any()
    pm, start = nan_list()
    e = pkg.EgoParams.default(reweighting=rw, **KITTI)
    got = pkg.refit_motion(e, [pm], start[None], np.ones(1))
    check_refit((got[0][0], got[1][0], got[2][0]), ro.refit(pm, start, Cal(reweighting=rw, **KITTI)), "nan")
    if rw:   # the update cap: still UPDATED after 102 calls
        got = pkg.refit_motion(e, [cap_list()], np.zeros((1, 6)), np.ones(1))
        check_refit((got[0][0], got[1][0], got[2][0]), ro.refit(cap_list(), np.zeros(6), Cal(reweighting=1, **KITTI)), "cap")
        assert not got[1][0] and got[2][0] == 102 and not got[0].any()


@pytest.mark.gpu
def test_child_checking_build(pkg, gpu):
    """The stateless cases once more on libviso_hip_check.so (-DVH_CHECK)."""
    assert os.path.exists(pkg.CHECK_LIB_PATH), "build() makes it"
    env = dict(os.environ, VISO_HIP_LIB=pkg.CHECK_LIB_PATH)
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-q", "-x", "-m", "gpu", "-k", "stateless_parity or identical_records"],
                       env=env, capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "4 passed" in r.stdout and " skipped" not in r.stdout, r.stdout[-2000:]
    assert "VH_CHECK" not in r.stderr


def check_handle_refit(pkg, ob, g, what, rows=None):
    """estimateMotion, motionInliers, refitMotion on the handle's current lists: tr / ok / n_updates byte-equal to the
    stateless entry on getInlierMatches(s) from the same start, counts untouched; then reclassify = True: the same refit,
    and flags, counts, records and positions byte-equal to a fresh motionInliers(tr_out, ok_out)."""
    e = mi.hego(pkg)
    tr0, ok0, _ = g.estimateMotion(e, mi.rand3_of(ob, e, g.S))
    ok0 = ok0.astype(np.int32)
    counts = g.motionInliers(e, tr0, ok0)
    inl = [g.getInlierMatches(s)[0] for s in range(g.S)]
    tr, ok, nupd, c1 = g.refitMotion(e)
    tr_s, ok_s, nupd_s = pkg.refit_motion(e, inl, tr0, ok0)
    assert tr.tobytes() == tr_s.tobytes() and np.array_equal(ok, ok_s) and np.array_equal(nupd, nupd_s), (what, tr, tr_s, nupd, nupd_s)
    assert np.array_equal(c1, counts) and all(g.getInlierMatches(s)[0].tobytes() == inl[s].tobytes() for s in range(g.S)), what
    for s in range(g.S):
        assert (nupd[s] >= 1) == bool(ok0[s] and counts[s] >= 6), (what, s, nupd, ok0, counts)
        assert ok[s] or not tr[s].any(), (what, s)
    if rows is not None:
        assert all(not ok[r] and nupd[r] == 0 for r in range(g.S) if r not in rows), (what, ok, nupd)
    again = g.refitMotion(e)                                          # the classification's own start is untouched: the same bytes
    assert again[0].tobytes() == tr.tobytes() and np.array_equal(again[2], nupd), what
    tr2, ok2, nupd2, c2 = g.refitMotion(e, reclassify=True)
    assert tr2.tobytes() == tr.tobytes() and np.array_equal(ok2, ok) and np.array_equal(nupd2, nupd), what
    seen = [(g.getInlierFlags(s).tobytes(), g.getInlierMatches(s)[0].tobytes(), g.getInlierMatches(s)[1].tobytes()) for s in range(g.S)]
    fresh = g.motionInliers(e, tr2, ok2.astype(np.int32))
    assert np.array_equal(c2, fresh), (what, c2, fresh)
    assert seen == [(g.getInlierFlags(s).tobytes(), g.getInlierMatches(s)[0].tobytes(), g.getInlierMatches(s)[1].tobytes()) for s in range(g.S)], what
    return ok, nupd, counts


@pytest.mark.gpu
@pytest.mark.parametrize("refinement,multi", [(0, False), (2, False), (0, True)])
def test_gpu_group_of_three(refinement, multi, pkg, ob, gpu):
    """A group of S = 3 (one stream of constant images: empty lists), refinement 0 and 2, multi-stage matching on."""
    dims = sr.dims_of(pkg)
    frames = [sr.frames_of(pkg, 3, seed) for seed in (71, 72, 73)]
    frames[1] = [(np.full_like(a, 90), np.full_like(b, 90)) for a, b in frames[1]]
    g = pkg.StreamGroup(3, pkg.Params.default(refinement=refinement, multi_stage=1 if multi else 0))
    if multi:
        g.setMultiStageMatching(True)
    started = 0
    for t in range(3):
        g.pushBack(np.stack([f[t][0] for f in frames]), np.stack([f[t][1] for f in frames]), dims)
        if t == 0:
            continue
        g.matchFeatures(QUAD)
        ok, nupd, counts = check_handle_refit(pkg, ob, g, f"group r{refinement} m{multi} t{t}")
        assert not ok[1] and nupd[1] == 0 and counts[1] == 0
        started += int((nupd >= 1).sum())
    assert started >= 2
    g.close()


@pytest.mark.gpu
def test_gpu_sequence_handle_and_lone_matcher(pkg, ob, gpu):
    """A sequence handle with chunks of 4 and 2 frames (rows without a pair: ok = 0, no update), and a lone matcher whose
    list removeOutliers replaced on the host."""
    dims = sr.dims_of(pkg)
    frames = sr.frames_of(pkg, 6, 74)
    g = pkg.SequenceGroup(4, pkg.Params.default())
    sr.push(g, frames, 0, 4, dims)
    g.matchFeatures(QUAD)
    check_handle_refit(pkg, ob, g, "sequence chunk 0", rows=(1, 2, 3))
    sr.push(g, frames, 4, 2, dims)
    g.matchFeatures(QUAD)
    check_handle_refit(pkg, ob, g, "sequence chunk 1", rows=(0, 1))
    g.close()
    m = pkg.Matcher(pkg.Params.default(), outlier_removal=True)
    for left, right in frames[:2]:
        m.pushBack(left, right, dims)
    m.matchFeatures(QUAD)
    e = mi.hego(pkg, inlier_threshold=2.5)
    n = m.motionInliers(e, mi.TR2)
    inl = m.getInlierMatches()[0]
    assert n == len(inl) > 6
    tr, ok, nupd, cnt = m.refitMotion(e)
    tr_s, ok_s, nupd_s = pkg.refit_motion(e, [inl], np.array([mi.TR2]), np.ones(1))
    assert tr.tobytes() == tr_s[0].tobytes() and ok == ok_s[0] and nupd == nupd_s[0] >= 1 and cnt == n
    tr2, ok2, nupd2, cnt2 = m.refitMotion(e, reclassify=True)
    assert tr2.tobytes() == tr.tobytes() and ok2 == ok and nupd2 == nupd
    seen = (m.getInlierMatches()[0].tobytes(), m.getInlierMatches()[1].tobytes())
    assert m.motionInliers(e, tr2, ok=ok2) == cnt2
    assert seen == (m.getInlierMatches()[0].tobytes(), m.getInlierMatches()[1].tobytes())
    m.close()


@pytest.mark.gpu
def test_gpu_state_rules_failed_allocation_and_off_state(pkg, ob, gpu):
    """VH_ERR_STATE before a classification, after a mono classification, after the next match and on flow lists; a
    refused allocation is VH_ERR_HIP, leaves the bytes and the classification as they were, and the repeated call gives
    what an undisturbed one gives; a handle that never calls the feature holds the same bytes and has no motion_refit
    launch, one that calls it grows by 56 bytes per stream (three arrays, each rounded up to 256 bytes)."""
    dims = sr.dims_of(pkg)
    frames = sr.frames_of(pkg, 3, 75)
    e = mi.hego(pkg, inlier_threshold=2.5)
    tr = np.array([mi.TR2]); ok = np.ones(1, np.int32)
    state = pkg.VH_ERR_STATE
    g = pkg.StreamGroup(1, pkg.Params.default())
    g.profileEnable(True)
    refit = lambda: g.refitMotion(e)  # noqa: E731
    expect(pkg, state, refit)                                         # nothing pushed
    g.pushBack(frames[0][0][None], frames[0][1][None], dims)
    g.pushBack(frames[1][0][None], frames[1][1][None], dims)
    g.matchFeatures(FLOW)
    expect(pkg, state, refit)                                         # flow lists, nothing classified
    model = np.zeros(1, pkg.MONO_MODEL_DTYPE)
    mono = pkg.MonoParams.default(f=mi.HCAL["f"], cu=mi.HCAL["cu"], cv=mi.HCAL["cv"])
    g.motionInliersMono(mono, model, np.zeros(1, np.int32))
    expect(pkg, state, refit)                                         # flow lists under a mono classification
    g.matchFeatures(QUAD)
    expect(pkg, state, refit)                                         # not classified yet
    g.motionInliersMono(mono, model, np.zeros(1, np.int32))
    expect(pkg, state, refit)                                         # a mono classification of quad lists
    n0 = g.motionInliers(e, tr, ok)[0]
    flags0 = g.getInlierFlags(0).tobytes()
    g.synchronize()
    bytes0 = g.deviceBytes()
    assert g.profileRead("motion_refit")[1] == 0                      # the off state: nothing allocated, nothing launched
    g.debugFailNextAlloc()
    expect(pkg, pkg.VH_ERR_HIP, refit)
    assert g.deviceBytes() == bytes0 and g.getInlierFlags(0).tobytes() == flags0
    g.synchronize()
    assert g.profileRead("motion_refit")[1] == 0                      # refused before any launch
    got = g.refitMotion(e)                                            # the repeated call
    want = pkg.refit_motion(e, [g.getInlierMatches(0)[0]], tr, ok)
    assert got[0].tobytes() == want[0].tobytes() and np.array_equal(got[1], want[1]) and np.array_equal(got[2], want[2]) and got[3][0] == n0
    assert g.deviceBytes() == bytes0 + 3 * 256
    g.refitMotion(e, reclassify=True)
    g.synchronize()
    assert g.deviceBytes() == bytes0 + 3 * 256 and g.profileRead("motion_refit")[1] == 2
    g.matchFeatures(QUAD)
    expect(pkg, state, refit)                                         # the next match ends the classification
    g.motionInliers(e, tr, ok)
    g.pushBack(frames[2][0][None], frames[2][1][None], dims)
    expect(pkg, state, refit)                                         # pushed, not matched
    g.close()
