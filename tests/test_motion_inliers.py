"""Motion inliers: VisualOdometryStereo::getInlier (reference src/viso_stereo.cpp:159-177) on whole
match lists under a given motion -- vh_motion_inliers on caller-owned lists, vh_group_motion_inliers / vh_match_inliers on
the device-resident lists of a handle, and their getters.  tests/inlier_oracle.py is the restatement; the CPU part ties it
to the estimator's own inlier set, the GPU part holds the kernels to it byte for byte."""
import ctypes as C
import os

import numpy as np
import pytest

import inlier_oracle as io
import test_sequence_recon as sr   # its helpers: the synthetic frames, expect()
from conftest import ROOT
from egomotion_scene import rot

SYMBOLS = ("vh_motion_inliers", "vh_group_motion_inliers", "vh_match_inliers", "vh_group_get_inlier_flags",
           "vh_group_get_inlier_matches", "vh_group_get_inlier_matches_all", "vh_get_inlier_matches", "vh_group_inliers_device")
SCOPES = ("inlier_flag", "inlier_compact")
FLOW, QUAD = sr.FLOW, sr.QUAD
TILE = 1024                      # VH_INLIER_TILE
KITTI = dict(f=645.24, cu=635.96, cv=194.13, base=0.5707)
TR = (0.004, -0.012, 0.002, 0.03, -0.01, -0.85)
ptr, expect = sr.ptr, sr.expect


def projected(dtype, n, seed, tr=TR, outliers=0.2, threshold=2.0, cal=KITTI):
    """n records: exact projections of 3-d points before and after the motion tr, rounded to float; a share `outliers`
    of them (exactly round(outliers * n)) has one to four current coordinates displaced by 10 .. 30 x threshold.
    -> (p_match[n], displaced mask)"""
    rng = np.random.default_rng(seed)
    f, cu, cv, base = cal["f"], cal["cu"], cal["cv"], cal["base"]
    R, t = rot(*tr[:3]), np.array(tr[3:])
    out = np.zeros(n, dtype)
    bad = np.zeros(n, bool)
    bad[rng.permutation(n)[:int(round(outliers * n))]] = True
    k = 0
    while k < n:
        Z = rng.uniform(4, 60); P = np.array([rng.uniform(-1, 1) * Z * 0.9, rng.uniform(-0.3, 0.25) * Z, Z])
        Q = R @ P + t
        if Q[2] < 2:
            continue
        vals = np.array([f * P[0] / P[2] + cu, f * P[1] / P[2] + cv, f * (P[0] - base) / P[2] + cu, f * P[1] / P[2] + cv,
                         f * Q[0] / Q[2] + cu, f * Q[1] / Q[2] + cv, f * (Q[0] - base) / Q[2] + cu, f * Q[1] / Q[2] + cv])
        if bad[k]:
            which = rng.permutation(4)[:rng.integers(1, 5)]
            vals[4 + which] += rng.uniform(10, 30, len(which)) * threshold * rng.choice([-1.0, 1.0], len(which))
        r = out[k]
        r["u1p"], r["v1p"], r["u2p"], r["v2p"], r["u1c"], r["v1c"], r["u2c"], r["v2c"] = vals.astype(np.float32)
        r["i1p"] = r["i2p"] = r["i1c"] = r["i2c"] = k
        k += 1
    return out, bad


# ------------------------------------------------------------------------------------------------------------ CPU
def test_symbols_declared_exported_mirrored_and_argument_errors(pkg):
    """Every new symbol is declared, exported and mirrored; n_sets = 0 and lists without records are VH_OK without a
    device; null and negative arguments are VH_ERR_INVALID_ARG."""
    header = open(os.path.join(ROOT, "include", "viso_hip.h")).read()
    lib = pkg._lib()
    for name in SYMBOLS:
        assert name + "(" in header and hasattr(C.CDLL(pkg.LIB_PATH), name) and name in pkg.ABI_SYMBOLS, name
    assert callable(pkg.motion_inliers) and "motionInliers" in vars(pkg.Matcher) and "getInlierMatches" in vars(pkg.Matcher)
    for meth in ("motionInliers", "getInlierMatches", "getInlierFlags", "getInlierMatchesAll", "inliersDevice"):
        assert meth in vars(pkg.StreamGroup) and hasattr(pkg.SequenceGroup, meth), meth
    e = pkg.EgoParams.default(**KITTI)
    pm = np.zeros(4, pkg.P_MATCH_DTYPE)
    off = np.array([0, 4], np.int32)
    tr = np.zeros((1, 6)); ok = np.ones(1, np.int32); fl = np.zeros(4, np.uint8); cnt = np.full(1, 7, np.int32)
    call = lambda *a: lib.vh_motion_inliers(*a, None, None)  # noqa: E731
    assert call(C.byref(e), 0, 0, None, None, None, None, None, None) == pkg.VH_OK
    empty = np.array([3, 3, 3], np.int32); cnt2 = np.full(2, 7, np.int32)
    assert call(C.byref(e), 0, 2, None, ptr(empty), ptr(np.zeros((2, 6))), ptr(np.ones(2, np.int32)), None, ptr(cnt2)) == pkg.VH_OK
    assert cnt2.tolist() == [0, 0]
    inv = pkg.VH_ERR_INVALID_ARG
    assert call(None, 0, 1, ptr(pm), ptr(off), ptr(tr), ptr(ok), ptr(fl), ptr(cnt)) == inv
    assert call(C.byref(e), 0, -1, ptr(pm), ptr(off), ptr(tr), ptr(ok), ptr(fl), ptr(cnt)) == inv
    assert call(C.byref(e), 0, 1, None, ptr(off), ptr(tr), ptr(ok), ptr(fl), ptr(cnt)) == inv
    assert call(C.byref(e), 0, 1, ptr(pm), None, ptr(tr), ptr(ok), ptr(fl), ptr(cnt)) == inv
    assert call(C.byref(e), 0, 1, ptr(pm), ptr(off), None, ptr(ok), ptr(fl), ptr(cnt)) == inv
    assert call(C.byref(e), 0, 1, ptr(pm), ptr(off), ptr(tr), None, ptr(fl), ptr(cnt)) == inv
    assert call(C.byref(e), 0, 1, ptr(pm), ptr(off), ptr(tr), ptr(ok), None, ptr(cnt)) == inv
    assert call(C.byref(e), 0, 1, ptr(pm), ptr(off), ptr(tr), ptr(ok), ptr(fl), None) == inv
    assert call(C.byref(e), 0, 1, ptr(pm), ptr(np.array([4, 0], np.int32)), ptr(tr), ptr(ok), ptr(fl), ptr(cnt)) == inv
    assert call(C.byref(e), 0, 1, ptr(pm), ptr(np.array([-1, 3], np.int32)), ptr(tr), ptr(ok), ptr(fl), ptr(cnt)) == inv
    n = C.c_int32(0)
    assert lib.vh_group_motion_inliers(None, C.byref(e), ptr(tr), ptr(ok), ptr(cnt)) == inv
    assert lib.vh_match_inliers(None, C.byref(e), ptr(tr), 1, C.byref(n)) == inv
    assert lib.vh_group_get_inlier_flags(None, 0, ptr(fl), 4, C.byref(n)) == inv
    assert lib.vh_group_get_inlier_matches(None, 0, ptr(pm), None, 4, C.byref(n)) == inv
    assert lib.vh_group_get_inlier_matches_all(None, ptr(pm), None, 4, ptr(cnt)) == inv
    assert lib.vh_get_inlier_matches(None, ptr(pm), None, 4, C.byref(n)) == inv
    assert lib.vh_group_inliers_device(None, None, None, None, None) == inv


ESTIMATOR_CASES = [(40, 1, 0.10), (117, 2, 0.30), (300, 3, 0.20), (64, 4, 0.25)]


@pytest.mark.parametrize("n,seed,outliers", ESTIMATOR_CASES)
def test_restatement_gives_the_estimators_inlier_set(n, seed, outliers, ob, oracle):
    """On exact projections with 10-30 % gross outliers the pinned restatement of estimateMotion (and the reference's own
    code where oracle/_ref is built) returns ok, tr and the inlier set; getInlier restated under that tr gives exactly
    that set, with reweighting 0 and 1 (getInlier compares unweighted values), and no sum lies within 1e-6 relative of
    the threshold^2."""
    pm, bad = projected(ob.P_MATCH_DTYPE, n, seed, outliers=outliers)
    assert 0.1 * n - 1 <= bad.sum() <= 0.3 * n + 1
    for rw in (0, 1):
        e = ob.EgoParams.default(reweighting=rw, **KITTI)
        ok, tr, inl = oracle.estimate_motion_stereo(e, pm, oracle.draw_samples(n, e.ransac_iters))
        assert ok
        flags, sums = io.inliers(pm, tr, e)
        assert not io.near_threshold(sums, e, 1e-6).any()
        assert np.array_equal(np.flatnonzero(flags), inl)
        assert np.array_equal(flags.astype(bool), ~bad)       # ... and it is the set the scene was built with
        if ob.Reference.available():
            ok_r, tr_r, inl_r = ob.Reference().estimate_motion_stereo(e, pm)
            assert ok_r and np.array_equal(inl_r, inl)
            assert np.array_equal(np.flatnonzero(io.inliers(pm, tr_r, e)[0]), inl_r)


def test_restatement_edges():
    """ok = 0: no inliers.  NaN, infinity and Z1c = 0 are outliers, never errors; the 0.0001f clamp and the strict compare."""
    dt = _parity_dtype()
    e = _Cal(inlier_threshold=2.0, **KITTI)
    pm, _ = projected(dt, 50, 9)
    assert io.inliers(pm, TR, e, ok=False)[0].sum() == 0 and io.inliers(pm, TR, e)[0].sum() == 40
    q = pm.copy()
    q["u1c"][0] = np.nan; q["u2p"][1] = np.nan; q["v1p"][2] = np.inf; q["u1p"][3] = -np.inf
    f, s = io.inliers(q, TR, e)
    assert f[:4].sum() == 0 and not np.isfinite(s[:4]).any()
    z = pm[:1].copy(); z["u1p"] = 700; z["u2p"] = 690
    Z = KITTI["f"] * KITTI["base"] / float(np.float32(10))
    f, s = io.inliers(z, (0, 0, 0, 0, 0, -Z), e)
    assert f[0] == 0 and not np.isfinite(s[0])


class _Cal:
    def __init__(self, **kw):
        self.__dict__.update(kw)


def _parity_dtype():
    return np.dtype([(n, "<f4" if n[0] in "uv" else "<i4") for n in
                     ("u1p", "v1p", "i1p", "u2p", "v2p", "i2p", "u1c", "v1c", "i1c", "u2c", "v2c", "i2c")])


LENGTHS = (0, 1, 5, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 3 * TILE + 1)
_PARITY = {}


def parity_lists():
    """The 17 lists of the stateless parity test, built once: one per length of LENGTHS (several of them the edge lists:
    all inliers, no inlier, clamped disparities, NaN / infinity, Z1c = 0 and < 0) and four more of odd lengths.
    -> (lists, tr [17, 6], ok [17])"""
    if not _PARITY:
        dt = _parity_dtype()
        lists, trs, oks = [], [], []
        for k, n in enumerate(LENGTHS):
            pm, _ = projected(dt, n, 100 + k, outliers=0.0 if n == 63 else 0.25)
            tr, ok = TR, 1
            if n == 64:        # no inlier: every current position far away
                pm["v1c"] += 50
            if n == 255:       # u1p <= u2p on every second record: zero and negative disparity, clamped to 0.0001f
                pm["u2p"][::2] = pm["u1p"][::2] + np.arange(len(pm[::2]), dtype=np.float32) % 3
            if n == 256:       # NaN and infinities in every field that is read, one record each
                for j, name in enumerate(("u1p", "v1p", "u2p", "u1c", "v1c", "u2c", "v2c")):
                    pm[name][3 * j] = np.nan; pm[name][3 * j + 1] = np.inf; pm[name][3 * j + 2] = -np.inf
            if n == 257:       # zero rotation and tz = -Z of the first records (d = 8: Z exact): Z1c = 0 there, < 0 for the farther ones
                pm["u2p"][:9] = pm["u1p"][:9] - 8
                tr = (0, 0, 0, 0.1, 0, -(KITTI["f"] * KITTI["base"] / 8.0))
            if n == 65:
                ok = 0
            lists.append(pm); trs.append(tr); oks.append(ok)
        for k, n in enumerate((777, 2049, 11, 130)):
            lists.append(projected(dt, n, 200 + k, tr=(0.01 * k, -0.02, 0.003, 0.1 * k, 0, -1.2), outliers=0.3)[0])
            trs.append((0.01 * k, -0.02, 0.003, 0.1 * k, 0, -1.2)); oks.append(0 if k == 2 else 1)
        _PARITY["v"] = (lists, np.array(trs, np.float64), np.array(oks, np.int32))
    return _PARITY["v"]


def parity_expectation():
    """flags, sums and the near-threshold mask (relative 1e-9) of every parity list, once."""
    if "want" not in _PARITY:
        lists, trs, oks = parity_lists()
        e = _Cal(inlier_threshold=2.0, **KITTI)
        want = []
        for pm, tr, ok in zip(lists, trs, oks):
            f, s = io.inliers(pm, tr, e, ok=bool(ok))
            want.append((f, s, io.near_threshold(s, e, 1e-9)))
        _PARITY["want"] = want
    return _PARITY["want"]


def test_parity_inputs_hold_their_premises():
    """The premises of the GPU parity test, checked on the restatement alone: at most 0.1 % of any list within 1e-9
    relative of the threshold^2, and every edge the test names is in the lists."""
    lists, trs, oks = parity_lists()
    want = parity_expectation()
    assert tuple(len(pm) for pm in lists[:len(LENGTHS)]) == LENGTHS and len(lists) == 17 and 0 < oks.sum() < 17
    for pm, (f, s, near) in zip(lists, want):
        assert near.sum() <= 0.001 * len(pm)
    by_len = {len(pm): (pm, w) for pm, w in zip(lists, want)}
    assert by_len[63][1][0].all() and not by_len[64][1][0].any() and not by_len[65][1][0].any()
    pm, (f, s, _) = by_len[255]
    assert (pm["u1p"] <= pm["u2p"]).sum() >= 100 and np.isfinite(s).all() and f[1::2].sum() > 50
    pm, (f, s, _) = by_len[256]
    inf_u2p = [7, 8]   # u2p = +inf: the difference is -inf, clamped; u2p = -inf: d = inf, the point (0, 0, 0) -- both finite sums
    assert not f[:21].any() and np.isfinite(s[inf_u2p]).all() and not np.isfinite(np.delete(s[:21], inf_u2p)).any() and f[21:].sum() > 100
    pm, (f, s, _) = by_len[257]
    assert not np.isfinite(s[:9]).any() and not f[:9].any()           # Z1c = 0
    Z = KITTI["f"] * KITTI["base"] / (pm["u1p"] - pm["u2p"]).astype(np.float64)
    assert (Z[9:] < KITTI["f"] * KITTI["base"] / 8.0).sum() > 50      # Z1c < 0: finite sums
    assert np.isfinite(s[9:]).all()


def test_device_functions_on_the_host_equal_the_restatement(tmp_path):
    """csrc/vh_ego.h (ego_observe, ego_rot, ego_is_inlier: what inlier_flag_kernel runs per record) compiled for the host
    with -ffp-contract=off: the flags of every parity list and of the floats around the threshold are the restatement's,
    byte for byte (libm on both sides, so nothing is excluded)."""
    import subprocess
    exe = str(tmp_path / "inlier_check")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", os.path.join(ROOT, "tests", "cpp", "inlier_check.cpp"), "-lm", "-o", exe])
    lists, trs, oks = parity_lists()
    want = parity_expectation()
    cal = _Cal(inlier_threshold=2.0, **KITTI)
    for k, (pm, tr) in enumerate(zip(lists, trs)):
        fin, fout = str(tmp_path / f"in{k}"), str(tmp_path / f"out{k}")
        with open(fin, "wb") as fh:
            fh.write(np.array([cal.f, cal.cu, cal.cv, cal.base, cal.inlier_threshold, *tr], np.float64).tobytes())
            fh.write(np.int64(len(pm)).tobytes()); fh.write(pm.tobytes())
        subprocess.check_call([exe, fin, fout], timeout=60)
        got = np.fromfile(fout, np.uint8)
        assert got.tobytes() == io.inliers(pm, tr, cal)[0].tobytes(), (k, len(pm))
        if oks[k]:
            assert got.tobytes() == want[k][0].tobytes()


# ------------------------------------------------------------------------------------------------------------ GPU
def check_against(pm, want, flags, count, out, pos, what):
    """Device results of one list against the restatement: everything is exact but for the records within 1e-9 of the
    threshold (`near`), which are left out of flags, positions and records alike."""
    f, _, near = want
    assert len(flags) == len(pm) and flags.dtype == np.uint8 and set(np.unique(flags)) <= {0, 1}, what
    assert np.array_equal(flags[~near], f[~near]), (what, np.flatnonzero(flags != f)[:5])
    assert count == flags.sum() == len(out) == len(pos), what
    assert np.array_equal(pos, np.flatnonzero(flags)), what                    # list order, a function of the flags alone
    assert out.tobytes() == pm[pos].tobytes(), what
    assert np.array_equal(pos[~near[pos]], np.flatnonzero((f == 1) & ~near)), what
    if not near.any():
        assert flags.tobytes() == f.tobytes() and count == f.sum(), what


@pytest.mark.gpu
def test_gpu_stateless_parity(pkg, gpu):
    """vh_motion_inliers: flags, counts, compacted records and positions byte-equal to the restatement on lists of
    0 .. 3 * tile + 1 records, 1, 2 and 17 lists per call with mixed ok, the 0.0001f clamp, NaN and infinite coordinates,
    Z1c = 0 and < 0, a list of inliers only and one without any; twice, byte-equal from run to run."""
    lists, trs, oks = parity_lists()
    want = parity_expectation()
    e = pkg.EgoParams.default(**KITTI)
    for sel in (list(range(17)), [8], [12, 3], list(range(16, -1, -1))):
        args = ([lists[i] for i in sel], trs[sel], oks[sel])
        flags, ninl, outs, poss = pkg.motion_inliers(e, *args)
        again = pkg.motion_inliers(e, *args)
        for k, i in enumerate(sel):
            check_against(lists[i], want[i], flags[k], ninl[k], outs[k], poss[k], (sel, i))
            assert flags[k].tobytes() == again[0][k].tobytes() and outs[k].tobytes() == again[2][k].tobytes()
            assert poss[k].tobytes() == again[3][k].tobytes() and ninl[k] == again[1][k]
    # reweighting and ransac_iters are not read
    e2 = pkg.EgoParams.default(reweighting=0, ransac_iters=1, **KITTI)
    assert pkg.motion_inliers(e2, [lists[12]], trs[[12]], oks[[12]])[0][0].tobytes() == flags[4].tobytes()


@pytest.mark.gpu
@pytest.mark.parametrize("threshold", [2.0, 0.5, 3.0])
def test_gpu_strict_compare_at_the_threshold(threshold, pkg, gpu):
    """Zero rotation (sin and cos exact), non-zero translation: one record's u1c walked float by float (nextafter; the
    sum grows monotonically with it, so the walk is a bisection) to where the restatement's flag flips.  The last inlier,
    the first outlier and their neighbours are classified as the restatement does, nothing excluded; a sum exactly equal
    to the threshold^2 is an outlier."""
    dt = _parity_dtype()
    tr = (0.0, 0.0, 0.0, 0.05, -0.02, -0.9)
    cal = _Cal(inlier_threshold=threshold, **KITTI)
    base_pm, _ = projected(dt, 8, 31, tr=tr, outliers=0.0)
    recs, exact = [], 0
    for r0 in base_pm:
        one = np.array([r0], dt)
        assert io.inliers(one, tr, cal)[0][0] == 1
        lo = int(np.float32(r0["u1c"]).view(np.int32))   # positive floats: their bit patterns order as they do
        hi = int(np.float32(r0["u1c"] + 2 * threshold + 1).view(np.int32))

        def flag_at(bits):
            one["u1c"] = np.int32(bits).view(np.float32)
            return io.inliers(one, tr, cal)
        assert flag_at(hi)[0][0] == 0
        while hi - lo > 1:
            mid = (lo + hi) // 2
            lo, hi = (mid, hi) if flag_at(mid)[0][0] else (lo, mid)
        assert np.nextafter(np.int32(lo).view(np.float32), np.float32(np.inf)).view(np.int32) == hi
        for bits in range(lo - 3, hi + 4):
            f, s = flag_at(bits)
            if s[0] == threshold * threshold:
                exact += 1
                assert f[0] == 0
            recs.append(one.copy())
    pm = np.concatenate(recs)
    f, s = io.inliers(pm, tr, cal)
    assert 0 < f.sum() < len(pm)
    e = pkg.EgoParams.default(inlier_threshold=threshold, **KITTI)
    flags, ninl, outs, poss = pkg.motion_inliers(e, [pm], np.array([tr]), np.ones(1))
    assert flags[0].tobytes() == f.tobytes(), (np.flatnonzero(flags[0] != f), exact)
    assert ninl[0] == f.sum() and np.array_equal(poss[0], np.flatnonzero(f)) and outs[0].tobytes() == pm[f == 1].tobytes()


HCAL = dict(f=300.0, cu=160.0, cv=80.0, base=0.5)
# The synthetic frames pan by (5, 1) pixels per frame at a constant disparity of 6: a plane at Z = f base / 6 = 25 whose flow
# a sideways translation of (-5, -1) Z / f explains.  With a roll of 0.02 rad on top, the residual grows with the distance
# from the principal point: records inside a radius of about threshold / (0.02 sqrt 2) agree, the others do not.
TR2 = (0.0, 0.0, 0.02, -5 * 25 / 300.0, -1 * 25 / 300.0, 0.0)


def hego(pkg, **kw):
    return pkg.EgoParams.default(ransac_iters=50, **HCAL, **kw)


def rand3_of(ob, e, S):
    r = ob.glibc_rand_after_srand0(3 * e.ransac_iters).reshape(e.ransac_iters, 3)
    return np.stack([r] * S)


def hip_read(address, count, dtype):
    """`count` elements at a device address (the runtime the library is linked against)."""
    hip = C.CDLL("libamdhip64.so")
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    out = np.zeros(count, dtype)
    if count:
        assert hip.hipMemcpy(ptr(out), C.c_void_p(address), out.nbytes, 2) == 0
    return out


def check_handle(pkg, g, e, tr, ok, what, min_inliers=0):
    """One classification of the handle's current lists under (tr, ok): the flags are the restatement's on the lists
    getMatchesAll returns; the inlier matches are list[flags] with their positions; the per-stream form, the _all form
    and the device arrays agree.  -> counts"""
    rec, n = g.getMatchesAll()
    counts = g.motionInliers(e, tr, ok)
    cal = _Cal(**{k: getattr(e, k) for k in ("f", "cu", "cv", "base", "inlier_threshold")})
    cap = max(int(n.max(initial=0)), 1)
    arec, apos, acnt = g.getInlierMatchesAll(cap)
    d_flags, d_pm, d_pos, stride = g.inliersDevice()
    assert np.array_equal(acnt, counts) and stride >= cap
    for s in range(g.S):
        pm = rec[s, :n[s]]
        want = io.inliers(pm, tr[s], cal, ok=bool(ok[s]))
        want = (want[0], want[1], io.near_threshold(want[1], cal, 1e-9))
        assert want[2].sum() <= 0.001 * len(pm), what
        flags = g.getInlierFlags(s)
        out, pos = g.getInlierMatches(s)
        check_against(pm, want, flags, counts[s], out, pos, (what, s))
        assert arec[s, :acnt[s]].tobytes() == out.tobytes() and np.array_equal(apos[s, :acnt[s]], pos), (what, s)
        assert hip_read(d_flags + s * stride, n[s], np.uint8).tobytes() == flags.tobytes(), (what, s)
        assert hip_read(d_pm + s * stride * 48, counts[s], pkg.P_MATCH_DTYPE).tobytes() == out.tobytes(), (what, s)
        assert np.array_equal(hip_read(d_pos + s * stride * 4, counts[s], np.int32), pos), (what, s)
    assert counts.sum() >= min_inliers, (what, counts)
    return counts


def classify_twice(pkg, ob, g, what, rows=None):
    """tr from the estimator, then another tr with every ok set: the second call replaces the result."""
    e = hego(pkg)
    tr, ok, _ = g.estimateMotion(e, rand3_of(ob, e, g.S))
    c1 = check_handle(pkg, g, e, tr, ok.astype(np.int32), what + " estimated")
    tr2 = np.tile(np.array(TR2), (g.S, 1)); tr2[:, 2] += 0.002 * np.arange(g.S)
    e2 = hego(pkg, inlier_threshold=2.5)
    c2 = check_handle(pkg, g, e2, tr2, np.ones(g.S, np.int32), what + " given")
    _, n = g.getMatchesAll()
    if rows is not None:   # a sequence handle: rows without a pair hold nothing
        assert all(n[r] == 0 and c1[r] == 0 and c2[r] == 0 for r in range(g.S) if r not in rows), (what, n, rows)
        assert all(n[r] > 100 for r in rows), (what, n)
    assert 0 < c2.sum() < n.sum(), (what, c2, n)   # the roll of TR2: the records near the principal point agree, the others do not
    return c1, c2


@pytest.mark.gpu
@pytest.mark.parametrize("refinement,multi", [(0, False), (2, False), (0, True)])
def test_gpu_group_of_three(refinement, multi, pkg, ob, gpu):
    """A group of S = 3 (one stream of constant images: empty lists), refinement 0 and 2, multi-stage matching on; at the
    end the lists are replaced by vh_group_remove_outliers and classified once more."""
    dims = sr.dims_of(pkg)
    frames = [sr.frames_of(pkg, 3, seed) for seed in (71, 72, 73)]
    frames[1] = [(np.full_like(a, 90), np.full_like(b, 90)) for a, b in frames[1]]
    g = pkg.StreamGroup(3, pkg.Params.default(refinement=refinement, multi_stage=1 if multi else 0))
    if multi:
        g.setMultiStageMatching(True)
    for t in range(3):
        g.pushBack(np.stack([f[t][0] for f in frames]), np.stack([f[t][1] for f in frames]), dims)
        if t == 0:
            continue
        g.matchFeatures(QUAD)
        c1, c2 = classify_twice(pkg, ob, g, f"group r{refinement} m{multi} t{t}")
        assert c1[1] == 0 and c2[1] == 0
    # lists replaced on the host: the lists the getters return now are the ones classified
    before = g.getMatchesAll()[1]
    g.removeOutliers(2)
    assert (g.getMatchesAll()[1] <= before).all()
    e2 = hego(pkg, inlier_threshold=2.5)
    c3 = check_handle(pkg, g, e2, np.tile(np.array(TR2), (3, 1)), np.ones(3, np.int32), "group, voted lists")
    assert 0 < c3.sum() < g.getMatchesAll()[1].sum()
    g.close()


@pytest.mark.gpu
def test_gpu_sequence_handle_and_lone_matcher(pkg, ob, gpu):
    """A sequence handle with chunks of 4 and 2 frames (row 0 of the first chunk and rows 2, 3 of the second hold no pair;
    row 0 of the second chunk crosses the chunk boundary), and a lone matcher with and without removeOutliers."""
    dims = sr.dims_of(pkg)
    frames = sr.frames_of(pkg, 6, 74)
    g = pkg.SequenceGroup(4, pkg.Params.default())
    sr.push(g, frames, 0, 4, dims)
    g.matchFeatures(QUAD)
    classify_twice(pkg, ob, g, "sequence chunk 0", rows=(1, 2, 3))
    sr.push(g, frames, 4, 2, dims)
    g.matchFeatures(QUAD)
    classify_twice(pkg, ob, g, "sequence chunk 1", rows=(0, 1))
    g.close()
    for removal in (True, False):   # matchFeatures ends with removeOutliers on the host, or leaves the device list as it is
        m = pkg.Matcher(pkg.Params.default(), outlier_removal=removal)
        for left, right in frames[:2]:
            m.pushBack(left, right, dims)
        m.matchFeatures(QUAD)
        pm = m.getMatches()
        e = hego(pkg, inlier_threshold=2.5)
        cal = _Cal(inlier_threshold=2.5, **HCAL)
        f, s = io.inliers(pm, TR2, cal)
        assert not io.near_threshold(s, cal, 1e-9).any() and 0 < f.sum() < len(pm)
        assert m.motionInliers(e, TR2) == f.sum()
        out, pos = m.getInlierMatches()
        assert np.array_equal(pos, np.flatnonzero(f)) and out.tobytes() == pm[f == 1].tobytes()
        assert m.motionInliers(e, TR2, ok=False) == 0 and len(m.getInlierMatches()[0]) == 0
        m.close()


@pytest.mark.gpu
def test_gpu_state_rules_capacity_and_failed_allocation(pkg, ob, gpu):
    """VH_ERR_STATE before any push, before any match, after a flow match, from the getters before a classification and
    after the next match call; the getters' capacity rule; a refused first allocation is VH_ERR_HIP and the repeated call
    gives what an undisturbed one gives."""
    lib = pkg._lib()
    dims = sr.dims_of(pkg)
    frames = sr.frames_of(pkg, 3, 75)
    e = hego(pkg, inlier_threshold=2.5)
    tr = np.array([TR2]); ok = np.ones(1, np.int32)
    g = pkg.StreamGroup(1, pkg.Params.default())
    getters = (lambda: g.getInlierFlags(0), lambda: g.getInlierMatches(0), lambda: g.getInlierMatchesAll(8), g.inliersDevice)
    state = pkg.VH_ERR_STATE
    expect(pkg, state, lambda: g.motionInliers(e, tr, ok))            # nothing pushed
    g.pushBack(frames[0][0][None], frames[0][1][None], dims)
    expect(pkg, state, lambda: g.motionInliers(e, tr, ok))            # nothing matched
    g.pushBack(frames[1][0][None], frames[1][1][None], dims)
    g.matchFeatures(FLOW)
    expect(pkg, state, lambda: g.motionInliers(e, tr, ok))            # flow lists carry no disparity
    g.matchFeatures(QUAD)
    for call in getters:
        expect(pkg, state, call)                                      # not classified yet
    bytes0 = g.deviceBytes()
    g.debugFailNextAlloc()
    expect(pkg, pkg.VH_ERR_HIP, lambda: g.motionInliers(e, tr, ok))
    assert g.deviceBytes() == bytes0
    for call in getters:
        expect(pkg, state, call)
    pm = g.getMatches(0)
    f, s = io.inliers(pm, TR2, _Cal(inlier_threshold=2.5, **HCAL))
    assert not io.near_threshold(s, _Cal(inlier_threshold=2.5, **HCAL), 1e-9).any() and 1 < f.sum() < len(pm)
    assert g.motionInliers(e, tr, ok)[0] == f.sum()                   # the repeated call
    assert g.getInlierFlags(0).tobytes() == f.tobytes()
    out, pos = g.getInlierMatches(0)
    assert out.tobytes() == pm[f == 1].tobytes() and np.array_equal(pos, np.flatnonzero(f))
    # capacity rule: the full number, the first cap elements, VH_ERR_CAPACITY
    n = C.c_int32(0)
    k = int(f.sum())
    buf = np.zeros(k, pkg.P_MATCH_DTYPE); bpos = np.full(k, -7, np.int32); bfl = np.full(len(pm), 9, np.uint8)
    assert lib.vh_group_get_inlier_matches(g._h, 0, ptr(buf), ptr(bpos), k - 1, C.byref(n)) == pkg.VH_ERR_CAPACITY
    assert n.value == k and buf[:k - 1].tobytes() == out[:k - 1].tobytes() and bpos[k - 1] == -7 and np.array_equal(bpos[:k - 1], pos[:k - 1])
    assert lib.vh_group_get_inlier_matches(g._h, 0, ptr(buf), None, k, C.byref(n)) == pkg.VH_OK and buf.tobytes() == out.tobytes()
    assert lib.vh_group_get_inlier_flags(g._h, 0, ptr(bfl), len(pm) - 1, C.byref(n)) == pkg.VH_ERR_CAPACITY
    assert n.value == len(pm) and bfl[:-1].tobytes() == f[:-1].tobytes() and bfl[-1] == 9
    cnt = np.zeros(1, np.int32)
    assert lib.vh_group_get_inlier_matches_all(g._h, ptr(buf), None, k - 1, ptr(cnt)) == pkg.VH_ERR_CAPACITY and cnt[0] == k
    assert lib.vh_group_get_inlier_flags(g._h, 1, ptr(bfl), len(pm), C.byref(n)) == pkg.VH_ERR_INVALID_ARG
    # the next match call ends the classification
    g.matchFeatures(QUAD)
    for call in getters:
        expect(pkg, state, call)
    assert g.motionInliers(e, tr, ok)[0] == f.sum()
    g.pushBack(frames[2][0][None], frames[2][1][None], dims)
    expect(pkg, state, lambda: g.motionInliers(e, tr, ok))            # pushed, not matched
    g.close()


@pytest.mark.gpu
def test_gpu_unused_means_untouched(pkg, ob, gpu):
    """A group that never calls the feature holds the bytes it held without it and has no inlier_* scope; its lists equal
    those of a group that does call it, whose device bytes grow by 1 + 48 + 4 per record slot, the tile counts and 56
    bytes per stream (each array rounded up to 256 bytes)."""
    dims = sr.dims_of(pkg)
    frames = [sr.frames_of(pkg, 3, seed) for seed in (76, 77)]
    e = hego(pkg, inlier_threshold=2.5)
    seen = {}
    for name in ("off", "on"):
        g = pkg.StreamGroup(2, pkg.Params.default())
        g.profileEnable(True)
        lists, sizes = [], []
        for t in range(3):
            g.pushBack(np.stack([f[t][0] for f in frames]), np.stack([f[t][1] for f in frames]), dims)
            if t == 0:
                continue
            g.matchFeatures(QUAD)
            sizes.append(g.deviceBytes())
            if name == "on":
                g.motionInliers(e, np.tile(np.array(TR2), (2, 1)), np.ones(2, np.int32))
                stride = g.inliersDevice()[3]
            lists.append([g.getMatches(s).tobytes() for s in range(2)])
        g.synchronize()
        seen[name] = (lists, sizes, g.deviceBytes(), [g.profileRead(k)[1] for k in SCOPES])
        g.close()
    assert seen["off"][0] == seen["on"][0]
    assert seen["off"][3] == [0, 0] and seen["on"][3] == [2, 2]
    assert seen["off"][1][0] == seen["on"][1][0] and seen["off"][1][1] == seen["off"][2]   # (on: taken before its first call)
    slots = 2 * stride
    tiles = 2 * ((stride + TILE - 1) // TILE)
    grown = seen["on"][2] - seen["off"][2]
    assert 53 * slots + 4 * tiles + 56 * 2 <= grown <= 53 * slots + 4 * tiles + 56 * 2 + 7 * 255, (grown, slots, tiles)
