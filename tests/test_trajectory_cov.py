"""The pose covariance: vh_trajectory_cov on caller-owned chains of rows, and the covariance that
vh_group_trajectory propagates beside the pose on plain groups, lone matchers and sequence handles.

The bounds.  Where every rotation is zero, sin and cos are exact and nothing of any math library enters: the device must
give the float64 restatement (tests/trajectory_cov_oracle.py) byte for byte.  For general motions the device's sin / cos may
differ from the host's in the last place, so every covariance is held to 16 x d_ref of the longdouble restatement, d_ref
being the float64 restatement's own largest distance from the longdouble one over these very chains, in
max_mn |dSigma_mn| / sqrt(Sigma_mm Sigma_nn) -- the margin sections 4.15 and 4.23 give the device.  Handles are held to the
stateless form byte for byte: same kernel, same inputs.  d_ref = 6.3e-15; on an MI355X the device used 6.2 % of the bound."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import test_motion_inliers as mi
import test_post_dense as pd
import test_sequence_landmarks as sl
import test_sequence_recon as sr
import trajectory_cov_oracle as tc
import trajectory_oracle as to
from conftest import ROOT

SYMBOLS = ("vh_default_traj_cov_params", "vh_trajectory_cov", "vh_group_set_trajectory_covariance", "vh_sequence_set_trajectory_covariance",
           "vh_set_trajectory_covariance", "vh_group_get_pose_covariances", "vh_get_pose_covariance", "vh_group_pose_covariances_device",
           "vh_group_set_pose_covariance")
R = 128                                     # VH_TRAJ_COV_ROUND: asserted against the header and the package below
LENGTHS = (1, 0, 2, R - 1, R, R + 1, 255, 256, 257, 513)   # the issue's lengths, and those around the kernel's own round
QUAD = 2
S0 = np.diag([1e-6, 2e-6, 3e-6, 1e-4, 2e-4, 3e-4]) + 1e-7
_CACHE = {}


def ptr(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def expect(pkg, code, fn):
    with pytest.raises(pkg.VisoHipError) as ei:
        fn()
    assert ei.value.code == code, (ei.value.code, code)


def random_covs(rng, n):
    """correlated 6x6: A A^T with rotations near 1e-3 rad and translations near 1e-2 m"""
    A = rng.normal(size=(n, 6, 6)) * np.array([1e-3, 1e-3, 1e-3, 1e-2, 1e-2, 1e-2])[None, :, None]
    return A @ A.transpose(0, 2, 1)


def edge_rows(n, seed, tr, cov):
    """-> (ok, ok_cov); tr and cov get their non-finite entries in place.  Mostly accepted rows with covariances; the five
    kinds of row that are not -- ok == 0, a non-finite tr, ok < 0, ok_cov == 0, a NaN in C -- on the five rows in front
    of and the five behind every multiple of R, their order turning from boundary to boundary so that each kind comes to
    lie right at one"""
    rng = np.random.default_rng(seed)
    ok = (rng.random(n) < 0.85).astype(np.int32)
    okc = (rng.random(n) < 0.9).astype(np.int32)
    ok[rng.random(n) < 0.03] = -1
    kinds = []
    for q, b in enumerate(range(R, n + 5, R)):
        for side, rows in ((0, range(b - 5, b)), (1, range(b, b + 5))):
            for m, r in enumerate(rows):
                if 0 <= r < n:
                    kinds.append((r, (m + q + 2 * side) % 5))
    for r, kind in kinds:
        ok[r], okc[r] = 1, 1
        if kind == 0:
            ok[r] = 0
        elif kind == 1:
            tr[r, 1 + r % 5] = np.nan if r % 2 else np.inf
        elif kind == 2:
            ok[r] = -1
        elif kind == 3:
            okc[r] = 0
        else:
            cov[r, r % 6, (r // 6) % 6] = np.nan
    return ok, okc


def make_chains(seed, translations):
    """translations: rx = ry = rz = 0 and translations on a grid of 1 / 128 m below 1 m (test_trajectory's: the status
    then is exact too); else |r| <= 0.05 rad, |t| <= 2 m"""
    rng = np.random.default_rng(seed)
    out = []
    for c, n in enumerate(LENGTHS):
        if translations:
            tr = np.zeros((n, 6)); tr[:, 3:] = rng.integers(-127, 128, (n, 3)) / 128.0
        else:
            tr = np.concatenate([rng.uniform(-0.05, 0.05, (n, 3)), rng.uniform(-2, 2, (n, 3))], 1)
        cov = random_covs(rng, n)
        ok, okc = edge_rows(n, seed + 10 + c, tr, cov)
        out.append((tr, ok, cov, okc))
    if len(out[0][1]):
        out[0][1][0] = 0                                   # REPEAT before any accepted row: holds
    return out


def chains_of(kind):
    """the chains and their statuses, made once: (chains, statuses)"""
    if kind not in _CACHE:
        ch = make_chains(5 if kind == "translations" else 11, kind == "translations")
        _CACHE[kind] = (ch, [tc.statuses(t, o) for t, o, _, _ in ch])
    return _CACHE[kind]


def oracle(kind, on_fail, ft=np.float64, S0s=None, fill_scale=1.0):
    key = (kind, on_fail, ft, S0s is not None, fill_scale)
    if key not in _CACHE:
        ch, st = chains_of(kind)
        _CACHE[key] = [tc.chain(t, o, cv, oc, None if S0s is None else S0s[c], None, on_fail, fill_scale, ft, st[c])
                       for c, (t, o, cv, oc) in enumerate(ch)]
    return _CACHE[key]


def general_reference():
    """-> (float64 results, longdouble results, d_ref) over the general chains, HOLD"""
    w64, wld = oracle("general", to.HOLD), oracle("general", to.HOLD, np.longdouble)
    if "d_ref" not in _CACHE:
        _CACHE["d_ref"] = max(float(tc.corr_diff(a[0]["cov"], b[0]["cov"])) for a, b in zip(w64, wld))
    return w64, wld, _CACHE["d_ref"]


def same_records(got, want, what):
    assert got.dtype == want.dtype and len(got) == len(want), (what, len(got), len(want))
    if got.tobytes() != want.tobytes():
        for f in ("status", "step", "n_filled", "cov"):
            bad = [r for r in range(len(got)) if got[f][r].tobytes() != want[f][r].tobytes()]
            assert not bad, (what, f, bad[:5], got[f][bad[0]], want[f][bad[0]])
        raise AssertionError(what)


def run_stateless(pkg, chains, S0s=None, carry=None, on_fail=0, fill_scale=1.0):
    return pkg.trajectory_cov([c[0] for c in chains], [c[1] for c in chains], [c[2] for c in chains], [c[3] for c in chains], S0s, carry,
                              pkg.TrajParams.default(on_fail=on_fail), pkg.TrajCovParams.default(fill_scale=fill_scale))


# ------------------------------------------------------------------------------------------------------------ CPU
def test_symbols_layout_and_host_refusals(pkg):
    """Every symbol is declared, exported and in ABI_SYMBOLS, vh_abi_version stays 1; the records are 304 and 880 bytes;
    the round is the header's; both units are in the Makefile's SRCS; the Python layer has its entries; chains without
    rows are VH_OK without a device; the refusals of the stateless entry and of null handles."""
    header = open(os.path.join(ROOT, "include", "viso_hip.h")).read()
    lib = pkg._lib()
    for name in SYMBOLS:
        assert name + "(" in header and hasattr(C.CDLL(pkg.LIB_PATH), name) and name in pkg.ABI_SYMBOLS, name
    assert pkg.abi_version() == 1
    assert pkg.TRAJ_COV_DTYPE.itemsize == 304 and pkg.TRAJ_COV_CARRY_DTYPE.itemsize == 880
    assert pkg.TRAJ_COV_DTYPE == tc.COV and pkg.TRAJ_COV_CARRY_DTYPE == tc.CARRY and C.sizeof(pkg.TrajCovParams) == 16
    assert f"#define VH_TRAJ_COV_ROUND {R}\n" in open(os.path.join(pkg.CSRC, "vh_trajectory_cov.h")).read() and pkg.TRAJ_COV_ROUND == R
    srcs = open(os.path.join(pkg.CSRC, "Makefile")).read().split("SRCS", 1)[1].split("ONLY", 1)[0]
    assert "kernels_trajectory_cov.hip" in srcs and "engine_trajectory_cov.hip" in srcs
    for cls in (pkg.Matcher, pkg.StreamGroup, pkg.SequenceGroup):
        assert all(hasattr(cls, n) for n in ("setTrajectoryCovariance", "getPoseCovariances", "setPoseCovariance")), cls
    tp, tcp = pkg.TrajParams.default(), pkg.TrajCovParams.default()
    assert tcp.fill_scale == 1.0
    a = (C.byref(tp), C.byref(tcp), 0)
    assert lib.vh_trajectory_cov(*a, 0, None, None, None, None, None, None, None, None, None) == pkg.VH_OK
    off = np.zeros(3, np.int32); cout = np.zeros(2, tc.CARRY)
    s0 = np.stack([S0, np.zeros((6, 6))]).reshape(2, 36).copy()
    assert lib.vh_trajectory_cov(*a, 2, ptr(off), None, None, None, None, ptr(s0), None, None, ptr(cout)) == pkg.VH_OK
    assert np.array_equal(cout["cov"][0], S0) and not cout["cov"][1].any() and not cout["has_ad"].any() and not cout["n_filled"].any()
    inv = pkg.VH_ERR_INVALID_ARG
    off = np.array([0, 1], np.int32); tr = np.zeros((1, 6)); ok = np.ones(1, np.int32); cv = np.zeros((1, 36)); out = np.zeros(1, tc.COV)
    good = [1, ptr(off), ptr(tr), ptr(ok), ptr(cv), ptr(ok), None, None, ptr(out), None]
    for bad in (-1.0, np.nan, np.inf):
        assert lib.vh_trajectory_cov(C.byref(tp), C.byref(pkg.TrajCovParams.default(fill_scale=bad)), 0, *good) == inv, bad
    assert lib.vh_trajectory_cov(None, C.byref(tcp), 0, *good) == inv and lib.vh_trajectory_cov(C.byref(tp), None, 0, *good) == inv
    assert lib.vh_trajectory_cov(C.byref(pkg.TrajParams.default(on_fail=2)), C.byref(tcp), 0, *good) == inv
    for k in (1, 2, 3, 4, 5, 8):                                                  # a null pointer where rows need one
        args = list(good); args[k] = None
        assert lib.vh_trajectory_cov(*a, *args) == inv, k
    assert lib.vh_trajectory_cov(*a, -1, *good[1:]) == inv
    assert lib.vh_group_set_trajectory_covariance(None, C.byref(tcp), None) == inv and lib.vh_group_get_pose_covariances(None, None) == inv


@pytest.mark.gpu
def test_gpu_handle_refusals_before_any_push(pkg, gpu):
    """The covariance needs the trajectory; fill_scale and Sigma0 are judged; the wrong kind of handle; the mono source;
    switching the trajectory off takes the covariance with it."""
    lib = pkg._lib()
    tcp = pkg.TrajCovParams.default()
    g = pkg.StreamGroup(2, pkg.Params.default())
    expect(pkg, pkg.VH_ERR_STATE, lambda: g.setTrajectoryCovariance())
    g.setTrajectory()
    expect(pkg, pkg.VH_ERR_INVALID_ARG, lambda: g.setTrajectoryCovariance(pkg.TrajCovParams.default(fill_scale=-0.5)))
    bad = np.zeros((2, 6, 6)); bad[1, 2, 3] = np.nan
    expect(pkg, pkg.VH_ERR_INVALID_ARG, lambda: g.setTrajectoryCovariance(None, bad))
    g.setTrajectoryCovariance(None, S0)
    assert lib.vh_sequence_set_trajectory_covariance(g._h, C.byref(tcp), None) == pkg.VH_ERR_UNSUPPORTED
    expect(pkg, pkg.VH_ERR_INVALID_ARG, lambda: g.setPoseCovariance(2, S0))
    expect(pkg, pkg.VH_ERR_INVALID_ARG, lambda: g.setPoseCovariance(0, bad[1]))
    expect(pkg, pkg.VH_ERR_UNSUPPORTED, lambda: g.trajectory(pkg.TRAJ_MONO))      # the mono source has no 6x6 covariance
    expect(pkg, pkg.VH_ERR_STATE, lambda: g.getPoseCovariances())
    g.setTrajectory(on=False)                                                     # takes the covariance with it
    expect(pkg, pkg.VH_ERR_STATE, lambda: g.setPoseCovariance(0, S0))
    g.close()


def run_check(tmp_path, exe, name, chain, on_fail, fill_scale, S0m):
    tr, ok, cov, okc = chain
    fin, fout = str(tmp_path / (name + ".in")), str(tmp_path / (name + ".out"))
    with open(fin, "wb") as fh:
        fh.write(np.array([on_fail, len(tr)], np.int32).tobytes()); fh.write(np.array([fill_scale], np.float64).tobytes())
        fh.write(np.asarray(S0m, np.float64).tobytes())
        fh.write(np.ascontiguousarray(tr, np.float64).tobytes()); fh.write(np.ascontiguousarray(ok, np.int32).tobytes())
        fh.write(np.ascontiguousarray(cov, np.float64).tobytes()); fh.write(np.ascontiguousarray(okc, np.int32).tobytes())
    subprocess.check_call([exe, fin, fout], timeout=60)
    raw = np.fromfile(fout, np.uint8)
    return raw[:304 * len(tr)].view(tc.COV), raw[304 * len(tr):].view(tc.CARRY)


def test_header_on_the_host(tmp_path):
    """csrc/vh_trajectory_cov.h compiled for the host (tests/cpp/trajectory_cov_check.cpp, built as
    test_trajectory.py::test_header_on_the_host builds its program): byte for byte the float64 restatement, records and
    carry, on every chain of the GPU tests -- translations and general motions (both use the C library's sin / cos here),
    both policies."""
    exe = str(tmp_path / "trajectory_cov_check")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", os.path.join(ROOT, "tests", "cpp", "trajectory_cov_check.cpp"), "-lm", "-o", exe])
    for kind in ("translations", "general"):
        chains, _ = chains_of(kind)
        for on_fail in (to.HOLD, to.REPEAT):
            want = oracle(kind, on_fail)
            for c, ch in enumerate(chains):
                got, gc = run_check(tmp_path, exe, f"{kind}{on_fail}_{c}", ch, on_fail, 1.0, np.zeros((6, 6)))
                same_records(got, tc.records(want[c][0]), ("host", kind, on_fail, c))
                assert gc.tobytes() == tc.carry_record(want[c][1]).tobytes(), (kind, on_fail, c)
    ch = chains[-1]
    want = tc.chain(*ch, S0, None, to.REPEAT, 0.25)
    got, gc = run_check(tmp_path, exe, "s0", ch, to.REPEAT, 0.25, S0)
    same_records(got, tc.records(want[0]), "host S0 fill 0.25")
    assert gc.tobytes() == tc.carry_record(want[1]).tobytes()


def test_d_ref_and_the_shape_of_the_records():
    """d_ref -- float64 against longdouble over the GPU tests' general chains -- is computed and printed (DESIGN.md section
    4.24 records it) and is rounding-sized; status, step and n_filled do not depend on the precision; every covariance is
    exactly symmetric; the chains hold every kind of row, and filled steps, on both policies."""
    w64, wld, d_ref = general_reference()
    print(f"d_ref = {d_ref:.3e} over chains of {LENGTHS} rows")
    assert 0 < d_ref < 1e-10
    for (a, _), (b, _) in zip(w64, wld):
        assert all(np.array_equal(a[f], b[f]) for f in ("status", "step", "n_filled"))
        assert np.array_equal(a["cov"], a["cov"].transpose(0, 2, 1))
    rep = oracle("general", to.REPEAT)
    assert rep[-1][0]["n_filled"][-1] > w64[-1][0]["n_filled"][-1] > 0
    assert set(np.concatenate([a["status"] for a, _ in w64]).tolist()) == {0, 1, 2, 4}


def first_order_log(M):
    return np.array([(M[2, 1] - M[1, 2]) / 2, (M[0, 2] - M[2, 0]) / 2, (M[1, 0] - M[0, 1]) / 2, M[0, 3], M[1, 3], M[2, 3]])


def test_meaning_by_monte_carlo():
    """What Sigma means: 20 rows of about 1 m forward with small rotations, random correlated motion covariances, 400
    draws of the motions; xi = the first-order log of inv(P) P_k.  The sample variance of each coordinate of xi over the
    restatement's Sigma must lie inside 1 +- 5 sqrt(2 / 399) (the project's Monte Carlo bound, section 4.15); the largest
    difference of the correlation matrices is printed."""
    rng = np.random.default_rng(2024)
    n, draws = 20, 400
    tr = np.concatenate([rng.uniform(-0.02, 0.02, (n, 3)), rng.normal(0, 0.05, (n, 2)), 1.0 + rng.normal(0, 0.1, (n, 1))], 1)
    cov = random_covs(rng, n)
    res, _ = tc.chain(tr, np.ones(n, np.int32), cov, np.ones(n, np.int32))
    Sigma = res["cov"][-1]
    assert res["n_filled"][-1] == 0 and res["step"][-1] == n

    def pose(trs):
        P = np.eye(4)
        for t in trs:
            P = P @ np.linalg.inv(np.array(to.transform(t), np.float64))
        return P
    Pinv = np.linalg.inv(pose(tr))
    Ls = [np.linalg.cholesky(c) for c in cov]
    xi = np.array([first_order_log(Pinv @ pose(tr + np.stack([L @ rng.normal(size=6) for L in Ls]))) for _ in range(draws)])
    ratio = xi.var(0, ddof=1) / np.diag(Sigma)
    sd = np.sqrt(np.diag(Sigma))
    corr = np.abs(np.corrcoef(xi.T) - Sigma / np.outer(sd, sd)).max()
    print("sample / predicted variance:", " ".join(f"{r:.3f}" for r in ratio), f"; largest correlation difference {corr:.3f}")
    bound = 5 * np.sqrt(2 / (draws - 1))
    assert np.all(np.abs(ratio - 1) <= bound), ratio


# ------------------------------------------------------------------------------------------------------------ GPU, stateless
@pytest.mark.gpu
def test_gpu_pure_translations_byte_equal(pkg, gpu):
    """Chains of 1, 0, 2, R - 1, R, R + 1, 255, 256, 257 and 513 rows in one call, every kind of row around every round
    boundary, both policies, with and without Sigma0: records (n_filled included) and carry byte for byte the float64
    restatement."""
    chains, _ = chains_of("translations")
    S0s = np.stack([S0 if c % 2 else np.zeros((6, 6)) for c in range(len(chains))])
    for on_fail in (to.HOLD, to.REPEAT):
        for s0 in (None, S0s):
            got, carry = run_stateless(pkg, chains, s0, None, on_fail)
            want = oracle("translations", on_fail, np.float64, s0)
            for c in range(len(chains)):
                same_records(got[c], tc.records(want[c][0]), ("translations", on_fail, s0 is not None, c))
                assert carry[c:c + 1].tobytes() == tc.carry_record(want[c][1]).tobytes(), (on_fail, c)
    assert got[-1]["n_filled"][-1] > 0 and (got[-1]["cov"][-1] != 0).all()


@pytest.mark.gpu
def test_gpu_general_motions_within_16_d_ref(pkg, gpu):
    """General motions, both policies: status, step and n_filled equal, cov within 16 x d_ref of the longdouble
    restatement and exactly symmetric; the share of the room used is printed.  The same bytes on a second run, and for a
    chain alone as among the others; fill_scale = 0.25 against the float64 restatement within the same bound."""
    chains, _ = chains_of("general")
    _, wld, d_ref = general_reference()
    got, carry = run_stateless(pkg, chains)
    worst = 0.0
    for c in range(len(chains)):
        assert all(np.array_equal(got[c][f], wld[c][0][f]) for f in ("status", "step", "n_filled")), c
        assert np.array_equal(got[c]["cov"], got[c]["cov"].transpose(0, 2, 1)), c
        worst = max(worst, float(tc.corr_diff(got[c]["cov"], wld[c][0]["cov"])))
    print(f"d_ref = {d_ref:.3e}; the device's largest distance {worst:.3e} = {worst / (16 * d_ref):.1%} of 16 x d_ref")
    assert worst <= 16 * d_ref
    again, carry2 = run_stateless(pkg, chains)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(got, again)) and carry.tobytes() == carry2.tobytes()
    c = len(chains) - 1
    alone, ca = run_stateless(pkg, chains[c:])
    assert alone[0].tobytes() == got[c].tobytes() and ca.tobytes() == carry[c:].tobytes()
    rep, _ = run_stateless(pkg, chains, None, None, to.REPEAT, 0.25)
    want = oracle("general", to.REPEAT, np.longdouble, None, 0.25)
    for c in range(len(chains)):
        assert all(np.array_equal(rep[c][f], want[c][0][f]) for f in ("status", "step", "n_filled")), c
        assert float(tc.corr_diff(rep[c]["cov"], want[c][0]["cov"])) <= 16 * d_ref, c


@pytest.mark.gpu
def test_gpu_two_calls_joined_by_the_carry(pkg, gpu):
    """Two calls, the second starting from the first's carry, equal one call over the concatenation -- split in front of,
    on and behind a round boundary, under REPEAT (Ad_last and Q_last cross the split), from a Sigma0."""
    for kind in ("general", "translations"):
        tr, ok, cov, okc = [x.copy() for x in chains_of(kind)[0][-1]]
        for cut in (1, R - 1, R, R + 1):
            tr[cut - 1] = tr[7]; ok[cut - 1] = 1; okc[cut - 1] = 1; cov[cut - 1] = cov[7]; ok[cut] = 0   # the row behind the split repeats
            whole, cw = run_stateless(pkg, [(tr, ok, cov, okc)], S0, None, to.REPEAT)
            a, ca = run_stateless(pkg, [(tr[:cut], ok[:cut], cov[:cut], okc[:cut])], S0, None, to.REPEAT)
            b, cb = run_stateless(pkg, [(tr[cut:], ok[cut:], cov[cut:], okc[cut:])], None, ca, to.REPEAT)
            assert np.concatenate([a[0], b[0]]).tobytes() == whole[0].tobytes() and cb.tobytes() == cw.tobytes(), (kind, cut)
            assert whole[0]["n_filled"][cut] == whole[0]["n_filled"][cut - 1] + 1     # (it did repeat)


@pytest.mark.gpu
def test_gpu_edges_stateless(pkg, gpu):
    """What a poisoned buffer would show (the child of test_gpu_child_on_poisoned_buffers runs this): empty chains among
    others keep their start; chains of status-4 rows only keep Sigma0 and count nothing; a shorter call behind a longer one
    reads nothing the longer one left."""
    rng = np.random.default_rng(3)
    n = R + 3
    tr = np.zeros((n, 6)); tr[:, 3:] = rng.integers(-127, 128, (n, 3)) / 128.0
    cov = random_covs(rng, n)
    none = (tr, np.full(n, -1, np.int32), cov, np.ones(n, np.int32))
    full = (tr, np.ones(n, np.int32), cov, np.ones(n, np.int32))
    empty = (tr[:0], np.zeros(0, np.int32), cov[:0], np.zeros(0, np.int32))
    got, carry = run_stateless(pkg, [empty, none, empty, full, empty], S0, None, to.REPEAT)
    for c in (0, 2, 4):
        assert len(got[c]) == 0 and carry[c:c + 1].tobytes() == tc.carry_record(dict(cov=S0, Ad=None, Q=None, n_filled=0, step=0)).tobytes()
    assert (got[1]["status"] == 4).all() and not got[1]["step"].any() and not got[1]["n_filled"].any()
    assert all(got[1]["cov"][r].tobytes() == S0.tobytes() for r in range(n)) and carry[1:2].tobytes() == carry[0:1].tobytes()
    want = tc.chain(*full, S0, None, to.REPEAT)
    same_records(got[3], tc.records(want[0]), "full")
    short = tuple(x[:3] for x in full)
    got2, c2 = run_stateless(pkg, [short], S0, None, to.REPEAT)
    same_records(got2[0], tc.records(want[0])[:3], "a shorter call behind a longer one")
    assert c2["step"][0] == 3 and c2["has_q"][0] == 1


# ------------------------------------------------------------------------------------------------------------ GPU, handles
def stateless_step(pkg, tr, ok, cov, okc, carry, tp=None, tcp=None):
    """one row per chain from `carry` -> (records [S], carry)"""
    S = len(tr)
    got, c = pkg.trajectory_cov([np.asarray(tr[s])[None] for s in range(S)], [[int(ok[s])] for s in range(S)],
                                [np.asarray(cov[s])[None] for s in range(S)], [[int(okc[s])] for s in range(S)], None, carry, tp, tcp)
    return np.concatenate(got), c


def start_carry(S, Sg=None):
    c = np.zeros(S, tc.CARRY)
    if Sg is not None:
        c["cov"] = Sg
    return c


@pytest.mark.gpu
def test_gpu_group_of_three(pkg, ob, gpu):
    """A group of 3 streams (one of constant images: never ok; its list is empty) over 3 steps under REPEAT with
    fill_scale 0.5 from a Sigma0 per stream.  trajectory() without a current motion covariance is VH_ERR_STATE and leaves
    poses and carries as they were; behind motionCovariance(e) the covariance records are byte for byte the stateless form
    fed the handle's own tr / ok / cov / ok_cov and the carry of the step before; a call repeated behind
    refitMotion(reclassify=True) + motionCovariance recomputes from the same base; a covariance under a caller's tr does
    not count; setPose / setPoseCovariance re-anchor; both kernels are profiled once per call."""
    fr, dims = pd.frames_of(pkg), pd.dims_of(pkg)
    e = pd.ego_of(pkg)
    S = pd.S
    tp = pkg.TrajParams.default(on_fail=pkg.TRAJ_REPEAT)
    tcp = pkg.TrajCovParams.default(fill_scale=0.5)
    S0s = np.stack([np.zeros((6, 6)), S0, 2 * S0])
    g = pkg.StreamGroup(S, pkg.Params.default())
    g.setTrajectory(tp)
    g.setTrajectoryCovariance(tcp, S0s)
    g.profileEnable(True)
    carry, calls = start_carry(S, S0s), 0
    for t in range(3):
        pd.push(g, fr, t, dims)
        if t == 0:
            expect(pkg, pkg.VH_ERR_STATE, lambda: g.setTrajectoryCovariance(tcp))   # after the first push
            continue
        g.matchFeatures(QUAD)
        tr0, ok0, _ = g.estimateMotion(e, mi.rand3_of(ob, e, S))
        g.motionInliers(e, tr0, ok0.astype(np.int32))
        expect(pkg, pkg.VH_ERR_STATE, lambda: g.trajectory())                       # no motion covariance for this classification
        g.motionCovariance(e, tr0, ok0.astype(np.int32))
        expect(pkg, pkg.VH_ERR_STATE, lambda: g.trajectory())                       # under a caller's tr: not the classification's own
        expect(pkg, pkg.VH_ERR_STATE, lambda: g.getPoseCovariances())
        cov, _, okc, _ = g.motionCovariance(e)
        poses = g.trajectory(); calls += 1
        got = g.getPoseCovariances()
        want, _ = stateless_step(pkg, tr0, ok0, cov, okc, carry, tp, tcp)
        same_records(got, want, f"group t{t}")
        assert np.array_equal(got["status"], poses["status"]) and np.array_equal(got["step"], poses["step"])
        tr, ok, _, _ = g.refitMotion(e, reclassify=True)
        expect(pkg, pkg.VH_ERR_STATE, lambda: g.trajectory())                       # classified again: the covariance is the old lists'
        assert g.getPoses().tobytes() == poses.tobytes() and g.getPoseCovariances().tobytes() == got.tobytes()
        cov, _, okc, _ = g.motionCovariance(e)
        poses = g.trajectory(); calls += 1
        got = g.getPoseCovariances()
        want, c2 = stateless_step(pkg, tr, ok, cov, okc, carry, tp, tcp)            # one step from the latched base, not two
        same_records(got, want, f"group t{t} refit")
        d, stride = g.poseCovariancesDevice()
        assert stride == 1 and mi.hip_read(d, S, tc.COV).tobytes() == got.tobytes()
        base, carry = carry, c2
    # (the stream of constant images never is ok: before any accepted row REPEAT holds, so nothing is filled there)
    assert carry["step"].max() >= 2 and (got["status"] == 1).any() and (np.diagonal(got["cov"][2], 0, -2, -1) > 0).all()
    # re-anchoring inside a pair: stream 1 starts again (zero, nothing to repeat), stream 2 goes on from a given Sigma
    g.setPose(1, np.eye(4))
    g.setPoseCovariance(2, 3 * S0)
    expect(pkg, pkg.VH_ERR_STATE, lambda: g.getPoseCovariances())
    base = base.copy(); base[1] = start_carry(1)[0]; base["cov"][2] = 3 * S0; base["n_filled"][2] = 0
    g.trajectory(); calls += 1
    same_records(g.getPoseCovariances(), stateless_step(pkg, tr, ok, cov, okc, base, tp, tcp)[0], "re-anchored")
    g.synchronize()
    assert g.profileRead("trajectory")[1] == calls == g.profileRead("trajectory_cov")[1]
    g.close()


@pytest.mark.gpu
def test_gpu_edges_lone_matcher_first_call_and_replace_push(pkg, gpu):
    """A lone matcher (the poisoned child runs this too: the first call on a handle reads a block nothing has written but
    the start): step; replace push -- the getter is VH_ERR_STATE -- match, step under another motion: byte for byte ONE
    step from the base of the replaced pair; then a shifted push goes on from the carry."""
    frames = sr.frames_of(pkg, 4, 74)
    dims = sr.dims_of(pkg)
    e = mi.hego(pkg, inlier_threshold=2.5)
    other = np.array(mi.TR2, np.float64) + np.array([0.002, -0.001, 0.003, 0.25, -0.125, 0.5])
    m = pkg.Matcher(pkg.Params.default(), outlier_removal=True)
    m.setTrajectory()
    m.setTrajectoryCovariance(None, S0)
    base = start_carry(1, S0)

    def step(tr):
        m.matchFeatures(QUAD)
        n = m.motionInliers(e, tr)
        cov, _, okc, _ = m.motionCovariance(e)
        poses = m.trajectory()
        got = m.getPoseCovariances()
        assert got["status"][0] == poses["status"][0] and got["step"][0] == poses["step"][0]
        return got, cov, okc, n
    for left, right in frames[:2]:
        m.pushBack(left, right, dims)
    got, cov, okc, n = step(mi.TR2)
    want, _ = stateless_step(pkg, [mi.TR2], [1], [cov], [okc], base)
    same_records(got, want, "first call")
    assert n > 6 and okc and np.all(np.diag(got["cov"][0]) > np.diag(S0) * 0.5)
    m.pushBack(frames[2][0], frames[2][1], dims, True)
    expect(pkg, pkg.VH_ERR_STATE, lambda: m.getPoseCovariances())
    got, cov, okc, _ = step(other)                                              # (few or no inliers under it: the step may be a filled one)
    want, carry = stateless_step(pkg, [other], [1], [cov], [okc], base)
    same_records(got, want, "behind the replace push")
    assert got["step"][0] == 1
    m.pushBack(frames[3][0], frames[3][1], dims)
    got, cov, okc, _ = step(mi.TR2)
    same_records(got, stateless_step(pkg, [mi.TR2], [1], [cov], [okc], carry)[0], "behind the shifted push")
    assert got["step"][0] == 2
    m.close()


@pytest.mark.gpu
def test_gpu_sequence_handle_two_chunks(pkg, gpu):
    """SequenceGroup, chunks of 4 and 2 frames: the rows' covariances byte for byte ONE stateless chain over all rows fed
    the downloaded cov / ok_cov (row 0 of the first chunk holds no pair; the rows behind the short chunk: status 4, Sigma
    held); a repeated call gives the same bytes."""
    dims = sr.dims_of(pkg)
    frames = sr.frames_of(pkg, 6, sl.SEED)
    e = mi.hego(pkg, inlier_threshold=2.5)
    ROWS = sl.ROWS
    g = pkg.SequenceGroup(ROWS, pkg.Params.default(), max_matches=sl.MM)
    g.setTrajectory()
    g.setTrajectoryCovariance(None, S0)
    assert pkg._lib().vh_group_set_trajectory_covariance(g._h, C.byref(pkg.TrajCovParams.default()), None) == pkg.VH_ERR_UNSUPPORTED
    rows_in, got_rows = [], []
    for F, n in ((0, 4), (4, 2)):
        sr.push(g, frames, F, n, dims)
        g.matchFeatures(QUAD)
        tr = sl.motions(F)
        g.motionInliers(e, tr, np.ones(ROWS, np.int32))
        expect(pkg, pkg.VH_ERR_STATE, lambda: g.trajectory())
        cov, _, okc, _ = g.motionCovariance(e)
        poses = g.trajectory()
        got = g.getPoseCovariances()
        g.trajectory()
        assert g.getPoseCovariances().tobytes() == got.tobytes()
        assert np.array_equal(got["status"], poses["status"]) and np.array_equal(got["step"], poses["step"])
        assert (got["status"][n:] == 4).all() and all(got["cov"][r].tobytes() == got["cov"][n - 1].tobytes() for r in range(n, ROWS))
        got_rows.append(got[:n])
        rows_in.append((tr[:n], np.array([-1 if F + r == 0 else 1 for r in range(n)], np.int32), cov[:n], okc[:n]))
    one = tuple(np.concatenate([r[k] for r in rows_in]) for k in range(4))
    want, _ = run_stateless(pkg, [one], S0)
    same_records(np.concatenate(got_rows), want[0], "sequence rows")
    assert want[0]["status"].tolist() == [4, 0, 0, 0, 0, 0] and want[0]["step"][-1] == 5
    g.close()


@pytest.mark.gpu
def test_gpu_switch_off_and_the_block(pkg, ob, gpu):
    """Off: deviceBytes equals that of a handle that never heard of the switch, no "trajectory_cov" launch is profiled, the
    poses are byte for byte those of the handle with the switch on, the getters are VH_ERR_STATE.  On: the first call adds
    exactly the documented blocks, once; a refused allocation is VH_ERR_HIP, leaves the bytes and the poses' state as they
    were, and the repeated call is right."""
    fr, dims = pd.frames_of(pkg), pd.dims_of(pkg)
    e = pd.ego_of(pkg)
    S = pd.S
    hs = []
    for on in (False, True):
        g = pkg.StreamGroup(S, pkg.Params.default())
        g.setTrajectory()
        if on:
            g.setTrajectoryCovariance()
        g.profileEnable(True)
        for t in range(2):
            pd.push(g, fr, t, dims)
        g.matchFeatures(QUAD)
        tr0, ok0, _ = g.estimateMotion(e, mi.rand3_of(ob, e, S))
        g.motionInliers(e, tr0, ok0.astype(np.int32))
        cov, _, okc, _ = g.motionCovariance(e)
        g.synchronize()
        hs.append(g)
    off, on = hs
    bytes0 = on.deviceBytes()
    assert off.deviceBytes() == bytes0
    on.debugFailNextAlloc()
    expect(pkg, pkg.VH_ERR_HIP, lambda: on.trajectory())
    expect(pkg, pkg.VH_ERR_STATE, lambda: on.getPoses())
    on.synchronize()
    assert on.deviceBytes() == bytes0 and on.profileRead("trajectory")[1] == 0 and on.profileRead("trajectory_cov")[1] == 0
    poses_on = on.trajectory()
    same_records(on.getPoseCovariances(), stateless_step(pkg, tr0, ok0, cov, okc, start_carry(S))[0], "after the refused allocation")
    on.trajectory()
    up = lambda b: (b + 255) // 256 * 256  # noqa: E731
    assert on.deviceBytes() == bytes0 + 3 * up(272 * S) + up(304 * S) + 2 * up(880 * S)
    poses_off = off.trajectory()
    assert poses_off.tobytes() == poses_on.tobytes() and off.deviceBytes() == bytes0 + 3 * up(272 * S)
    expect(pkg, pkg.VH_ERR_STATE, lambda: off.getPoseCovariances())
    expect(pkg, pkg.VH_ERR_STATE, lambda: off.setPoseCovariance(0, S0))
    off.synchronize()
    assert off.profileRead("trajectory_cov")[1] == 0 and off.profileRead("trajectory")[1] == 1
    off.close(); on.close()


@pytest.mark.gpu
def test_gpu_child_on_poisoned_buffers(gpu):
    """DESIGN.md section 4.0's rule for new output arrays: ONE child process with VH_POISON=1 runs this file's edge cases
    (test_gpu_edges_*: empty chains, chains of status-4 rows only, a shorter call behind a longer one, the first call on a
    handle) on buffers that start as 0xA5 bytes."""
    cmd = [sys.executable, "-m", "pytest", os.path.abspath(__file__), "-q", "-x", "-m", "gpu", "-k", "edges"]
    r = subprocess.run(cmd, env=dict(os.environ, VH_POISON="1"), capture_output=True, text=True, timeout=120, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    assert "2 passed" in r.stdout and " skipped" not in r.stdout, r.stdout[-2000:]
