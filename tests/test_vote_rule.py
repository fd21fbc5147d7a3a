"""The rule of the outlier vote (include/viso_hip.h: vh_vote_rule, vh_set_vote_rule): VH_VOTE_REFERENCE is the vote as
it was, VH_VOTE_STOCK is stock libviso2's per-method rule with the disparity term, stated as a contract and restated in
numpy float32 by tests/vote_rule_oracle.py over the pinned triangulation.  Every comparison is byte for byte.

Discrimination: every list of at least MIN_PLANTED_N records that is voted under methods 1 and 2 carries planted records
-- a disparity off by more than twice the tolerance among consistent neighbours, flow untouched -- and is required, on
the restatement alone and before anything is compared, to lose at least 5 records under STOCK that REFERENCE keeps.
Shorter lists (4, 5, ... records: the size edges) cannot hold five such records with their neighbours; they are planted
the same way and compared, but carry no such requirement."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import multistage_oracle as mo
import vote_rule_oracle as vo
from conftest import GOLDEN, ROOT

F32 = np.float32
SYMBOLS = ("vh_remove_outliers_pm_rule", "vh_remove_outliers_device_rule", "vh_set_vote_rule", "vh_group_set_vote_rule")
CASES = ("small_default", "small_bin20_r60", "dense_gain4")
TOL = 5.0
MIN_PLANTED_N = 60
METHODS = (0, 1, 2)


def golden():
    return np.load(os.path.join(GOLDEN, "outliers.npz"))


def planted(pkg, rng, n, W=640, H=240, tol=TOL, flow_outliers=0.08):
    """n quad records on distinct integer pixels: a smooth flow with a few flow outliers, a smooth disparity, and planted
    records whose disparity is off by more than 2 x tol while their flow is untouched."""
    cells = rng.choice(W * H, n, replace=False)
    pm = np.zeros(n, pkg.P_MATCH_DTYPE)
    pm["u1c"] = (cells % W).astype(F32)
    pm["v1c"] = (cells // W).astype(F32)
    pm["u1p"] = pm["u1c"] + 3
    pm["v1p"] = pm["v1c"] - 1
    pm["u2c"] = pm["u1c"] - 7
    pm["v2c"] = pm["v1c"]
    pm["u2p"] = pm["u1p"] - 7
    pm["v2p"] = pm["v1p"]
    for f in ("i1p", "i2p", "i1c", "i2c"):
        pm[f] = np.arange(n)
    k = rng.permutation(n)
    n_flow = int(n * flow_outliers)
    bad = k[:n_flow]
    pm["u1p"][bad] += rng.integers(-25, 26, n_flow).astype(F32)
    pm["v1p"][bad] += rng.integers(-9, 10, n_flow).astype(F32)
    n_disp = max(1, n // 10) if n < MIN_PLANTED_N else max(8, n // 10)
    off = k[n_flow:n_flow + n_disp]
    pm["u2c"][off] -= (2 * tol + 1 + rng.integers(0, 30, len(off))).astype(F32) * rng.choice([-1, 1], len(off)).astype(F32)
    return pm


def with_planted_disparities(pm, rng, tol=TOL):
    """A flow list of the reference's (u2c = -1 everywhere) given a smooth disparity and planted records"""
    pm = pm.copy()
    pm["u2c"] = pm["u1c"] - 7
    off = rng.choice(len(pm), max(8, len(pm) // 10), replace=False)
    pm["u2c"][off] -= F32(2 * tol + 3)
    return pm


def discriminates(oracle, pm, method, tol=TOL):
    """The condition of the module docstring, on the restatement alone"""
    ref = vo.votes(oracle, pm, None) >= 4
    stock = vo.votes(oracle, pm, vo.stock(method, tol, tol)) >= 4
    return int(np.sum(ref & ~stock))


def require_discrimination(oracle, lists, method):
    if method == 0:
        return
    for k, pm in enumerate(lists):
        if len(pm) >= MIN_PLANTED_N:
            lost = discriminates(oracle, pm, method)
            assert lost >= 5, (k, len(pm), method, lost)


def golden_lists(rng):
    z = golden()
    return [with_planted_disparities(z[name + "__in"], rng) for name in CASES]


# ------------------------------------------------------------------ CPU
def test_restatement_with_the_reference_rule_equals_the_pinned_oracle(oracle):
    z = golden()
    for name in CASES:
        pm = z[name + "__in"]
        want, _ = oracle.remove_outliers(pm)
        assert want.tobytes() == pm[z[name + "__kept"]].tobytes()
        assert vo.remove_outliers(oracle, pm, None).tobytes() == want.tobytes()
        assert vo.remove_outliers(oracle, pm, (vo.VOTE_REFERENCE, 7, -1.0, -1.0)).tobytes() == want.tobytes()  # (method, tolerances: not read)


@pytest.mark.parametrize("method", METHODS)
def test_host_form_equals_the_restatement(method, pkg, oracle):
    rng = np.random.default_rng(100 + method)
    lists = golden_lists(rng) + [planted(pkg, rng, int(n)) for n in rng.integers(4, 601, 200)]
    require_discrimination(oracle, lists, method)
    dropped = 0
    for k, pm in enumerate(lists):
        rule = vo.stock(method, TOL, TOL)
        got = pkg.remove_outliers(pm, rule=pkg.VoteRule.stock(method, TOL, TOL))
        assert got.tobytes() == vo.remove_outliers(oracle, pm, rule).tobytes(), (k, len(pm))
        dropped += len(pm) - len(got)
        if method == 0:  # the identity that ties the new path to the pinned one
            assert got.tobytes() == pkg.remove_outliers(pm).tobytes() == oracle.remove_outliers(pm)[0].tobytes(), k
        assert pkg.remove_outliers(pm, rule=pkg.VoteRule.reference()).tobytes() == pkg.remove_outliers(pm).tobytes()
    assert dropped > 200
    # other tolerances than the default pair
    for pm in lists[:20]:
        for ft, dt in ((2.0, 9.0), (11.5, 1.0)):
            assert pkg.remove_outliers(pm, rule=(1, method, ft, dt)).tobytes() == vo.remove_outliers(oracle, pm, (1, method, ft, dt)).tobytes()


def edge_lists(pkg, oracle):
    """[(name, list, rule as a tuple)] -- the edges of the contract, shared by the host and the device tests"""
    rng = np.random.default_rng(7)
    out = []
    base = planted(pkg, rng, 300)
    # a difference exactly equal to the tolerance is excluded, the next float below is included: a smooth list whose
    # record 0 differs from all its neighbours by exactly 4 in disparity (and 4 in flow)
    exact = planted(pkg, rng, 200, flow_outliers=0.0)
    exact["u2c"] = exact["u1c"] - 7
    exact["u2c"][0] -= 4
    exact["u1p"][0] += 4
    below = float(np.nextafter(F32(4), F32(0)))
    above = float(np.nextafter(F32(4), F32(9)))
    for m in METHODS:
        out.append((f"tol == diff m{m}", exact, (1, m, 4.0, 4.0)))
        out.append((f"tol just above diff m{m}", exact, (1, m, above, above)))
        out.append((f"tol just below diff m{m}", exact, (1, m, below, below)))
        out.append((f"tol 0 m{m}", base, (1, m, 0.0, 0.0)))
        out.append((f"tol -1 m{m}", base, (1, m, -1.0, -1.0)))
        out.append((f"tol huge m{m}", base, (1, m, 3e38, 3e38)))
        nan = base.copy()
        nan["u2c"][::17] = np.nan
        out.append((f"NaN u2c m{m}", nan, (1, m, TOL, TOL)))
        for n in (0, 3, 4):
            out.append((f"n={n} m{m}", base[:n].copy(), (1, m, TOL, TOL)))
        line = base[:12].copy()
        line["v1c"] = 50
        line["u1c"] = np.arange(12) * 7
        out.append((f"collinear m{m}", line, (1, m, 3e38, 3e38)))
    return out, exact


def test_host_form_edges(pkg, oracle):
    cases, exact = edge_lists(pkg, oracle)
    got = {}
    for name, pm, rule in cases:
        g = pkg.remove_outliers(pm, rule=rule)
        assert g.tobytes() == vo.remove_outliers(oracle, pm, rule).tobytes(), name
        got[name] = (pm, g)
    for m in METHODS:
        # record 0 of `exact` differs from every neighbour by exactly 4: out under 4 and below, in just above
        kept = lambda name: bool(np.any(got[name][1]["i1c"] == 0))
        assert not kept(f"tol == diff m{m}") and not kept(f"tol just below diff m{m}") and kept(f"tol just above diff m{m}"), m
        for name in (f"tol 0 m{m}", f"tol -1 m{m}", f"collinear m{m}"):
            assert len(got[name][1]) == 0, name
        for n in (0, 3):
            assert len(got[f"n={n} m{m}"][1]) == n
        pm, g = got[f"tol huge m{m}"]
        tri, _ = oracle.delaunay(np.stack([pm["u1c"], pm["v1c"]], 1))
        incident = np.bincount(tri.ravel(), minlength=len(pm)) * 2  # two edge-votes per triangle a record is a corner of
        assert g.tobytes() == pm[incident >= 4].tobytes()
        pm, g = got[f"NaN u2c m{m}"]
        if m != 0:
            assert not np.isnan(g["u2c"]).any()  # a NaN term disagrees with everything
    lib = pkg._lib()
    n = C.c_int32(0)
    pm = got["tol huge m0"][0].copy()
    P = pm.ctypes.data_as(C.c_void_p)
    for bad in ((2, 0, 5.0, 5.0), (-1, 0, 5.0, 5.0), (1, 3, 5.0, 5.0), (1, -1, 5.0, 5.0)):
        assert lib.vh_remove_outliers_pm_rule(P, len(pm), C.byref(pkg.VoteRule(*bad)), C.byref(n)) == pkg.VH_ERR_INVALID_ARG, bad
        assert lib.vh_remove_outliers_pm_rule(P, 2, C.byref(pkg.VoteRule(*bad)), C.byref(n)) == pkg.VH_ERR_INVALID_ARG, bad
    assert lib.vh_remove_outliers_pm_rule(P, len(pm), C.byref(pkg.VoteRule(0, 9, 0.0, 0.0)), C.byref(n)) == pkg.VH_OK  # (not read)
    assert lib.vh_remove_outliers_pm_rule(P, len(pm), None, None) == pkg.VH_ERR_INVALID_ARG
    assert lib.vh_set_vote_rule(None, 1) == pkg.VH_ERR_INVALID_ARG and lib.vh_group_set_vote_rule(None, 0) == pkg.VH_ERR_INVALID_ARG


def test_symbols_struct_size_and_the_shim(pkg, tmp_path):
    header = open(os.path.join(ROOT, "include", "viso_hip.h")).read()
    lib = C.CDLL(pkg.LIB_PATH)
    for name in SYMBOLS:
        assert name + "(" in header and hasattr(lib, name) and name in pkg.ABI_SYMBOLS, name
    assert C.sizeof(pkg.VoteRule) == 16 and pkg.VOTE_REFERENCE == 0 and pkg.VOTE_STOCK == 1
    for cls in (pkg.Matcher, pkg.StreamGroup, pkg.SequenceGroup):
        assert callable(cls.setVoteRule)
    inc = os.path.join(ROOT, "include")
    src = tmp_path / "use.c"
    src.write_text('#include <stddef.h>\n#include "viso_hip.h"\n'
                   "typedef char size_is_16[sizeof(vh_vote_rule) == 16 ? 1 : -1];\n"
                   "typedef char offsets[offsetof(vh_vote_rule, rule) == 0 && offsetof(vh_vote_rule, method) == 4 &&\n"
                   "                     offsetof(vh_vote_rule, flow_tolerance) == 8 && offsetof(vh_vote_rule, disp_tolerance) == 12 ? 1 : -1];\n"
                   "int main(void) {\n"
                   "  vh_vote_rule r = {VH_VOTE_STOCK, VH_METHOD_STEREO, 5.0f, 5.0f};\n"
                   "  vh_p_match pm[3]; int32_t n = -1;\n"
                   "  if (VH_VOTE_REFERENCE != 0 || VH_VOTE_STOCK != 1) return 1;\n"
                   "  if (vh_remove_outliers_pm_rule(pm, 3, &r, &n) != VH_OK || n != 3) return 2;\n"
                   "  r.method = 3;\n"
                   "  if (vh_remove_outliers_pm_rule(pm, 3, &r, &n) != VH_ERR_INVALID_ARG) return 3;\n"
                   "  return vh_set_vote_rule(NULL, VH_VOTE_STOCK) == VH_ERR_INVALID_ARG && vh_group_set_vote_rule(NULL, 0) == VH_ERR_INVALID_ARG ? 0 : 4;\n}\n")
    subprocess.check_call(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-fsyntax-only", "-I" + inc, str(src)])
    libdir = os.path.dirname(pkg.LIB_PATH)
    exe = str(tmp_path / "use")
    subprocess.check_call(["gcc", "-std=c99", "-I" + inc, str(src), "-o", exe, "-L" + libdir, "-lviso_hip", "-Wl,-rpath," + libdir])
    assert subprocess.run([exe]).returncode == 0
    cpp = tmp_path / "shim.cpp"
    cpp.write_text('#include "viso_hip_matcher.hpp"\n'
                   "int main() { Matcher::parameters p; Matcher *m = 0; bool (Matcher::*f)(bool) = &Matcher::setStockOutlierRule;\n"
                   "  return (f != 0 && sizeof(p) == sizeof(vh_params) && !m) ? 0 : 1; }\n")
    exe2 = str(tmp_path / "shim")
    subprocess.check_call(["g++", "-std=gnu++11", "-O1", "-Wall", "-Werror", "-I" + inc, str(cpp), "-o", exe2, "-L" + libdir, "-lviso_hip",
                           "-Wl,-rpath," + libdir])
    assert subprocess.run([exe2]).returncode == 0


# ------------------------------------------------------------------ GPU, stateless
def size_lists(pkg, rng):
    return [planted(pkg, rng, n) for n in (4, 5, 63, 64, 65, 1800)]


def stateless_check(pkg, oracle, lists, method, lanes, rule=None, **kw):
    rule = rule or (1, method, TOL, TOL)
    got, _, _ = pkg.remove_outliers_device(lists, lanes_per_wave=lanes, rule=rule, **kw)
    for k, (g, pm) in enumerate(zip(got, lists)):
        want = vo.remove_outliers(oracle, pm, rule)
        if kw.get("max_features", 0) >= 1:
            want = oracle.bucket_features(want, kw["max_features"], kw["bucket_width"], kw["bucket_height"])
        assert g.tobytes() == want.tobytes(), (k, len(pm), len(g), len(want), rule)
    return got


@pytest.mark.gpu
@pytest.mark.parametrize("method", METHODS)
def test_gpu_stateless_sizes_lanes_and_bucketing(method, pkg, oracle, gpu):
    rng = np.random.default_rng(200 + method)
    lists = size_lists(pkg, rng) + golden_lists(rng) + [planted(pkg, rng, int(n)) for n in rng.integers(60, 400, 8)]  # 17 lists
    assert len(lists) == 17
    require_discrimination(oracle, lists, method)
    for n_lists in (1, 2, 17):
        for lanes in (1, 16):
            stateless_check(pkg, oracle, lists[5:6] if n_lists == 1 else lists[:n_lists], method, lanes)
    stateless_check(pkg, oracle, lists, method, 16, max_features=2, bucket_width=50.0, bucket_height=50.0)
    if method == 0:  # STOCK, method 0, tolerance 5 is REFERENCE
        a, _, _ = pkg.remove_outliers_device(lists, lanes_per_wave=16, rule=(1, 0, 5.0, 5.0))
        b, _, _ = pkg.remove_outliers_device(lists, lanes_per_wave=16)
        c, _, _ = pkg.remove_outliers_device(lists, lanes_per_wave=16, rule=pkg.VoteRule.reference())
        for x, y, w in zip(a, b, c):
            assert x.tobytes() == y.tobytes() == w.tobytes()


@pytest.mark.gpu
@pytest.mark.parametrize("method", METHODS)
def test_gpu_stateless_global_tally(method, pkg, oracle, gpu):
    """One list of 16 500 records: beyond the LDS counters, the thread-per-triangle tally with global atomics"""
    rng = np.random.default_rng(300 + method)
    lists = [planted(pkg, rng, 16500, W=1920, H=1080), planted(pkg, rng, 70)]
    require_discrimination(oracle, lists, method)
    got = stateless_check(pkg, oracle, lists, method, 2)
    assert 8000 < len(got[0]) < 16500


@pytest.mark.gpu
def test_gpu_stateless_edges_and_refusals(pkg, oracle, gpu):
    cases, _ = edge_lists(pkg, oracle)
    by_rule = {}
    for name, pm, rule in cases:
        by_rule.setdefault(rule, []).append(pm)
    for rule, lists in by_rule.items():
        stateless_check(pkg, oracle, lists, rule[1], 16, rule=rule)
    rng = np.random.default_rng(9)
    # a refused list (NaN coordinate) is refused alone
    lists = [planted(pkg, rng, 200), planted(pkg, rng, 90), planted(pkg, rng, 150)]
    lists[1]["u1c"][7] = np.nan
    for m in METHODS:
        rule = (1, m, TOL, TOL)
        got, _, _, rc = pkg.remove_outliers_device(lists, lanes_per_wave=16, strict=False, rule=rule)
        assert rc == pkg.VH_ERR_UNSUPPORTED and len(got[1]) == 0
        for k in (0, 2):
            assert got[k].tobytes() == vo.remove_outliers(oracle, lists[k], rule).tobytes()
    for bad in ((2, 0, 5.0, 5.0), (1, 3, 5.0, 5.0), (1, -1, 5.0, 5.0)):
        with pytest.raises(pkg.VisoHipError) as ex:
            pkg.remove_outliers_device(lists[:1], rule=bad)
        assert ex.value.code == pkg.VH_ERR_INVALID_ARG


@pytest.mark.gpu
def test_gpu_child_checking_build(pkg, gpu):
    """The stateless cases once more on libviso_hip_check.so (-DVH_CHECK)"""
    assert os.path.exists(pkg.CHECK_LIB_PATH), "build() makes it"
    env = dict(os.environ, VISO_HIP_LIB=pkg.CHECK_LIB_PATH)
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-q", "-x", "-m", "gpu", "-k", "gpu_stateless"],
                       env=env, capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "7 passed" in r.stdout and " skipped" not in r.stdout, r.stdout[-2000:]
    assert "VH_CHECK" not in r.stderr


# ------------------------------------------------------------------ GPU, handles
W, H, S, T = 240, 120, 3, 6
CAP = 4096
_FRAMES = {}


def dims_of(pkg):
    return [W, H, pkg.synth.bytes_per_line(W)]


def frames_of(pkg):
    """[stream][t] -> (left, right): stream 0 with a patch of its right images shifted (the matcher itself then produces
    disparity outliers), stream 1 empty, stream 2 short"""
    if "f" not in _FRAMES:
        fr = [pkg.synth.stereo_sequence(W, H, T, disparity=6, blur=3, seed=seed) for seed in (71, 72, 73)]
        shifted = []
        for a, b in fr[0]:
            src, b, k = b, b.copy(), 0
            for v0 in range(10, H - 17, 40):       # small patches: their few features have no like-minded neighbours
                for u0 in range(20, W - 32, 40):
                    b[v0:v0 + 12, u0:u0 + 12] = np.roll(src, (9, -8, 11, -10)[k % 4], axis=1)[v0:v0 + 12, u0:u0 + 12]
                    k += 1
            shifted.append((a, b))
        fr[0] = shifted
        fr[1] = [(np.full_like(a, 90), np.full_like(b, 90)) for a, b in fr[1]]
        half = []
        for a, b in fr[2]:
            a, b = a.copy(), b.copy()
            a[:, int(0.45 * W):] = 90; b[:, int(0.45 * W):] = 90
            half.append((a, b))
        fr[2] = half
        _FRAMES["f"] = fr
    return _FRAMES["f"]


def push(g, fr, t, dims):
    g.pushBack(np.stack([f[t][0] for f in fr]), np.stack([f[t][1] for f in fr]), dims)


def handle_rule(method):
    return (1, method, 5.0, 5.0)  # (float) of the default outlier_flow_tolerance / outlier_disp_tolerance


@pytest.mark.gpu
@pytest.mark.parametrize("method", METHODS)
def test_gpu_group_votes_under_the_stock_rule(method, pkg, oracle, gpu):
    """vh_group_remove_outliers, the host post chain and the device post chain (2 steps x 2 batches, the ring coming
    round) against the stateless entry on the lists fetched before voting; a default-rule group on the same frames gives
    the parent's bits."""
    fr, dims = frames_of(pkg), dims_of(pkg)
    g = pkg.StreamGroup(S, pkg.Params.default())
    d = pkg.StreamGroup(S, pkg.Params.default())   # the default rule
    g.setVoteRule(pkg.VOTE_STOCK)
    g.postDeviceConfig(2, 2, 16)
    d.postDeviceConfig(2, 2, 16)
    push(g, fr, 0, dims); push(d, fr, 0, dims)
    raw, dev, dev_d = {}, {}, {}
    lost = 0
    for t in range(1, T):
        push(g, fr, t, dims); push(d, fr, t, dims)
        g.matchFeatures(method); d.matchFeatures(method)
        raw[t] = [g.getMatches(s) for s in range(S)]
        assert [x.tobytes() for x in raw[t]] == [d.getMatches(s).tobytes() for s in range(S)]
        assert len(raw[t][0]) > 100 and len(raw[t][1]) == 0 and 3 < len(raw[t][2]) < len(raw[t][0])
        rule = handle_rule(method)
        want = [vo.remove_outliers(oracle, pm, rule) for pm in raw[t]]
        want_d = [pm.copy() if method == 1 else oracle.remove_outliers(pm)[0] for pm in raw[t]]
        if method != 0:  # (what the default rule keeps: a stereo list whole, a quad list by its flow)
            ref_keeps = np.ones(len(raw[t][0]), bool) if method == 1 else vo.votes(oracle, raw[t][0], None) >= 4
            lost += int(np.sum(ref_keeps & ~(vo.votes(oracle, raw[t][0], rule) >= 4)))
        stateless, _, _ = pkg.remove_outliers_device(raw[t], lanes_per_wave=16, rule=rule)
        assert [x.tobytes() for x in stateless] == [x.tobytes() for x in want]
        # the device chain first (it reads the device lists), then the host chain, then the in-place host vote
        for grp in (g, d):
            grp.postBeginDevice(CAP, 2, 50.0, 50.0, want_lists=True)
            grp.postBegin(CAP)
        host = g.postFinish(0, 2, 50.0, 50.0, host_threads=2)
        host_d = d.postFinish(0, 2, 50.0, 50.0, host_threads=2)
        for s in range(S):
            assert host["lists"][s].tobytes() == oracle.bucket_features(want[s], 2, 50, 50).tobytes(), (t, s)
            assert host_d["lists"][s].tobytes() == oracle.bucket_features(want_d[s], 2, 50, 50).tobytes(), (t, s)
        if t >= 3:  # two steps ahead: the step of t - 2 comes out while two are in flight
            dev[t - 2] = g.postFinishDevice(2, want_lists=True, list_cap=CAP, estimator=False)["lists"]
            dev_d[t - 2] = d.postFinishDevice(2, want_lists=True, list_cap=CAP, estimator=False)["lists"]
        g.removeOutliers(host_threads=2); d.removeOutliers(host_threads=2)
        for s in range(S):
            assert g.getMatches(s).tobytes() == want[s].tobytes(), (t, s)
            assert d.getMatches(s).tobytes() == want_d[s].tobytes(), (t, s)
    for age, t in ((1, T - 2), (0, T - 1)):
        dev[t] = g.postFinishDevice(age, want_lists=True, list_cap=CAP, estimator=False)["lists"]
        dev_d[t] = d.postFinishDevice(age, want_lists=True, list_cap=CAP, estimator=False)["lists"]
    for t in range(1, T):
        rule = handle_rule(method)
        for s in range(S):
            want = oracle.bucket_features(vo.remove_outliers(oracle, raw[t][s], rule), 2, 50, 50)
            want_d = oracle.bucket_features(raw[t][s] if method == 1 else oracle.remove_outliers(raw[t][s])[0], 2, 50, 50)
            assert dev[t][s].tobytes() == want.tobytes(), (t, s)
            assert dev_d[t][s].tobytes() == want_d.tobytes(), (t, s)
    if method != 0:
        assert lost >= 5, lost  # the shifted patches gave the matcher disparity outliers that only the stock rule drops
    # state rules: the setters are legal before the first push only, on either kind of handle
    for rule in (pkg.VOTE_REFERENCE, pkg.VOTE_STOCK):
        with pytest.raises(pkg.VisoHipError) as ex:
            g.setVoteRule(rule)
        assert ex.value.code == pkg.VH_ERR_STATE
    g.postBeginDevice(CAP, 2, 50.0, 50.0, want_lists=True)   # ... and with a step in flight
    with pytest.raises(pkg.VisoHipError) as ex:
        g.setVoteRule(pkg.VOTE_REFERENCE)
    assert ex.value.code == pkg.VH_ERR_STATE
    g.postFinishDevice(0, want_lists=True, list_cap=CAP, estimator=False)
    g.close(); d.close()


@pytest.mark.gpu
def test_gpu_setter_arguments_and_off_state(pkg, gpu):
    """A bad rule is refused; with the rule at its default (never set, or set to VOTE_REFERENCE) a group reports the same
    device bytes and lists as one that never heard of the rule, and times no tally scope but the reference one."""
    fr, dims = frames_of(pkg), dims_of(pkg)
    res = []
    for setter in (None, pkg.VOTE_REFERENCE, pkg.VOTE_STOCK):
        g = pkg.StreamGroup(S, pkg.Params.default())
        for bad in (-1, 2):
            with pytest.raises(pkg.VisoHipError) as ex:
                g.setVoteRule(bad)
            assert ex.value.code == pkg.VH_ERR_INVALID_ARG
        if setter is not None:
            g.setVoteRule(setter)
        g.postDeviceConfig(1, 2, 16)
        g.profileEnable(True)
        push(g, fr, 0, dims); push(g, fr, 1, dims)
        g.matchFeatures(pkg.METHOD_QUAD)
        g.postBeginDevice(CAP, 2, 50.0, 50.0, want_lists=True)
        lists = g.postFinishDevice(0, want_lists=True, list_cap=CAP, estimator=False)["lists"]
        g.synchronize()
        scopes = {name: g.profileRead(name) for name in ("vote_tally", "vote_tally_flow", "vote_tally_disp", "vote_tally_quad")}
        res.append(([x.tobytes() for x in lists], g.deviceBytes(), scopes))
        g.close()
    assert res[0][0] == res[1][0] and res[0][1] == res[1][1] == res[2][1]  # no rule needs a byte more
    launches = lambda sc: {k: int(v[1]) for k, v in sc.items()}
    assert launches(res[0][2]) == launches(res[1][2]) == {"vote_tally": 1, "vote_tally_flow": 0, "vote_tally_disp": 0, "vote_tally_quad": 0}
    assert launches(res[2][2]) == {"vote_tally": 0, "vote_tally_flow": 0, "vote_tally_disp": 0, "vote_tally_quad": 1}


@pytest.mark.gpu
def test_gpu_sequence_handle(pkg, oracle, gpu):
    """A sequence handle with chunks of 4 and 2 frames: vh_group_remove_outliers under the stock rule, every row's list"""
    fr, dims = frames_of(pkg)[0], dims_of(pkg)
    q = pkg.SequenceGroup(4, pkg.Params.default())
    q.setVoteRule(pkg.VOTE_STOCK)
    for lo, hi in ((0, 4), (4, 6)):
        q.pushBack(np.stack([fr[t][0] for t in range(lo, hi)]), np.stack([fr[t][1] for t in range(lo, hi)]), dims)
        for method in (2, 1):
            q.matchFeatures(method)
            first, n = q.position()
            raw = [q.getMatches(r) for r in range(n)]
            q.removeOutliers(host_threads=2)
            rows = [r for r in range(n) if len(raw[r]) > 3]
            assert rows
            for r in rows:
                assert q.getMatches(r).tobytes() == vo.remove_outliers(oracle, raw[r], handle_rule(method)).tobytes(), (lo, method, r)
            assert sum(len(raw[r]) - len(q.getMatches(r)) for r in rows) > 0
    with pytest.raises(pkg.VisoHipError) as ex:
        q.setVoteRule(pkg.VOTE_REFERENCE)
    assert ex.value.code == pkg.VH_ERR_STATE
    q.close()


@pytest.mark.gpu
def test_gpu_lone_matcher_and_its_tolerances(pkg, oracle, gpu):
    """A lone matcher: matchFeatures(method) votes with its method under (float) of the handle's two tolerances"""
    fr, dims = frames_of(pkg)[0], dims_of(pkg)
    p = pkg.Params.default(outlier_flow_tolerance=3, outlier_disp_tolerance=2)
    m = pkg.Matcher(p)
    bare = pkg.Matcher(p, outlier_removal=False)
    m.setVoteRule(pkg.VOTE_STOCK)
    for t in range(3):
        m.pushBack(fr[t][0], fr[t][1], dims, False); bare.pushBack(fr[t][0], fr[t][1], dims, False)
    for method in METHODS:
        m.matchFeatures(method); bare.matchFeatures(method)
        raw = bare.getMatches()
        want = vo.remove_outliers(oracle, raw, (1, method, 3.0, 2.0))
        assert m.getMatches().tobytes() == want.tobytes(), method
        assert method == 0 or len(want) < len(raw), method  # (the frames' flow is clean; their disparities are not)
    with pytest.raises(pkg.VisoHipError) as ex:
        m.setVoteRule(pkg.VOTE_REFERENCE)
    assert ex.value.code == pkg.VH_ERR_STATE
    m.close(); bare.close()


@pytest.mark.gpu
@pytest.mark.parametrize("device_mode", [False, True])
def test_gpu_multi_stage_votes_the_sparse_list(device_mode, pkg, ob, oracle, gpu):
    """Multi-stage matching under the stock rule, host and device mode: the sparse list returned is STOCK applied to the
    unvoted pass-1 list (from a plain group whose nms_n is the sparse distance), and the pass-2 list is what
    tests/multistage_oracle.py gives when fed that voted list."""
    fr, dims = frames_of(pkg), dims_of(pkg)
    p = pkg.Params.default(multi_stage=1)
    sparse_nms = min(p.nms_n * 4, max(p.nms_n, 10)) if p.nms_n * 4 > 10 else p.nms_n * 4
    g = pkg.StreamGroup(S, p)
    g.setVoteRule(pkg.VOTE_STOCK)
    g.setMultiStageMatching(True)
    if device_mode:
        g.setMultiStageDevice(True)
    plain = pkg.StreamGroup(S, pkg.Params.default(nms_n=sparse_nms))
    po = ob.Params.default(multi_stage=1)
    for t in range(2):
        push(g, fr, t, dims); push(plain, fr, t, dims)
    feats = [[g.getFeatures(s, k) for k in range(4)] for s in range(S)]
    for method in (1, 2, 0):
        g.matchFeatures(method); plain.matchFeatures(method)
        for s in (0, 2):
            unvoted = plain.getMatches(s)
            voted = vo.remove_outliers(oracle, unvoted, handle_rule(method))
            assert len(unvoted) > 3
            assert g.getSparseMatches(s).tobytes() == voted.tobytes(), (method, s)
            dense_sets = [feats[s][r] if r in mo.NEED[method] else None for r in range(4)]
            want = mo.ranged_matching(po, dims, method, *dense_sets, mo.statistics(po, dims, method, voted))
            assert g.getMatches(s).tobytes() == want.tobytes(), (method, s)
        if method == 1:
            assert any(len(vo.remove_outliers(oracle, plain.getMatches(s), handle_rule(1))) < len(plain.getMatches(s)) for s in (0, 2))
    g.close(); plain.close()
