"""Monocular egomotion (csrc/kernels_mono.hip) at the edges of its structure: the shortest accepted lists, hypothesis
counts around mono_hyp's 128-wide workgroups, exact ties between workgroups, the LDS / global-memory switch of the
refit (MONO_LDS_ROWS = 640) and its 8-rows-per-lane boundary (2048), every rejection path and the parameter space.
CPU part: the oracle equals the reference (recorded answers and tests/golden/mono_edges.npz,
oracle/gen_golden_mono.py) on one scene of every new kind.  GPU part: the device equals the oracle -- success flag and
inlier list exact, tr to 1e-9 relative, all zero on failure -- in the fast form of the hypothesis kernel and, through
one child process with VH_MONO_SIGNED=1, in the signed one.  Premises are asserted on the oracle first."""
import os

import numpy as np
import pytest

import egomotion_scene as es
from conftest import GOLDEN, entry

_D = entry.load_oracle().P_MATCH_DTYPE
_CASES = es.mono_edge_cases(_D)


def _mono(mod, kw):
    return mod.MonoParams.default() if kw is None else mod.MonoParams.default(**kw)


def _close(tr, want):
    return np.allclose(tr, want, rtol=1e-9, atol=1e-12)


def _glibc(ob, iters, n_sets):
    r = ob.glibc_rand_after_srand0(8 * iters).reshape(iters, 8)
    return np.stack([r] * n_sets)


def _samples(oracle, n, iters, raw=None):
    if n < 10:
        return np.zeros((iters, 8), np.int32)
    return oracle.draw_samples_n(n, 8, iters, None if raw is None else np.ascontiguousarray(raw).reshape(-1))


def _compare(pkg, ob, oracle, kw, lists, raw, label=""):
    """One batched launch against the oracle, list by list -> the oracle's results."""
    e, ge = _mono(ob, kw), _mono(pkg, kw)
    tr, ok, inl = pkg.estimate_motion_mono(ge, lists, raw)
    want = []
    for s, pm in enumerate(lists):
        ok_o, tr_o, inl_o = oracle.estimate_motion_mono(e, pm, _samples(oracle, len(pm), e.ransac_iters, raw[s]))
        assert ok[s] == ok_o, (label, s, len(pm), ok[s], ok_o, len(inl[s]), len(inl_o))
        assert np.array_equal(inl[s], inl_o), (label, s, len(pm), len(inl[s]), len(inl_o))
        assert _close(tr[s], tr_o), (label, s, tr[s], tr_o)
        if not ok_o:
            assert tr[s].tobytes() == bytes(48), (label, s, tr[s])
        want.append((ok_o, tr_o, inl_o))
    return want


# ---------------------------------------------------------------------------------------------- CPU: trust the oracle

@pytest.mark.parametrize("name", sorted(_CASES))
def test_oracle_equals_reference_at_edges_mono(name, ob, oracle, reference):
    pm, kw = _CASES[name]
    e = _mono(ob, kw)
    ok_o, tr_o, inl_o = oracle.estimate_motion_mono(e, pm, _samples(oracle, len(pm), e.ransac_iters))
    ok_r, tr_r, inl_r = reference.estimate_motion_mono(e, pm)
    assert ok_o == ok_r and np.array_equal(inl_o, inl_r), name
    assert tr_o.tobytes() == tr_r.tobytes(), (tr_o, tr_r)


@pytest.mark.parametrize("name", sorted(_CASES))
def test_oracle_golden_edges_mono(name, ob, oracle):
    """The same against vectors recorded from the reference, on the recorded match lists; the builders still produce
    those lists."""
    z = np.load(os.path.join(GOLDEN, "mono_edges.npz"))
    pm = np.ascontiguousarray(z[name + "__pm"]).view(ob.P_MATCH_DTYPE).reshape(-1)
    assert pm.tobytes() == _CASES[name][0].tobytes()
    e = _mono(ob, _CASES[name][1])
    ok_o, tr_o, inl_o = oracle.estimate_motion_mono(e, pm, _samples(oracle, len(pm), e.ransac_iters))
    assert ok_o == bool(z[name + "__ok"]) and np.array_equal(inl_o, z[name + "__inliers"]) and tr_o.tobytes() == z[name + "__tr"].tobytes()


def test_mono_scene_kinds_are_what_they_claim(ob, oracle):
    def run(name):
        pm, kw = _CASES[name]
        e = _mono(ob, kw)
        return oracle.estimate_motion_mono(e, pm, _samples(oracle, len(pm), e.ransac_iters))
    ok, _, inl = run("n9")
    assert not ok and len(inl) == 0                       # empty below 10 matches, as the reference
    assert run("n11")[0] and run("n12")[0]
    ok, _, inl = run("identical30")
    assert not ok and len(inl) == 0                       # degenerate scale
    ok, _, inl = run("no_motion")
    assert not ok and len(inl) >= 10                      # rejected after the refit: motion_threshold
    ok, _, inl = run("pure_rotation")
    assert not ok and len(inl) >= 10                      # near-pure rotation: rejected after the refit as well
    for n, _ in es.MONO_FEW_INLIER_SEEDS:
        ok, _, inl = run(f"few_inliers_{n}")
        assert not ok and 0 < len(inl) < 10, (n, len(inl))


def _sampson_equal(ob, oracle):
    """The list, the one sample and the threshold at which one match's Sampson distance EQUALS inlier_threshold, asserted
    on the oracle: the match is out at the threshold (strict `<`) and in at the next double, and it is the only change."""
    pm = _CASES["sampson_equal"][0]
    sample = oracle.draw_samples_n(len(pm), 8, 1)
    thr = es.SAMPSON_EQUAL_THRESHOLD
    _, _, at = oracle.estimate_motion_mono(_mono(ob, _CASES["sampson_equal"][1]), pm, sample)
    _, _, above = oracle.estimate_motion_mono(_mono(ob, _CASES["sampson_next"][1]), pm, sample)
    assert _CASES["sampson_next"][1]["inlier_threshold"] == np.nextafter(thr, 1.0) > thr
    assert len(at) + 1 == len(above) and len(at) >= 10, (len(at), len(above))
    assert es.SAMPSON_EQUAL_MATCH not in at and sorted(set(above) - set(at)) == [es.SAMPSON_EQUAL_MATCH]
    return pm, sample[0], at, above


def test_sampson_equality_premise(ob, oracle):
    _sampson_equal(ob, oracle)


TIE_SAMPLES = ([2, 9, 17, 24, 33, 41, 50, 58], [1, 8, 15, 22, 36, 44, 51, 59])  # positions inside A, inside B
#: (hypothesis of the all-A sample, of the all-B sample) among 512: different workgroups of mono_hyp in both orders, the
#: two sides of a workgroup boundary, a late one against an early one
TIE_PLACES = [(3, 130), (130, 3), (127, 128), (400, 5)]


def _tie_scene(ob, oracle):
    """mono_two_motion_scene(60, 60) with the tie asserted on the oracle -> (pm, sample in A, sample in B, filler sample,
    the two inlier sets)."""
    pm, is_a = es.mono_two_motion_scene(ob.P_MATCH_DTYPE, 60, 60, 20)
    A, B = np.flatnonzero(is_a), np.flatnonzero(~is_a)
    sa, sb = A[TIE_SAMPLES[0]].astype(np.int32), B[TIE_SAMPLES[1]].astype(np.int32)
    mixed = np.concatenate([A[[0, 5, 12, 30]], B[[0, 6, 13, 31]]]).astype(np.int32)
    e1 = _mono(ob, dict(es.MONO_KITTI, ransac_iters=1))
    _, _, inl_a = oracle.estimate_motion_mono(e1, pm, sa[None])
    _, _, inl_b = oracle.estimate_motion_mono(e1, pm, sb[None])
    _, _, inl_m = oracle.estimate_motion_mono(e1, pm, mixed[None])
    assert len(inl_a) == len(inl_b) >= 60, ("not a tie", len(inl_a), len(inl_b))
    assert not np.array_equal(inl_a, inl_b) and set(A) <= set(inl_a) and set(B) <= set(inl_b)
    assert len(inl_m) < len(inl_a), "the mixed filler sample must lose against both"
    return pm, sa, sb, mixed, inl_a, inl_b


def _tie_rows(pm, sa, sb, mixed, ka, kb, seed, iters=512):
    rng = np.random.default_rng(seed)
    want = np.tile(mixed, (iters, 1))
    want[ka] = sa
    want[kb] = sb
    return np.stack([es.invert_draw(len(pm), row, rng) for row in want]), want


def test_mono_tie_rows_draw_the_intended_samples_and_the_earlier_pose_wins(ob, oracle):
    pm, sa, sb, mixed, inl_a, inl_b = _tie_scene(ob, oracle)
    for q, (ka, kb) in enumerate(TIE_PLACES):
        raw, want = _tie_rows(pm, sa, sb, mixed, ka, kb, q)
        assert np.array_equal(oracle.draw_samples_n(len(pm), 8, 512, raw.reshape(-1)), want)
        _, _, inl = oracle.estimate_motion_mono(_mono(ob, dict(es.MONO_KITTI, ransac_iters=512)), pm, want)
        assert np.array_equal(inl, inl_a if ka < kb else inl_b), (ka, kb)


# ------------------------------------------------------------------------------------------------------------ GPU

@pytest.mark.gpu
def test_gpu_mono_shortest_lists(pkg, ob, oracle, gpu):
    """n = 9, 10, 11, 12 in one batch: 9 is empty as in the reference, 10 runs (the draw's `% (N - k)` at its smallest)."""
    lists = [_CASES[f"n{n}"][0] for n in (9, 10, 11, 12)]
    want = _compare(pkg, ob, oracle, _CASES["n9"][1], lists, _glibc(ob, 256, 4), "short")
    assert not want[0][0] and len(want[0][2]) == 0 and len(want[1][2]) >= 8 and want[2][0] and want[3][0]
    raw = np.random.default_rng(21).integers(0, 2 ** 31 - 1, (4, 256, 8)).astype(np.int32)
    _compare(pkg, ob, oracle, _CASES["n9"][1], lists, raw, "short, raw")


@pytest.mark.gpu
def test_gpu_mono_lds_global_switch(pkg, ob, oracle, gpu):
    """Noise-free, outlier-free scenes of 639, 640 and 641 matches, every match an inlier (asserted): the refit system of
    the first two lives in LDS, the third takes the global-memory path.  In the same batch, lists whose lengths -- and,
    every match being an inlier, whose inlier lists -- end at the 64-lane waves and the 256-thread trips of the ordered
    compaction."""
    lengths = (63, 64, 65, 255, 256, 257, 513, 639, 640, 641)
    lists = [es.mono_two_motion_scene(ob.P_MATCH_DTYPE, n, 0, 90)[0] for n in lengths]
    want = _compare(pkg, ob, oracle, dict(es.MONO_KITTI, ransac_iters=128), lists, _glibc(ob, 128, len(lengths)), "lds switch")
    assert [len(w[2]) for w in want] == list(lengths) and all(w[0] for w in want)


@pytest.mark.gpu
def test_gpu_mono_rows_per_lane_boundary(pkg, ob, oracle, gpu):
    """2047, 2048 and 2049 matches with 30 % outliers at 128 hypotheses: eight rows per lane of the cooperative SVD and
    one more; the inlier sets (above 640: asserted) take the global-memory refit."""
    lists = [es.mono_scene(ob.P_MATCH_DTYPE, n, 95, outliers=0.3, noise=0.2)[0] for n in (2047, 2048, 2049)]
    raw = np.random.default_rng(22).integers(0, 2 ** 31 - 1, (3, 128, 8)).astype(np.int32)
    want = _compare(pkg, ob, oracle, dict(es.MONO_KITTI, ransac_iters=128), lists, raw, "rows per lane")
    assert all(w[0] and len(w[2]) > 640 for w in want), [len(w[2]) for w in want]


@pytest.mark.gpu
@pytest.mark.parametrize("stream", ["raw", "glibc"])
def test_gpu_mono_iteration_counts(stream, pkg, ob, oracle, gpu):
    """One list of 300 at hypothesis counts around mono_hyp's 128-wide workgroups, each a prefix of one rand() stream."""
    pm = _CASES["iters1"][0]
    full = _glibc(ob, 500, 1) if stream == "glibc" else np.random.default_rng(23).integers(0, 2 ** 31 - 1, (1, 500, 8)).astype(np.int32)
    counts = {}
    for iters in (1, 127, 128, 129, 256, 500):
        want = _compare(pkg, ob, oracle, dict(es.MONO_KITTI, ransac_iters=iters), [pm], np.ascontiguousarray(full[:, :iters]), iters)
        counts[iters] = len(want[0][2])
    assert counts[1] <= counts[127] <= counts[128] <= counts[129] <= counts[256] <= counts[500] and counts[1] < counts[500]


@pytest.mark.gpu
def test_gpu_mono_ties_across_hypothesis_workgroups(pkg, ob, oracle, gpu):
    """Equal inlier counts from two different poses, placed in different workgroups of mono_hyp (their atomicMax on
    the list's key meets in any order): the earlier hypothesis wins.  Four placements as four lists of one launch."""
    pm, sa, sb, mixed, inl_a, inl_b = _tie_scene(ob, oracle)
    rows = [_tie_rows(pm, sa, sb, mixed, ka, kb, q) for q, (ka, kb) in enumerate(TIE_PLACES)]
    raw = np.stack([r[0] for r in rows])
    for s, (_, want) in enumerate(rows):
        assert np.array_equal(oracle.draw_samples_n(len(pm), 8, 512, raw[s].reshape(-1)), want)
    res = _compare(pkg, ob, oracle, dict(es.MONO_KITTI, ransac_iters=512), [pm] * 4, raw, "ties")
    for (ka, kb), r in zip(TIE_PLACES, res):
        assert np.array_equal(r[2], inl_a if ka < kb else inl_b), (ka, kb)


@pytest.mark.gpu
def test_gpu_mono_degenerate_and_rejection_paths(pkg, ob, oracle, gpu):
    """Identical matches (degenerate scale), hardly any motion (motion_threshold rejects: ok false with >= 10 inliers),
    near-pure rotation, winners with fewer than 10 inliers (MONO_FEW_INLIER_SEEDS), beside a healthy list."""
    healthy = _CASES["iters1"][0]
    few = [_CASES[f"few_inliers_{n}"][0] for n, _ in es.MONO_FEW_INLIER_SEEDS]
    lists = [healthy, _CASES["identical30"][0], _CASES["no_motion"][0], _CASES["pure_rotation"][0]] + few + [healthy]
    want = _compare(pkg, ob, oracle, dict(es.MONO_KITTI, ransac_iters=300), lists, _glibc(ob, 300, len(lists)), "rejections")
    assert want[0][0] and want[-1][0]
    assert not want[1][0] and len(want[1][2]) == 0
    assert not want[2][0] and len(want[2][2]) >= 10
    assert not want[3][0] and len(want[3][2]) >= 10
    assert all(not w[0] and 0 < len(w[2]) < 10 for w in want[4:-1]), [len(w[2]) for w in want]
    raw = np.random.default_rng(24).integers(0, 2 ** 31 - 1, (len(lists), 300, 8)).astype(np.int32)
    _compare(pkg, ob, oracle, dict(es.MONO_KITTI, ransac_iters=300), lists, raw, "rejections, raw")


@pytest.mark.gpu
def test_gpu_mono_sampson_distance_equal_to_the_threshold(pkg, ob, oracle, gpu):
    """The Sampson test is a strict `<`, and a distance equal to the threshold is where mono_hyp's division-free
    shortcut must hand the decision to the division.  inlier_threshold is set to the very double that is match 172's
    distance under one hypothesis (premise on the oracle: out at that value, in at the next double, nothing else
    changes); the hypothesis is placed alone, and at 0, 127, 128 and 300 of 301 among mixed fillers that count fewer."""
    pm, sample, at, above = _sampson_equal(ob, oracle)
    raw1 = es.invert_draw(len(pm), sample, np.random.default_rng(26))[None, None]
    assert np.array_equal(oracle.draw_samples_n(len(pm), 8, 1, raw1.reshape(-1))[0], sample)
    for name, inl in (("sampson_equal", at), ("sampson_next", above)):
        want = _compare(pkg, ob, oracle, _CASES[name][1], [pm], raw1, name)
        assert np.array_equal(want[0][2], inl)
    filler = np.arange(8, dtype=np.int32) * 7 + 2  # a sample that counts fewer inliers than the placed one (asserted)
    kw1 = dict(_CASES["sampson_equal"][1])
    _, _, inl_f = oracle.estimate_motion_mono(_mono(ob, kw1), pm, filler[None])
    assert len(inl_f) < len(at)
    rng = np.random.default_rng(27)
    rows = []
    for k in (0, 127, 128, 300):
        want_s = np.tile(filler, (301, 1)); want_s[k] = sample
        rows.append(np.stack([es.invert_draw(len(pm), r, rng) for r in want_s]))
    res = _compare(pkg, ob, oracle, dict(kw1, ransac_iters=301), [pm] * 4, np.stack(rows), "placed")
    assert all(np.array_equal(r[2], at) for r in res)


@pytest.mark.gpu
def test_gpu_mono_parameters(pkg, ob, oracle, gpu):
    """height 1.0 / 1.65, pitch 0 / -0.08, inlier_threshold 1e-6 / 1e-5 / 1e-4, a second intrinsics set and the untouched
    vh_default_mono_params."""
    import ctypes as C
    base, h1 = _CASES["iters1"][0], _CASES["height1"][0]
    raw = np.random.default_rng(25).integers(0, 2 ** 31 - 1, (2, 500, 8)).astype(np.int32)
    n_inl = []
    for height in (1.0, 1.65):
        for pitch in (0.0, -0.08):
            _compare(pkg, ob, oracle, dict(es.MONO_KITTI, ransac_iters=500, height=height, pitch=pitch), [base, h1], raw, (height, pitch))
    for thr in (1e-6, 1e-5, 1e-4):
        want = _compare(pkg, ob, oracle, dict(es.MONO_KITTI, ransac_iters=500, inlier_threshold=thr), [base, h1], raw, thr)
        n_inl.append(sum(len(w[2]) for w in want))
    assert n_inl[0] < n_inl[1] < n_inl[2]
    want = _compare(pkg, ob, oracle, _CASES["second_intrinsics"][1], [_CASES["second_intrinsics"][0]], raw[:1], "second intrinsics")
    assert want[0][0]
    gm = pkg.MonoParams()
    pkg._lib().vh_default_mono_params(C.byref(gm))
    assert bytes(gm) == bytes(pkg.MonoParams.default()) == bytes(ob.MonoParams.default())
    want = _compare(pkg, ob, oracle, None, [_CASES["defaults"][0]], _glibc(ob, 2000, 1), "defaults")
    assert want[0][0]


@pytest.mark.gpu
def test_gpu_mono_edges_signed_form(gpu):
    """Every GPU case of this file again with VH_MONO_SIGNED=1 (all hypotheses through the signed kernel; read once per
    process, hence one child process)."""
    import subprocess, sys
    env = dict(os.environ, VH_MONO_SIGNED="1")
    cmd = [sys.executable, "-m", "pytest", os.path.abspath(__file__), "-q", "-x", "-m", "gpu", "-k", "not signed_form", "-p", "no:cacheprovider"]
    try:
        r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=300)
    except subprocess.TimeoutExpired:
        pytest.exit("the signed-form child did not finish: nothing more is started on this GPU", returncode=3)
    if r.returncode < 0 or r.returncode in (134, 139):
        pytest.exit(f"the signed-form child died abnormally ({r.returncode}): nothing more is started on this GPU\n" + r.stdout[-2000:] + r.stderr[-2000:], returncode=3)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    assert " passed" in r.stdout and "skipped" not in r.stdout
