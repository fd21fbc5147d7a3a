"""Stereo egomotion (csrc/kernels_ego.hip) at the edges of its structure: list lengths and hypothesis counts around
the 256-wide passes and chunks, exact ties between different poses, every failure path, degenerate geometry, the
parameter space and wide batches.  CPU part: the oracle equals the reference (recorded answers and
tests/golden/egomotion_edges.npz, oracle/gen_golden_ego.py) on one scene of every new kind.  GPU part: the device
equals the oracle -- success flag and inlier list exact, tr to 1e-9 relative, all zero on failure.  Every tie,
boundary-count and failure test asserts its premise on the oracle before it looks at the device."""
import os

import numpy as np
import pytest

import egomotion_scene as es
from conftest import GOLDEN, entry

_D = entry.load_oracle().P_MATCH_DTYPE
_CASES = es.stereo_edge_cases(_D)


def _ego(mod, kw):
    return mod.EgoParams.default() if kw is None else mod.EgoParams.default(**kw)


def _close(tr, want):
    return np.allclose(tr, want, rtol=1e-9, atol=1e-12)


def _glibc(ob, iters, n_sets):
    r = ob.glibc_rand_after_srand0(3 * iters).reshape(iters, 3)
    return np.stack([r] * n_sets)


def _oracle(oracle, e, pm, raw):
    """The oracle on the samples the kernel draws from the same rand() values."""
    samples = oracle.draw_samples(len(pm), e.ransac_iters, np.ascontiguousarray(raw).reshape(-1)) if len(pm) >= 6 else np.zeros((e.ransac_iters, 3), np.int32)
    return oracle.estimate_motion_stereo(e, pm, samples)


def _compare(pkg, ob, oracle, kw, lists, raw, label=""):
    """One batched launch against the oracle, list by list -> the oracle's results."""
    e, ge = _ego(ob, kw), _ego(pkg, kw)
    tr, ok, inl = pkg.estimate_motion_stereo(ge, lists, raw)
    want = []
    for s, pm in enumerate(lists):
        ok_o, tr_o, inl_o = _oracle(oracle, e, pm, raw[s])
        assert ok[s] == ok_o, (label, s, len(pm), ok[s], ok_o, len(inl[s]), len(inl_o))
        assert np.array_equal(inl[s], inl_o), (label, s, len(pm), len(inl[s]), len(inl_o))
        assert _close(tr[s], tr_o), (label, s, tr[s], tr_o)
        if not ok_o:
            assert tr[s].tobytes() == bytes(48), (label, s, tr[s])
        want.append((ok_o, tr_o, inl_o))
    return want


# ---------------------------------------------------------------------------------------------- CPU: trust the oracle

@pytest.mark.parametrize("name", sorted(_CASES))
def test_oracle_equals_reference_at_edges(name, ob, oracle, reference):
    pm, kw = _CASES[name]
    e = _ego(ob, kw)
    ok_o, tr_o, inl_o = oracle.estimate_motion_stereo(e, pm, oracle.draw_samples(len(pm), e.ransac_iters))
    ok_r, tr_r, inl_r = reference.estimate_motion_stereo(e, pm)
    assert ok_o == ok_r and np.array_equal(inl_o, inl_r), name
    assert tr_o.tobytes() == tr_r.tobytes(), (tr_o, tr_r)


@pytest.mark.parametrize("name", sorted(_CASES))
def test_oracle_golden_edges(name, ob, oracle):
    """The same against vectors recorded from the reference (what pins the oracle where the reference build is absent),
    on the recorded match lists; the builders still produce those lists."""
    z = np.load(os.path.join(GOLDEN, "egomotion_edges.npz"))
    pm = np.ascontiguousarray(z[name + "__pm"]).view(ob.P_MATCH_DTYPE).reshape(-1)
    assert pm.tobytes() == _CASES[name][0].tobytes()
    e = _ego(ob, _CASES[name][1])
    ok_o, tr_o, inl_o = oracle.estimate_motion_stereo(e, pm, oracle.draw_samples(len(pm), e.ransac_iters))
    assert ok_o == bool(z[name + "__ok"]) and np.array_equal(inl_o, z[name + "__inliers"]) and tr_o.tobytes() == z[name + "__tr"].tobytes()


def test_scene_kinds_are_what_they_claim(ob, oracle):
    """The failure scenes fail the way their names say, on the oracle."""
    def run(name):
        pm, kw = _CASES[name]
        e = _ego(ob, kw)
        return oracle.estimate_motion_stereo(e, pm, oracle.draw_samples(len(pm), e.ransac_iters))
    ok, _, inl = run("identical30")
    assert not ok and len(inl) == 0
    seen = set()
    for n, seed in es.FEW_INLIER_SEEDS:
        ok, _, inl = run(f"few_inliers_{n}_{seed}")
        assert not ok and 0 < len(inl) < 6, (n, len(inl))
        seen.add(len(inl))
    for n, k, _ in es.FEW_INLIER_PLANTED:
        ok, _, inl = run(f"few_planted_{n}_{k}")
        assert not ok and len(inl) == k, (n, k, len(inl))
        seen.add(len(inl))
    assert seen == {1, 2, 3, 4, 5}
    for n, _ in es.REFIT_FAIL_SEEDS:
        ok, _, inl = run(f"refit_fail_{n}")
        assert not ok and len(inl) >= 6, (n, len(inl))
    for name in ("full512", "full513"):
        ok, _, inl = run(name)
        assert ok and len(inl) == len(_CASES[name][0])


def _tie_scene(ob, oracle, seed=21, kw=None):
    """two_motion_scene(40, 40) with the tie asserted on the oracle: a sample inside A and one inside B each count 40
    inliers, and not the same 40 -> (pm, A indices, B indices)."""
    pm, is_a = es.two_motion_scene(ob.P_MATCH_DTYPE, 40, 40, seed)
    A, B = np.flatnonzero(is_a), np.flatnonzero(~is_a)
    e1 = _ego(ob, dict(kw or es.KITTI, ransac_iters=1))
    ok_a, _, inl_a = oracle.estimate_motion_stereo(e1, pm, np.array([A[[3, 10, 25]]], np.int32))
    ok_b, _, inl_b = oracle.estimate_motion_stereo(e1, pm, np.array([B[[4, 11, 30]]], np.int32))
    assert ok_a and ok_b
    assert len(inl_a) == len(inl_b) == 40, ("not a tie", len(inl_a), len(inl_b))
    assert not np.array_equal(inl_a, inl_b) and np.array_equal(inl_a, A) and np.array_equal(inl_b, B)
    ok_m, _, inl_m = oracle.estimate_motion_stereo(e1, pm, np.array([[A[0], A[1], B[0]]], np.int32))
    assert len(inl_m) < 40, "the mixed filler sample must lose against both"
    return pm, A, B


#: (hypotheses, place of the first all-A sample, of the first all-B sample, winner)
TIES = [(64, 5, 20, "A"), (64, 20, 5, "B"), (320, 300, 3, "B"), (300, 255, 256, "A"), (640, 10, 600, "A")]


def _tie_rows(pm, A, B, iters, ka, kb, seed):
    rng = np.random.default_rng(seed)
    n = len(pm)
    want = np.tile(np.array([A[0], A[1], B[0]], np.int32), (iters, 1))  # a mixed sample everywhere else
    want[ka] = A[[3, 10, 25]]
    want[kb] = B[[4, 11, 30]]
    raw = np.stack([es.invert_draw(n, row, rng) for row in want])
    return raw, want


def test_tie_rows_draw_the_intended_samples_and_the_earlier_pose_wins(ob, oracle):
    pm, A, B = _tie_scene(ob, oracle)
    for q, (iters, ka, kb, winner) in enumerate(TIES):
        raw, want = _tie_rows(pm, A, B, iters, ka, kb, q)
        assert np.array_equal(oracle.draw_samples(len(pm), iters, raw.reshape(-1)), want)
        ok, _, inl = oracle.estimate_motion_stereo(_ego(ob, dict(es.KITTI, ransac_iters=iters)), pm, want)
        assert ok and np.array_equal(inl, A if winner == "A" else B), (iters, ka, kb)


def test_invert_draw_any_order(ob, oracle):
    rng = np.random.default_rng(3)
    for n in (6, 7, 8, 80):
        want = np.stack([rng.choice(n, 3, replace=False) for _ in range(50)]).astype(np.int32)
        raw = np.stack([es.invert_draw(n, row, rng) for row in want])
        assert np.array_equal(oracle.draw_samples(n, 50, raw.reshape(-1)), want)
        want8 = np.stack([rng.choice(n + 4, 8, replace=False) for _ in range(20)]).astype(np.int32)
        raw8 = np.stack([es.invert_draw(n + 4, row, rng) for row in want8])
        assert np.array_equal(oracle.draw_samples_n(n + 4, 8, 20, raw8.reshape(-1)), want8)


# ------------------------------------------------------------------------------------------------------------ GPU

LENGTHS = [0, 5, 6, 7, 8, 255, 256, 257, 511, 512, 513, 768, 769, 63, 64, 65]  # (appended: the lists before keep their rand() rows)


@pytest.mark.gpu
def test_gpu_list_lengths_around_the_chunks(pkg, ob, oracle, gpu):
    """One batch of lists of 0 .. 769 matches (lengths around the 64-lane waves and the 256-thread trips of the ordered
    compaction), 30 % outliers (inlier lists that cross the 256-chunks at assorted offsets), at 64 hypotheses; a second
    one at inlier_threshold 10 with a noise-free, outlier-free list of exactly
    512 and one of 513 whose every match is an inlier (every chunk full; asserted on the oracle)."""
    lists = [es.scene(ob.P_MATCH_DTYPE, n, 400 + n, outliers=0.0 if n < 9 else 0.3, noise=0.0 if n < 9 else 0.2)[0] for n in LENGTHS]
    raw = np.random.default_rng(11).integers(0, 2 ** 31 - 1, (len(lists), 64, 3)).astype(np.int32)
    want = _compare(pkg, ob, oracle, dict(es.KITTI, ransac_iters=64), lists, raw, "lengths")
    assert [w[0] for w in want[:2]] == [False, False] and all(w[0] for w in want[2:])
    assert {len(w[2]) // 256 for w in want[5:]} >= {0, 1, 2}  # inlier lists end in the first, second and third chunk
    full = [_CASES["full512"][0], _CASES["n7"][0], _CASES["full513"][0]]
    want = _compare(pkg, ob, oracle, _CASES["full512"][1], full, raw[:3], "full chunks")
    assert [len(w[2]) for w in want] == [512, 7, 513]


@pytest.mark.gpu
@pytest.mark.parametrize("stream", ["raw", "glibc"])
def test_gpu_iteration_counts_around_the_passes(stream, pkg, ob, oracle, gpu):
    """One list of 200 matches at hypothesis counts around the 256-wide passes, each a prefix of one rand() stream: more
    hypotheses never find fewer inliers, and the later ones do win (asserted on the oracle's counts)."""
    pm = es.scene(ob.P_MATCH_DTYPE, 200, 63, outliers=0.3, noise=0.2)[0]
    counts = {}
    full = _glibc(ob, 513, 1) if stream == "glibc" else np.random.default_rng(12).integers(0, 2 ** 31 - 1, (1, 513, 3)).astype(np.int32)
    for iters in (1, 2, 63, 64, 65, 255, 256, 257, 512, 513):
        raw = np.ascontiguousarray(full[:, :iters])
        counts[iters] = len(_compare(pkg, ob, oracle, dict(es.KITTI, ransac_iters=iters), [pm], raw, iters)[0][2])
    assert counts[1] <= counts[64] <= counts[256] <= counts[513]
    assert counts[1] < counts[513]  # later hypotheses do win


@pytest.mark.gpu
def test_gpu_ties_between_two_poses(pkg, ob, oracle, gpu):
    """Equal inlier counts, different samples, different poses: the earlier hypothesis wins -- inside a pass, across
    the pass boundary (255 | 256), and from pass 0 against passes 1 and 2."""
    pm, A, B = _tie_scene(ob, oracle)
    for q, (iters, ka, kb, winner) in enumerate(TIES):
        raw, want = _tie_rows(pm, A, B, iters, ka, kb, q)
        assert np.array_equal(oracle.draw_samples(len(pm), iters, raw.reshape(-1)), want)
        res = _compare(pkg, ob, oracle, dict(es.KITTI, ransac_iters=iters), [pm], raw[None], (iters, ka, kb))
        assert res[0][0] and np.array_equal(res[0][2], A if winner == "A" else B)


@pytest.mark.gpu
def test_gpu_failure_paths(pkg, ob, oracle, gpu):
    """Every way estimateMotion fails with >= 6 matches: all solves singular (identical matches: ok = 0, no inliers); a
    winner with 1, 2, 3, 4 and 5 inliers (8..12 unrelated matches at inlier_threshold 0.3: FEW_INLIER_SEEDS give 1 and 2,
    FEW_INLIER_PLANTED with 3..5 matches of one motion among them the rest); a refit on >= 6
    inliers that does not converge (REFIT_FAIL_SEEDS: matches without disparity at inlier_threshold 40, found in a 3 s
    search).  Premises asserted on the oracle."""
    healthy = es.scene(ob.P_MATCH_DTYPE, 100, 64, outliers=0.2, noise=0.2)[0]
    want = _compare(pkg, ob, oracle, dict(es.KITTI), [healthy, _CASES["identical30"][0], healthy], _glibc(ob, 200, 3), "identical")
    assert want[0][0] and want[2][0] and not want[1][0] and len(want[1][2]) == 0
    few = [_CASES[f"few_inliers_{n}_{seed}"][0] for n, seed in es.FEW_INLIER_SEEDS] + [_CASES[f"few_planted_{n}_{k}"][0] for n, k, _ in es.FEW_INLIER_PLANTED]
    want = _compare(pkg, ob, oracle, _CASES["few_inliers_8_9"][1], few + [healthy], _glibc(ob, 200, len(few) + 1), "few inliers")
    assert all(not w[0] and 0 < len(w[2]) < 6 for w in want[:-1]), [len(w[2]) for w in want]
    assert {len(w[2]) for w in want[:-1]} == {1, 2, 3, 4, 5}  # every count the failure reports below 6
    bad = [_CASES[f"refit_fail_{n}"][0] for n, _ in es.REFIT_FAIL_SEEDS]
    want = _compare(pkg, ob, oracle, _CASES["refit_fail_20"][1], bad + [healthy], _glibc(ob, 200, len(bad) + 1), "refit")
    assert all(not w[0] and len(w[2]) >= 6 for w in want[:-1]), [len(w[2]) for w in want]
    assert want[-1][0]


@pytest.mark.gpu
def test_gpu_hypotheses_that_take_all_22_updates(pkg, ob, oracle, gpu):
    """Lists (SLOW_HYPOTHESIS_SEEDS: matches without disparity, inlier_threshold 40) on which hypotheses are still
    updating at the cap of 22 Gauss-Newton updates and the last update decides the inlier set: an estimator that stops
    after 21 reports other inliers (that is how the lists were chosen; the reference agrees with the oracle on them)."""
    lists = [_CASES[f"slow_hypothesis_{n}_{seed}"][0] for n, seed in es.SLOW_HYPOTHESIS_SEEDS]
    want = _compare(pkg, ob, oracle, dict(es.KITTI, inlier_threshold=40.0), lists, _glibc(ob, 200, len(lists)), "22 updates")
    assert all(len(w[2]) >= 6 for w in want)


@pytest.mark.gpu
def test_gpu_degenerate_geometry_beside_healthy_lists(pkg, ob, oracle, gpu):
    """Zero and negative disparity (a fifth of a list, and a whole list), points that a sampled motion carries behind the
    camera, coordinates of 1e30, identical matches: each as one list of a batch whose other lists are healthy.  Every
    list equals the oracle -- the degenerate ones, and the healthy ones beside them."""
    D = ob.P_MATCH_DTYPE
    healthy = [es.scene(D, n, 500 + n, outliers=0.3, noise=0.2)[0] for n in (150, 300, 90)]
    base = _CASES["bad_disparity"][0]
    behind, hit = es.behind_camera(es.scene(D, 300, 31, outliers=0.3, noise=0.2)[0], 12, 35)
    assert behind.tobytes() == _CASES["behind_camera"][0].tobytes()
    z = es.depths_under_sample(behind, hit[:3])
    assert (z <= 0).sum() > 100 and np.all(z[hit] > 0)  # the sample's own motion puts most other points behind the camera
    lists = [healthy[0], base, _CASES["all_bad_disparity"][0], healthy[1], behind, _CASES["huge"][0], _CASES["identical30"][0], healthy[2]]
    rng = np.random.default_rng(13)
    raw = rng.integers(0, 2 ** 31 - 1, (len(lists), 300, 3)).astype(np.int32)
    for k in range(0, 300, 7):  # hypotheses that sample inside the turning points
        raw[4, k] = es.invert_draw(300, hit[rng.choice(12, 3, replace=False)], rng)
    want = _compare(pkg, ob, oracle, dict(es.KITTI, ransac_iters=300), lists, raw, "degenerate")
    assert [w[0] for w in want] == [True, True, False, True, True, True, False, True]
    alone = _compare(pkg, ob, oracle, dict(es.KITTI, ransac_iters=300), healthy, raw[[0, 3, 7]], "healthy alone")
    for a, b in zip(alone, (want[0], want[3], want[7])):
        assert a[1].tobytes() == b[1].tobytes() and np.array_equal(a[2], b[2])


@pytest.mark.gpu
def test_gpu_residuals_of_exactly_zero_are_not_inliers_at_threshold_zero(pkg, ob, oracle, gpu):
    """The inlier test is a strict `<`.  exact_static_scene makes every residual exactly 0.0: at inlier_threshold 1e-9
    every match is an inlier, at 0.0 none is (both asserted on the oracle) -- a `<=` would accept them all."""
    pm = _CASES["exact_thr0"][0]
    raw = np.random.default_rng(17).integers(0, 2 ** 31 - 1, (1, 64, 3)).astype(np.int32)
    want = _compare(pkg, ob, oracle, _CASES["exact_thr1e-9"][1], [pm], raw, "1e-9")
    assert want[0][0] and len(want[0][2]) == len(pm)
    want = _compare(pkg, ob, oracle, _CASES["exact_thr0"][1], [pm], raw, "0")
    assert not want[0][0] and len(want[0][2]) == 0


@pytest.mark.gpu
@pytest.mark.parametrize("reweighting", [0, 1])
def test_gpu_reweighting_and_thresholds(reweighting, pkg, ob, oracle, gpu):
    lists = [es.scene(ob.P_MATCH_DTYPE, 60 + 37 * s, 600 + s, outliers=0.1 * (s % 5), noise=0.1 * (s % 4))[0] for s in range(8)]
    raw = np.random.default_rng(14).integers(0, 2 ** 31 - 1, (8, 100, 3)).astype(np.int32)
    n_inl = []
    for thr in (0.5, 2.0, 10.0):
        want = _compare(pkg, ob, oracle, dict(es.KITTI, ransac_iters=100, reweighting=reweighting, inlier_threshold=thr), lists, raw, thr)
        n_inl.append(sum(len(w[2]) for w in want))
    assert n_inl[0] < n_inl[1] < n_inl[2]


@pytest.mark.gpu
def test_gpu_second_intrinsics_and_defaults(pkg, ob, oracle, gpu):
    """f = 400, cu = 240, cv = 100, base = 0.12, with a match at exactly u1c == cu (the largest weight); and the untouched
    vh_default_ego_params (cu = 0: every weight is 1 / inf = 0, every system singular -- and 0 / 0 for the match at
    u1c == 0, where the reference itself is undefined: egomotion_scene.defaults_zero_match)."""
    import ctypes as C
    sec, at_cu = _CASES["second_intrinsics"][0], _CASES["at_cu_second"][0]
    assert at_cu["u1c"][17] == 240.0 and sec["u1c"][17] != 240.0
    want = _compare(pkg, ob, oracle, dict(es.SECOND), [sec, at_cu], _glibc(ob, 200, 2), "second intrinsics")
    assert want[0][0] and want[1][0] and want[0][1].tobytes() != want[1][1].tobytes()
    ge = pkg.EgoParams()
    pkg._lib().vh_default_ego_params(C.byref(ge))
    assert bytes(ge) == bytes(pkg.EgoParams.default()) == bytes(ob.EgoParams.default()) and ge.cu == 0.0
    zero = es.defaults_zero_match(ob.P_MATCH_DTYPE)
    assert zero["u1c"][5] == 0.0
    want = _compare(pkg, ob, oracle, None, [_CASES["defaults_cu0"][0], zero], _glibc(ob, 200, 2), "defaults")
    assert not want[0][0] and not want[1][0]


@pytest.mark.gpu
def test_gpu_batch_width(pkg, ob, oracle, gpu):
    """300 lists of 40 matches in one launch (with two empty lists inside), and a launch of a single list."""
    D = ob.P_MATCH_DTYPE
    lists = [es.scene(D, 40, 1000 + s, outliers=0.05 * (s % 7), noise=0.1 * (s % 3))[0] for s in range(300)]
    lists[17] = lists[17][:0]; lists[299] = lists[299][:0]
    raw = np.random.default_rng(15).integers(0, 2 ** 31 - 1, (300, 64, 3)).astype(np.int32)
    want = _compare(pkg, ob, oracle, dict(es.KITTI, ransac_iters=64), lists, raw, "wide")
    assert sum(w[0] for w in want) > 250 and not want[17][0] and not want[299][0]
    one = _compare(pkg, ob, oracle, dict(es.KITTI, ransac_iters=64), [lists[5]], raw[5:6], "single")
    assert one[0][1].tobytes() == want[5][1].tobytes()


@pytest.mark.gpu
def test_gpu_group_with_empty_and_tiny_streams(pkg, ob, oracle, gpu):
    """vh_group_estimate_motion (device-side counts, fixed stride) on a 4-stream group at 480 x 200: a stream of blank
    images (0 matches), one that is blank but for a 14 x 14 textured patch at (200, 80) (2 quad matches), two healthy
    ones.  Per stream equal to the oracle."""
    S, W, H = 4, 480, 200
    dims = [W, H, pkg.synth.bytes_per_line(W)]
    seqs = [pkg.synth.stereo_sequence(W, H, 2, disparity=6 + s, blur=4, seed=230 + s) for s in range(S)]
    for t in range(2):
        for c in range(2):
            blank = np.zeros_like(seqs[0][t][c]); blank[:, :W] = 128
            patch = blank.copy(); patch[80:94, 200:214] = seqs[1][t][c][80:94, 200:214]
            seqs[0][t] = tuple(blank if q == c else seqs[0][t][q] for q in range(2))
            seqs[1][t] = tuple(patch if q == c else seqs[1][t][q] for q in range(2))
    g = pkg.StreamGroup(S, pkg.Params.default())
    for t in range(2):
        g.pushBack(np.stack([seqs[s][t][0] for s in range(S)]), np.stack([seqs[s][t][1] for s in range(S)]), dims, False)
    g.matchFeatures(pkg.METHOD_QUAD)
    kw = dict(f=400.0, cu=W / 2, cv=H / 2, base=0.5)
    raw = np.random.default_rng(16).integers(0, 2 ** 31 - 1, (S, 200, 3)).astype(np.int32)
    tr, ok, ninl = g.estimateMotion(_ego(pkg, kw), raw)
    n = [len(g.getMatches(s)) for s in range(S)]
    assert n[0] == 0 and 0 < n[1] < 6 and n[2] > 100 and n[3] > 100, n
    for s in range(S):
        ok_o, tr_o, inl_o = _oracle(oracle, _ego(ob, kw), g.getMatches(s), raw[s])
        assert ok[s] == ok_o and ninl[s] == len(inl_o) and _close(tr[s], tr_o), (s, tr[s], tr_o)
        if not ok_o:
            assert tr[s].tobytes() == bytes(48)
    assert not ok[0] and not ok[1] and ok[2] and ok[3]
    g.close()
