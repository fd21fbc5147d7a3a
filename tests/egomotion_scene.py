"""Synthetic stereo-odometry scenes for the egomotion tests: 3-d points seen by a rectified
stereo rig before and after a rigid motion, projected to integer pixel positions (features sit
on pixels), with a share of gross outliers -- as p_match records (Matcher::p_match).

Builders for the estimators' edge tests (tests/test_egomotion_edges.py, tests/test_mono_edges.py), all pure
numpy and deterministic by seed:
  two_motion_scene / mono_two_motion_scene   two disjoint point sets A and B under two clearly different rigid
      motions, unrounded (noise-free to float precision) and interleaved in index order; -> (p_match, is_a mask).
      A hypothesis sampled inside A counts n_a inliers, one inside B n_b: with n_a == n_b an exact tie of two poses.
  invert_draw        the rand() values that make VisualOdometry::getRandomSample return chosen indices.
  all_identical      every match a copy of the first (singular systems, degenerate scale).
  bad_disparity      zero and negative disparity on a share of the matches.
  match_at_cu        one match at exactly u1c == cu (the reweighting's smallest denominator; 0/0 when cu == 0).
  behind_camera      previous-frame points so close that a hypothesis fitted to them carries others to Z <= 0.
  huge_coordinates   coordinates of magnitude 1e30f on a few matches.
  exact_static_scene a standing camera whose every reprojection residual is exactly 0.0 in double precision."""
import numpy as np


def rot(rx, ry, rz):
    sx, cx, sy, cy, sz, cz = np.sin(rx), np.cos(rx), np.sin(ry), np.cos(ry), np.sin(rz), np.cos(rz)
    return np.array([[+cy * cz, -cy * sz, +sy],
                     [+sx * sy * cz + cx * sz, -sx * sy * sz + cx * cz, -sx * cy],
                     [-cx * sy * cz + sx * sz, +cx * sy * sz + sx * cz, +cx * cy]])


def scene(dtype, n, seed, tr=(0.004, -0.012, 0.002, 0.03, -0.01, -0.85), outliers=0.25, f=645.24, cu=635.96, cv=194.13,
          base=0.5707, W=1241, H=376, noise=0.0):
    """-> (p_match[n], true tr).  tr maps previous-frame coordinates to current-frame coordinates
    (p_t = R p_{t-1} + t, src/viso.h:80-86)."""
    rng = np.random.default_rng(seed)
    out = np.zeros(n, dtype)
    R, t = rot(*tr[:3]), np.array(tr[3:])
    k = 0
    while k < n:
        Z = rng.uniform(4, 60); X = rng.uniform(-1, 1) * Z * 0.9; Y = rng.uniform(-0.3, 0.25) * Z
        P = np.array([X, Y, Z]); Q = R @ P + t
        if Q[2] < 2:
            continue
        u1p, v1p, u2p = f * P[0] / P[2] + cu, f * P[1] / P[2] + cv, f * (P[0] - base) / P[2] + cu
        u1c, v1c, u2c = f * Q[0] / Q[2] + cu, f * Q[1] / Q[2] + cv, f * (Q[0] - base) / Q[2] + cu
        vals = np.array([u1p, v1p, u2p, v1p, u1c, v1c, u2c, v1c]) + (rng.normal(0, noise, 8) if noise else 0)
        vals = np.round(vals)
        if rng.random() < outliers:
            vals[4:] += rng.integers(-40, 41, 4)
        if not (np.all(vals[[0, 2, 4, 6]] >= 0) and np.all(vals[[0, 2, 4, 6]] < W) and np.all(vals[[1, 3, 5, 7]] >= 0) and np.all(vals[[1, 3, 5, 7]] < H)):
            continue
        if vals[0] < vals[2] or vals[4] < vals[6]:
            continue
        r = out[k]
        r["u1p"], r["v1p"], r["u2p"], r["v2p"], r["u1c"], r["v1c"], r["u2c"], r["v2c"] = vals
        r["i1p"] = r["i2p"] = r["i1c"] = r["i2c"] = k
        k += 1
    return out, np.array(tr)


def mono_scene(dtype, n, seed, tr=(0.002, -0.01, 0.001, 0.02, -0.005, -0.9), outliers=0.2, ground=0.45, height=1.65, f=645.24, cu=635.96,
               cv=194.13, W=1241, H=376, noise=0.0):
    """Flow matches of ONE camera (right-camera fields = -1, as Matcher::matching method 0 emits them):
    a share `ground` of the points lies on the road plane Y = height below the camera (the mono
    estimator scales its translation by that plane), the rest is structure above it."""
    rng = np.random.default_rng(seed)
    out = np.zeros(n, dtype)
    for name in out.dtype.names:
        out[name] = -1
    R, t = rot(*tr[:3]), np.array(tr[3:])
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
        vals = np.round(vals + (rng.normal(0, noise, 4) if noise else 0))
        if rng.random() < outliers:
            vals[2:] += rng.integers(-40, 41, 2)
        if not (0 <= vals[0] < W and 0 <= vals[2] < W and 0 <= vals[1] < H and 0 <= vals[3] < H):
            continue
        r = out[k]
        r["u1p"], r["v1p"], r["u1c"], r["v1c"] = vals
        r["i1p"] = r["i1c"] = k
        k += 1
    return out, np.array(tr)


def _two_motions(n_a, n_b):
    """index -> True for set A: the two sets alternate as long as both last."""
    is_a = np.zeros(n_a + n_b, bool)
    ia = ib = 0
    for i in range(n_a + n_b):
        take_a = ib >= n_b or (ia < n_a and ia * n_b <= ib * n_a)
        is_a[i] = take_a
        ia += take_a; ib += not take_a
    return is_a


TR_A = (0.004, -0.012, 0.002, 0.03, -0.01, -0.85)
TR_B = (-0.01, 0.06, -0.02, 0.7, 0.05, 0.4)


def two_motion_scene(dtype, n_a, n_b, seed, tr_a=TR_A, tr_b=TR_B, f=645.24, cu=635.96, cv=194.13, base=0.5707, W=1241, H=376):
    """-> (p_match[n_a + n_b], is_a[n_a + n_b]).  Stereo quad matches, not rounded to pixels."""
    rng = np.random.default_rng(seed)
    is_a = _two_motions(n_a, n_b)
    out = np.zeros(n_a + n_b, dtype)
    k = 0
    while k < len(out):
        tr = tr_a if is_a[k] else tr_b
        R, t = rot(*tr[:3]), np.array(tr[3:])
        Z = rng.uniform(5, 40); P = np.array([rng.uniform(-1, 1) * Z * 0.8, rng.uniform(-0.25, 0.2) * Z, Z]); Q = R @ P + t
        if Q[2] < 3:
            continue
        vals = np.array([f * P[0] / P[2] + cu, f * P[1] / P[2] + cv, f * (P[0] - base) / P[2] + cu, f * P[1] / P[2] + cv,
                         f * Q[0] / Q[2] + cu, f * Q[1] / Q[2] + cv, f * (Q[0] - base) / Q[2] + cu, f * Q[1] / Q[2] + cv])
        if not (np.all(vals[[0, 2, 4, 6]] >= 0) and np.all(vals[[0, 2, 4, 6]] < W) and np.all(vals[[1, 3, 5, 7]] >= 0) and np.all(vals[[1, 3, 5, 7]] < H)):
            continue
        r = out[k]
        r["u1p"], r["v1p"], r["u2p"], r["v2p"], r["u1c"], r["v1c"], r["u2c"], r["v2c"] = vals
        r["i1p"] = r["i2p"] = r["i1c"] = r["i2c"] = k
        k += 1
    return out, is_a


MONO_TR_B = (0.015, 0.05, -0.01, 0.5, -0.1, -0.6)


def mono_two_motion_scene(dtype, n_a, n_b, seed, tr_a=(0.002, -0.01, 0.001, 0.02, -0.005, -0.9), tr_b=MONO_TR_B, height=1.65, f=645.24,
                          cu=635.96, cv=194.13, W=1241, H=376):
    """-> (p_match[n_a + n_b], is_a).  Flow matches of one camera (right-camera fields = -1), not rounded to pixels; a
    fifth of each set lies on the road plane."""
    rng = np.random.default_rng(seed)
    is_a = _two_motions(n_a, n_b)
    out = np.zeros(n_a + n_b, dtype)
    for name in out.dtype.names:
        out[name] = -1
    k = 0
    while k < len(out):
        tr = tr_a if is_a[k] else tr_b
        R, t = rot(*tr[:3]), np.array(tr[3:])
        Z = rng.uniform(4, 50)
        if rng.random() < 0.2:
            X, Y = rng.uniform(-0.8, 0.8) * Z * 0.6, height
        else:
            X, Y = rng.uniform(-1, 1) * Z * 0.9, rng.uniform(-0.28, 0.02) * Z
        P = np.array([X, Y, Z]); Q = R @ P + t
        if Q[2] < 2:
            continue
        vals = np.array([f * P[0] / P[2] + cu, f * P[1] / P[2] + cv, f * Q[0] / Q[2] + cu, f * Q[1] / Q[2] + cv])
        if not (0 <= vals[0] < W and 0 <= vals[2] < W and 0 <= vals[1] < H and 0 <= vals[3] < H):
            continue
        r = out[k]
        r["u1p"], r["v1p"], r["u1c"], r["v1c"] = vals
        r["i1p"] = r["i1c"] = k
        k += 1
    return out, is_a


def invert_draw(n, indices, rng=None):
    """The rand() values for which VisualOdometry::getRandomSample(n, len(indices)) (src/viso.cpp:86-106: draw j = rand() % left,
    take and erase the j-th of the indices left) returns `indices` in this order.  With rng, a random multiple of `left`
    is added to each value (the same draw from a larger number)."""
    out, taken = [], []
    for k, idx in enumerate(indices):
        assert 0 <= idx < n and idx not in taken
        left = n - k
        j = int(idx) - sum(1 for t in taken if t < idx)
        if rng is not None:
            j += left * int(rng.integers(0, (2 ** 31 - 1 - j) // left))
        out.append(j)
        taken.append(int(idx))
    return np.array(out, np.int32)


def all_identical(pm):
    out = pm.copy()
    out[:] = pm[0]
    return out


def bad_disparity(pm, share, seed):
    """A share of the matches with u1p == u2p (zero disparity) or u1p < u2p (negative), alternately."""
    rng = np.random.default_rng(seed)
    out = pm.copy()
    hit = np.flatnonzero(rng.random(len(pm)) < share)
    for q, i in enumerate(hit):
        out["u2p"][i] = out["u1p"][i] + (0 if q % 2 == 0 else rng.integers(1, 30))
    return out, hit


def match_at_cu(pm, cu, index):
    """Match `index` at exactly u1c == cu (cu must be a float value)."""
    assert float(np.float32(cu)) == float(cu)
    out = pm.copy()
    out["u2c"][index] = np.float32(cu) - (out["u1c"][index] - out["u2c"][index])
    out["u1c"][index] = np.float32(cu)
    return out


TR_TURN = (0.0, 2.5, 0.0, 0.0, 0.0, 6.0)   # 143 degrees about the vertical axis


def behind_camera(pm, count, seed, f=645.24, cu=635.96, cv=194.13, base=0.5707):
    """`count` matches (unrounded) of points two or three metres ahead that follow TR_TURN exactly -> (p_match, their
    indices).  The motion that a sample of them defines carries the scene's ordinary points behind the camera
    (depths_under_sample counts them)."""
    rng = np.random.default_rng(seed)
    out = pm.copy()
    hit = np.sort(rng.choice(len(pm), count, replace=False))
    R, t = rot(*TR_TURN[:3]), np.array(TR_TURN[3:])
    for i in hit:
        P = np.array([rng.uniform(-0.5, 0.5), rng.uniform(-0.3, 0.3), rng.uniform(1.5, 3.0)]); Q = R @ P + t
        r = out[i]
        r["u1p"], r["v1p"], r["u2p"] = f * P[0] / P[2] + cu, f * P[1] / P[2] + cv, f * (P[0] - base) / P[2] + cu
        r["u1c"], r["v1c"], r["u2c"] = f * Q[0] / Q[2] + cu, f * Q[1] / Q[2] + cv, f * (Q[0] - base) / Q[2] + cu
        r["v2p"], r["v2c"] = r["v1p"], r["v1c"]
    return out, hit


def depths_under_sample(pm, sample, f=645.24, cu=635.96, cv=194.13, base=0.5707):
    """Z of every match's previous-frame point after the rigid motion (least squares, Kabsch) that takes the sampled
    matches' previous-frame points to their current-frame points."""
    def points(u1, v1, u2):
        d = np.maximum(u1.astype(np.float64) - u2, 1e-4)
        return np.stack([(u1 - cu) * base / d, (v1 - cv) * base / d, f * base / d], 1)
    P, Q = points(pm["u1p"], pm["v1p"], pm["u2p"]), points(pm["u1c"], pm["v1c"], pm["u2c"])
    a, b = P[sample], Q[sample]
    ca, cb = a.mean(0), b.mean(0)
    U, _, Vt = np.linalg.svd((a - ca).T @ (b - cb))
    D = np.diag([1.0, 1.0, np.sign(np.linalg.det(Vt.T @ U.T))])
    R = Vt.T @ D @ U.T
    return (P @ R.T + (cb - R @ ca))[:, 2]


def huge_coordinates(pm, count, seed):
    """`count` matches with one coordinate each replaced by +-1e30f."""
    rng = np.random.default_rng(seed)
    out = pm.copy()
    hit = rng.choice(len(pm), count, replace=False)
    fields = ["u1p", "v1p", "u2p", "u1c", "v1c", "u2c", "v2c"]
    for q, i in enumerate(hit):
        out[fields[q % len(fields)]][i] = np.float32(1e30 if q % 2 == 0 else -1e30)
    return out, hit


EXACT = dict(f=512.0, cu=256.0, cv=128.0, base=0.5)


def exact_static_scene(dtype, n, seed):
    """A camera that does not move, integer positions, every disparity 4, seen with the power-of-two intrinsics EXACT:
    X = (u - 256) / 8, Z = 64 and f X / Z + cu = u are all exact, the first Gauss-Newton step of every hypothesis is
    exactly zero, and every residual of every match is exactly 0.0 -- the value at which `<` and `<=` part."""
    rng = np.random.default_rng(seed)
    out = np.zeros(n, dtype)
    out["u1p"] = out["u1c"] = rng.integers(260, 500, n); out["v1p"] = out["v2p"] = out["v1c"] = out["v2c"] = rng.integers(0, 250, n)
    out["u2p"] = out["u2c"] = out["u1p"] - 4
    out["i1p"] = out["i2p"] = out["i1c"] = out["i2c"] = np.arange(n)
    return out


KITTI = dict(f=645.24, cu=635.96, cv=194.13, base=0.5707)
SECOND = dict(f=400.0, cu=240.0, cv=100.0, base=0.12)   # the second intrinsics set of the edge tests (a 480 x 200 camera)

#: (n, seed) of random_matches(n, seed) for which the stereo oracle, at inlier_threshold 0.3 and rand() after srand(0),
#: ends with a winner of 1 inlier (the first) and of 2 (the others; unrelated matches give no more in 30 000 seeds each):
#: found on the CPU with the oracle; the tests assert the property
FEW_INLIER_SEEDS = ((8, 9), (8, 660), (10, 382), (12, 869))
#: (n, k, seed) of few_inliers_planted: winners of exactly k = 3, 4, 5 inliers, the rest of the range below 6
FEW_INLIER_PLANTED = ((9, 3, 1), (10, 4, 2), (12, 5, 3))


#: (n, seed) of bad_disparity(scene(n, seed, outliers=0.5), all) for which, at inlier_threshold 40, the winner has >= 6
#: inliers and the refit on them does not converge (found in a 3 s search with the oracle; the tests assert the property)
REFIT_FAIL_SEEDS = ((20, 12), (40, 30))


#: (n, seed) of the same construction whose result (inlier count or set, at inlier_threshold 40, rand() after srand(0))
#: depends on the 22nd Gauss-Newton update of a hypothesis: a restatement that stops after 21 gives other inliers
#: (found by running such a restatement beside the oracle for 5 s)
SLOW_HYPOTHESIS_SEEDS = ((40, 5), (12, 14), (12, 18))


def defaults_zero_match(dtype):
    """The defaults_cu0 scene with match 5 at u1c == 0: under the untouched default parameters (cu = 0) its weight is
    0 / 0.  The reference then searches a pivot in an all-NaN system and uses indices it never set (it crashes in the
    build the oracle is pinned to); the oracle starts them at 0, and that is what the device is held to."""
    return match_at_cu(scene(dtype, 60, 38)[0], 0.0, 5)


def random_matches(dtype, n, seed, W=1241, H=376):
    """n unrelated matches: integer positions drawn independently, positive disparities."""
    rng = np.random.default_rng(seed)
    out = np.zeros(n, dtype)
    for k in range(n):
        r = out[k]
        r["u1p"] = rng.integers(100, W); r["u2p"] = r["u1p"] - rng.integers(1, 100); r["v1p"] = r["v2p"] = rng.integers(0, H)
        r["u1c"] = rng.integers(100, W); r["u2c"] = r["u1c"] - rng.integers(1, 100); r["v1c"] = r["v2c"] = rng.integers(0, H)
        r["i1p"] = r["i2p"] = r["i1c"] = r["i2c"] = k
    return out


def few_inliers_planted(dtype, n, k, seed):
    """n unrelated matches of which k (at random places) follow one rigid motion exactly: a hypothesis sampled inside the
    k counts k inliers and nothing counts more."""
    out = random_matches(dtype, n, 5000 + seed)
    hit = np.sort(np.random.default_rng(seed).choice(n, k, replace=False))
    out[hit] = two_motion_scene(dtype, k, 0, 700 + seed)[0]
    out["i1p"] = out["i2p"] = out["i1c"] = out["i2c"] = np.arange(n)
    return out


def stereo_edge_cases(dtype):
    """name -> (p_match, EgoParams keywords; None = the untouched defaults).  One of every new stereo scene kind, none
    above 600 matches: what tests/golden/egomotion_edges.npz records the reference's answers to."""
    c = {}
    c["tie40"] = (two_motion_scene(dtype, 40, 40, 21)[0], dict(KITTI))
    c["tie40_plain"] = (two_motion_scene(dtype, 40, 40, 22)[0], dict(KITTI, reweighting=0, ransac_iters=64))
    c["identical30"] = (all_identical(scene(dtype, 30, 10)[0]), dict(KITTI))
    for n, seed in FEW_INLIER_SEEDS:
        c[f"few_inliers_{n}_{seed}"] = (random_matches(dtype, n, seed), dict(KITTI, inlier_threshold=0.3))
    for n, k, seed in FEW_INLIER_PLANTED:
        c[f"few_planted_{n}_{k}"] = (few_inliers_planted(dtype, n, k, seed), dict(KITTI, inlier_threshold=0.3))
    base = scene(dtype, 300, 31, outliers=0.3, noise=0.2)[0]
    c["bad_disparity"] = (bad_disparity(base, 0.2, 32)[0], dict(KITTI))
    c["all_bad_disparity"] = (bad_disparity(scene(dtype, 40, 33)[0], 1.1, 34)[0], dict(KITTI))
    c["behind_camera"] = (behind_camera(base, 12, 35)[0], dict(KITTI, ransac_iters=300))
    c["huge"] = (huge_coordinates(base, 7, 36)[0], dict(KITTI))
    sec = scene(dtype, 200, 37, outliers=0.3, noise=0.2, W=480, H=200, **SECOND)[0]
    c["second_intrinsics"] = (sec, dict(SECOND))
    c["at_cu_second"] = (match_at_cu(sec, 240.0, 17), dict(SECOND))
    c["defaults_cu0"] = (scene(dtype, 60, 38)[0], None)   # (with a match at u1c == 0 the reference reads pivots it never set: defaults_zero_match)
    for n, seed in REFIT_FAIL_SEEDS:
        c[f"refit_fail_{n}"] = (bad_disparity(scene(dtype, n, seed, outliers=0.5)[0], 1.1, seed)[0], dict(KITTI, inlier_threshold=40.0))
    for n, seed in SLOW_HYPOTHESIS_SEEDS:
        c[f"slow_hypothesis_{n}_{seed}"] = (bad_disparity(scene(dtype, n, seed, outliers=0.5)[0], 1.1, seed)[0], dict(KITTI, inlier_threshold=40.0))
    c["exact_thr0"] = (exact_static_scene(dtype, 40, 39), dict(EXACT, inlier_threshold=0.0, ransac_iters=64))
    c["exact_thr1e-9"] = (exact_static_scene(dtype, 40, 39), dict(EXACT, inlier_threshold=1e-9, ransac_iters=64))
    for n in (6, 7, 8):
        c[f"n{n}"] = (scene(dtype, n, 40 + n, outliers=0.0)[0], dict(KITTI, ransac_iters=64))
    for n in (255, 256, 257, 512, 513):
        c[f"n{n}"] = (scene(dtype, n, 40 + n, outliers=0.3, noise=0.2)[0], dict(KITTI, ransac_iters=64))
    c["full512"] = (scene(dtype, 512, 61, outliers=0.0)[0], dict(KITTI, ransac_iters=64, inlier_threshold=10.0))
    c["full513"] = (scene(dtype, 513, 62, outliers=0.0)[0], dict(KITTI, ransac_iters=64, inlier_threshold=10.0))
    for it in (1, 2, 255, 256, 257, 513):
        c[f"iters{it}"] = (scene(dtype, 200, 63, outliers=0.3, noise=0.2)[0], dict(KITTI, ransac_iters=it))
    return c


MONO_KITTI = dict(f=645.24, cu=635.96, cv=194.13, height=1.65)
MONO_SECOND = dict(f=400.0, cu=240.0, cv=100.0, height=1.2)

#: (n, seed) of random_flow_matches for which the mono oracle's winner has fewer than 10 inliers (rand() after srand(0),
#: 300 hypotheses; found on the CPU with the oracle, the tests assert the property)
MONO_FEW_INLIER_SEEDS = ((14, 1), (20, 2))


#: inlier_threshold equal, to the bit, to the Sampson distance of match SAMPSON_EQUAL_MATCH of mono_scene(300, 78,
#: outliers 0.3, noise 0.3) under the one hypothesis that rand() after srand(0) draws first: found by bisecting the oracle's
#: one-hypothesis inlier count over the doubles between 1e-5 and 2e-5 (the next double admits the match; the tests assert it)
SAMPSON_EQUAL_THRESHOLD = float.fromhex("0x1.506dda366c409p-17")
SAMPSON_EQUAL_MATCH = 172


def random_flow_matches(dtype, n, seed, W=1241, H=376):
    """n unrelated flow matches of one camera."""
    rng = np.random.default_rng(seed)
    out = np.zeros(n, dtype)
    for name in out.dtype.names:
        out[name] = -1
    out["u1p"] = rng.integers(0, W, n); out["v1p"] = rng.integers(0, H, n)
    out["u1c"] = rng.integers(0, W, n); out["v1c"] = rng.integers(0, H, n)
    out["i1p"] = out["i1c"] = np.arange(n)
    return out


def mono_edge_cases(dtype):
    """name -> (p_match, MonoParams keywords; None = the untouched defaults): one of every new mono scene kind, none above
    600 matches (tests/golden/mono_edges.npz)."""
    c = {}
    for n in (9, 10, 11, 12):
        c[f"n{n}"] = (mono_scene(dtype, n, 70 + n, outliers=0.0)[0], dict(MONO_KITTI, ransac_iters=256))
    c["tie60"] = (mono_two_motion_scene(dtype, 60, 60, 20)[0], dict(MONO_KITTI, ransac_iters=500))
    c["identical30"] = (all_identical(mono_scene(dtype, 30, 75)[0]), dict(MONO_KITTI, ransac_iters=128))
    c["no_motion"] = (mono_scene(dtype, 300, 76, tr=(0.0, 0.0002, 0.0, 0.0005, 0.0, -0.002), outliers=0.1)[0], dict(MONO_KITTI, ransac_iters=500))
    c["pure_rotation"] = (mono_scene(dtype, 300, 77, tr=(0.002, 0.04, -0.001, 0.001, 0.0, -0.003), outliers=0.1)[0], dict(MONO_KITTI, ransac_iters=500))
    for n, seed in MONO_FEW_INLIER_SEEDS:
        c[f"few_inliers_{n}"] = (random_flow_matches(dtype, n, seed), dict(MONO_KITTI, ransac_iters=300))
    base = mono_scene(dtype, 300, 78, outliers=0.3, noise=0.3)[0]
    for it in (1, 127, 128, 129, 256, 500):
        c[f"iters{it}"] = (base, dict(MONO_KITTI, ransac_iters=it))
    c["height1"] = (mono_scene(dtype, 300, 79, height=1.0, outliers=0.2, noise=0.2)[0], dict(MONO_KITTI, height=1.0, ransac_iters=500))
    c["pitch"] = (base, dict(MONO_KITTI, pitch=-0.08, ransac_iters=500))
    c["thr1e-6"] = (base, dict(MONO_KITTI, inlier_threshold=1e-6, ransac_iters=500))
    c["thr1e-4"] = (base, dict(MONO_KITTI, inlier_threshold=1e-4, ransac_iters=500))
    c["sampson_equal"] = (base, dict(MONO_KITTI, inlier_threshold=SAMPSON_EQUAL_THRESHOLD, ransac_iters=1))
    c["sampson_next"] = (base, dict(MONO_KITTI, inlier_threshold=float(np.nextafter(SAMPSON_EQUAL_THRESHOLD, 1.0)), ransac_iters=1))
    c["second_intrinsics"] = (mono_scene(dtype, 250, 80, outliers=0.2, noise=0.2, W=480, H=200, **MONO_SECOND)[0], dict(MONO_SECOND, ransac_iters=500))
    c["defaults"] = (mono_scene(dtype, 200, 81, outliers=0.2, noise=0.2)[0], None)
    return c
