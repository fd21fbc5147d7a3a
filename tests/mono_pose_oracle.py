"""The mono pose on whole lists (vh_pose_mono) restated in numpy: the rest of
VisualOdometryMono::estimateMotion after the refit (reference src/viso_mono.cpp:83-158, EtoRt :317-348, triangulateChieral
:364-399, smallerThanMedian :162-185) over EVERY record of a list, under the model the list comes with.

The contract, as include/viso_hip.h states it: F out of the model's frame and E (rank 2), EtoRt's four candidates and
their projection matrices, the chirality count per record and candidate, the winner (first strictly largest), X / X(3,:),
the points in front in list order with dist = |x|+|y|+|z| and d = cos(-pitch)*y + sin(-pitch)*z, the median as the
element of rank np/2 by counting, the ground-plane vote with sequential sums from j = 0, tr.  Every product and sum is an
operation of its own in the reference's order (numpy never fuses a*b+c; np.cumsum adds left to right); the 3 x 3 and 4 x 4
decompositions are the pinned Matrix::svd (oracle.binding.Oracle.svd); exp / arcsin / cos / sin are numpy's.

    res = pose(svd, pm, model, e, ok=True)      e: anything with f, cu, cv, height, pitch, motion_threshold
    res: dict(tr [6], ok, R [9], t [3], scale, median, plane, chirality [4], candidate, n_front, reason, margin)

margin: the relative gap between the winning sum of the vote and the largest sum among elements whose d differs from the
winner's (None where the vote is not reached, inf where no other element has a sum): a device whose exp differs in the
last bits picks the same plane as long as the margin is far above rounding.
A record with a non-finite coordinate is in front of no camera (every comparison with NaN is false): it is not handed
to the pinned svd, its point is NaN."""
import numpy as np

import mono_inlier_oracle as mo
import mono_refit_oracle as mr

F64 = np.float64
MIN_RECORDS = 10   # src/viso_mono.cpp:45, :105
WM = np.array([[0, -1, 0], [1, 0, 0], [0, 0, 1]], F64)
ZM = np.array([[0, 1, 0], [-1, 0, 0], [0, 0, 0]], F64)


def essential(svd, model, K):
    """steps 1: ~Tc*F*Tp, ~K*F*K, rank 2 -> E [3, 3]"""
    c, s = np.asarray(model["c"], F64), np.asarray(model["s"], F64)
    Tp = np.array([[s[0], 0, -s[0] * c[0]], [0, s[0], -s[0] * c[1]], [0, 0, 1]], F64)
    Tc = np.array([[s[1], 0, -s[1] * c[2]], [0, s[1], -s[1] * c[3]], [0, 0, 1]], F64)
    F = mo.matmul(mo.matmul(Tc.T, np.asarray(model["F"], F64).reshape(3, 3)), Tp)
    E = mo.matmul(mo.matmul(K.T, F), K)
    if not np.isfinite(E).all():
        return np.full((3, 3), np.nan)
    U, W, V = svd(E)
    W = np.array(W, F64); W[2] = 0
    return mo.matmul(mo.matmul(U, np.diag(W)), V.T)


def candidates(svd, E, K):
    """step 2 -> (Ra, Rb, t0, P1 [3, 4], P2 [4, 3, 4])"""
    if not np.isfinite(E).all():
        nan3 = np.full((3, 3), np.nan)
        return nan3, nan3.copy(), np.full(3, np.nan), np.hstack([K, np.zeros((3, 1))]), np.full((4, 3, 4), np.nan)
    U, _, V = svd(E)
    T = mo.matmul(mo.matmul(U, ZM), U.T)
    Ra = mo.matmul(mo.matmul(U, WM), V.T)
    Rb = mo.matmul(mo.matmul(U, WM.T), V.T)
    t0 = np.array([T[2, 1], T[0, 2], T[1, 0]], F64)
    if np.linalg.det(Ra) < 0:   # (|det| = 1 up to rounding: the sign is Matrix::det's)
        Ra = -Ra
    if np.linalg.det(Rb) < 0:
        Rb = -Rb
    P1 = np.hstack([K, np.zeros((3, 1))])
    P2 = np.stack([mo.matmul(K, np.hstack([R, (sg * t0).reshape(3, 1)])) for R, sg in ((Ra, 1.0), (Ra, -1.0), (Rb, 1.0), (Rb, -1.0))])
    return Ra, Rb, t0, P1, P2


def triangulate(svd, pm, P1, P2):
    """step 3 for one candidate -> (X [n, 4] up to the sign of each row, good [n])"""
    n = len(pm)
    X = np.full((n, 4), np.nan)
    u1p, v1p, u1c, v1c = (pm[k].astype(F64) for k in ("u1p", "v1p", "u1c", "v1c"))
    with np.errstate(all="ignore"):
        J = np.stack([P1[2][None, :] * u1p[:, None] - P1[0][None, :], P1[2][None, :] * v1p[:, None] - P1[1][None, :],
                      P2[2][None, :] * u1c[:, None] - P2[0][None, :], P2[2][None, :] * v1c[:, None] - P2[1][None, :]], axis=1)
    for i in range(n):
        if np.isfinite(J[i]).all():
            X[i] = svd(J[i])[2][:, 3]
    with np.errstate(all="ignore"):
        a = np.cumsum(P1[2][None, :] * X, axis=1)[:, 3]
        b = np.cumsum(P2[2][None, :] * X, axis=1)[:, 3]
        good = (a * X[:, 3] > 0) & (b * X[:, 3] > 0)
    return X, good


def front_points(X, pitch):
    """step 4 -> (dist [np], d [np]) of the points with z > 0, in list order"""
    with np.errstate(all="ignore"):
        w = X[:, 3]
        P = np.where((w != 0)[:, None], X[:, :3] / w[:, None], 0.0)
        front = P[:, 2] > 0
        x, y, z = P[front, 0], P[front, 1], P[front, 2]
        dist = np.abs(x) + np.abs(y) + np.abs(z)
        n0, n1 = np.cos(-F64(pitch)), np.sin(-F64(pitch))
        d = (0.0 + n0 * y) + n1 * z
    return dist, d


def median_by_rank(dist):
    """step 5: the element with exactly np/2 elements smaller, or equal and earlier; NaN where there is none"""
    n = len(dist)
    if np.isfinite(dist).all():
        return F64(dist[np.argsort(dist, kind="stable")[n // 2]])
    idx = np.arange(n)
    with np.errstate(all="ignore"):
        rank = ((dist[None, :] < dist[:, None]) | ((dist[None, :] == dist[:, None]) & (idx[None, :] < idx[:, None]))).sum(axis=1)
    hit = np.nonzero(rank == n // 2)[0]
    return F64(dist[hit[-1]]) if len(hit) else F64(np.nan)


def vote(d, median, motion_threshold):
    """step 6 -> (best_idx, sums [np], margin)"""
    with np.errstate(all="ignore"):
        sigma = median / F64(50.0)
        weight = F64(1.0) / (F64(2.0) * sigma * sigma)
        active = d > median / F64(motion_threshold)
        sums = np.zeros(len(d), F64)
        for lo in range(0, len(d), 256):   # (blocks of rows: the N x N table of a long list does not fit comfortably)
            q = d[None, :] - d[lo:lo + 256, None]
            sums[lo:lo + 256] = np.cumsum(np.exp(-q * q * weight), axis=1)[:, -1]
        sums = np.where(active, sums, 0.0)
    cmp = np.where(np.isnan(sums), -np.inf, sums)
    if not (cmp.max() > 0):
        return 0, sums, None
    best = int(np.argmax(cmp))   # the first of the largest
    others = cmp[d != d[best]]
    margin = float((cmp[best] - others.max()) / cmp[best]) if len(others) else np.inf
    return best, sums, margin


def _result(reason, **kw):
    out = dict(tr=np.zeros(6), ok=False, R=np.zeros(9), t=np.zeros(3), scale=0.0, median=0.0, plane=0.0, chirality=np.zeros(4, np.int32),
               candidate=-1, n_front=0, reason=reason, margin=None)
    out.update(kw)
    return out


def pose(svd, pm, model, e, ok=True, parts=None):
    """The whole contract.  parts (a dict, optional) receives the intermediate results: E, Ra, Rb, t0, P1, P2, X [4]."""
    if not ok:
        return _result(1)
    if len(pm) < MIN_RECORDS:
        return _result(2)
    K = np.array([[e.f, 0, e.cu], [0, e.f, e.cv], [0, 0, 1]], F64)
    E = essential(svd, model, K)
    Ra, Rb, t0, P1, P2 = candidates(svd, E, K)
    tri = [triangulate(svd, pm, P1, P2[c]) for c in range(4)]
    if parts is not None:
        parts.update(E=E, Ra=Ra, Rb=Rb, t0=t0, P1=P1, P2=P2, X=[x for x, _ in tri])
    counts = np.array([int(g.sum()) for _, g in tri], np.int32)
    cbest, most = -1, 0
    for c in range(4):
        if counts[c] > most:
            most, cbest = counts[c], c
    if cbest < 0:
        return _result(3, chirality=counts)
    R = (Ra if cbest < 2 else Rb).reshape(9)
    t = -t0 if cbest & 1 else t0.copy()
    dist, d = front_points(tri[cbest][0], e.pitch)
    known = dict(chirality=counts, candidate=cbest, n_front=len(dist), R=R.copy(), t=t)
    if len(dist) < MIN_RECORDS:
        return _result(4, **known)
    median = median_by_rank(dist)
    known["median"] = float(median)
    if median > e.motion_threshold:
        return _result(5, **known)
    best, _, margin = vote(d, median, e.motion_threshold)
    plane = d[best]
    known.update(plane=float(plane), margin=margin)
    if abs(plane) < 1e-20:
        return _result(6, **known)
    with np.errstate(all="ignore"):
        known["scale"] = float(F64(e.height) / plane)
        tt = (t * F64(e.height)) / plane
        ry = np.arcsin(R[2])
        tr = np.array([np.arcsin(-R[5] / np.cos(ry)), ry, np.arcsin(-R[1] / np.cos(ry)), tt[0], tt[1], tt[2]], F64)
    if not (np.isfinite(tr).all() and np.isfinite(R).all() and np.isfinite(t).all() and np.isfinite(median) and np.isfinite(plane)):
        return _result(7, **known)
    return _result(0, tr=tr, ok=True, **known)


# ---- scenes: flow over a road plane below a pitched camera plus general structure, under a known motion ----------------
CAL = mr.CAL
MOTION = mr.MOTION        # sideways plus forward translation, a small rotation
HEIGHT, PITCH = 1.65, -0.03


def ground_scene(dtype, n, seed, noise=0.3, tr=MOTION, cal=CAL, height=HEIGHT, pitch=PITCH, ground=0.45, swapped=0):
    """n flow records: a share `ground` of the points on the plane cos(-pitch)*y + sin(-pitch)*z = height of the previous
    camera's frame, the rest spread in depth 5 .. 50 m above it; exact projections before and after the motion plus Gaussian
    noise, rounded to float.  The last `swapped` records have their two positions exchanged (the reversed motion: such a
    point triangulates behind the cameras)."""
    rng = np.random.default_rng(seed)
    f, cu, cv = cal["f"], cal["cu"], cal["cv"]
    R, t = mr._rot(*tr[:3]), np.array(tr[3:], F64)
    out = np.zeros(n, dtype)
    for name in out.dtype.names:
        out[name] = -1
    Z = rng.uniform(5, 50, n)
    X = rng.uniform(-0.9, 0.9, n) * Z
    on_ground = rng.random(n) < ground
    n0, n1 = np.cos(-pitch), np.sin(-pitch)
    Y = np.where(on_ground, (height - n1 * Z) / n0, rng.uniform(-0.28, 0.0, n) * Z)
    X = np.where(on_ground, X * 0.5, X)
    P = np.stack([X, Y, Z], axis=1)
    Q = P @ R.T + t
    assert (Q[:, 2] > 2).all()
    vals = np.stack([f * P[:, 0] / P[:, 2] + cu, f * P[:, 1] / P[:, 2] + cv, f * Q[:, 0] / Q[:, 2] + cu, f * Q[:, 1] / Q[:, 2] + cv], axis=1)
    vals = vals + noise * rng.standard_normal(vals.shape)
    if swapped:
        vals[n - swapped:] = vals[n - swapped:][:, [2, 3, 0, 1]]
    for k, name in enumerate(("u1p", "v1p", "u1c", "v1c")):
        out[name] = vals[:, k].astype(np.float32)
    out["i1p"] = out["i1c"] = np.arange(n)
    return out


def distance_to_truth(tr, truth=MOTION):
    """-> (largest rotation error, largest translation error)"""
    tr = np.asarray(tr, F64); truth = np.asarray(truth, F64)
    return float(np.abs(tr[:3] - truth[:3]).max()), float(np.abs(tr[3:] - truth[3:]).max())
