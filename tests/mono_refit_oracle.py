"""The mono model refit (vh_refit_model_mono) restated twice: fundamentalMatrix (reference
src/viso_mono.cpp:235-266) over EVERY record of a list, in the normalised frame of the model the list comes with.

The contract, as include/viso_hip.h states it:
  1. normalisation: the incoming model's c[4], s[2], copied to the output unchanged; a record is normalised by
     mono_inlier_oracle.normalise_record (a float rounding per step);
  2. rows: a = (u1c*u1p, u1c*v1p, u1c, v1c*u1p, v1c*v1p, v1c, u1p, v1p, 1): float products, then widened;
  3. moments: M = sum a a^T, the upper triangle mirrored;
  4. null direction: f = the column of V that Matrix::svd's descending sort of the 9 x 9 M puts last; w = (w[8], w[7]);
     f is negated when dot(f, F_in) (nine terms, row-major, in double) is negative, a zero or NaN product leaves it;
  5. rank 2: the 3 x 3 step of :262-265;
  6. ok = 0, the zero model and w = 0 where ok_in == 0, fewer than 10 records, or a non-finite entry of F, w[8], w[7].

    model, ok, w = refit(svd, pm, model_in)         float64, a sequential sum, svd = the pinned Matrix::svd (Oracle.svd)
    model, ok, w = refit_ext(pm, model_in)          numpy.longdouble, a cyclic Jacobi of its own on the 9 x 9 (and on the
                                                    3 x 3 of the rank-2 step); rows are formed as in `refit`

A model is a dict(c [4], s [2], F [9], valid), the fields of vh_mono_model (mono_inlier_oracle).  The device adds in
another order (a tree fixed by the list's length) and is held to 16 times the largest deviation of `refit` from
`refit_ext` over the test's own lists (tests/test_mono_refit.py)."""
import numpy as np

import mono_inlier_oracle as mo

F64, LD = np.float64, np.longdouble
EXTENDED = np.finfo(LD).eps < np.finfo(F64).eps
MIN_RECORDS = 10   # src/viso_mono.cpp:76


def rows(pm, model):
    """The N x 9 system of fundamentalMatrix over every record, float64 (every entry a float32 value widened)."""
    u1p, v1p, u1c, v1c = mo.normalise_record(pm, model["c"], model["s"])
    with np.errstate(all="ignore"):
        return np.stack([(u1c * u1p).astype(F64), (u1c * v1p).astype(F64), u1c.astype(F64),
                         (v1c * u1p).astype(F64), (v1c * v1p).astype(F64), v1c.astype(F64),
                         u1p.astype(F64), v1p.astype(F64), np.ones(len(pm), F64)], axis=1)


def moments(A):
    """M = sum a a^T, rows added one after the other from 0 (np.cumsum adds left to right), upper triangle mirrored."""
    with np.errstate(all="ignore"):
        M = np.cumsum(A[:, :, None] * A[:, None, :], axis=0)[-1]
    return np.triu(M) + np.triu(M, 1).T


def _refused():
    return dict(mo.ZERO_MODEL), False, np.zeros(2, F64)


def _signed(f, F_in):
    """f, or -f when dot(f, F_in) < 0 (sequential, in the arithmetic of f); zero and NaN leave it."""
    d = f.dtype.type(0)
    with np.errstate(all="ignore"):
        for q in range(9):
            d = d + f[q] * f.dtype.type(F_in[q])
    return -f if d < 0 else f


def _result(model, F, w):
    F = np.asarray(F, F64).reshape(9); w = np.asarray(w, F64)
    if not (np.isfinite(F).all() and np.isfinite(w).all()):
        return _refused()
    return dict(c=np.array(model["c"], F64), s=np.array(model["s"], F64), F=F, valid=1.0), True, w


def refit(svd, pm, model, ok=True):
    """The double form -> (model_out, ok_out, w [2] = (w[8], w[7]))."""
    if not ok or len(pm) < MIN_RECORDS:
        return _refused()
    M = moments(rows(pm, model))
    if not np.isfinite(M).all():   # (the pinned routine is not asked to decompose NaN)
        return _refused()
    _, W, V = svd(M)
    f = _signed(np.array(V[:, 8], F64), np.asarray(model["F"], F64).reshape(9))
    U3, W3, V3 = svd(f.reshape(3, 3))
    W3 = np.array(W3, F64); W3[2] = 0
    return _result(model, mo.matmul(mo.matmul(U3, np.diag(W3)), V3.T), (W[8], W[7]))


def jacobi_eigh(A, sweeps=60):
    """Cyclic Jacobi on a symmetric matrix in its own dtype -> (eigenvalues ascending, eigenvectors in columns)."""
    A = np.array(A); T = A.dtype.type
    n = A.shape[0]
    V = np.eye(n, dtype=A.dtype)
    for _ in range(sweeps):   # (a huge theta overflows its square to inf: t = 0, as it should be)
        off = sum(A[p, q] * A[p, q] for p in range(n) for q in range(p + 1, n))
        if off == 0:
            break
        for p in range(n):
            for q in range(p + 1, n):
                if A[p, q] == 0:
                    continue
                with np.errstate(over="ignore"):
                    theta = (A[q, q] - A[p, p]) / (T(2) * A[p, q])
                    t = (T(1) if theta >= 0 else T(-1)) / (abs(theta) + np.sqrt(theta * theta + T(1)))
                c = T(1) / np.sqrt(t * t + T(1)); s = t * c
                J = np.eye(n, dtype=A.dtype)
                J[p, p] = c; J[q, q] = c; J[p, q] = s; J[q, p] = -s
                A = J.T @ A @ J
                A[p, q] = A[q, p] = T(0)
                V = V @ J
    lam = np.array([A[k, k] for k in range(n)])
    order = np.argsort(lam)
    return lam[order], V[:, order]


def refit_ext(pm, model, ok=True):
    """The numpy.longdouble form -> (model_out, ok_out, w [2]) as float64 roundings of the long double results, and the
    long double F and w themselves as a fourth and fifth value (None where refused)."""
    if not ok or len(pm) < MIN_RECORDS:
        return _refused() + (None, None)
    A = rows(pm, model).astype(LD)
    with np.errstate(all="ignore"):
        M = (A[:, :, None] * A[:, None, :]).sum(axis=0, dtype=LD)
    if not np.isfinite(M).all():
        return _refused() + (None, None)
    lam, V = jacobi_eigh(M)
    f = _signed(V[:, 0] / np.sqrt((V[:, 0] * V[:, 0]).sum()), np.asarray(model["F"], F64).reshape(9))
    F0 = f.reshape(3, 3)
    # rank 2: F0 less its smallest singular triple, sigma3 u3 v3^T = (F0 v3) v3^T, v3 the eigenvector of F0^T F0
    _, V3 = jacobi_eigh(F0.T @ F0)
    v3 = V3[:, 0] / np.sqrt((V3[:, 0] * V3[:, 0]).sum())
    Fx = (F0 - np.outer(F0 @ v3, v3)).reshape(9)
    wx = np.array([lam[0], lam[1]], LD)
    return _result(model, Fx.astype(F64), wx.astype(F64)) + (Fx, wx)


def deviation_F(F, Fx):
    """|| F - Fx ||_F (F has unit norm up to the rank-2 step: absolute is relative)."""
    d = np.asarray(F, LD).reshape(9) - np.asarray(Fx, LD).reshape(9)
    return float(np.sqrt((d * d).sum()))


def deviation_w(w, wx):
    """max |w - wx| / |wx| over w[8], w[7]."""
    w = np.asarray(w, LD); wx = np.asarray(wx, LD)
    return float(np.max(np.abs(w - wx) / np.abs(wx)))


def gap(M_or_w9):
    """(w[7] - w[8]) / w[0] of the singular values of M, descending: how well the null direction is determined."""
    w = np.sort(np.asarray(M_or_w9, F64))[::-1]
    return float((w[7] - w[8]) / w[0])


def T_of(c_u, c_v, s):
    """normalizeFeaturePoints' transformation matrix (src/viso_mono.cpp:226-227)."""
    return np.array([[s, 0, -s * c_u], [0, s, -s * c_v], [0, 0, 1]], F64)


def denormalise(model):
    """F of the pixel frame: ~Tc * F * Tp (src/viso_mono.cpp:83)."""
    c, s = model["c"], model["s"]
    return T_of(c[2], c[3], s[1]).T @ np.asarray(model["F"], F64).reshape(3, 3) @ T_of(c[0], c[1], s[0])


def normalised_F(F_pixel, c, s):
    """A pixel-frame F in the normalised frame of (c, s), unit Frobenius norm: Tc^-T F Tp^-1."""
    Fn = np.linalg.inv(T_of(c[2], c[3], s[1])).T @ np.asarray(F_pixel, F64).reshape(3, 3) @ np.linalg.inv(T_of(c[0], c[1], s[0]))
    return (Fn / np.linalg.norm(Fn)).reshape(9)


def sin_angle(Fa, Fb):
    """The sine of the angle between two F as 9-vectors, signs ignored."""
    a = np.asarray(Fa, F64).reshape(9); b = np.asarray(Fb, F64).reshape(9)
    a = a / np.linalg.norm(a); b = b / np.linalg.norm(b)
    return float(min(np.linalg.norm(a - b), np.linalg.norm(a + b)))


# ---- scenes: flow of a general 3-d scene under a known motion ---------------------------------------------------
CAL = dict(f=645.24, cu=635.96, cv=194.13)
MOTION = (0.004, -0.02, 0.003, 0.35, -0.04, -0.9)   # sideways plus forward translation, a small rotation


def _rot(rx, ry, rz):
    cx, sx, cy, sy, cz, sz = np.cos(rx), np.sin(rx), np.cos(ry), np.sin(ry), np.cos(rz), np.sin(rz)
    return np.array([[cy * cz, -cy * sz, sy],
                     [sx * sy * cz + cx * sz, -sx * sy * sz + cx * cz, -sx * cy],
                     [-cx * sy * cz + sx * sz, cx * sy * sz + sx * cz, cx * cy]])


def true_F(tr=MOTION, cal=CAL):
    """The pixel-frame F with x_c^T F x_p = 0 for Q = R P + t: K^-T [t]x R K^-1."""
    R, t = _rot(*tr[:3]), np.array(tr[3:], F64)
    K = np.array([[cal["f"], 0, cal["cu"]], [0, cal["f"], cal["cv"]], [0, 0, 1]], F64)
    tx = np.array([[0, -t[2], t[1]], [t[2], 0, -t[0]], [-t[1], t[0], 0]], F64)
    Ki = np.linalg.inv(K)
    return Ki.T @ tx @ R @ Ki


def flow_scene(dtype, n, seed, noise=0.3, tr=MOTION, cal=CAL, quad=False):
    """n flow records of points spread in depth 5 .. 50 m over the whole field of view (no dominant plane), exact
    projections before and after the motion plus Gaussian pixel noise of `noise` pixels on all four coordinates, rounded to
    float.  The right-camera fields are -1 (quad: the left camera's values shifted, as a quad list carries them)."""
    rng = np.random.default_rng(seed)
    f, cu, cv = cal["f"], cal["cu"], cal["cv"]
    R, t = _rot(*tr[:3]), np.array(tr[3:], F64)
    out = np.zeros(n, dtype)
    for name in out.dtype.names:
        out[name] = -1
    Z = rng.uniform(5, 50, n)
    P = np.stack([rng.uniform(-0.9, 0.9, n) * Z, rng.uniform(-0.28, 0.26, n) * Z, Z], axis=1)
    Q = P @ R.T + t
    assert (Q[:, 2] > 2).all()
    vals = np.stack([f * P[:, 0] / P[:, 2] + cu, f * P[:, 1] / P[:, 2] + cv, f * Q[:, 0] / Q[:, 2] + cu, f * Q[:, 1] / Q[:, 2] + cv], axis=1)
    vals = vals + noise * rng.standard_normal(vals.shape)
    for k, name in enumerate(("u1p", "v1p", "u1c", "v1c")):
        out[name] = vals[:, k].astype(np.float32)
    out["i1p"] = out["i1c"] = np.arange(n)
    if quad:
        out["u2p"] = out["u1p"] - np.float32(12); out["v2p"] = out["v1p"]; out["u2c"] = out["u1c"] - np.float32(12); out["v2c"] = out["v1c"]
        out["i2p"] = out["i2c"] = np.arange(n)
    return out


def start_model(pm, tr=MOTION, cal=CAL, tilt=0.0):
    """An incoming model for a whole list: its own normalisation and the true F in that frame (unit norm), tilted by
    `tilt` towards a fixed direction so that it is a model to refine, not the answer."""
    nrm = mo.normalise(pm)
    assert nrm is not None
    F = normalised_F(true_F(tr, cal), nrm[0], nrm[1])
    F = F + tilt * np.array([0.3, -0.1, 0.2, 0.1, 0.4, -0.2, 0.1, -0.3, 0.2])
    return dict(c=nrm[0], s=nrm[1], F=F / np.linalg.norm(F), valid=1.0)
