"""VisualOdometryMono's inlier test (getInlier, reference src/viso_mono.cpp:268-315) and the model it needs
(normalizeFeaturePoints :187-233, fundamentalMatrix :235-266) restated in numpy: what vh_motion_inliers_mono computes
per record and what vh_estimate_motion_mono_model exports.  float32 where the reference's p_match fields are float,
float64 elsewhere; every product and sum is an operation of its own, in the reference's order (numpy never fuses
a*b+c; np.cumsum adds left to right).

    model = model_of(svd, pm, inlier_indices)       svd: the pinned Matrix::svd (oracle.binding.Oracle.svd)
    flags, d = inliers(pm, model, threshold)        flags[i] = |d[i]| < threshold   (strict; NaN compares false)

A model is a dict(c [4], s [2], F [9], valid) of float64, the fields of vh_mono_model."""
import numpy as np

F32, F64 = np.float32, np.float64
ZERO_MODEL = dict(c=np.zeros(4), s=np.zeros(2), F=np.zeros(9), valid=0.0)


def _seq_sum(x):
    """x[0] + x[1] + .. in this order, in double (the reference's `for ... sum += term`)."""
    x = np.asarray(x, F64)
    return F64(np.cumsum(x)[-1]) if len(x) else F64(0)


def center(u, c):
    """it->u1p -= cpu: the difference in double, stored into the float field."""
    with np.errstate(all="ignore"):
        return (np.asarray(u, F32).astype(F64) - F64(c)).astype(F32)


def scale(q, s):
    """it->u1p *= sp: the product in double, stored into the float field."""
    with np.errstate(all="ignore"):
        return (np.asarray(q, F32).astype(F64) * F64(s)).astype(F32)


def normalise_record(pm, c, s):
    """The four normalised coordinates (u1p, v1p, u1c, v1c) of every record under centroids c[4] and scales s[2]."""
    return (scale(center(pm["u1p"], c[0]), s[0]), scale(center(pm["v1p"], c[1]), s[0]),
            scale(center(pm["u1c"], c[2]), s[1]), scale(center(pm["v1c"], c[3]), s[1]))


def normalise(pm):
    """normalizeFeaturePoints -> (c [4], s [2]) or None where it returns false (or the list has fewer than 10 records)."""
    n = len(pm)
    if n < 10:
        return None
    c = np.array([_seq_sum(pm[k]) / F64(n) for k in ("u1p", "v1p", "u1c", "v1c")], F64)
    q = [center(pm[k], c[j]) for j, k in enumerate(("u1p", "v1p", "u1c", "v1c"))]
    with np.errstate(all="ignore"):
        dp = np.sqrt(q[0] * q[0] + q[1] * q[1])   # float products, float sum, float sqrt
        dc = np.sqrt(q[2] * q[2] + q[3] * q[3])
    assert dp.dtype == F32 and dc.dtype == F32
    sp, sc = _seq_sum(dp), _seq_sum(dc)
    if abs(sp) < 1e-10 or abs(sc) < 1e-10:
        return None
    s = np.array([np.sqrt(F64(2.0)) * F64(n) / sp, np.sqrt(F64(2.0)) * F64(n) / sc], F64)
    return c, s


def matmul(A, B):
    """Matrix::operator* (src/matrix.cpp:263-277): every element a sum from 0, k ascending."""
    A = np.asarray(A, F64); B = np.asarray(B, F64)
    C = np.zeros((A.shape[0], B.shape[1]), F64)
    with np.errstate(all="ignore"):
        for i in range(A.shape[0]):
            for j in range(B.shape[1]):
                acc = F64(0)
                for k in range(A.shape[1]):
                    acc = acc + A[i, k] * B[k, j]
                C[i, j] = acc
    return C


def fundamental_matrix(svd, pn, active):
    """fundamentalMatrix on the normalised coordinates pn = (u1p, v1p, u1c, v1c) and the index set `active` -> F [9]."""
    u1p, v1p, u1c, v1c = (np.asarray(x, F32)[active] for x in pn)
    A = np.stack([(u1c * u1p).astype(F64), (u1c * v1p).astype(F64), u1c.astype(F64),     # float products (:244-251)
                  (v1c * u1p).astype(F64), (v1c * v1p).astype(F64), v1c.astype(F64),
                  u1p.astype(F64), v1p.astype(F64), np.ones(len(active), F64)], axis=1)
    _, _, V = svd(A)
    F0 = V[:, 8].reshape(3, 3)
    U, W, V = svd(F0)
    W = np.array(W, F64); W[2] = 0
    return matmul(matmul(U, np.diag(W)), V.T).reshape(9)


def model_of(svd, pm, active):
    """The model of a list whose best hypothesis has the inlier set `active` (ob.estimate_motion_mono's indices)."""
    nrm = normalise(pm)
    if nrm is None or len(active) < 10:
        return dict(ZERO_MODEL)
    c, s = nrm
    return dict(c=c, s=s, F=fundamental_matrix(svd, normalise_record(pm, c, s), np.asarray(active, np.int64)), valid=1.0)


def distances(pm, model):
    """The Sampson distance of every record (:283-306), float64; NaN / inf where the reference's quotient is."""
    u1, v1, u2, v2 = (x.astype(F64) for x in normalise_record(pm, model["c"], model["s"]))
    f = [F64(v) for v in np.asarray(model["F"], F64).reshape(9)]
    with np.errstate(all="ignore"):
        Fx1u = f[0] * u1 + f[1] * v1 + f[2]
        Fx1v = f[3] * u1 + f[4] * v1 + f[5]
        Fx1w = f[6] * u1 + f[7] * v1 + f[8]
        Ftx2u = f[0] * u2 + f[3] * v2 + f[6]
        Ftx2v = f[1] * u2 + f[4] * v2 + f[7]
        x2tFx1 = u2 * Fx1u + v2 * Fx1v + Fx1w
        return x2tFx1 * x2tFx1 / (Fx1u * Fx1u + Fx1v * Fx1v + Ftx2u * Ftx2u + Ftx2v * Ftx2v)


def inliers(pm, model, threshold, ok=True):
    """-> (flags uint8 [n], distances float64 [n]); ok = False: no inliers (the distances are still the model's)."""
    d = distances(pm, model)
    with np.errstate(invalid="ignore"):
        flags = (np.abs(d) < F64(threshold)).astype(np.uint8)
    if not ok:
        flags[:] = 0
    return flags, d


def as_array(models, dtype):
    """A list of model dicts as an array of `dtype` (the package's MONO_MODEL_DTYPE)."""
    out = np.zeros(len(models), dtype)
    for k, m in enumerate(models):
        out["c"][k] = m["c"]; out["s"][k] = m["s"]; out["F"][k] = np.asarray(m["F"]).reshape(9); out["valid"][k] = m["valid"]
    return out


def from_array(rec):
    return dict(c=np.array(rec["c"], F64), s=np.array(rec["s"], F64), F=np.array(rec["F"], F64), valid=float(rec["valid"]))
