"""The covariance of a stereo motion over a quad list (include/viso_hip.h, vh_motion_covariance),
restated in numpy: what vh_motion_covariance computes.

    J (4N x 6), r (4N)   the rows of computeResidualsAndJacobian (reference src/viso_stereo.cpp:274-330) at tr, weighted
    A = J^T J, ssr = sum r^2, dof = 4N - 6, sigma2 = ssr / dof, cov = sigma2 * A^-1 (upper triangle, mirrored)

    cov, ssr, ok = covariance(pm, tr, cal, ok=True)       float64, operation for operation the contract: the rows are
                                                          refit_oracle.rows, every sum runs sequentially in list order,
                                                          the inverse is reconstruction_oracle.matrix_solve on the unit matrix
    cov, ssr, ok = covariance_ext(pm, tr, cal, ok=True)   the same in a wider arithmetic: np.longdouble where that is wider
                                                          than double (EXTENDED), else float64 terms summed by math.fsum
                                                          and the 6x6 inverse in fractions.Fraction
    deviation(cov, ref), deviation_ssr(ssr, ref)          the measures the tests bound

cal: anything with f, cu, cv, base, reweighting.  Refusals as the contract's: ok false, N < 6, the elimination refuses,
a non-finite ssr or entry of cov -> zeros and ok = False."""
import math
from fractions import Fraction

import numpy as np

import refit_oracle as ro
from reconstruction_oracle import matrix_solve

EXTENDED = np.finfo(np.longdouble).eps < np.finfo(np.float64).eps


def rows_in(pm, tr, cal, T):
    """refit_oracle.rows in the arithmetic T (np.float64: the same bytes; tests assert it) -> (J [4N][6], res [4N])."""
    f, cu, cv, base = T(cal.f), T(cal.cu), T(cal.cv), T(cal.base)
    rx, ry, rz, tx, ty, tz = (T(v) for v in tr)
    if T is np.float64:
        sx, cx, sy, cy, sz, cz = (T(v) for v in (math.sin(rx), math.cos(rx), math.sin(ry), math.cos(ry), math.sin(rz), math.cos(rz)))
    else:
        sx, cx, sy, cy, sz, cz = np.sin(rx), np.cos(rx), np.sin(ry), np.cos(ry), np.sin(rz), np.cos(rz)
    r = [[+cy * cz, -cy * sz, +sy],
         [+sx * sy * cz + cx * sz, -sx * sy * sz + cx * cz, -sx * cy],
         [-cx * sy * cz + sx * sz, +cx * sy * sz + sx * cz, +cx * cy]]
    zero = T(0)
    drx = [[zero, zero, zero],
           [+cx * sy * cz - sx * sz, -cx * sy * sz - sx * cz, -cx * cy],
           [+sx * sy * cz + cx * sz, -sx * sy * sz + cx * cz, -sx * cy]]
    dry = [[-sy * cz, +sy * sz, +cy],
           [+sx * cy * cz, -sx * cy * sz, +sx * sy],
           [-cx * cy * cz, +cx * cy * sz, -cx * sy]]
    drz = [[-cy * sz, -cy * cz],
           [-sx * sy * sz + cx * cz, -sx * sy * cz - cx * sz],
           [+cx * sy * sz + sx * cz, +cx * sy * cz - sx * sz]]
    u1p, v1p, u2p = (np.asarray(pm[k], np.float32) for k in ("u1p", "v1p", "u2p"))
    n = len(u1p)
    with np.errstate(all="ignore"):
        df = u1p - u2p                                                    # float (:83)
        df = np.where(df < np.float32(0.0001), np.float32(0.0001), df)
        d = df.astype(T)
        X = (u1p.astype(T) - cu) * base / d
        Y = (v1p.astype(T) - cv) * base / d
        Z = f * base / d
        obs = [np.asarray(pm[k], np.float32).astype(T) for k in ("u1c", "v1c", "u2c", "v2c")]
        X1c = r[0][0] * X + r[0][1] * Y + r[0][2] * Z + tx
        Y1c = r[1][0] * X + r[1][1] * Y + r[1][2] * Z + ty
        Z1c = r[2][0] * X + r[2][1] * Y + r[2][2] * Z + tz
        weight = np.ones(n, T)
        if cal.reweighting:
            weight = T(1) / (np.abs(obs[0] - cu) / abs(cu) + T(0.05))     # (the contract's 0.05 is the double)
        X2c = X1c - base
        zeros, ones = np.zeros(n, T), np.ones(n, T)
        deriv = [(zeros, drx[1][0] * X + drx[1][1] * Y + drx[1][2] * Z, drx[2][0] * X + drx[2][1] * Y + drx[2][2] * Z),
                 (dry[0][0] * X + dry[0][1] * Y + dry[0][2] * Z, dry[1][0] * X + dry[1][1] * Y + dry[1][2] * Z,
                  dry[2][0] * X + dry[2][1] * Y + dry[2][2] * Z),
                 (drz[0][0] * X + drz[0][1] * Y, drz[1][0] * X + drz[1][1] * Y, drz[2][0] * X + drz[2][1] * Y),
                 (ones, zeros, zeros), (zeros, ones, zeros), (zeros, zeros, ones)]
        J = np.zeros((4 * n, 6), T)
        for j, (X1cd, Y1cd, Z1cd) in enumerate(deriv):
            J[0::4, j] = weight * f * (X1cd * Z1c - X1c * Z1cd) / (Z1c * Z1c)
            J[1::4, j] = weight * f * (Y1cd * Z1c - Y1c * Z1cd) / (Z1c * Z1c)
            J[2::4, j] = weight * f * (X1cd * Z1c - X2c * Z1cd) / (Z1c * Z1c)
            J[3::4, j] = weight * f * (Y1cd * Z1c - Y1c * Z1cd) / (Z1c * Z1c)
        p = (f * X1c / Z1c + cu, f * Y1c / Z1c + cv, f * X2c / Z1c + cu, f * Y1c / Z1c + cv)
        res = np.zeros(4 * n, T)
        for k in range(4):
            res[k::4] = weight * (obs[k] - p[k])
    return J, res


def _refused():
    return np.zeros((6, 6)), 0.0, False


def _finish(Ainv, ssr, n):
    """sigma2 * the upper triangle of Ainv, mirrored; the last refusal rule -> (cov float64, ssr float64, ok)."""
    sigma2 = ssr / type(ssr)(4 * n - 6)
    cov = np.zeros((6, 6))
    with np.errstate(all="ignore"):
        for m in range(6):
            for q in range(m, 6):
                cov[m, q] = cov[q, m] = float(sigma2 * Ainv[m][q])
    ssr = float(ssr)
    if not (math.isfinite(ssr) and np.isfinite(cov).all()):
        return _refused()
    return cov, ssr, True


def covariance(pm, tr, cal, ok=True):
    n = len(pm)
    if not ok or n < 6:
        return _refused()
    J, res, _ = ro.rows(pm, [float(v) for v in tr], cal)
    A, _ = ro.normal_equations(J, res)
    with np.errstate(all="ignore"):
        ssr = ro._seq_sum(res * res)
        B = [[1.0 if i == j else 0.0 for j in range(6)] for i in range(6)]
        if not matrix_solve(A, B):
            return _refused()
        return _finish(B, ssr, n)


def _inverse_fraction(A):
    """The exact inverse of a 6x6 matrix of finite floats by Gauss-Jordan in Fraction; None where it is singular."""
    n = len(A)
    M = [[Fraction(x) for x in row] + [Fraction(int(i == j)) for j in range(n)] for i, row in enumerate(A)]
    for c in range(n):
        p = max(range(c, n), key=lambda r: abs(M[r][c]))
        if M[p][c] == 0:
            return None
        M[c], M[p] = M[p], M[c]
        M[c] = [x / M[c][c] for x in M[c]]
        for r in range(n):
            if r != c and M[r][c] != 0:
                M[r] = [x - M[r][c] * y for x, y in zip(M[r], M[c])]
    return [row[n:] for row in M]


def covariance_ext(pm, tr, cal, ok=True, extended=None):
    """extended: None = np.longdouble where it is wider than double; False forces the fsum / Fraction form."""
    n = len(pm)
    if not ok or n < 6:
        return _refused()
    extended = EXTENDED if extended is None else extended
    with np.errstate(all="ignore"):
        if extended:
            T = np.longdouble
            J, res = rows_in(pm, tr, cal, T)
            A = [[np.sum(J[:, m] * J[:, q]) for q in range(6)] for m in range(6)]
            ssr = np.sum(res * res)
            B = [[T(i == j) for j in range(6)] for i in range(6)]
            if not np.isfinite(np.array(A, T)).all() or not matrix_solve(A, B):
                return _refused()
            return _finish(B, ssr, n)
        J, res, _ = ro.rows(pm, [float(v) for v in tr], cal)
        if not (np.isfinite(J).all() and np.isfinite(res).all()):
            return _refused()
        A = [[math.fsum(J[:, m] * J[:, q]) for q in range(6)] for m in range(6)]
        ssr = math.fsum(res * res)
        inv = _inverse_fraction(A)
        if inv is None:
            return _refused()
        scale = Fraction(ssr) / (4 * n - 6)
        cov = np.zeros((6, 6))
        for m in range(6):
            for q in range(m, 6):
                cov[m, q] = cov[q, m] = float(scale * inv[m][q])
        return cov, ssr, True


def deviation(cov, ref):
    """max over m, n of |cov_mn - ref_mn| / sqrt(ref_mm * ref_nn)."""
    d = np.sqrt(np.diag(ref))
    return float(np.max(np.abs(np.asarray(cov) - ref) / np.outer(d, d)))


def deviation_ssr(ssr, ref):
    return abs(ssr - ref) / abs(ref)
