"""The motion refit on the landmarks (include/viso_hip_lmk_refit.h) restated in numpy: which 3-d point a
record enters the fit with (steps 1-4 of the rule, every product and sum an operation of its own, sums left to right),
and refit_oracle's loop over those points.  The loop, the normal equations and the solve are refit_oracle's own, called
with its `rows` replaced for the call by `rows_points`, which differs from it in one thing: X, Y, Z are passed in
(tests/test_landmark_refit.py holds the two to the same bytes where the points are the records' own).

    prior = priors(pm, prev_pos, prev_state, Tw, cal, min_obs, max_depth_ratio)     REFIT_PRIOR records
    tr, ok, n_updates, steps = refit(pm, prior, tr, cal, ok=True)"""
import math

import numpy as np

import refit_oracle as ro

PRIOR = np.dtype([("X", "<f8"), ("Y", "<f8"), ("Z", "<f8"), ("source", "<i4"), ("reason", "<i4")])


def own_points(pm, cal):
    """the previous pair's point of every record (src/viso_stereo.cpp:83-86)"""
    f, cu, cv, base = np.float64(cal.f), np.float64(cal.cu), np.float64(cal.cv), np.float64(cal.base)
    u1p, v1p, u2p = (np.asarray(pm[k], np.float32) for k in ("u1p", "v1p", "u2p"))
    with np.errstate(all="ignore"):
        df = u1p - u2p
        df = np.where(df < np.float32(0.0001), np.float32(0.0001), df)
        d = df.astype(np.float64)
        return (u1p.astype(np.float64) - cu) * base / d, (v1p.astype(np.float64) - cv) * base / d, f * base / d


def priors(pm, prev_pos, prev_state, Tw, cal, min_obs=2, max_depth_ratio=0.0):
    """prev_state: None (no predecessor) or the predecessor list's LANDMARK_STATE records; Tw: 4x4"""
    X, Y, Z = own_points(pm, cal)
    Tw = np.asarray(Tw, np.float64).reshape(16)
    n_prev = 0 if prev_state is None else len(prev_state)
    out = np.zeros(len(pm), PRIOR)
    with np.errstate(all="ignore"):
        for i in range(len(pm)):
            out[i] = (X[i], Y[i], Z[i], 0, 0)
            p = int(prev_pos[i])
            if not 0 <= p < n_prev:
                out[i]["reason"] = 1
                continue
            st = prev_state[p]
            if int(st["n_obs"]) < min_obs:
                out[i]["reason"] = 2
                continue
            sw = np.float64(st["sw"])
            m = [np.float64(st[k]) / sw for k in ("swx", "swy", "swz")]
            d = [m[0] - Tw[3], m[1] - Tw[7], m[2] - Tw[11]]
            L = [Tw[0 + c] * d[0] + Tw[4 + c] * d[1] + Tw[8 + c] * d[2] for c in range(3)]
            if sw <= 0 or not all(math.isfinite(v) for v in m + L):
                out[i]["reason"] = 3
            elif L[2] <= 0:
                out[i]["reason"] = 4
            else:
                q = L[2] / Z[i]
                if max_depth_ratio > 1 and (not math.isfinite(q) or q < np.float64(1.0) / np.float64(max_depth_ratio) or q > max_depth_ratio):
                    out[i]["reason"] = 5
                else:
                    out[i] = (L[0], L[1], L[2], 1, 0)
    return out


def rows_points(pm, X, Y, Z, tr, cal):
    """refit_oracle.rows with the points given: J [4 n][6], the weighted residuals [4 n], the weights [n]"""
    f, cu, cv, base = np.float64(cal.f), np.float64(cal.cu), np.float64(cal.cv), np.float64(cal.base)
    rx, ry, rz = float(tr[0]), float(tr[1]), float(tr[2])
    tx, ty, tz = np.float64(tr[3]), np.float64(tr[4]), np.float64(tr[5])
    sx, cx, sy, cy, sz, cz = (np.float64(v) for v in (math.sin(rx), math.cos(rx), math.sin(ry), math.cos(ry), math.sin(rz), math.cos(rz)))
    r = [[+cy * cz, -cy * sz, +sy], [+sx * sy * cz + cx * sz, -sx * sy * sz + cx * cz, -sx * cy],
         [-cx * sy * cz + sx * sz, +cx * sy * sz + sx * cz, +cx * cy]]
    drx = [None, [+cx * sy * cz - sx * sz, -cx * sy * sz - sx * cz, -cx * cy], [+sx * sy * cz + cx * sz, -sx * sy * sz + cx * cz, -sx * cy]]
    dry = [[-sy * cz, +sy * sz, +cy], [+sx * cy * cz, -sx * cy * sz, +sx * sy], [-cx * cy * cz, +cx * cy * sz, -cx * sy]]
    drz = [[-cy * sz, -cy * cz], [-sx * sy * sz + cx * cz, -sx * sy * cz - cx * sz], [+cx * sy * sz + sx * cz, +cx * sy * cz - sx * sz]]
    n = len(pm)
    with np.errstate(all="ignore"):
        obs = [np.asarray(pm[k], np.float32).astype(np.float64) for k in ("u1c", "v1c", "u2c", "v2c")]
        X1c = r[0][0] * X + r[0][1] * Y + r[0][2] * Z + tx
        Y1c = r[1][0] * X + r[1][1] * Y + r[1][2] * Z + ty
        Z1c = r[2][0] * X + r[2][1] * Y + r[2][2] * Z + tz
        weight = np.ones(n)
        if cal.reweighting:
            weight = 1.0 / (np.abs(obs[0] - cu) / abs(cu) + 0.05)
        X2c = X1c - base
        zero, one = np.zeros(n), np.ones(n)
        deriv = [(zero, drx[1][0] * X + drx[1][1] * Y + drx[1][2] * Z, drx[2][0] * X + drx[2][1] * Y + drx[2][2] * Z),
                 tuple(dry[k][0] * X + dry[k][1] * Y + dry[k][2] * Z for k in range(3)),
                 tuple(drz[k][0] * X + drz[k][1] * Y for k in range(3)),
                 (one, zero, zero), (zero, one, zero), (zero, zero, one)]
        J = np.zeros((4 * n, 6))
        for j, (X1cd, Y1cd, Z1cd) in enumerate(deriv):
            J[0::4, j] = weight * f * (X1cd * Z1c - X1c * Z1cd) / (Z1c * Z1c)
            J[1::4, j] = weight * f * (Y1cd * Z1c - Y1c * Z1cd) / (Z1c * Z1c)
            J[2::4, j] = weight * f * (X1cd * Z1c - X2c * Z1cd) / (Z1c * Z1c)
            J[3::4, j] = weight * f * (Y1cd * Z1c - Y1c * Z1cd) / (Z1c * Z1c)
        p = (f * X1c / Z1c + cu, f * Y1c / Z1c + cv, f * X2c / Z1c + cu, f * Y1c / Z1c + cv)
        res = np.zeros(4 * n)
        for k in range(4):
            res[k::4] = weight * (obs[k] - p[k])
    return J, res, weight


def refit(pm, prior, tr, cal, ok=True):
    """refit_oracle.refit over the points of `prior` -> (tr [6], ok, n_updates, steps)"""
    X, Y, Z = (np.asarray(prior[k], np.float64) for k in ("X", "Y", "Z"))
    saved = ro.rows
    ro.rows = lambda pm_, tr_, cal_: rows_points(pm_, X, Y, Z, tr_, cal_)   # (refit passes every record, in list order)
    try:
        return ro.refit(pm, tr, cal, ok=ok)
    finally:
        ro.rows = saved
