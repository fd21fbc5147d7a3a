"""Scene points restated in numpy: the contract of vh_scene_points_stereo / vh_scene_points_mono,
operation for operation, in double (T = np.float64, what the device computes) and in np.longdouble (the yardstick of the
double form's own error).  numpy neither contracts nor reassociates, so every product and sum rounds on its own as in
the kernels, which are built with -ffp-contract=off.

The mono form takes the triangulated direction of a record from the pinned decomposition (mono_pose_oracle.triangulate,
double only -- there is no wider form of it); what follows it -- the division by w, the reprojections, the scale, R X + t,
Tw -- is restated in T."""
import numpy as np

import mono_inlier_oracle as mo
import mono_pose_oracle as mp

F32, F64 = np.float32, np.float64
POINT = np.dtype([("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("sigma_z", "<f4"), ("err", "<f4"), ("src_pos", "<i4"), ("i1p", "<i4"), ("i1c", "<i4")])
FLOATS = ("x", "y", "z", "sigma_z", "err")


def params(frame=1, min_disp=0.0, max_depth=0.0, max_err=0.0):
    return dict(frame=frame, min_disp=F32(min_disp), max_depth=F64(max_depth), max_err=F64(max_err))


def rotation(tr, T=F64):
    """ego_rot's r[9] (csrc/vh_ego.h)"""
    rx, ry, rz = (T(v) for v in tr[:3])
    sx, cx, sy, cy, sz, cz = np.sin(rx), np.cos(rx), np.sin(ry), np.cos(ry), np.sin(rz), np.cos(rz)
    return [+cy * cz, -cy * sz, +sy,
            +sx * sy * cz + cx * sz, -sx * sy * sz + cx * cz, -sx * cy,
            -cx * sy * cz + sx * sz, +cx * sy * sz + sx * cz, +cx * cy]


def _finish(out, x, y, z, sigma, err, sp, Tw, T, extra_drop=None):
    """the shared filters, Tw, the one rounding to float -> the result dict"""
    with np.errstate(all="ignore"):
        keep = np.isfinite(x) & np.isfinite(y) & np.isfinite(z) & np.isfinite(err) & (z > 0)
        margin = np.inf
        for lim, val in ((T(sp["max_depth"]), z), (T(sp["max_err"]), err)):
            if lim > 0:
                keep &= ~(val > lim)
                near = np.abs(val[np.isfinite(val)] - lim) / lim
                margin = min(margin, float(near.min())) if len(near) else margin
        if extra_drop is not None:
            keep &= ~extra_drop[0]
            margin = min(margin, extra_drop[1])
        cam = np.stack([x, y, z], axis=1)
        if Tw is not None:
            M = np.asarray(Tw, F64).reshape(4, 4).astype(T)
            x, y, z = (M[r, 0] * x + M[r, 1] * y + M[r, 2] * z + M[r, 3] for r in range(3))
        vals = [x, y, z, sigma, err]
        f32 = [v.astype(F32) for v in vals]
        for v in f32:
            keep &= np.isfinite(v)
    pts = np.zeros(int(keep.sum()), POINT)
    for name, v in zip(FLOATS, f32):
        pts[name] = v[keep]
    pts["src_pos"] = np.nonzero(keep)[0]
    pts["i1p"] = out["i1p"][keep]; pts["i1c"] = out["i1c"][keep]
    wide = np.stack(vals, axis=1)[keep]
    return dict(points=pts, keep=keep, wide=wide, cam=cam[keep], margin=margin)


def _empty():
    return dict(points=np.zeros(0, POINT), keep=np.zeros(0, bool), wide=np.zeros((0, 5)), cam=np.zeros((0, 3)), margin=np.inf)


def stereo(pm, tr, cal, sp, Tw=None, ok=True, T=F64):
    """cal: f, cu, cv, base (attributes).  -> dict(points POINT [k], keep [n], wide [k, 5] in T, cam [k, 3], margin)"""
    if not ok or len(pm) == 0:
        r = _empty(); r["keep"] = np.zeros(len(pm), bool)
        return r
    f, cu, cv, base = T(cal.f), T(cal.cu), T(cal.cv), T(cal.base)
    u1p, v1p, u2p, u1c, v1c, u2c, v2c = (pm[k].astype(F32) for k in ("u1p", "v1p", "u2p", "u1c", "v1c", "u2c", "v2c"))
    with np.errstate(all="ignore"):
        df0 = u1p - u2p                                   # float
        df = np.where(df0 < F32(0.0001), F32(0.0001), df0)   # (a NaN difference stays NaN)
        d = df.astype(T)
        X = (u1p.astype(T) - cu) * base / d
        Y = (v1p.astype(T) - cv) * base / d
        Z = f * base / d
        r = rotation(tr, T)
        t = [T(v) for v in tr[3:]]
        X1 = r[0] * X + r[1] * Y + r[2] * Z + t[0]
        Y1 = r[3] * X + r[4] * Y + r[5] * Z + t[1]
        Z1 = r[6] * X + r[7] * Y + r[8] * Z + t[2]
        X2 = X1 - base
        p = [f * X1 / Z1 + cu, f * Y1 / Z1 + cv, f * X2 / Z1 + cu, f * Y1 / Z1 + cv]
        d0, d1, d2, d3 = u1c.astype(T) - p[0], v1c.astype(T) - p[1], u2c.astype(T) - p[2], v2c.astype(T) - p[3]
        err = np.sqrt(d0 * d0 + d1 * d1 + d2 * d2 + d3 * d3)
        x, y, z = (X, Y, Z) if sp["frame"] == 0 else (X1, Y1, Z1)
        sigma = z * z / (f * base)
        extra = None
        if sp["min_disp"] > 0:
            lim = T(F32(sp["min_disp"]))
            dd = df0.astype(T)
            near = np.abs(dd[np.isfinite(dd)] - lim) / lim
            extra = (dd < lim, float(near.min()) if len(near) else np.inf)
    return _finish(pm, x, y, z, sigma, err, sp, Tw, T, extra)


def projections(pose, e):
    """P1 = K [I | 0], P2 = K [R | t] by the statements of mono_pose_candidates"""
    K = np.array([[e.f, 0, e.cu], [0, e.f, e.cv], [0, 0, 1]], F64)
    R = np.asarray(pose["R"], F64).reshape(3, 3); t = np.asarray(pose["t"], F64)
    P1 = np.hstack([K, np.zeros((3, 1))])
    P2 = mo.matmul(K, np.hstack([R, t.reshape(3, 1)]))
    return P1, P2, R, t


def mono(svd, pm, pose, e, sp, Tw=None, ok=True, T=F64):
    """pose: R [9], t [3], scale; e: f, cu, cv (attributes).  The result of stereo(), and raw [k, 3]: the points before the
    scale, in double."""
    if not ok or len(pm) == 0:
        r = _empty(); r["keep"] = np.zeros(len(pm), bool); r["raw"] = np.zeros((0, 3))
        return r
    P1, P2, R, t = projections(pose, e)
    X, _ = mp.triangulate(svd, pm, P1, P2)
    with np.errstate(all="ignore"):
        w = X[:, 3]
        P = np.where((w != 0)[:, None], X[:, :3] / w[:, None], 0.0)     # (double: the device's division)
        raw = P.copy()
        x, y, z = (P[:, k].astype(T) for k in range(3))
        one = np.ones_like(x)
        proj = []
        for M in (P1.astype(T), P2.astype(T)):
            rows = []
            for i in range(3):
                s = T(0.0) + M[i, 0] * x
                s = s + M[i, 1] * y
                s = s + M[i, 2] * z
                s = s + M[i, 3] * one
                rows.append(s)
            proj.append(rows)
        u1p, v1p, u1c, v1c = (pm[k].astype(F32).astype(T) for k in ("u1p", "v1p", "u1c", "v1c"))
        d0 = u1p - proj[0][0] / proj[0][2]; d1 = v1p - proj[0][1] / proj[0][2]
        d2 = u1c - proj[1][0] / proj[1][2]; d3 = v1c - proj[1][1] / proj[1][2]
        err = np.sqrt(d0 * d0 + d1 * d1 + d2 * d2 + d3 * d3)
        scale = T(pose["scale"])
        if sp["frame"] == 0:
            xs, ys, zs = x * scale, y * scale, z * scale
        else:
            Rt, tt = R.astype(T), t.astype(T)
            xs, ys, zs = ((Rt[r, 0] * x + Rt[r, 1] * y + Rt[r, 2] * z + tt[r]) * scale for r in range(3))
        sigma = np.zeros_like(xs)
    out = _finish(pm, xs, ys, zs, sigma, err, sp, Tw, T)
    out["raw"] = raw[out["keep"]]
    return out


def deviation(a, b):
    """the largest difference of a's x, y, z, err from b's, relative to the point's norm (b: the wider form)"""
    if len(a["wide"]) == 0:
        return 0.0
    assert np.array_equal(a["keep"], b["keep"])
    wa, wb = a["wide"].astype(np.longdouble), b["wide"].astype(np.longdouble)
    norm = np.sqrt((wb[:, :3] ** 2).sum(axis=1))
    return float((np.abs(wa[:, [0, 1, 2, 4]] - wb[:, [0, 1, 2, 4]]).max(axis=1) / norm).max())


def float_differences(a, b):
    """-> (float values that differ, float values compared, the largest difference in float ulps)"""
    pa, pb = a["points"], b["points"]
    assert len(pa) == len(pb)
    differ = total = 0
    worst = 0
    for name in FLOATS:
        ia, ib = ordered(pa[name]), ordered(pb[name])
        dd = np.abs(ia - ib)
        differ += int((dd != 0).sum()); total += len(dd)
        worst = max(worst, int(dd.max()) if len(dd) else 0)
    return differ, total, worst


def ordered(f):
    """float32 -> int64 keys in which neighbouring floats differ by one"""
    i = np.ascontiguousarray(f, F32).view(np.int32).astype(np.int64)
    return np.where(i < 0, -(i & 0x7FFFFFFF), i)
