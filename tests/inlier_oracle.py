"""VisualOdometryStereo::getInlier (reference src/viso_stereo.cpp:159-177) restated in numpy for any quad list and any
tr[6]: what vh_motion_inliers computes.  math.sin / math.cos per list, float32 for the disparity, float64 elsewhere;
every product and sum is an operation of its own, in the reference's order (numpy never fuses a*b+c).

    flags, sums = inliers(pm, tr, cal)      cal: anything with f, cu, cv, base, inlier_threshold
    flags[i] = sums[i] < inlier_threshold**2     (strict; a NaN or infinite sum is not an inlier)"""
import math

import numpy as np


def rotation(tr):
    """r00 .. r22 as src/viso_stereo.cpp:244-250."""
    rx, ry, rz = float(tr[0]), float(tr[1]), float(tr[2])
    sx, cx, sy, cy, sz, cz = math.sin(rx), math.cos(rx), math.sin(ry), math.cos(ry), math.sin(rz), math.cos(rz)
    return (+cy * cz, -cy * sz, +sy,
            +sx * sy * cz + cx * sz, -sx * sy * sz + cx * cz, -sx * cy,
            -cx * sy * cz + sx * sz, +cx * sy * sz + sx * cz, +cx * cy)


def squared_sums(pm, tr, cal):
    """The sum of the four squared reprojection differences per record, added left to right (float64)."""
    f, cu, cv, base = np.float64(cal.f), np.float64(cal.cu), np.float64(cal.cv), np.float64(cal.base)
    r00, r01, r02, r10, r11, r12, r20, r21, r22 = (np.float64(v) for v in rotation(tr))
    tx, ty, tz = np.float64(tr[3]), np.float64(tr[4]), np.float64(tr[5])
    u1p, v1p, u2p = (np.asarray(pm[k], np.float32) for k in ("u1p", "v1p", "u2p"))
    with np.errstate(all="ignore"):
        df = u1p - u2p                                              # float (:83)
        df = np.where(df < np.float32(0.0001), np.float32(0.0001), df)   # std::max(df, 0.0001f): a NaN stays
        d = df.astype(np.float64)
        X = (u1p.astype(np.float64) - cu) * base / d                # (:84-86)
        Y = (v1p.astype(np.float64) - cv) * base / d
        Z = f * base / d
        X1c = r00 * X + r01 * Y + r02 * Z + tx                      # (:274-276)
        Y1c = r10 * X + r11 * Y + r12 * Z + ty
        Z1c = r20 * X + r21 * Y + r22 * Z + tz
        X2c = X1c - base
        p = (f * X1c / Z1c + cu, f * Y1c / Z1c + cv, f * X2c / Z1c + cu, f * Y1c / Z1c + cv)   # (:317-321)
        obs = tuple(np.asarray(pm[k], np.float32).astype(np.float64) for k in ("u1c", "v1c", "u2c", "v2c"))
        dd = [o - q for o, q in zip(obs, p)]
        return dd[0] * dd[0] + dd[1] * dd[1] + dd[2] * dd[2] + dd[3] * dd[3]  # (:171-174)


def inliers(pm, tr, cal, ok=True):
    """-> (flags uint8 [n], sums float64 [n]); ok = False: no inliers (the sums are still those under tr)."""
    sums = squared_sums(pm, tr, cal)
    thr = np.float64(cal.inlier_threshold)
    with np.errstate(invalid="ignore"):
        flags = (sums < thr * thr).astype(np.uint8)
    if not ok:
        flags[:] = 0
    return flags, sums


def near_threshold(sums, cal, rel):
    """Records whose sum lies within relative `rel` of inlier_threshold^2."""
    t2 = float(cal.inlier_threshold) ** 2
    with np.errstate(invalid="ignore"):
        return np.abs(sums - t2) <= rel * t2
