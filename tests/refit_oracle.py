"""VisualOdometryStereo::updateParameters (reference src/viso_stereo.cpp:179-224, with computeObservations and
computeResidualsAndJacobian, :226-327) and the "final optimization" loop around it (:126-139), restated in numpy for any
quad list: what vh_refit_motion computes.  math.sin / math.cos per update, float32 for the disparity, float64 elsewhere;
every product and sum is an operation of its own (numpy never fuses a*b+c), the sums over the rows run sequentially in
the reference's order (np.cumsum adds left to right; np.sum would add pairwise), the solve is
reconstruction_oracle.matrix_solve.

    result, tr, step = update_parameters(pm, active, tr, eps, cal)     cal: anything with f, cu, cv, base, reweighting
    tr, ok, n_updates, steps = refit(pm, tr, cal)                      steps[k]: the largest |b| of update k
    ok, tr, inliers = estimate_motion(pm, samples, cal)                the whole estimateMotion (cal.inlier_threshold too)"""
import math

import numpy as np

import inlier_oracle as io
from reconstruction_oracle import matrix_solve

UPDATED, FAILED, CONVERGED = 0, 1, 2


def _seq_sum(x):
    """a = 0; for v in x: a += v"""
    return float(np.cumsum(np.concatenate(([0.0], x)))[-1])


def rows(pm, tr, cal):
    """J [4 n][6], the weighted residuals [4 n] and the weights [n] of all records under tr (:237-327)."""
    f, cu, cv, base = np.float64(cal.f), np.float64(cal.cu), np.float64(cal.cv), np.float64(cal.base)
    rx, ry, rz = float(tr[0]), float(tr[1]), float(tr[2])
    tx, ty, tz = np.float64(tr[3]), np.float64(tr[4]), np.float64(tr[5])
    sx, cx, sy, cy, sz, cz = (np.float64(v) for v in (math.sin(rx), math.cos(rx), math.sin(ry), math.cos(ry), math.sin(rz), math.cos(rz)))
    r00 = +cy * cz; r01 = -cy * sz; r02 = +sy
    r10 = +sx * sy * cz + cx * sz; r11 = -sx * sy * sz + cx * cz; r12 = -sx * cy
    r20 = -cx * sy * cz + sx * sz; r21 = +cx * sy * sz + sx * cz; r22 = +cx * cy
    rdrx10 = +cx * sy * cz - sx * sz; rdrx11 = -cx * sy * sz - sx * cz; rdrx12 = -cx * cy
    rdrx20 = +sx * sy * cz + cx * sz; rdrx21 = -sx * sy * sz + cx * cz; rdrx22 = -sx * cy
    rdry00 = -sy * cz; rdry01 = +sy * sz; rdry02 = +cy
    rdry10 = +sx * cy * cz; rdry11 = -sx * cy * sz; rdry12 = +sx * sy
    rdry20 = -cx * cy * cz; rdry21 = +cx * cy * sz; rdry22 = -cx * sy
    rdrz00 = -cy * sz; rdrz01 = -cy * cz
    rdrz10 = -sx * sy * sz + cx * cz; rdrz11 = -sx * sy * cz - cx * sz
    rdrz20 = +cx * sy * sz + sx * cz; rdrz21 = +cx * sy * cz - sx * sz
    u1p, v1p, u2p = (np.asarray(pm[k], np.float32) for k in ("u1p", "v1p", "u2p"))
    n = len(u1p)
    with np.errstate(all="ignore"):
        df = u1p - u2p                                                    # float (:83)
        df = np.where(df < np.float32(0.0001), np.float32(0.0001), df)    # std::max(df, 0.0001f): a NaN stays
        d = df.astype(np.float64)
        X = (u1p.astype(np.float64) - cu) * base / d                      # (:84-86)
        Y = (v1p.astype(np.float64) - cv) * base / d
        Z = f * base / d
        obs = [np.asarray(pm[k], np.float32).astype(np.float64) for k in ("u1c", "v1c", "u2c", "v2c")]
        X1c = r00 * X + r01 * Y + r02 * Z + tx                            # (:274-276)
        Y1c = r10 * X + r11 * Y + r12 * Z + ty
        Z1c = r20 * X + r21 * Y + r22 * Z + tz
        weight = np.ones(n)
        if cal.reweighting:
            weight = 1.0 / (np.abs(obs[0] - cu) / abs(cu) + 0.05)         # (:279-281)
        X2c = X1c - base
        zero, one = np.zeros(n), np.ones(n)
        deriv = [(zero, rdrx10 * X + rdrx11 * Y + rdrx12 * Z, rdrx20 * X + rdrx21 * Y + rdrx22 * Z),
                 (rdry00 * X + rdry01 * Y + rdry02 * Z, rdry10 * X + rdry11 * Y + rdry12 * Z, rdry20 * X + rdry21 * Y + rdry22 * Z),
                 (rdrz00 * X + rdrz01 * Y, rdrz10 * X + rdrz11 * Y, rdrz20 * X + rdrz21 * Y),
                 (one, zero, zero), (zero, one, zero), (zero, zero, one)]
        J = np.zeros((4 * n, 6))
        for j, (X1cd, Y1cd, Z1cd) in enumerate(deriv):                    # (:309-312)
            J[0::4, j] = weight * f * (X1cd * Z1c - X1c * Z1cd) / (Z1c * Z1c)
            J[1::4, j] = weight * f * (Y1cd * Z1c - Y1c * Z1cd) / (Z1c * Z1c)
            J[2::4, j] = weight * f * (X1cd * Z1c - X2c * Z1cd) / (Z1c * Z1c)
            J[3::4, j] = weight * f * (Y1cd * Z1c - Y1c * Z1cd) / (Z1c * Z1c)
        p = (f * X1c / Z1c + cu, f * Y1c / Z1c + cv, f * X2c / Z1c + cu, f * Y1c / Z1c + cv)   # (:316-319)
        res = np.zeros(4 * n)
        for k in range(4):
            res[k::4] = weight * (obs[k] - p[k])                          # (:322-325)
    return J, res, weight


def normal_equations(J, res):
    """A [6][6], B [6] as :194-207: every entry a sequential sum over the rows."""
    with np.errstate(all="ignore"):
        A = [[_seq_sum(J[:, m] * J[:, n]) for n in range(6)] for m in range(6)]
        B = [_seq_sum(J[:, m] * res) for m in range(6)]
    return A, B


def update_parameters(pm, active, tr, eps, cal):
    """-> (result, tr after the update, largest |b| or None).  step_size is 1 at both of the reference's call sites."""
    active = np.asarray(active, np.int64)
    tr = [float(v) for v in tr]
    if len(active) < 3:
        return FAILED, tr, None
    J, res, _ = rows(pm[active], tr, cal)
    A, B = normal_equations(J, res)
    Bm = [[b] for b in B]
    if not matrix_solve(A, Bm):
        return FAILED, tr, None
    converged = True
    step = 0.0
    for m in range(6):
        b = Bm[m][0]
        tr[m] += 1.0 * b
        if abs(b) > eps:
            converged = False
        step = max(step, abs(b)) if b == b else float("nan")
    return (CONVERGED if converged else UPDATED), tr, step


def refit(pm, tr, cal, ok=True):
    """The loop of :126-139 on every record of pm from tr -> (tr [6], ok, n_updates, steps)."""
    zero = np.zeros(6)
    if not ok or len(pm) < 6:
        return zero, False, 0, []
    active = np.arange(len(pm))
    it, steps = 0, []
    result = UPDATED
    while result == UPDATED:
        result, tr, step = update_parameters(pm, active, tr, 1e-8, cal)
        steps.append(step)
        it += 1
        if it - 1 > 100 or result == CONVERGED:
            break
    if result != CONVERGED:
        return zero, False, len(steps), steps
    return np.array(tr, np.float64), True, len(steps), steps


def estimate_motion(pm, samples, cal):
    """estimateMotion (:54-157) with given samples [iters][3] -> (ok, tr [6], inlier indices)."""
    if len(pm) < 6:
        return False, np.zeros(6), np.zeros(0, np.int32)
    best, best_tr = np.zeros(0, np.int64), None
    for active in samples:
        tr = [0.0] * 6
        it, result = 0, UPDATED
        while result == UPDATED:
            result, tr, _ = update_parameters(pm, active, tr, 1e-6, cal)
            it += 1
            if it - 1 > 20 or result == CONVERGED:
                break
        if result != FAILED:
            inl = np.flatnonzero(io.inliers(pm, tr, cal)[0])
            if len(inl) > len(best):
                best, best_tr = inl, tr
    if len(best) < 6:
        return False, np.zeros(6), best.astype(np.int32)
    tr, ok, _, _ = refit(pm[best], best_tr, cal)
    return ok, tr, best.astype(np.int32)


def cost(pm, tr, cal):
    """The sum of the squared weighted residuals under tr."""
    _, res, _ = rows(pm, tr, cal)
    return float(np.sum(res * res))
