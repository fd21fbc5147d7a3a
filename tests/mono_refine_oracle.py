"""The mono pose refinement (vh_pose_mono_refined) restated in numpy, in float64 and in longdouble:
Gauss-Newton on the signed Sampson distance of EVERY record over (R, unit t) from the winner of vh_pose_mono's chirality
counts, the covariance of the refined pose, the scale tail under the refined pose.  Neither the reference nor stock
libviso2 has a counterpart; the contract is include/viso_hip.h's, term by term, and csrc/vh_mono_refine.h is its C form.

Every product and sum is an operation of its own, bracketed as the header brackets it (numpy never fuses a*b+c); the sums
over the records are sequential from the first record (np.cumsum adds left to right) -- the device adds in another, fixed
order, which is what the bound of tests/test_mono_pose_refined.py allows for.  Steps 1-3 (the start) and 4-7 (the tail)
are tests/mono_pose_oracle.py's, in float64 in both forms; ft = np.longdouble carries steps 2-6 of the refinement in long
double from the same float64 start.

    res, ref = refine(svd, pm, model, e, ok=True, ft=np.float64)
    res: what mono_pose_oracle.pose returns (under the refined pose where ref["status"] == 0, else that call's own result)
    ref: dict(status, n_updates, R [9], t [3], B [6], cov [25], ssr_start, ssr, moved_R, moved_t, steps [max |delta| per update])
"""
import numpy as np

import mono_inlier_oracle as mo
import mono_pose_oracle as mp
from reconstruction_oracle import matrix_solve

F64 = np.float64
NP, MAX_UPDATES, STEP_TOL = 5, 102, 1e-8


def matmul(A, B, ft):
    """Matrix::operator*: every element a sum from 0, k ascending"""
    C = np.zeros((A.shape[0], B.shape[1]), ft)
    for i in range(A.shape[0]):
        for j in range(B.shape[1]):
            c = ft(0)
            for k in range(A.shape[1]):
                c = c + A[i, k] * B[k, j]
            C[i, j] = c
    return C


def skew(v, ft):
    z = ft(0)
    return np.array([[z, -v[2], v[1]], [v[2], z, -v[0]], [-v[1], v[0], z]], ft)


def basis(t, ft):
    """-> B [6]: b0, b1"""
    m = 0
    if abs(t[1]) < abs(t[0]):
        m = 1
    if abs(t[2]) < abs(t[m]):
        m = 2
    with np.errstate(all="ignore"):
        v = np.array([(ft(1) if q == m else ft(0)) - t[m] * t[q] for q in range(3)], ft)
        nv = np.sqrt((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2])
        b0 = v / nv
        b1 = np.array([t[1] * b0[2] - t[2] * b0[1], t[2] * b0[0] - t[0] * b0[2], t[0] * b0[1] - t[1] * b0[0]], ft)
    return np.concatenate([b0, b1])


def uniforms(R, t, ft):
    """-> (U [6, 9]: E and the five E_k, B [6])"""
    with np.errstate(all="ignore"):
        T = skew(t, ft)
        U = [matmul(T, R, ft)]
        for k in range(3):
            G = skew(np.eye(3, dtype=ft)[k], ft)
            U.append(matmul(T, matmul(G, R, ft), ft))
        B = basis(t, ft)
        for k in range(2):
            U.append(matmul(skew(B[3 * k:3 * k + 3], ft), R, ft))
    return np.stack([u.reshape(9) for u in U]), B


def records(pm, e, ft):
    f, cu, cv = ft(e.f), ft(e.cu), ft(e.cv)
    with np.errstate(all="ignore"):
        return ((pm["u1p"].astype(ft) - cu) / f, (pm["v1p"].astype(ft) - cv) / f, (pm["u1c"].astype(ft) - cu) / f, (pm["v1c"].astype(ft) - cv) / f)


def forms(M, x):
    xp0, xp1, xc0, xc1 = x
    a0 = (M[0] * xp0 + M[1] * xp1) + M[2]
    a1 = (M[3] * xp0 + M[4] * xp1) + M[5]
    a2 = (M[6] * xp0 + M[7] * xp1) + M[8]
    b0 = (M[0] * xc0 + M[3] * xc1) + M[6]
    b1 = (M[1] * xc0 + M[4] * xc1) + M[7]
    n = (xc0 * a0 + xc1 * a1) + a2
    return n, a0, a1, b0, b1


def residuals(U, x, f, ft):
    """-> (r [n], J [n, 5])"""
    f, two = ft(f), ft(2)
    with np.errstate(all="ignore"):
        n, a0, a1, b0, b1 = forms(U[0], x)
        s = ((a0 * a0 + a1 * a1) + b0 * b0) + b1 * b1
        q = np.sqrt(s)
        r = (f * n) / q
        den = (two * s) * q
        J = []
        for k in range(NP):
            dn, da0, da1, db0, db1 = forms(U[1 + k], x)
            ds = two * (((a0 * da0 + a1 * da1) + b0 * db0) + b1 * db1)
            J.append(f * (dn / q - (n * ds) / den))
    return r, np.stack(J, axis=1)


def accumulate(r, J, ft):
    """-> acc [21]: J^T J (upper triangle by rows), J^T r, r^2; sequential sums"""
    with np.errstate(all="ignore"):
        cols = [J[:, i] * J[:, j] for i in range(NP) for j in range(i, NP)] + [J[:, i] * r for i in range(NP)] + [r * r]
        return np.array([np.cumsum(c.astype(ft))[-1] for c in cols], ft)


def full(acc, ft):
    A = np.zeros((NP, NP), ft)
    k = 0
    for i in range(NP):
        for j in range(i, NP):
            A[i, j] = A[j, i] = acc[k]; k += 1
    return A


def solve(A, B, ft):
    """Matrix::solve -> the solutions [n, nb] or None"""
    a = [[ft(v) for v in row] for row in A]
    b = [[ft(v) for v in row] for row in B]
    with np.errstate(all="ignore"):
        if not matrix_solve(a, b):
            return None
    return np.array(b, ft)


def step(delta, R, t, ft):
    with np.errstate(all="ignore"):
        w = delta[:3]
        th2 = (w[0] * w[0] + w[1] * w[1]) + w[2] * w[2]
        th = np.sqrt(th2)
        W = skew(w, ft)
        eye = np.eye(3, dtype=ft)
        if th < 1e-12:
            X = eye + W
        else:
            W2 = matmul(W, W, ft)
            h = np.sin(ft(0.5) * th)
            ca, cb = np.sin(th) / th, (ft(2) * (h * h)) / th2
            X = (eye + ca * W) + cb * W2
        Rn = matmul(X, R, ft)
        B = basis(t, ft)
        u = (t + delta[3] * B[:3]) + delta[4] * B[3:]
        nu = np.sqrt((u[0] * u[0] + u[1] * u[1]) + u[2] * u[2])
        return Rn, u / nu


def angle(a, b, ft):
    a, b = np.asarray(a, ft).reshape(-1), np.asarray(b, ft).reshape(-1)
    d2 = ft(0)
    for q in range(len(a)):
        d = a[q] - b[q]
        d2 = d2 + d * d
    chord = ft(2) * np.sqrt(ft(2)) if len(a) == 9 else ft(2)
    return ft(2) * np.arcsin(min(ft(1), np.sqrt(d2) / chord))


def tangent(t_ref, t):
    """the direction t in the tangent coordinates (tau0, tau1) of the basis at t_ref (first order)"""
    B = basis(np.asarray(t_ref, F64), F64)
    d = np.asarray(t, F64) - np.asarray(t_ref, F64)
    return np.array([B[:3] @ d, B[3:] @ d])


def gauss_newton(pm, e, R0, t0, ft=F64):
    """Steps 2-6 from the start (R0, t0) -> ref (see the module's text); R, t are the state the loop ended in."""
    x = records(pm, e, ft)
    R, t = np.asarray(R0, ft).reshape(3, 3).copy(), np.asarray(t0, ft).copy()
    out = dict(status=0, n_updates=0, B=np.zeros(6, ft), cov=np.zeros(25, ft), ssr_start=ft(0), ssr=ft(0), moved_R=ft(0), moved_t=ft(0), steps=[])
    status, updates, converged = 0, 0, False
    while True:
        U, B = uniforms(R, t, ft)
        acc = accumulate(*residuals(U, x, e.f, ft), ft)
        if updates == 0 and not converged and np.isfinite(acc[20]):
            out["ssr_start"] = acc[20]
        if not np.isfinite(acc).all():
            status = 4; break
        A = full(acc, ft)
        if converged:
            inv = solve(A, np.eye(NP, dtype=ft), ft)
            if inv is None:
                status = 2; break
            with np.errstate(all="ignore"):
                sigma2 = acc[20] / ft(len(pm) - NP)
                cov = np.zeros((NP, NP), ft)
                for i in range(NP):
                    for j in range(i, NP):
                        cov[i, j] = cov[j, i] = sigma2 * inv[i, j]
            if not np.isfinite(cov).all():
                status = 4; break
            out.update(cov=cov.reshape(25), ssr=acc[20], B=B)
            break
        sol = solve(A, acc[15:20].reshape(NP, 1), ft)
        if sol is None:
            status = 2; break
        delta = -sol[:, 0]
        R, t = step(delta, R, t, ft)
        updates += 1
        with np.errstate(all="ignore"):
            out["steps"].append(float(np.abs(delta).max()))
            small = bool((np.abs(delta) < STEP_TOL).all())
        if not (np.isfinite(R).all() and np.isfinite(t).all()):
            status = 4; break
        if small:
            converged = True
        elif updates >= MAX_UPDATES:
            status = 3; break
    out.update(status=status, n_updates=updates, R=R.reshape(9), t=t)
    if status == 0:
        out.update(moved_R=angle(R, R0, ft), moved_t=angle(t, t0, ft))
    else:
        out.update(cov=np.zeros(25, ft), ssr=ft(0), B=np.zeros(6, ft))
    return out


def tail(svd, pm, e, P1, R, t, counts, cbest):
    """Steps 4-7 of mono_pose_oracle.pose under (R [9], t): the winner's projection matrix is K [R | t]."""
    R = np.asarray(R, F64).reshape(9); t = np.asarray(t, F64)
    K = np.array([[e.f, 0, e.cu], [0, e.f, e.cv], [0, 0, 1]], F64)
    P2 = mo.matmul(K, np.hstack([R.reshape(3, 3), t.reshape(3, 1)]))
    X, _ = mp.triangulate(svd, pm, P1, P2)
    dist, d = mp.front_points(X, e.pitch)
    known = dict(chirality=counts, candidate=cbest, n_front=len(dist), R=R.copy(), t=t.copy())
    if len(dist) < mp.MIN_RECORDS:
        return mp._result(4, **known)
    median = mp.median_by_rank(dist)
    known["median"] = float(median)
    if median > e.motion_threshold:
        return mp._result(5, **known)
    best, _, margin = mp.vote(d, median, e.motion_threshold)
    plane = d[best]
    known.update(plane=float(plane), margin=margin)
    if abs(plane) < 1e-20:
        return mp._result(6, **known)
    with np.errstate(all="ignore"):
        known["scale"] = float(F64(e.height) / plane)
        tt = (t * F64(e.height)) / plane
        ry = np.arcsin(R[2])
        tr = np.array([np.arcsin(-R[5] / np.cos(ry)), ry, np.arcsin(-R[1] / np.cos(ry)), tt[0], tt[1], tt[2]], F64)
    if not (np.isfinite(tr).all() and np.isfinite(R).all() and np.isfinite(t).all() and np.isfinite(median) and np.isfinite(plane)):
        return mp._result(7, **known)
    return mp._result(0, tr=tr, ok=True, **known)


def refine(svd, pm, model, e, ok=True, ft=F64, with_tail=True):
    """The whole contract.  with_tail=False: res is the unrefined pose's (for the long-double form, whose tail is not used)."""
    parts = {}
    base = mp.pose(svd, pm, model, e, ok=ok, parts=parts)
    if base["reason"] in (1, 2, 3):
        return base, dict(status=1, n_updates=0, R=np.zeros(9, ft), t=np.zeros(3, ft), B=np.zeros(6, ft), cov=np.zeros(25, ft), ssr_start=ft(0),
                          ssr=ft(0), moved_R=ft(0), moved_t=ft(0), steps=[])
    ref = gauss_newton(pm, e, base["R"], base["t"], ft)
    if ref["status"] != 0 or not with_tail:
        return base, ref
    return tail(svd, pm, e, parts["P1"], ref["R"].astype(F64), ref["t"].astype(F64), base["chirality"], base["candidate"]), ref
