"""The pose covariance's rule (include/viso_hip.h) in scalars, one row at a time, in the rule's own
order: G, Q = G C G^T, Ad, Sigma' = Ad (Sigma + Q) Ad^T, the fill rule -- in float64 (Python floats and the C library's
sin / cos: what the host build of csrc/vh_trajectory_cov.h is held to byte for byte, and the device where sin / cos are
exact) or in longdouble (what the float64 result is measured against).  Which rows step is trajectory_oracle's."""
import math

import numpy as np

import trajectory_oracle as to

HOLD, REPEAT = 0, 1
COV = np.dtype([("cov", "<f8", (6, 6)), ("status", "<i4"), ("step", "<i4"), ("n_filled", "<i4"), ("reserved", "<i4")])
CARRY = np.dtype([("cov", "<f8", (6, 6)), ("Ad_last", "<f8", (6, 6)), ("Q_last", "<f8", (6, 6)), ("n_filled", "<i4"), ("has_ad", "<i4"),
                  ("has_q", "<i4"), ("step", "<i4")])


def _scalar(ft):
    """float64 runs on Python floats: the same IEEE doubles, one rounding per operation, no numpy in the way"""
    return float if ft is np.float64 else ft


def rot(tr, ft=np.float64):
    """ego_rot of csrc/vh_ego.h -> (r, drx, dry, drz) as flat lists of 9"""
    f = _scalar(ft)
    rx, ry, rz = f(tr[0]), f(tr[1]), f(tr[2])
    if f is float:
        sx, cx, sy, cy, sz, cz = math.sin(rx), math.cos(rx), math.sin(ry), math.cos(ry), math.sin(rz), math.cos(rz)
    else:
        sx, cx, sy, cy, sz, cz = np.sin(rx), np.cos(rx), np.sin(ry), np.cos(ry), np.sin(rz), np.cos(rz)
    z = f(0)
    r = [+cy * cz, -cy * sz, +sy,
         +sx * sy * cz + cx * sz, -sx * sy * sz + cx * cz, -sx * cy,
         -cx * sy * cz + sx * sz, +cx * sy * sz + sx * cz, +cx * cy]
    drx = [z, z, z,
           +cx * sy * cz - sx * sz, -cx * sy * sz - sx * cz, -cx * cy,
           +sx * sy * cz + cx * sz, -sx * sy * sz + cx * cz, -sx * cy]
    dry = [-sy * cz, +sy * sz, +cy,
           +sx * cy * cz, -sx * cy * sz, +sx * sy,
           -cx * cy * cz, +cx * cy * sz, -cx * sy]
    drz = [-cy * sz, -cy * cz, z,
           -sx * sy * sz + cx * cz, -sx * sy * cz - cx * sz, z,
           +cx * sy * sz + sx * cz, +cx * sy * cz - sx * sz, z]
    return r, drx, dry, drz


def dot6(a, b, zero):
    c = zero
    for k in range(6):
        c = c + a[k] * b[k]
    return c


def row(tr, C, ok_cov, ft=np.float64):
    """Steps 1 - 3 for an accepted row -> (Ad 6x6, Q 6x6 symmetric, own)"""
    f = _scalar(ft)
    z = f(0)
    r, drx, dry, drz = rot(tr, ft)
    t = [f(tr[3]), f(tr[4]), f(tr[5])]
    G = [[z] * 6 for _ in range(6)]
    for k, dR in enumerate((drx, dry, drz)):
        w21 = w02 = w10 = z
        for m in range(3):
            w21 = w21 + r[3 * m + 2] * dR[3 * m + 1]
            w02 = w02 + r[3 * m + 0] * dR[3 * m + 2]
            w10 = w10 + r[3 * m + 1] * dR[3 * m + 0]
        G[0][k], G[1][k], G[2][k] = w21, w02, w10
    for a in range(3):
        for b in range(3):
            G[3 + a][3 + b] = r[3 * b + a]
    Cm = [[f(x) for x in rw] for rw in np.asarray(C).reshape(6, 6)]
    fin = all(math.isfinite(float(x)) for rw in Cm for x in rw)
    Q = [[z] * 6 for _ in range(6)]
    for i in range(6):
        W = [dot6(G[i], [Cm[k][j] for k in range(6)], z) for j in range(6)]
        for j in range(i, 6):
            Q[i][j] = Q[j][i] = dot6(W, G[j], z)
            fin = fin and math.isfinite(float(Q[i][j]))
    tx = [[z, -t[2], t[1]], [t[2], z, -t[0]], [-t[1], t[0], z]]
    Ad = [[z] * 6 for _ in range(6)]
    for i in range(3):
        for j in range(3):
            c = z
            for m in range(3):
                c = c + tx[i][m] * r[3 * m + j]
            Ad[i][j] = r[3 * i + j]; Ad[3 + i][3 + j] = r[3 * i + j]; Ad[3 + i][j] = c
    return Ad, Q, bool(ok_cov != 0 and fin)


def step(Sigma, add, Ad, ft=np.float64):
    """Step 4: Ad (Sigma + add) Ad^T"""
    z = _scalar(ft)(0)
    S = [[Sigma[i][j] + add[i][j] for j in range(6)] for i in range(6)]
    U = [[dot6(Ad[i], [S[k][j] for k in range(6)], z) for j in range(6)] for i in range(6)]
    out = [[z] * 6 for _ in range(6)]
    for i in range(6):
        for j in range(i, 6):
            out[i][j] = out[j][i] = dot6(U[i], Ad[j], z)
    return out


def statuses(tr, ok):
    """the pose chain's status of every row (trajectory_oracle.inverse, float64)"""
    return [to.inverse(tr[r], int(ok[r]))[0] for r in range(len(tr))]


def chain(tr, ok, cov, ok_cov, S0=None, carry=None, on_fail=HOLD, fill_scale=1.0, ft=np.float64, status=None):
    """One chain of rows -> (records: dict cov [n, 6, 6] in ft, status, step, n_filled; the carry as a dict)"""
    f = _scalar(ft)
    z = f(0)
    n = len(tr)
    zero = [[z] * 6 for _ in range(6)]
    if carry is not None:
        c = dict(carry)
    else:
        Sg = zero if S0 is None else [[f(x) for x in rw] for rw in np.asarray(S0).reshape(6, 6)]
        c = dict(cov=Sg, Ad=None, Q=None, n_filled=0, step=0)
    Sg, Adl, Ql, n_filled, stp = c["cov"], c["Ad"], c["Q"], c["n_filled"], c["step"]
    status = statuses(tr, ok) if status is None else status
    out = np.zeros((n, 6, 6), np.float64 if f is float else ft)
    nf, steps = np.zeros(n, np.int32), np.zeros(n, np.int32)
    fs = f(fill_scale)
    with np.errstate(all="ignore"):
        for r in range(n):
            st = status[r]
            act = 1 if st == 0 else 2 if (st != 4 and on_fail == REPEAT and Adl is not None) else 0
            own = False
            if act == 1:
                Adl, Q, own = row(tr[r], cov[r], int(ok_cov[r]), ft)
                stp += 1
                if own:
                    Ql = Q
            if act:
                if own:
                    add = Ql
                else:
                    add = zero if Ql is None else [[fs * Ql[i][j] for j in range(6)] for i in range(6)]
                    n_filled += 1
                Sg = step(Sg, add, Adl, ft)
            out[r] = np.array(Sg, out.dtype)
            nf[r], steps[r] = n_filled, stp
    return (dict(cov=out, status=np.array(status, np.int32).reshape(n), step=steps, n_filled=nf),
            dict(cov=Sg, Ad=Adl, Q=Ql, n_filled=n_filled, step=stp))


def records(res):
    """chain()'s float64 records as a COV array (the bytes vh_trajectory_cov writes)"""
    out = np.zeros(len(res["status"]), COV)
    out["cov"], out["status"], out["step"], out["n_filled"] = res["cov"], res["status"], res["step"], res["n_filled"]
    return out


def carry_record(c):
    """chain()'s float64 carry as a CARRY record"""
    o = np.zeros(1, CARRY)
    o["cov"][0] = np.array(c["cov"], np.float64)
    if c["Ad"] is not None:
        o["Ad_last"][0] = np.array(c["Ad"], np.float64); o["has_ad"] = 1
    if c["Q"] is not None:
        o["Q_last"][0] = np.array(c["Q"], np.float64); o["has_q"] = 1
    o["n_filled"], o["step"] = c["n_filled"], c["step"]
    return o


def corr_diff(a, b):
    """max over records and (m, n) of |a_mn - b_mn| / sqrt(b_mm b_nn), in longdouble; records whose b has a diagonal
    entry that is not positive are left out (nothing to scale by)"""
    a, b = np.asarray(a, np.longdouble).reshape(-1, 6, 6), np.asarray(b, np.longdouble).reshape(-1, 6, 6)
    worst = np.longdouble(0)
    for x, y in zip(a, b):
        d = np.diagonal(y)
        if np.all(np.isfinite(d)) and np.all(d > 0):
            worst = max(worst, np.max(np.abs(x - y) / np.sqrt(np.outer(d, d))))
    return worst
