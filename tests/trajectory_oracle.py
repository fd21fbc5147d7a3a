"""The trajectory's rule (include/viso_hip.h) in numpy scalars, one row at a time: T from the
motion vector, Matrix::inv through reconstruction_oracle.matrix_solve, the status, the policy and Matrix::operator*'s
product -- in float64 (what the device is held to, byte for byte where sin / cos are exact) or in longdouble (what the
float64 result is measured against)."""
import numpy as np

import reconstruction_oracle as ro

HOLD, REPEAT = 0, 1
POSE = np.dtype([("Tw_prev", "<f8", (4, 4)), ("Tw_cur", "<f8", (4, 4)), ("status", "<i4"), ("step", "<i4"), ("reserved", "<i4", (2,))])
CARRY = np.dtype([("Tw", "<f8", (4, 4)), ("Tinv", "<f8", (4, 4)), ("step", "<i4"), ("has_tinv", "<i4"), ("reserved", "<i4", (2,))])


def transform(tr, ft=np.float64):
    """VisualOdometry::transformationVectorToMatrix (src/viso.cpp:59-84) -> 4 x 4 list of ft scalars; the rotation as
    the estimators' oracles state it"""
    rx, ry, rz, tx, ty, tz = [ft(v) for v in tr]
    sx, cx, sy, cy, sz, cz = np.sin(rx), np.cos(rx), np.sin(ry), np.cos(ry), np.sin(rz), np.cos(rz)
    z, o = ft(0), ft(1)
    return [[+cy * cz, -cy * sz, +sy, tx],
            [+sx * sy * cz + cx * sz, -sx * sy * sz + cx * cz, -sx * cy, ty],
            [-cx * sy * cz + sx * sz, +cx * sy * sz + sx * cz, +cx * cy, tz],
            [z, z, z, o]]


def inverse(tr, ok, ft=np.float64):
    """-> (status, Tinv or None): steps 1 - 3 of the rule"""
    if ok < 0:
        return 4, None
    if ok == 0:
        return 1, None
    if not np.all(np.isfinite(np.asarray(tr, np.float64))):
        return 2, None
    A = transform(tr, ft)
    B = [[ft(1) if i == j else ft(0) for j in range(4)] for i in range(4)]
    with np.errstate(all="ignore"):
        if not ro.matrix_solve(A, B):
            return 3, None
    if not all(np.isfinite(x) for row in B for x in row):
        return 2, None
    return 0, B


def product(P, M, ft=np.float64):
    """Matrix::operator* (src/matrix.cpp:272-275): c = 0; c += P[i][k] * M[k][j], k ascending"""
    C = [[ft(0)] * 4 for _ in range(4)]
    for i in range(4):
        for j in range(4):
            c = ft(0)
            for k in range(4):
                c = c + P[i][k] * M[k][j]
            C[i][j] = c
    return C


def chain(tr, ok, T0=None, carry=None, on_fail=HOLD, ft=np.float64):
    """One chain of rows -> (records: dict of arrays Tw_prev [n, 4, 4], Tw_cur, status, step in ft; the carry as the tuple
    (P, last Tinv or None, step))"""
    n = len(tr)
    if carry is not None:
        P, last, step = carry
    else:
        P = [[ft(1) if i == j else ft(0) for j in range(4)] for i in range(4)] if T0 is None else [[ft(x) for x in row] for row in np.asarray(T0).reshape(4, 4)]
        last, step = None, 0
    prev_out, cur_out = np.zeros((n, 4, 4), ft), np.zeros((n, 4, 4), ft)
    status, steps = np.zeros(n, np.int32), np.zeros(n, np.int32)
    for r in range(n):
        st, Tinv = inverse(tr[r], int(ok[r]), ft)
        prev_out[r] = np.array(P, ft)
        if st == 0:
            last = Tinv; step += 1
            P = product(P, last, ft)
        elif st != 4 and on_fail == REPEAT and last is not None:
            P = product(P, last, ft)
        cur_out[r] = np.array(P, ft)
        status[r], steps[r] = st, step
    return dict(Tw_prev=prev_out, Tw_cur=cur_out, status=status, step=steps), (P, last, step)


def records(res):
    """chain()'s float64 records as a POSE array (the bytes vh_trajectory writes)"""
    out = np.zeros(len(res["status"]), POSE)
    out["Tw_prev"], out["Tw_cur"], out["status"], out["step"] = res["Tw_prev"], res["Tw_cur"], res["status"], res["step"]
    return out


def carry_record(carry):
    """chain()'s float64 carry as a CARRY record"""
    P, last, step = carry
    c = np.zeros(1, CARRY)
    c["Tw"][0] = np.array(P, np.float64)
    if last is not None:
        c["Tinv"][0] = np.array(last, np.float64); c["has_tinv"] = 1
    c["step"] = step
    return c


def carry_tuple(rec):
    """a CARRY record as chain()'s carry"""
    rec = np.asarray(rec).reshape(-1)[0]
    P = [[np.float64(x) for x in row] for row in rec["Tw"]]
    last = [[np.float64(x) for x in row] for row in rec["Tinv"]] if rec["has_tinv"] else None
    return P, last, int(rec["step"])


def demo_loop(tr, ok):
    """The literal loop of src/demo.cpp in numpy's own linear algebra: pose = pose @ inv(T) where process() succeeded"""
    pose = np.eye(4)
    out = np.zeros((len(tr), 4, 4))
    for r in range(len(tr)):
        if ok[r] > 0:
            pose = pose @ np.linalg.inv(np.array(transform(tr[r]), np.float64))
        out[r] = pose
    return out


def rel_diff(a, b):
    """largest element-wise |a - b| / max(1, |b|), in longdouble"""
    a, b = np.asarray(a, np.longdouble), np.asarray(b, np.longdouble)
    if a.size == 0:
        return np.longdouble(0)
    return np.max(np.abs(a - b) / np.maximum(1, np.abs(b)))
