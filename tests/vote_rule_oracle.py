"""The outlier vote under a rule (include/viso_hip.h: vh_vote_rule), restated in numpy float32 over the triangles of
oracle.delaunay(xy) -- the pinned triangulation.  Rule None / (VOTE_REFERENCE, ...) is the reference's vote
(src/remove_outliers.cpp:34-90: flow under the literal 5); (VOTE_STOCK, M, flow_tolerance, disp_tolerance) is

    fu(i) = u1c - u1p,  fv(i) = v1c - v1p,  d(i) = u1c - u2c
    F(a,b) = |fu(a) - fu(b)| + |fv(a) - fv(b)| < flow_tolerance
    D(a,b) = |d(a) - d(b)| < disp_tolerance
    agree(a,b) = M == 0 ? F : M == 1 ? D : (D && F)

every step rounded to float32; n <= 3 returns the list; a triangle gives each corner one vote per agreeing edge it lies
on; a record survives with at least 4 votes, in list order.  Strict compares: NaN disagrees, a tolerance <= 0 agrees with
nothing."""
import numpy as np

F32 = np.float32
VOTE_REFERENCE, VOTE_STOCK = 0, 1


def stock(method, flow_tolerance=5.0, disp_tolerance=5.0):
    return (VOTE_STOCK, int(method), float(flow_tolerance), float(disp_tolerance))


def votes(oracle, pm, rule=None):
    """-> votes per record (int64 [n]) of a list of more than 3 records"""
    n = len(pm)
    xy = np.stack([pm["u1c"], pm["v1c"]], 1).astype(F32)
    tri, _ = oracle.delaunay(xy)
    is_stock = rule is not None and rule[0] != VOTE_REFERENCE
    if is_stock:
        assert rule[0] == VOTE_STOCK and 0 <= rule[1] <= 2
    method = rule[1] if is_stock else 0
    ftol = F32(rule[2]) if is_stock else F32(5)
    dtol = F32(rule[3]) if is_stock else F32(0)
    fu = (pm["u1c"].astype(F32) - pm["u1p"].astype(F32)).astype(F32)
    fv = (pm["v1c"].astype(F32) - pm["v1p"].astype(F32)).astype(F32)
    d = (pm["u1c"].astype(F32) - pm["u2c"].astype(F32)).astype(F32)
    count = np.zeros(n, np.int64)
    if len(tri) == 0:
        return count
    with np.errstate(invalid="ignore"):
        for i, j in ((0, 1), (1, 2), (0, 2)):
            a, b = tri[:, i], tri[:, j]
            flow = (np.abs((fu[a] - fu[b]).astype(F32)) + np.abs((fv[a] - fv[b]).astype(F32))).astype(F32) < ftol
            disp = np.abs((d[a] - d[b]).astype(F32)) < dtol
            agree = flow if method == 0 else (disp if method == 1 else (disp & flow))
            np.add.at(count, a, agree.astype(np.int64))
            np.add.at(count, b, agree.astype(np.int64))
    return count


def remove_outliers(oracle, pm, rule=None):
    pm = np.ascontiguousarray(pm).copy()
    if len(pm) <= 3:
        return pm
    return pm[votes(oracle, pm, rule) >= 4].copy()
