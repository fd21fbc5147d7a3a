"""numpy / plain-Python restatement of the reference's Reconstruction (src/reconstruction.{h,cpp}) -- test infrastructure.

Doubles are Python floats (IEEE double, no fused multiply-add), every sum is written in the reference's order, and
np.float32 stands wherever the reference stores a float (point2d, point3d, `float w`).  Matrix::svd comes from the
oracle library (oracle.svd, pinned to the reference's), Matrix::solve / inv / operator* are restated here
(src/matrix.cpp:263-277, 378-387, 417-504), the road transform uses math.cos / math.sin.
tests/golden/reconstruction_reference.npz (tools/gen_golden_reconstruction.py) pins the whole class to the reference.

solve_track also returns what the reference does not keep -- a status in the order update tests, the point as `p` stood
when the track's fate was decided, distance and angle -- the contract of vh_reconstruct_tracks (include/viso_hip.h)."""
import math

import numpy as np

F32 = np.float32
ACCEPTED, SHORT, INFINITY, TYPE, NOT_REFINED, FAR_OR_NARROW = range(6)


def matrix_solve(A, B):
    """Matrix::solve (src/matrix.cpp:417-504): A [n][n], B [n][nb] lists of floats, changed in place -> success.
    On a singular pivot both stay where the elimination stood (Matrix::inv returns that state)."""
    n, nb = len(A), len(B[0])
    ipiv = [0] * n
    irow = icol = 0
    for _ in range(n):
        big = 0.0
        for j in range(n):
            if ipiv[j] != 1:
                for k in range(n):
                    if ipiv[k] == 0 and abs(A[j][k]) >= big:
                        big, irow, icol = abs(A[j][k]), j, k
        ipiv[icol] += 1
        if irow != icol:
            A[irow], A[icol] = A[icol], A[irow]
            B[irow], B[icol] = B[icol], B[irow]
        if abs(A[icol][icol]) < 1e-20:
            return False
        pivinv = 1.0 / A[icol][icol]
        A[icol][icol] = 1.0
        A[icol] = [x * pivinv for x in A[icol]]
        B[icol] = [x * pivinv for x in B[icol]]
        for ll in range(n):
            if ll != icol:
                dum = A[ll][icol]
                A[ll][icol] = 0.0
                A[ll] = [A[ll][l] - A[icol][l] * dum for l in range(n)]
                B[ll] = [B[ll][l] - B[icol][l] * dum for l in range(nb)]
    return True


def matrix_inv(M):
    """Matrix::inv(M) (src/matrix.cpp:378-387)."""
    n = len(M)
    A = [[float(x) for x in row] for row in M]
    B = [[1.0 if i == j else 0.0 for j in range(n)] for i in range(n)]
    matrix_solve(A, B)
    return B


def matrix_mul(A, B):
    """Matrix::operator* (src/matrix.cpp:263-277): C = 0, C[i][j] += A[i][k] * B[k][j], k ascending."""
    C = [[0.0] * len(B[0]) for _ in A]
    for i in range(len(A)):
        for j in range(len(B[0])):
            c = 0.0
            for k in range(len(B)):
                c += A[i][k] * B[k][j]
            C[i][j] = c
    return C


def eye(n):
    return [[1.0 if i == j else 0.0 for j in range(n)] for i in range(n)]


class Tables:
    """Tr_total, Tr_inv_total, P_total as the constructor, setCalibration and update build them (src/reconstruction.cpp:27-70)."""

    def __init__(self, f, cu, cv):
        self.K = [[float(f), 0.0, float(cu)], [0.0, float(f), float(cv)], [0.0, 0.0, 1.0]]
        pitch, height = -0.08, 1.6
        self.road = [[0.0] * 4 for _ in range(4)]
        self.road[0][0] = 1.0
        self.road[1][1] = +math.cos(pitch); self.road[1][2] = -math.sin(pitch)
        self.road[2][1] = +math.sin(pitch); self.road[2][2] = +math.cos(pitch)
        self.road[1][3] = -height
        self.Tr_total = [eye(4)]
        self.Tr_inv_total = [eye(4)]
        self.P_total = [matrix_mul(self.K, eye(4)[:3])]

    def push(self, Tr):
        Tr = [[float(x) for x in row] for row in np.asarray(Tr, np.float64).reshape(4, 4)]
        cur = matrix_mul(self.Tr_total[-1], matrix_inv(Tr))
        self.Tr_total.append(cur)
        self.Tr_inv_total.append(matrix_inv(cur))
        self.P_total.append(matrix_mul(self.K, matrix_inv(cur)[:3]))


def _f(x):
    return float(F32(x))


def init_point(tab, svd, first, last, pixels):
    """initPoint (src/reconstruction.cpp:153-182) -> [x, y, z] as Python floats holding float32 values, or None."""
    P1, P2 = tab.P_total[first], tab.P_total[last]
    u1, v1 = float(pixels[0][0]), float(pixels[0][1])
    u2, v2 = float(pixels[-1][0]), float(pixels[-1][1])
    J = [[P1[2][j] * u1 - P1[0][j] for j in range(4)], [P1[2][j] * v1 - P1[1][j] for j in range(4)],
         [P2[2][j] * u2 - P2[0][j] for j in range(4)], [P2[2][j] * v2 - P2[1][j] for j in range(4)]]
    V = svd(np.array(J, np.float64))[2]
    w = _f(V[3][3])
    if abs(w) < 1e-10:
        return None
    with np.errstate(all="ignore"):
        return [_f(np.float64(V[i][3]) / np.float64(w)) for i in range(3)]


def point_type(tab, first, last, p):
    """pointType (src/reconstruction.cpp:235-261)."""
    x = [[p[0]], [p[1]], [p[2]], [1.0]]
    x1c = matrix_mul(tab.Tr_inv_total[first], x)
    x2c = matrix_mul(tab.Tr_inv_total[last], x)
    x2r = matrix_mul(tab.road, x2c)
    if x1c[2][0] <= 1 or x2c[2][0] <= 1:
        return -1
    if x2r[1][0] > 0.5:
        return 0
    if x2r[1][0] > -1:
        return 1
    return 2


UPDATED, FAILED, CONVERGED = range(3)


def update_point(tab, first, pixels, p):
    """updatePoint(t, p, 1, 1e-5) (src/reconstruction.cpp:263-349); p is changed in place."""
    J, res = [], []
    for k, (u, v) in enumerate(pixels):
        P = tab.P_total[first + k]
        a = P[0][0] * p[0] + P[0][1] * p[1] + P[0][2] * p[2] + P[0][3]
        b = P[1][0] * p[0] + P[1][1] * p[1] + P[1][2] * p[2] + P[1][3]
        c = P[2][0] * p[0] + P[2][1] * p[1] + P[2][2] * p[2] + P[2][3]
        cc = c * c
        if cc < 1e-10:
            return FAILED
        J.append([(P[0][0] * c - P[2][0] * a) / cc, (P[0][1] * c - P[2][1] * a) / cc, (P[0][2] * c - P[2][2] * a) / cc])
        J.append([(P[1][0] * c - P[2][0] * b) / cc, (P[1][1] * c - P[2][1] * b) / cc, (P[1][2] * c - P[2][2] * b) / cc])
        res.append(float(u) - a / c)
        res.append(float(v) - b / c)
    A = [[0.0] * 3 for _ in range(3)]
    B = [[0.0] for _ in range(3)]
    for m in range(3):
        for n in range(3):
            s = 0.0
            for i in range(len(J)):
                s += J[i][m] * J[i][n]
            A[m][n] = s
        s = 0.0
        for i in range(len(J)):
            s += J[i][m] * res[i]
        B[m][0] = s
    if not matrix_solve(A, B):
        return FAILED
    for i in range(3):
        p[i] = _f(p[i] + 1.0 * B[i][0])
    if abs(B[0][0]) < 1e-5 and abs(B[1][0]) < 1e-5 and abs(B[2][0]) < 1e-5:
        return CONVERGED
    return UPDATED


def refine_point(tab, first, pixels, p):
    """refinePoint (src/reconstruction.cpp:184-207) -> (converged, number of updates run)."""
    it, result = 0, UPDATED
    while result == UPDATED:
        result = update_point(tab, first, pixels, p)
        stop = it > 20 or result == CONVERGED
        it += 1
        if stop:
            break
    return result == CONVERGED, it


def point_distance(tab, first, last, p):
    """pointDistance (src/reconstruction.cpp:209-215)."""
    T = tab.Tr_total[(first + last) // 2]
    dx, dy, dz = T[0][3] - p[0], T[1][3] - p[1], T[2][3] - p[2]
    return math.sqrt(dx * dx + dy * dy + dz * dz)


def ray_angle(tab, first, last, p):
    """rayAngle (src/reconstruction.cpp:217-233)."""
    v1 = [tab.Tr_total[first][i][3] - p[i] for i in range(3)]
    v2 = [tab.Tr_total[last][i][3] - p[i] for i in range(3)]
    n1 = n2 = 0.0
    for i in range(3):
        n1 += v1[i] * v1[i]
        n2 += v2[i] * v2[i]
    n1, n2 = math.sqrt(n1), math.sqrt(n2)
    if n1 < 1e-10 or n2 < 1e-10:
        return 1000.0
    dot = 0.0
    for i in range(3):
        dot += (v1[i] / n1) * (v2[i] / n2)
    d = abs(dot)
    return (math.acos(d) if d <= 1.0 else math.nan) * 180.0 / math.pi


def solve_track(tab, svd, first, pixels, point_type_min=1, min_track_length=2, max_dist=30.0, min_angle=2.0, info=None):
    """What update does with one lost track (src/reconstruction.cpp:131-142) -> (point float32 [3], status, distance, angle)."""
    last = first + len(pixels) - 1
    zero = np.zeros(3, F32)
    if min_track_length < 0 or len(pixels) < min_track_length:   # (size_t compare in the reference: negative = huge)
        return zero, SHORT, 0.0, 0.0
    p = init_point(tab, svd, first, last, pixels)
    if p is None:
        return zero, INFINITY, 0.0, 0.0
    if not point_type(tab, first, last, p) >= point_type_min:
        return np.array(p, F32), TYPE, 0.0, 0.0
    ok, updates = refine_point(tab, first, pixels, p)
    if info is not None:
        info["updates"] = updates
    if not ok:
        return np.array(p, F32), NOT_REFINED, 0.0, 0.0
    dist, angle = point_distance(tab, first, last, p), ray_angle(tab, first, last, p)
    status = ACCEPTED if dist < max_dist and angle > min_angle else FAR_OR_NARROW
    return np.array(p, F32), status, dist, angle


class Reconstruction:
    """The whole class: association (src/reconstruction.cpp:72-145) and the points of the lost tracks."""

    def __init__(self, svd):
        self.svd = svd
        self.tab = None
        self.tracks = []
        self.points = []
        self.lost_log = []   # (first_frame, pixels) of every lost track, in the order update met them

    def setCalibration(self, f, cu, cv):
        self.tab = Tables(f, cu, cv)

    def update(self, pm, Tr, point_type=1, min_track_length=2, max_dist=30.0, min_angle=2.0, solve=True):
        tab, tracks = self.tab, self.tracks
        tab.push(Tr)
        current_frame = len(tab.Tr_total) - 1
        track_idx_max = 0
        for m in pm:
            if m["i1p"] > track_idx_max:
                track_idx_max = int(m["i1p"])
        for t in tracks:
            if t["last_idx"] > track_idx_max:
                track_idx_max = t["last_idx"]
        track_idx = [-1] * (track_idx_max + 1)
        for i, t in enumerate(tracks):
            if t["last_idx"] >= 0:   # (the guard of the product: the reference would write before its table)
                track_idx[t["last_idx"]] = i
        for m in pm:
            idx = track_idx[int(m["i1p"])] if m["i1p"] >= 0 else -1   # (the guard: i1p < 0 starts a new track)
            if idx >= 0 and tracks[idx]["last_frame"] == current_frame - 1:
                tracks[idx]["pixels"].append((m["u1c"], m["v1c"]))
                tracks[idx]["last_frame"] = current_frame
                tracks[idx]["last_idx"] = int(m["i1c"])
            else:
                tracks.append(dict(pixels=[(m["u1p"], m["v1p"]), (m["u1c"], m["v1c"])], first_frame=current_frame - 1,
                                   last_frame=current_frame, last_idx=int(m["i1c"])))
        copy, self.tracks = tracks, []
        for t in copy:
            if t["last_frame"] == current_frame:
                self.tracks.append(t)
            else:
                self.lost_log.append((t["first_frame"], list(t["pixels"])))
                if solve:
                    p, status, _, _ = solve_track(tab, self.svd, t["first_frame"], t["pixels"], point_type, min_track_length, max_dist, min_angle)
                    if status == ACCEPTED:
                        self.points.append(p)

    def getPoints(self):
        return np.array(self.points, F32).reshape(-1, 3)
