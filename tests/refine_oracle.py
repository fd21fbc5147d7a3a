"""numpy restatement of the match refinement contract -- test infrastructure.

Stock libviso2 refines the matches between matching and removeOutliers [upstream-recollection; the reference tree has
no refinement function].  This file restates the contract, not any code: it is built on the full-resolution Sobel
planes of oracle.filters, the small descriptor of reference src/matcher.cpp:516-543 (computeSmallDescriptor), the
product order of Matrix::operator* (src/matrix.cpp:263-277) and the Gauss-Jordan elimination of Matrix::solve
(src/matrix.cpp:417-504).  Doubles are Python floats (IEEE double, no fused multiply-add); np.float32 where the
contract rounds to float."""
import numpy as np

P_MATCH_FIELDS = ("u1p", "v1p", "i1p", "u2p", "v2p", "i2p", "u1c", "v1c", "i1c", "u2c", "v2c", "i2c")
# (row, column) offsets of the 16 bytes of the small descriptor: 12 from du, then 4 from dv (src/matcher.cpp:516-543)
SMALL_DU = ((-2, 0), (-1, -2), (-1, 0), (-1, 2), (0, -1), (0, 0), (0, 0), (0, 1), (1, -2), (1, 0), (1, 2), (2, 0))
SMALL_DV = ((-1, 0), (0, -1), (0, 1), (1, 0))
F32 = np.float32


def descriptor_stack(du, dv):
    """[H, bpl, 16] int32: the small descriptor at every pixel (meaningful where the 5x5 neighbourhood is inside)."""
    h, w = du.shape
    pu, pv = np.pad(du, 2).astype(np.int32), np.pad(dv, 2).astype(np.int32)
    planes = [pu[2 + a:2 + a + h, 2 + b:2 + b + w] for a, b in SMALL_DU] + [pv[2 + a:2 + a + h, 2 + b:2 + b + w] for a, b in SMALL_DV]
    return np.stack(planes, axis=-1)


def solve(A, b):
    """Matrix::solve (src/matrix.cpp:417-504) with one right-hand side -> x, or None when singular."""
    A = [[float(x) for x in row] for row in A]
    b = [float(x) for x in b]
    n = len(A)
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
            b[irow], b[icol] = b[icol], b[irow]
        if abs(A[icol][icol]) < 1e-20:
            return None
        pivinv = 1.0 / A[icol][icol]
        A[icol][icol] = 1.0
        A[icol] = [x * pivinv for x in A[icol]]
        b[icol] *= pivinv
        for ll in range(n):
            if ll != icol:
                dum = A[ll][icol]
                A[ll][icol] = 0.0
                A[ll] = [A[ll][l] - A[icol][l] * dum for l in range(n)]
                b[ll] -= b[icol] * dum
    return b


# rows (x^2, y^2, xy, x, y, 1), y = -1..1 outer, x = -1..1 inner
DESIGN = [(float(x * x), float(y * y), float(x * y), float(x), float(y), 1.0) for y in (-1, 0, 1) for x in (-1, 0, 1)]


def mat_t_mul(A, B):
    """A^T * B in Matrix::operator*'s order: C = 0, C[i][j] += A^T[i][k] * B[k][j], k ascending."""
    m, n, p = len(A), len(A[0]), len(B[0])
    C = [[0.0] * p for _ in range(n)]
    for i in range(n):
        for j in range(p):
            for k in range(m):
                C[i][j] += A[k][i] * B[k][j]
    return C


def parabolic_offset(c9):
    """The sub-pixel step on the 3x3 cost table c9 (row-major, centre = the minimum) -> (ddu, ddv) as float32, or None
    when the contract drops the match."""
    r = parabolic_fit(c9)
    return None if isinstance(r, str) else r


def parabolic_fit(c9):
    """parabolic_offset, with the reason of a drop instead of None: "singular", "degenerate" (divisor or cross term
    below 1e-8) or "far" (|ddu| or |ddv| >= 1)."""
    AtA = mat_t_mul(DESIGN, DESIGN)
    b = [r[0] for r in mat_t_mul(DESIGN, [[float(c)] for c in c9])]
    x = solve(AtA, b)
    if x is None:
        return "singular"
    b0, b1, b2, b3, b4, _ = x
    divisor = F32(b2 * b2 - 4.0 * b0 * b1)
    # the second test is stock libviso2's: it also rejects fits whose cross term is exactly 0
    if abs(float(divisor)) < 1e-8 or abs(b2) < 1e-8:
        return "degenerate"
    ddu = F32((2.0 * b1 * b3 - b2 * b4) / float(divisor))
    ddv = F32((2.0 * b0 * b4 - b2 * b3) / float(divisor))
    if abs(ddu) >= 1 or abs(ddv) >= 1:
        return "far"
    return ddu, ddv


def refine_hop(dims, DA, DT, u1, v1, u2, v2, subpixel, stats=None):
    """One hop -> (u2, v2) as float32, or None (dropped).  stats (a dict, optional) counts the branch each hop takes:
    "outside", "moved", "border", "singular", "degenerate", "far"."""
    def seen(k):
        if stats is not None:
            stats[k] = stats.get(k, 0) + 1
    W, H = int(dims[0]), int(dims[1])
    R = 3 if subpixel else 2
    N = 2 * R + 1
    inside = (4 <= u1 <= W - 5 and 4 <= v1 <= H - 5 and 4 + R <= u2 <= W - 5 - R and 4 + R <= v2 <= H - 5 - R)
    if not inside:
        seen("outside")
        return None if subpixel else (u2, v2)
    a = DA[int(v1), int(u1)]
    x0, y0 = int(u2) - R, int(v2) - R
    cost = np.abs(DT[y0:y0 + N, x0:x0 + N] - a).sum(-1)
    m = int(np.argmin(cost))  # the first minimum in row-major order
    du0, dv0 = m % N, m // N
    if not subpixel:
        seen("moved")
        return F32(u2 + F32(F32(du0) - F32(2))), F32(v2 + F32(F32(dv0) - F32(2)))
    if du0 in (0, N - 1) or dv0 in (0, N - 1):
        seen("border")
        return None
    off = parabolic_fit(cost[dv0 - 1:dv0 + 2, du0 - 1:du0 + 2].reshape(9))
    if isinstance(off, str):
        seen(off)
        return None
    seen("moved")
    ddu, ddv = off
    return F32(u2 + F32(F32(F32(du0) - F32(3)) + ddu)), F32(v2 + F32(F32(F32(dv0) - F32(3)) + ddv))


def refine(pm, method, refinement, dims, images, filters, stats=None):
    """The refined records that are kept, in order.  images = (I1p, I2p, I1c, I2c) full-resolution [H, bpl] (None where the
    method reads none); filters = oracle.filters; stats: see refine_hop."""
    pm = np.array(pm, copy=True)
    if refinement <= 0 or len(pm) == 0:
        return pm
    subpixel = refinement == 2
    D = [None if I is None else descriptor_stack(*filters(I)[:2]) for I in images]
    hops = {0: ((0, "u1p", "v1p"),), 1: ((3, "u2c", "v2c"),),
            2: ((0, "u1p", "v1p"), (3, "u2c", "v2c"), (1, "u2p", "v2p"))}[method]
    keep = []
    for i in range(len(pm)):
        r = pm[i]
        u1, v1 = F32(r["u1c"]), F32(r["v1c"])
        ok = True
        for role, fu, fv in hops:
            out = refine_hop(dims, D[2], D[role], u1, v1, F32(r[fu]), F32(r[fv]), subpixel, stats)
            if out is None:
                ok = False
                break
            r[fu], r[fv] = out
        if ok:
            keep.append(i)
    return pm[keep].copy()
