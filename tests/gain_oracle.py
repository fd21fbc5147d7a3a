"""Matcher::getGain restated in numpy (test infrastructure): the reference's own Matcher::mean (src/matcher.cpp:347-354,
pinned by tests/golden/gain_reference.npz) under stock libviso2's getGain loop [upstream-recollection; the reference has
the body commented out, src/matcher.h:145-148], with the two rules DESIGN.md section 4.14 tightens: windows are clamped
to W - 1 / H - 1, and indices outside [0, n) and coordinates that are not finite or reach 2^24 are skipped.

Every scalar is an np.float32 and every sum is sequential: the order of `idx` is part of the result."""
import numpy as np

F32 = np.float32
LIMIT = F32(16777216.0)  # 2^24


def mean(I, bpl, u_min, u_max, v_min, v_max):
    """Matcher::mean: a float sum of the bytes, row-major, divided by the float of the window's pixel count.
    I: flat or 2-d uint8 array with `bpl` bytes per row."""
    I = np.asarray(I, np.uint8).reshape(-1)
    m = F32(0)
    for v in range(v_min, v_max + 1):
        row = I[v * bpl + u_min: v * bpl + u_max + 1]
        for b in row:
            m = F32(m + F32(b))
    return F32(m / F32((u_max - u_min + 1) * (v_max - v_min + 1)))


def window(u, v, W, H):
    """-> (u_min, u_max, v_min, v_max) of the 7 x 7 window around the truncated (u, v), clamped into the image."""
    up, vp = int(np.int32(np.trunc(u))), int(np.int32(np.trunc(v)))  # C truncation; |u|, |v| < 2^24 here
    return (min(max(up - 3, 0), W - 1), min(max(up + 3, 0), W - 1), min(max(vp - 3, 0), H - 1), min(max(vp + 3, 0), H - 1))


def usable(x):
    x = F32(x)
    return bool(np.isfinite(x)) and bool(abs(x) < LIMIT)


def ratios(pm, idx, Ip, Ic, dims):
    """The ratio of every index entry that counts, in the order of idx: a list of np.float32."""
    W, H, bpl = (int(d) for d in dims)
    n = len(pm)
    out = []
    for i in np.asarray(idx, np.int64):
        if i < 0 or i >= n:
            continue
        c = [pm[i][k] for k in ("u1p", "v1p", "u1c", "v1c")]
        if not all(usable(x) for x in c):
            continue
        mp = mean(Ip, bpl, *window(c[0], c[1], W, H))
        mc = mean(Ic, bpl, *window(c[2], c[3], W, H))
        if mp > F32(10):
            out.append(F32(mc / mp))
    return out


def gain(pm, idx, Ip, Ic, dims):
    """-> (gain np.float32, num int)."""
    r = ratios(pm, idx, Ip, Ic, dims)
    g = F32(0)
    for x in r:
        g = F32(g + x)
    return (F32(g / F32(len(r))) if r else F32(1), len(r))
