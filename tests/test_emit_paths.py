"""emit_features at the edges of its own structure: byte parity of the feature records and of one quad
matching with the oracle where a chunk of 1024 NMS blocks holds 1 / 15 / 16 / 17 survivors (partial lane
groups, dead slots of a trip), exactly 64 / 65 / 129 (the turn of the two register sets: 32 * NF, NF = 2),
none at all between chunks that hold some, blocks that emit several of their four classes, descriptor sums
at their extremes in both directions, every byte alignment of the sample windows, a row stride that is no multiple of 16 through
the device-pointer entry, a capacity below the feature count and at a chunk's running count, half resolution,
and chunks whose pixel rows do not fit the LDS row counters.  The same cases run on the checking build."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

MARGIN, CHUNK, ROWS_LDS = 7, 1024, 64  # VH_MARGIN, VH_CHUNK, emit_features' LDS row counters per class


def blocks(extent, n):
    """NMS blocks along an image extent (engine.hip block_count)."""
    return (extent - 2 * n - 2 * MARGIN - 1) // (n + 1) + 1


def chunk_counts(feats, dims, n, scale=1):
    """Survivors per chunk of 1024 blocks (block row-major), from the oracle's records."""
    W, H = dims[0] // scale, dims[1] // scale
    nbx = blocks(W, n)
    bx = (feats[:, 0] // scale - n - MARGIN) // (n + 1)
    by = (feats[:, 1] // scale - n - MARGIN) // (n + 1)
    nchunks = -(-(nbx * blocks(H, n)) // CHUNK)
    return np.bincount((by * nbx + bx) // CHUNK, minlength=nchunks)


def max_v_span(dims, n, scale=1):
    """Largest v_span of a chunk, as emit_features computes it."""
    W, H = dims[0] // scale, dims[1] // scale
    nbx, nblocks = blocks(W, n), blocks(W, n) * blocks(H, n)
    spans = []
    for first in range(0, nblocks, CHUNK):
        last = min(first + CHUNK, nblocks) - 1
        v_first = ((first // nbx) * (n + 1) + n + MARGIN) * scale
        spans.append(((last // nbx) * (n + 1) + n + MARGIN + n) * scale + scale - v_first)
    return max(spans)


def run_quad(pkg, ob, oracle, imgs, dims, min_feats=1, **over):
    """Four images through Matcher.pushBack / getFeatures / matchFeatures(quad) against the oracle."""
    p, po = pkg.Params.default(**over), ob.Params.default(**over)
    want = [oracle.compute_features(po, im, dims)[1] for im in imgs]
    assert min(len(w) for w in want) >= min_feats, [len(w) for w in want]
    m = pkg.Matcher(p, outlier_removal=False)
    try:
        assert m.pushBack(imgs[0], imgs[1], dims, False) and m.pushBack(imgs[2], imgs[3], dims, False)
        for k in range(4):
            assert np.array_equal(m.getFeatures(k), want[k]), (k, over)
        m.matchFeatures(pkg.METHOD_QUAD)
        assert m.getMatches().tobytes() == oracle.matching(po, dims, 2, *want).tobytes(), over
    finally:
        m.close()
    return want


# ---- one-chunk images with an exact number of survivors: a textured rectangle on constant grey
ONE_W, ONE_H, ONE_TAU = 190, 67, 20  # 58 x 17 = 986 blocks at nms_n = 2: one chunk
_counted = {}


def counted_image(pkg, ob, oracle, target):
    """A one-chunk image with exactly `target` features: texture in [0, x) x [0, y), grey elsewhere; (x, y) searched
    with the oracle on the CPU (deterministic), once per target."""
    if target in _counted:
        return _counted[target]
    dims = [ONE_W, ONE_H, pkg.synth.bytes_per_line(ONE_W)]
    po = ob.Params.default(nms_tau=ONE_TAU)
    tex = pkg.synth.frame(ONE_W, ONE_H, 0, 0, 2, 3, 41)

    def rect(x, y):
        img = np.full_like(tex, 128)
        img[:, ONE_W:] = 0
        img[:y, :x] = tex[:y, :x]
        return img, len(oracle.compute_features(po, img, dims)[1])

    for y in range(10, ONE_H + 1):
        if rect(ONE_W, y)[1] < target:
            continue
        for x in range(1, ONE_W + 1):
            img, cnt = rect(x, y)
            if cnt == target:
                _counted[target] = img
                return img
            if cnt > target + 8:
                break  # wider rectangles of this height hold more still: try the next height
    raise AssertionError(f"no rectangle with {target} features")


@pytest.mark.gpu
def test_lone_feature(pkg, ob, oracle, gpu):
    dims = [ONE_W, ONE_H, pkg.synth.bytes_per_line(ONE_W)]
    img = counted_image(pkg, ob, oracle, 1)
    want = run_quad(pkg, ob, oracle, [img] * 4, dims, nms_tau=ONE_TAU)
    assert [len(w) for w in want] == [1] * 4


@pytest.mark.gpu
def test_fifteen_seventeen(pkg, ob, oracle, gpu):
    dims = [ONE_W, ONE_H, pkg.synth.bytes_per_line(ONE_W)]
    imgs = [counted_image(pkg, ob, oracle, t) for t in (15, 16, 17, 16)]
    want = run_quad(pkg, ob, oracle, imgs, dims, nms_tau=ONE_TAU)
    assert [len(w) for w in want] == [15, 16, 17, 16]


@pytest.mark.gpu
def test_two_register_sets(pkg, ob, oracle, gpu):
    """32 * NF, 32 * NF + 1 and 64 * NF + 1 survivors in the chunk (NF = 2)."""
    dims = [ONE_W, ONE_H, pkg.synth.bytes_per_line(ONE_W)]
    imgs = [counted_image(pkg, ob, oracle, t) for t in (64, 65, 129, 65)]
    want = run_quad(pkg, ob, oracle, imgs, dims, nms_tau=ONE_TAU)
    assert [len(w) for w in want] == [64, 65, 129, 65]


@pytest.mark.gpu
def test_empty_chunk_between(pkg, ob, oracle, gpu):
    W, H = 320, 160  # 101 x 47 blocks: 5 chunks of ~10 block rows
    dims = [W, H, pkg.synth.bytes_per_line(W)]
    imgs = []
    for dx in (0, 4, 1, 5):
        im = pkg.synth.frame(W, H, dx, 0, 3, 2, 52).copy()
        im[40:120, :W] = 128
        imgs.append(im)
    want = run_quad(pkg, ob, oracle, imgs, dims, min_feats=50)
    cc = chunk_counts(want[0], dims, 2)
    assert cc[0] > 0 and cc[-1] > 0 and (cc[1:-1] == 0).any(), cc


@pytest.mark.gpu
def test_all_four_codes(pkg, ob, oracle, gpu):
    """nms_tau = 0 on a fine texture: blocks emit several of their four classes, in class order."""
    W, H = 230, 90
    dims = [W, H, pkg.synth.bytes_per_line(W)]
    imgs = [pkg.synth.frame(W, H, dx, 0, 1, 3, 63) for dx in (0, 3, 1, 4)]
    want = run_quad(pkg, ob, oracle, imgs, dims, min_feats=200, nms_tau=0)
    f = want[0]
    blk = ((f[:, 1] - 2 - MARGIN) // 3) * blocks(W, 2) + (f[:, 0] - 2 - MARGIN) // 3
    assert np.bincount(blk).max() >= 2
    assert len(np.unique(f[:, 3])) == 4


def checker(W, H, bpl, sq, invert):
    yy, xx = np.mgrid[0:H, 0:W]
    img = np.zeros((H, bpl), np.uint8)
    img[:, :W] = np.where((((xx // sq) + (yy // sq)) & 1).astype(bool) ^ invert, 255, 0)
    return img


@pytest.mark.gpu
@pytest.mark.parametrize("sq", [5, 6, 7])
def test_saturation(sq, pkg, ob, oracle, gpu):
    """A black / white checker and its inverse: the descriptor sums at their largest magnitude in both directions.
    Bytes 0 and 255 themselves cannot occur on 8-bit images: a 5x5 Sobel sum is at most 48 * 255 = 12240 in
    magnitude, and (-12240 >> 7) + 128 = 32, (12240 >> 7) + 128 = 223 -- the clamp of the reference is never
    reached.  32 and 223 are what the signed form has to reproduce; both must occur in the oracle's output."""
    W, H = 200, 80
    dims = [W, H, pkg.synth.bytes_per_line(W)]
    a, b = checker(W, H, dims[2], sq, False), checker(W, H, dims[2], sq, True)
    want = run_quad(pkg, ob, oracle, [a, b, b, a], dims, min_feats=20)
    for w in want:
        d = np.ascontiguousarray(w[:, 4:]).view(np.uint8)
        assert d.min() == 32 and d.max() == 223, (sq, d.min(), d.max())


@pytest.mark.gpu
def test_alignment_pans(pkg, ob, oracle, gpu):
    """The same texture panned by 0..3 px: every alignment of the patch's first byte."""
    W, H = 203, 75
    dims = [W, H, pkg.synth.bytes_per_line(W)]
    imgs = [pkg.synth.frame(W, H, dx, 0, 3, 2, 74) for dx in (0, 1, 2, 3)]
    run_quad(pkg, ob, oracle, imgs, dims, min_feats=50)


@pytest.mark.gpu
def test_alignment_odd_stride_device_pointer(pkg, ob, oracle, gpu):
    """Row stride 203 (no multiple of 16, nor of 4) through pushBackDevice."""
    W, H = 203, 75
    dims = [W, H, W]
    imgs = [np.ascontiguousarray(pkg.synth.frame(W, H, dx, 0, 3, 2, 74)[:, :W]) for dx in (0, 1, 2, 3)]
    po = ob.Params.default()
    want = [oracle.compute_features(po, im, dims)[1] for im in imgs]
    assert min(len(w) for w in want) > 50
    pkg._lib()  # (the HIP runtime the library is linked against)
    hip = C.CDLL("libamdhip64.so")
    hip.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    hip.hipFree.argtypes = [C.c_void_p]
    ptrs = []
    m = pkg.Matcher(pkg.Params.default(), outlier_removal=False)
    try:
        for im in imgs:
            d = C.c_void_p()
            assert hip.hipMalloc(C.byref(d), im.nbytes) == 0
            ptrs.append(d)
            assert hip.hipMemcpy(d, im.ctypes.data_as(C.c_void_p), im.nbytes, 1) == 0  # hipMemcpyHostToDevice
        m.pushBackDevice(ptrs[0].value, ptrs[1].value, dims, False)
        m.pushBackDevice(ptrs[2].value, ptrs[3].value, dims, False)
        for k in range(4):
            assert np.array_equal(m.getFeatures(k), want[k]), k
        m.matchFeatures(pkg.METHOD_QUAD)
        assert m.getMatches().tobytes() == oracle.matching(po, dims, 2, *want).tobytes()
    finally:
        m.close()
        for d in ptrs:
            hip.hipFree(d)


@pytest.mark.gpu
def test_capacity(pkg, ob, oracle, gpu):
    """max_features a few below the feature count, and exactly the running count at a chunk boundary: the first
    `capacity` records are exact, nothing lands behind them, and the true count is still reported."""
    W, H = 320, 160
    dims = [W, H, pkg.synth.bytes_per_line(W)]
    img = pkg.synth.frame(W, H, 0, 0, 4, 1, 85)
    full = oracle.compute_features(ob.Params.default(), img, dims)[1]
    cc = chunk_counts(full, dims, 2)
    assert len(cc) >= 3 and cc[0] > 0 and cc[1] > 0
    for cap in (len(full) - 3, int(cc[0] + cc[1])):
        m = pkg.Matcher(pkg.Params.default(), max_features=cap, max_matches=4096, outlier_removal=False)
        try:
            m.pushBack(img, None, dims, False)
            n = C.c_int32(0)
            buf = np.full((len(full) + 8, 12), -7, np.int32)
            rc = pkg._lib().vh_get_features(m._h, pkg.SET_1C, buf.ctypes.data_as(C.c_void_p), len(buf), C.byref(n))
        finally:
            m.close()
        assert rc == pkg.VH_ERR_CAPACITY and n.value == len(full), (cap, rc, n.value)
        assert np.array_equal(buf[:cap], full[:cap]) and (buf[cap:] == -7).all(), cap


@pytest.mark.gpu
def test_half_resolution(pkg, ob, oracle, gpu):
    W, H = 1000, 100
    dims = [W, H, pkg.synth.bytes_per_line(W)]
    assert max_v_span(dims, 2, 2) <= ROWS_LDS  # the LDS row counters, at scale 2
    imgs = [pkg.synth.frame(W, H, dx, 0, 5, 2, 96) for dx in (0, 6, 2, 8)]
    run_quad(pkg, ob, oracle, imgs, dims, min_feats=50, half_resolution=1)


@pytest.mark.gpu
@pytest.mark.parametrize("half", [0, 1])
def test_rows_not_in_lds(half, pkg, ob, oracle, gpu):
    """A narrow image: a chunk of 1024 blocks spans more than 64 pixel rows (global row atomics)."""
    W, H = (100, 260) if not half else (200, 300)
    dims = [W, H, pkg.synth.bytes_per_line(W)]
    assert max_v_span(dims, 2, 1 + half) > ROWS_LDS
    imgs = [pkg.synth.frame(W, H, dx, 0, 3 + 2 * half, 2, 107) for dx in (0, 4, 1, 5)]
    run_quad(pkg, ob, oracle, imgs, dims, min_feats=50, half_resolution=half)


@pytest.mark.gpu
def test_same_cases_on_the_checking_build(pkg, gpu):
    assert os.path.exists(pkg.CHECK_LIB_PATH), "build() makes it"
    env = dict(os.environ, VISO_HIP_LIB=pkg.CHECK_LIB_PATH)
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-q", "-x", "-m", "gpu", "-k", "not checking_build"],
                       env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert " passed" in r.stdout and "VH_CHECK" not in r.stderr
