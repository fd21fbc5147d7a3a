"""TEST INFRASTRUCTURE: inputs of Matcher::bucketFeatures (src/matcher.cpp:140-187) at the edges of its bucket grid,
inside the bounds in which the reference is defined -- buckets[126][256] on its stack (:154) and POINT_L records.

families(seed, dtype) yields (name, records, [(max_features, bucket_width, bucket_height), ...]); oracle/gen_golden.py
records the reference's outputs for seed 0 in tests/golden/bucket_edges.npz, tests/test_oracle.py replays them and
puts fresh seeds to the reference.  shape() restates the grid arithmetic in float32, step by step as the reference
computes it, so that every case can state -- and assert -- the grid, the empty buckets and the bucket lengths it has.
"""
import numpy as np

REF_BUCKETS, REF_BUCKET_LEN, REF_POINT_L = 126, 256, 14002  # matcher.cpp:154, matcher.h POINT_L
MF_ALL = 2 ** 30


def shape(pm, bw, bh):
    """-> (cols, rows, bucket id per record, records per bucket) of bucketFeatures(., bw, bh) on these records."""
    bw, bh = np.float32(bw), np.float32(bh)
    u, v = pm["u1c"].astype(np.float32), pm["v1c"].astype(np.float32)
    u_max = max(np.float32(0), u.max()) if len(pm) else np.float32(0)
    v_max = max(np.float32(0), v.max()) if len(pm) else np.float32(0)
    cols, rows = int(np.floor(u_max / bw)) + 1, int(np.floor(v_max / bh)) + 1
    ids = np.floor(v / bh).astype(np.int64) * cols + np.floor(u / bw).astype(np.int64)
    return cols, rows, ids, np.bincount(ids, minlength=cols * rows)


def within_reference_bounds(pm, bw, bh):
    cols, rows, ids, lens = shape(pm, bw, bh)
    return (len(pm) <= REF_POINT_L and cols * rows <= REF_BUCKETS and (len(pm) == 0 or ids.min() >= 0)
            and len(lens) == cols * rows and lens.max(initial=0) <= REF_BUCKET_LEN)


def records(dtype, u, v):
    """Records that differ only where bucketFeatures looks (u1c, v1c) and in i1c, which names them."""
    pm = np.zeros(len(u), dtype)
    pm["u1c"], pm["v1c"] = u, v
    pm["i1c"] = np.arange(len(u))
    for f in ("i1p", "i2p", "i2c"):
        pm[f] = -1
    return pm


def field(rng, dtype, n, W, H, frac=None):
    """n records on distinct pixels of a W x H field; frac: None (integer coordinates), "quarter" or "float32"."""
    cells = rng.choice(W * H, n, replace=False)
    u, v = (cells % W).astype(np.float32), (cells // W).astype(np.float32)
    if frac == "quarter":
        u, v = u + rng.integers(0, 4, n).astype(np.float32) / 4, v + rng.integers(0, 4, n).astype(np.float32) / 4
    elif frac == "float32":
        # (< 1 after rounding to float32 too: the field's last column and row keep their bucket)
        u, v = u + np.minimum(rng.random(n, np.float32), np.float32(0.99)), v + np.minimum(rng.random(n, np.float32), np.float32(0.99))
    return records(dtype, u, v)


def lattice(rng, dtype, n, ku, kv, bw, bh):
    """n records on distinct nodes (i * bw, j * bh), i < ku, j < kv, the products rounded to float32: every
    coordinate lies exactly on a bucket edge where the size is exact in float32 and beside one where it is not."""
    nodes = rng.choice(ku * kv, n, replace=False)
    u = ((nodes % ku).astype(np.float32) * np.float32(bw)).astype(np.float32)
    v = ((nodes // ku).astype(np.float32) * np.float32(bh)).astype(np.float32)
    return records(dtype, u, v)


def with_holes(pm, bw, bh, holes):
    """The records outside the buckets `holes` (which then are empty)."""
    cols, rows, ids, _ = shape(pm, bw, bh)
    pm = pm[~np.isin(ids, holes)].copy()
    assert shape(pm, bw, bh)[:2] == (cols, rows), "a hole must not shrink the grid"
    pm["i1c"] = np.arange(len(pm))
    return pm


def five(pm, bw, bh):
    """max_features of 1, one less than the fullest bucket's length, equal to it, one above it, and 2**30."""
    top = int(shape(pm, bw, bh)[3].max())
    assert top >= 3
    return [(1, bw, bh), (top - 1, bw, bh), (top, bw, bh), (top + 1, bw, bh), (MF_ALL, bw, bh)]


def families(seed, dtype):
    rng = np.random.default_rng([seed, 20240613])
    out = []

    def add(name, pm, calls, grid=None, empty=False):
        for mf, bw, bh in calls:
            assert within_reference_bounds(pm, bw, bh), (name, mf, bw, bh)
            cols, rows, ids, lens = shape(pm, bw, bh)
            if grid is not None:
                assert cols * rows == grid, (name, cols, rows)
                assert lens[-1] > 0, (name, "the last bucket is empty")
            if empty:
                assert (lens == 0).any(), (name, "no empty bucket")
        out.append((name, pm, [(int(mf), float(np.float32(bw)), float(np.float32(bh))) for mf, bw, bh in calls]))

    # bucket sizes that are no integers
    pm = field(rng, dtype, 300, 360, 110)
    add("size_33.3", pm, five(pm, 33.3, 33.3), grid=44)
    pm = field(rng, dtype, 120, 21, 9, "quarter")
    add("size_1.5_quarter_pixel", pm, [(1, 1.5, 1.5), (2, 1.5, 1.5), (MF_ALL, 1.5, 1.5)], grid=84, empty=True)
    pm = field(rng, dtype, 300, 500, 100)
    k = rng.choice(300, 60, replace=False)  # some of them exactly on 50, 100, ...: beside the edges of 49.999996
    pm["u1c"][k] = np.round(pm["u1c"][k] / 50) * 50
    pm["v1c"][k[:30]] = np.round(pm["v1c"][k[:30]] / 50) * 50
    add("size_49.999996", pm, [(1, 49.999996, 49.999996), (3, 49.999996, 49.999996)])
    pm = field(rng, dtype, 200, 200, 100)
    add("size_beyond_the_field", pm, five(pm, 1000.0, 1000.0), grid=1)
    # coordinates on multiples of the bucket size
    add("edges_exact_size", lattice(rng, dtype, 100, 12, 9, 8.0, 4.0), [(1, 8.0, 4.0), (MF_ALL, 8.0, 4.0), (2, 16.0, 8.0), (MF_ALL, 16.0, 8.0)])
    add("edges_inexact_size", lattice(rng, dtype, 110, 10, 12, 33.3, 1.7), [(1, 33.3, 1.7), (MF_ALL, 33.3, 1.7), (2, 66.6, 3.4), (MF_ALL, 66.6, 3.4)])
    # arbitrary float32 coordinates
    pm = field(rng, dtype, 300, 300, 120, "float32")
    add("float32_fractions", pm, [(2, 27.7, 31.1), (MF_ALL, 27.7, 31.1)], grid=44)
    # grids around 64 buckets and at the reference's last bucket, with empty buckets and a last one that is not
    for grid, W, H in ((63, 90, 70), (64, 80, 80), (65, 130, 50), (126, 140, 90)):
        pm = field(rng, dtype, 260, W, H)
        pm = with_holes(pm, 10.0, 10.0, [1, grid // 2, grid - 2])
        add(f"grid_{grid}", pm, five(pm, 10.0, 10.0) if grid == 126 else [(2, 10.0, 10.0)], grid=grid, empty=True)
    return out
