"""The snake index -> bin-order position mapping that the flow tiles of match_kernel read from VhSets::snake_pos
(csrc/kernels_bin.hip: bin_sort writes it once per set, csrc/kernels_match.hip: flow_queries gathers it).

Every case takes the oracle's own features of a small synthetic image, keeps the subset that makes the shape it claims
(asserted on that subset), and compares findMatch of every query (flow and stereo) and the three methods with the
oracle, byte for byte, as tests/test_match_tile_paths.py does.  A feature list is free to hold any subset: the
matcher only sees records."""
import os
import subprocess
import sys

import numpy as np
import pytest

import multistage_oracle as mo
from test_match_tile_paths import TILE_Q, _check_all, _class_counts, _feats, _frames
from test_multistage import images_of, lone_lists, scene

pytestmark = pytest.mark.gpu


def _columns(a, c, b):
    """Occupied u-bin columns of class c (bins of b px), ascending, and the features per column."""
    col, n = np.unique(a[a[:, 3] == c][:, 0] // b, return_counts=True)
    return col, n


def _keep(a, mask):
    return np.ascontiguousarray(a[mask])


def _base(pkg, ob, oracle, W, H, over, seed):
    po = ob.Params.default(**over)
    dims = [W, H, pkg.synth.bytes_per_line(W)]
    return dims, _feats(oracle, po, dims, _frames(pkg, W, H, 3, 3, seed))


def case_tile_ends(pkg, ob, oracle):
    """Classes of 1, 32, 33 and 65 queries: a tile of one query, a class that ends exactly at the tile size, one query
    past it, and two full tiles and one query."""
    over = {"nms_tau": 30}
    dims, f = _base(pkg, ob, oracle, 400, 160, over, 41)
    keep = (1, TILE_Q, TILE_Q + 1, 2 * TILE_Q + 1)
    out = []
    for a in f:
        cnt = _class_counts(a)
        assert all(cnt[c] >= keep[c] for c in range(4)), cnt
        rows = np.concatenate([np.flatnonzero(a[:, 3] == c)[:keep[c]] for c in range(4)])
        out.append(_keep(a, np.sort(rows)))
        assert _class_counts(out[-1]) == list(keep)
    return over, dims, out


def _case_columns(pkg, ob, oracle, parity):
    """Bins of 4 px.  Class 0: all queries in ONE column of the given parity (the whole tile is one run, ascending or
    descending).  Class 1: two neighbouring occupied columns, the first of the other parity, fewer than 32 queries: one
    tile that crosses exactly two columns.  Class 2: at most 8 queries per column, so every full tile of 32 crosses at
    least four columns, even and odd.  Class 3: two occupied columns with an EMPTY one between them."""
    b = 4
    over = {"nms_tau": 40, "match_binsize": b, "match_radius": 60}
    dims, f = _base(pkg, ob, oracle, 480, 96, over, 23)
    out = []
    for a in f:
        u, c = a[:, 0] // b, a[:, 3]
        col0, n0 = _columns(a, 0, b)
        one = col0[(col0 % 2 == parity) & (n0 >= 2)][0]
        col1, _ = _columns(a, 1, b)
        pair = next((x, y) for x, y in zip(col1[:-1], col1[1:]) if y == x + 1 and x % 2 == 1 - parity)
        col3, _ = _columns(a, 3, b)
        x3 = next(x for x in col3 if x + 1 in col3 and x + 2 in col3)
        rank = np.zeros(len(a), np.int64)  # rank of a feature inside its (class, column)
        for key in np.unique(c * 1000 + u):
            idx = np.flatnonzero(c * 1000 + u == key)
            rank[idx] = np.arange(len(idx))
        m = ((c == 0) & (u == one)) | ((c == 1) & ((u == pair[0]) | (u == pair[1]))) | ((c == 2) & (rank < 8)) | \
            ((c == 3) & ((u == x3) | (u == x3 + 2)))
        k = _keep(a, m)
        out.append(k)
        cols, n = _columns(k, 0, b)
        assert len(cols) == 1 and cols[0] % 2 == parity and n[0] >= 2, (cols, n)
        cols, n = _columns(k, 1, b)
        assert len(cols) == 2 and cols[1] == cols[0] + 1 and cols[0] % 2 == 1 - parity and 2 <= n.sum() <= TILE_Q, (cols, n)
        cols, n = _columns(k, 2, b)
        assert n.max() <= 8 and n.sum() > 2 * TILE_Q and (cols % 2 == 0).any() and (cols % 2 == 1).any(), (n.max(), n.sum())
        cols, n = _columns(k, 3, b)
        assert list(cols) == [x3, x3 + 2], cols
    return over, dims, out


def case_columns_even_first(pkg, ob, oracle):
    return _case_columns(pkg, ob, oracle, 0)


def case_columns_odd_first(pkg, ob, oracle):
    return _case_columns(pkg, ob, oracle, 1)


def case_past_column_63(pkg, ob, oracle):
    """320 px in bins of 4 px: 80 u-bin columns.  Class 0 keeps only the columns 56..71, so its tiles run from below
    column 63 to above it (the walk over column starts, one lane per column, had to reload there); class 1 is dropped
    (an empty class between classes with tiles); classes 2 and 3 keep every column, on both sides of 63."""
    b = 4
    over = {"nms_tau": 40, "match_binsize": b, "match_radius": 60}
    dims, f = _base(pkg, ob, oracle, 320, 128, over, 11)
    assert (dims[0] + b - 1) // b == 80
    out = []
    for a in f:
        u, c = a[:, 0] // b, a[:, 3]
        k = _keep(a, ((c == 0) & (u >= 56) & (u < 72)) | (c >= 2))
        out.append(k)
        cols, n = _columns(k, 0, b)
        assert cols.min() < 63 < cols.max() and n.sum() >= 2, (cols, n)
        # one tile of class 0 holds queries on both sides: the queries below column 63 do not fill whole tiles
        assert n[cols < 63].sum() % TILE_Q != 0 and n[cols >= 63].sum() > 0, n
        assert _class_counts(k)[1] == 0
        for cc in (2, 3):
            cols, n = _columns(k, cc, b)
            assert cols.min() < 63 < cols.max() and n.sum() > TILE_Q, (cc, cols, n.sum())
    return over, dims, out


CASES = {"tile_ends": case_tile_ends, "columns_even_first": case_columns_even_first,
         "columns_odd_first": case_columns_odd_first, "past_column_63": case_past_column_63}


@pytest.mark.parametrize("name", sorted(CASES))
def test_snake_record_case(name, pkg, ob, oracle, gpu):
    """Each case on the loops and the library the environment selects (the speculative loops of the shipped build by
    default; the tests below run it again on the tested loops, without the snake and on the checking build)."""
    over, dims, f = CASES[name](pkg, ob, oracle)
    _check_all(pkg, oracle, pkg.Params.default(**over), ob.Params.default(**over), dims, f, name)


def _rerun(env_over):
    env = dict(os.environ, **env_over)
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-q", "-x", "-m", "gpu", "-k", "snake_record_case"],
                       env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "%d passed" % len(CASES) in r.stdout, r.stdout[-500:]


def test_snake_record_tested_loops(gpu):
    """VH_FLOW_TESTED=1: match_kernel<false> gathers the same positions."""
    _rerun({"VH_FLOW_TESTED": "1"})


def test_snake_record_without_snake(pkg, gpu):
    """libviso_hip_nosnake.so (-DVH_SNAKE=0): tiles over the plain bin order, no gather; speculative and tested loops."""
    assert os.path.exists(pkg.NOSNAKE_LIB_PATH), "build() makes it"
    _rerun({"VISO_HIP_LIB": pkg.NOSNAKE_LIB_PATH})
    _rerun({"VISO_HIP_LIB": pkg.NOSNAKE_LIB_PATH, "VH_FLOW_TESTED": "1"})


def test_snake_record_checking_build(pkg, gpu):
    """libviso_hip_check.so: every position gathered through snake_pos inside its class's span of the bin order (code 14,
    csrc/vh_dev.h) and every winner in range."""
    assert os.path.exists(pkg.CHECK_LIB_PATH), "build() makes it"
    _rerun({"VISO_HIP_LIB": pkg.CHECK_LIB_PATH})


def test_two_streams_with_different_feature_counts(pkg, ob, oracle, gpu):
    """snake_pos is per set: stream 1 holds about half as many features as stream 0 (its right half is blank), so a
    tile of stream 0 that read stream 1's array (or the reverse) would gather other positions."""
    W, H = 320, 160
    dims = [W, H, pkg.synth.bytes_per_line(W)]
    p, po = pkg.Params.default(), ob.Params.default()
    seqs = [pkg.synth.stereo_sequence(W, H, 2, disparity=6, blur=4, seed=3), scene(pkg, 2, w=W, h=H, seed=9)]
    g = pkg.StreamGroup(2, p)
    for t in range(2):
        g.pushBack(np.stack([s[t][0] for s in seqs]), np.stack([s[t][1] for s in seqs]), dims, False)
    g.matchFeatures(pkg.METHOD_QUAD)
    counts = []
    for i, s in enumerate(seqs):
        f = _feats(oracle, po, dims, [s[0][0], s[0][1], s[1][0], s[1][1]])
        counts.append(len(f[2]))
        assert g.getMatches(i).tobytes() == oracle.matching(po, dims, 2, *f).tobytes(), i
    g.close()
    assert counts[1] < 0.75 * counts[0] and counts[1] > 4 * TILE_Q, counts


def test_multi_stage_pair(pkg, ob, oracle, gpu):
    """Multi-stage quad matching of one pair (the sparse and the ranged dense searches both run flow tiles)."""
    W, H = 320, 160
    dims = [W, H, pkg.synth.bytes_per_line(W)]
    fr = scene(pkg, 2, seed=5)
    got = lone_lists(pkg, pkg.Params.default(multi_stage=1), fr, dims, (2,), True)
    want = mo.multistage(ob, oracle, ob.Params.default(multi_stage=1), dims, 2, images_of(2, fr[0], fr[1]))
    assert len(want["dense"]) > 0 and len(want["sparse"]) > 0
    assert got[(1, 2)].tobytes() == want["dense"].tobytes() and got[(1, 2, "sparse")].tobytes() == want["sparse"].tobytes()


def test_sequence_rows(pkg, ob, oracle, gpu):
    """Sequence mode: row r matches frame r - 1 with frame r of one camera, the sets resolved through vh_row_set."""
    W, H = 320, 160
    dims = [W, H, pkg.synth.bytes_per_line(W)]
    po = ob.Params.default()
    fr = scene(pkg, 3, seed=5)
    g = pkg.SequenceGroup(3, pkg.Params.default())
    g.pushBack(np.stack([f[0] for f in fr]), np.stack([f[1] for f in fr]), dims)
    g.matchFeatures(pkg.METHOD_QUAD)
    got = [g.getMatches(r) for r in range(3)]
    g.close()
    assert len(got[0]) == 0
    for t in (1, 2):
        f = _feats(oracle, po, dims, [fr[t - 1][0], fr[t - 1][1], fr[t][0], fr[t][1]])
        want = oracle.matching(po, dims, 2, *f)
        assert len(want) > 0 and got[t].tobytes() == want.tobytes(), t
