"""match_kernel's per-tile code around the SAD loops (csrc/kernels_match.hip: the gathers of flow_tile and
rows_tile, join_phases, finish_tile, the LDS-DMA chunk walk) on the shapes that the KITTI frames of the other
files do not reach.  Everything is compared with the oracle, bit for bit, as tests/test_gpu_parity.py does it."""
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

TILE_Q = 32  # csrc/vh_dev.h: VH_TILE_Q, queries per search tile


def _frames(pkg, W, H, blur, gain, seed, disp=5, dx=6, dy=2):
    return [pkg.synth.frame(W, H, 0, 0, blur, gain, seed), pkg.synth.frame(W, H, disp, 0, blur, gain, seed),
            pkg.synth.frame(W, H, dx, dy, blur, gain, seed), pkg.synth.frame(W, H, dx + disp, dy, blur, gain, seed)]


def _feats(oracle, po, dims, imgs):
    return [oracle.compute_features(po, im, dims)[1] for im in imgs]


def _class_counts(f):
    return [int((f[:, 3] == c).sum()) for c in range(4)]


def _check_all(pkg, oracle, p, po, dims, f, tag):
    """findMatch of every query, both kinds of pass and both directions, then the three methods."""
    for flow in (True, False):
        for q, c in ((2, 0), (0, 2), (2, 3)):
            got, want = pkg.match_all(p, dims, f[q], f[c], flow=flow), oracle.match_all(po, dims, f[q], f[c], flow=flow)
            assert np.array_equal(got, want), (tag, flow, q, c, int((got != want).sum()))
    for method in (0, 1, 2):
        assert pkg.match(p, dims, method, *f).tobytes() == oracle.matching(po, dims, method, *f).tobytes(), (tag, method)


# ---- the cases: name -> (parameter overrides, dims, four feature sets); each asserts that it is the shape it claims
def case_partial_last_tile(pkg, ob, oracle):
    """Classes of 32 + 5, 64 + 31, 1 and 33 features: last tiles of 5, 31, 1 and 1 queries (lanes past the end repeat
    the tile's first query and must neither store nor ask for a second search)."""
    W, H = 400, 160
    over = {"nms_tau": 30}
    po = ob.Params.default(**over)
    dims = [W, H, pkg.synth.bytes_per_line(W)]
    f = _feats(oracle, po, dims, _frames(pkg, W, H, 3, 3, 41))
    keep = (TILE_Q + 5, 2 * TILE_Q + 31, 1, TILE_Q + 1)
    out = []
    for a in f:
        cnt = _class_counts(a)
        assert all(cnt[c] >= keep[c] for c in range(4)), cnt
        rows = np.concatenate([np.flatnonzero(a[:, 3] == c)[:keep[c]] for c in range(4)])
        out.append(np.ascontiguousarray(a[np.sort(rows)]))
    assert _class_counts(out[0]) == list(keep)
    return over, dims, out


def case_empty_class(pkg, ob, oracle):
    """No feature of class 1 in the query sets, none of class 2 in the candidate sets: a class without tiles between
    classes that have them, and queries whose whole region is empty (result: index 0, matcher.cpp:221)."""
    W, H = 400, 160
    over = {"nms_tau": 40}
    po = ob.Params.default(**over)
    dims = [W, H, pkg.synth.bytes_per_line(W)]
    f = _feats(oracle, po, dims, _frames(pkg, W, H, 4, 2, 7))
    drop = (1, 2, 1, 2)
    out = [np.ascontiguousarray(a[a[:, 3] != d]) for a, d in zip(f, drop)]
    for a, d in zip(out, drop):
        cnt = _class_counts(a)
        assert cnt[d] == 0 and min(cnt[c] for c in range(4) if c != d) > TILE_Q, cnt
    return over, dims, out


def case_three_or_more_columns(pkg, ob, oracle):
    """Bins of 4 px on a 480 px wide image: no (class, u-bin) column holds 16 features, so two columns hold fewer than
    32 and every full tile of 32 snake-ordered queries runs through at least three (even and odd ones: both directions of the snake)."""
    W, H = 480, 96
    over = {"nms_tau": 40, "match_binsize": 4, "match_radius": 60}
    po = ob.Params.default(**over)
    dims = [W, H, pkg.synth.bytes_per_line(W)]
    f = _feats(oracle, po, dims, _frames(pkg, W, H, 3, 3, 23))
    for a in f:
        col = a[:, 3] * 1000 + a[:, 0] // 4
        assert np.bincount(col).max() < 16 and min(_class_counts(a)) > 2 * TILE_Q, (np.bincount(col).max(), _class_counts(a))
    return over, dims, f


def case_noise(pkg, ob, oracle):
    """Four independent noise images: no feature has a partner, so a large share of the winners over the walked region
    lies outside the query's own window -- second searches (finish_tile: RedoGroup) in flow and stereo passes alike."""
    W, H = 320, 128
    over = {}
    po = ob.Params.default(**over)
    dims = [W, H, pkg.synth.bytes_per_line(W)]
    rng = np.random.default_rng(99)
    f = _feats(oracle, po, dims, [rng.integers(0, 256, (H, dims[2]), dtype=np.uint8) for _ in range(4)])
    assert min(min(_class_counts(a)) for a in f) > TILE_Q
    return over, dims, f


def case_wide_unmerged_regions(pkg, ob, oracle):
    """Bins of 2 px and a radius of 70 px: the own window of every query away from the left and right borders spans
    71 u-bin columns, more than one batch of the walkers' 64-column table, and the features are kept to a band of rows
    whose windows never reach the top row of bins, so no region -- of a tile or of a group of second searches -- is the
    single merged run of positions that KITTI-sized frames walk.  Noise images, as in case_noise: the second searches
    walk such regions too."""
    W, H = 480, 256
    b, r = 2, 70
    over = {"match_binsize": b, "match_radius": r}
    po = ob.Params.default(**over)
    dims = [W, H, pkg.synth.bytes_per_line(W)]
    assert 2 * r // b + 1 > 64 and 2 * r + b < H
    rng = np.random.default_rng(5)
    f = _feats(oracle, po, dims, [rng.integers(0, 256, (H, dims[2]), dtype=np.uint8) for _ in range(4)])
    f = [np.ascontiguousarray(a[(a[:, 1] >= 100) & (a[:, 1] <= 140)]) for a in f]
    vbn = (H + b - 1) // b
    for a in f:
        u, v = a[:, 0], a[:, 1]
        inner = (u >= r) & (u + r <= W - 1)
        assert inner.sum() > 4 * TILE_Q and ((u[inner] + r) // b - (u[inner] - r) // b + 1).min() > 64
        # any union of these windows starts below the first row of bins and ends above the last: never all v-bins
        assert (v.min() - r) // b > 0 and (v.max() + r) // b < vbn - 1
        assert min(_class_counts(a)) > TILE_Q, _class_counts(a)
    return over, dims, f


CASES = {"partial_last_tile": case_partial_last_tile, "empty_class": case_empty_class,
         "three_or_more_columns": case_three_or_more_columns, "noise": case_noise,
         "wide_unmerged_regions": case_wide_unmerged_regions}


@pytest.mark.parametrize("name", sorted(CASES))
def test_tile_paths_case(name, pkg, ob, oracle, gpu):
    """Each case under the loops the environment selects: the speculative ones with 16-bit position keys by default;
    the tests below run this test again with the tested loops and with the wider keys."""
    over, dims, f = CASES[name](pkg, ob, oracle)
    _check_all(pkg, oracle, pkg.Params.default(**over), ob.Params.default(**over), dims, f, name)


def _rerun(env_over):
    env = dict(os.environ, **env_over)
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-q", "-x", "-m", "gpu", "-k", "tile_paths_case"],
                       env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "%d passed" % len(CASES) in r.stdout, r.stdout[-500:]


@pytest.mark.parametrize("mode", ["1", "2"])
def test_tile_paths_wide_keys(mode, gpu):
    """KEY_W19 (VH_FLOW_WIDE_KEYS=1: the 32-bit join, another position mask) and KEY_64 (=2: the 64-bit join) through
    the same cases, speculative and tested loops (the switch is read once per process: a subprocess)."""
    _rerun({"VH_FLOW_WIDE_KEYS": mode})
    _rerun({"VH_FLOW_WIDE_KEYS": mode, "VH_FLOW_TESTED": "1"})


def test_tile_paths_tested_loops(gpu):
    """VH_FLOW_TESTED=1: match_kernel<false>, the accept test per pair in the flow and the stereo loops, no second
    searches; and =0, the speculative loops whatever the statistics say."""
    _rerun({"VH_FLOW_TESTED": "1"})
    _rerun({"VH_FLOW_TESTED": "0"})


def test_tile_paths_checking_build(pkg, gpu):
    """The same cases on libviso_hip_check.so: every winner position and row-order position in range."""
    assert os.path.exists(pkg.CHECK_LIB_PATH), "build() makes it"
    _rerun({"VISO_HIP_LIB": pkg.CHECK_LIB_PATH})


@pytest.mark.parametrize("method", ["flow", "stereo"])
def test_noise_forces_second_searches(method, pkg, ob, oracle, gpu, monkeypatch):
    """The noise case really reaches the second searches, for flow passes alone and for stereo passes alone: a group
    held to the speculative loops reports the share of re-searched queries, and its matches are the oracle's.  The bar is
    1 %: twice the share of frames whose features all have partners (0.5 %, kernels_match.hip), and with more than 4 000
    queries per launch here more than 40 second searches per launch -- both query slots, groups of two and a last group
    of one.  (Measured on MI355X: flow 5.8 %.)"""
    monkeypatch.setenv("VH_FLOW_TESTED", "0")
    W, H = 320, 128
    dims = [W, H, pkg.synth.bytes_per_line(W)]
    p, po = pkg.Params.default(), ob.Params.default()
    rng = np.random.default_rng(7)
    frames = [[rng.integers(0, 256, (H, dims[2]), dtype=np.uint8) for _ in range(2)] for _ in range(4)]
    g = pkg.StreamGroup(1, p)
    prev = None
    for left, right in frames:
        g.pushBack(left[None], right[None], dims, False)
        if method == "stereo":
            g.matchFeatures(pkg.METHOD_STEREO)
            fl, fr = _feats(oracle, po, dims, [left, right])
            assert g.getMatches(0).tobytes() == oracle.matching(po, dims, 1, m1c=fl, m2c=fr).tobytes()
        elif prev is not None:
            g.matchFeatures(pkg.METHOD_FLOW)
            fp, fc = _feats(oracle, po, dims, [prev, left])
            assert g.getMatches(0).tobytes() == oracle.matching(po, dims, 0, m1p=fp, m1c=fc).tobytes()
        prev = left
    spec, rate = g.searchStats()
    g.close()
    assert spec and rate > 0.01, (spec, rate)
