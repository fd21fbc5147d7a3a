"""The trip loop of flow_tile (csrc/kernels_match.hip): chunk-local keys, rebuilt into global keys once per query and
chunk, the unrolled full chunk against the counted partial one, and findMatch's first-minimum tie-break through both.
Synthetic feature sets of a few hundred records put an exact number of candidates into the region a tile walks and
identical descriptors at chosen bin-order positions; everything is compared with the oracle, bit for bit, through the
stateless entries, under the speculative loops (match_kernel<true>) and the tested ones (match_kernel<false>)."""
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

P, TRIP, CHUNK = 4, 8, 64  # csrc/vh_dev.h, kernels_match.hip: phases, candidates per trip, candidates per LDS buffer
W, H, BIN = 1200, 100, 50  # 24 x 2 bins; the candidates of interest live in u-bins UB and UB + 1
UB = 20
NQ = 40                    # queries per class: one full tile of 32 and one of 8
HI16_MAX = 0x10000 - 64    # kernels_match.hip: key_mode_of -- classes above this take the 19-bit key


def _rows(u, v, cls, desc):
    """Feature records [n, 12]: u, v, value, class, 32 descriptor bytes."""
    n = len(u)
    out = np.zeros((n, 12), np.int32)
    out[:, 0], out[:, 1], out[:, 2], out[:, 3] = u, v, 100, cls
    out[:, 4:] = np.ascontiguousarray(desc, dtype=np.uint8).reshape(n, 32).view(np.int32)
    return out


def _desc(f):
    return np.ascontiguousarray(f[:, 4:]).view(np.uint8).reshape(len(f), 32).astype(np.int32)


def _queries(rng, radius):
    """NQ queries per class.  u in [1050, 1100): with the radius of 200 the window starts at u - 200 >= 850, past u-bins
    0 .. 16 (where the 19-bit case parks its filler), and covers u-bins UB and UB + 1 whole.  With the small radius the windows cut
    through those bins: the tested loops then meet border columns, interior ones and rejected candidates."""
    parts = []
    for c in range(4):
        u = rng.integers(1050, 1100, NQ) if radius >= 200 else rng.integers(990, 1110, NQ)
        parts.append(_rows(u, rng.integers(0, H, NQ), c, rng.integers(0, 256, (NQ, 32))))
    return np.concatenate(parts[::-1])  # classes in descending order: a list index is not a bin-order position


def _column(rng, n, cls, ubin=UB):
    """n candidates of one class in ONE bin: their bin-order positions are their list order."""
    return _rows(rng.integers(ubin * BIN, ubin * BIN + BIN, n), rng.integers(0, BIN, n), cls, rng.integers(0, 256, (n, 32)))


def _check(pkg, ob, oracle, over, fq, fc, tag):
    p, po = pkg.Params.default(**over), ob.Params.default(**over)
    dims = [W, H, pkg.synth.bytes_per_line(W)]
    want = oracle.match_all(po, dims, fq, fc, flow=True)
    got = pkg.match_all(p, dims, fq, fc, flow=True)
    assert np.array_equal(got, want), (tag, int((got != want).sum()), np.flatnonzero(got != want)[:8])
    return want


# ---- candidate counts: one trip, partial chunks, chunk crossings
COUNTS = {"one_trip": (TRIP,), "partial_chunk": (TRIP + 1, CHUNK - 1), "chunk_crossing": (CHUNK, CHUNK + 1, 2 * CHUNK + 1)}


def case_counts(name, pkg, ob, oracle):
    """Every class holds exactly n candidates, all in one column (one bin) that every tile's region contains: the walk is
    n // 64 full chunks and one of n % 64 candidates, rounded up to whole trips with copies of the last candidate.  With
    random descriptors a copy that won, a position rebuilt with the wrong chunk base, or a counted path that disagrees
    with the unrolled one changes some query's answer."""
    for n in COUNTS[name]:
        for radius in (200, 30):
            rng = np.random.default_rng(1000 * n + radius)
            over = {"match_binsize": BIN, "match_radius": radius}
            fq = _queries(rng, radius)
            fc = np.concatenate([_column(rng, n, c) for c in (3, 2, 1, 0)])
            assert all(int((fc[:, 3] == c).sum()) == n for c in range(4))
            assert (fc[:, 0] // BIN == UB).all() and (fc[:, 1] // BIN == 0).all()
            want = _check(pkg, ob, oracle, over, fq, fc, (name, n, radius))
            if radius >= 200:  # every candidate is inside every window: each query has a winner
                assert (want >= 0).all()


# ---- ties
# (positions within the class, in bin order) of the candidates that share the best descriptor of one query each
TIES = {"same_lane": (5, 13),        # slots 5 and 13 of chunk 0: phase 1, steps k = 1 and 3 of one lane's sequence
        "two_phases": (18, 19),      # chunk 0, phases 2 and 3
        "two_chunks": (30, 100),     # chunks 0 and 1
        "later_chunk_smaller_k": (7, 70),  # chunk 0 step k = 1, chunk 1 step k = 1 of another phase: local keys tie-break alike
        "three_chunks": (60, 64, 130),     # last trip of chunk 0, first of chunk 1, the partial chunk 2
        "two_columns": (40, 140 + 7)}      # u-bins UB and UB + 1 (another column of the tested loops' walk)
N4, N5 = 140, 20  # candidates per class in u-bins UB and UB + 1: chunks of 64, 64 and 12 + 20 (merged run) or 12 | 20 (columns)


def _tie_sets(rng, big_class=None):
    fq = _queries(rng, 200)
    qd = _desc(fq)
    parts, first = [], {}
    for c in (3, 2, 1, 0):
        col = np.concatenate([_column(rng, N4, c, UB), _column(rng, N5, c, UB + 1)])
        cd = np.ascontiguousarray(col[:, 4:]).view(np.uint8).reshape(len(col), 32)
        qi = np.flatnonzero(fq[:, 3] == c)
        for k, (name, pos) in enumerate(TIES.items()):
            near = qd[qi[k]].copy()
            near[k] ^= 3  # the shared descriptor: the query's own but for one byte
            for q in pos:
                cd[q] = near
        col[:, 4:] = cd.view(np.int32).reshape(len(col), 8)
        if c == big_class:  # filler of the class in u-bins 0 .. 16, outside every window, AHEAD of the column in bin order
            n = HI16_MAX + 1 - len(col)
            col = np.concatenate([col, _rows(rng.integers(0, 17 * BIN, n), rng.integers(0, H, n), c, rng.integers(0, 256, (n, 32)))])
        first[c] = sum(len(x) for x in parts)
        parts.append(col)
    return fq, np.concatenate(parts), first


def _check_ties(pkg, ob, oracle, big_class=None):
    rng = np.random.default_rng(2024)
    fq, fc, first = _tie_sets(rng, big_class)
    over = {"match_binsize": BIN, "match_radius": 200}
    want = _check(pkg, ob, oracle, over, fq, fc, ("ties", big_class))
    qd, cd = _desc(fq), _desc(fc)
    for c in range(4):
        qi = np.flatnonzero(fq[:, 3] == c)
        for k, (name, pos) in enumerate(TIES.items()):
            # the case is what it claims: exactly these candidates share the query's smallest SAD ...
            sad = np.abs(cd[fc[:, 3] == c] - qd[qi[k]]).sum(1)
            assert sorted(np.flatnonzero(sad == sad.min())) == sorted(pos), (name, c)
            # ... and the winner is the one at the lowest bin-order position
            assert want[qi[k]] == first[c] + min(pos), (name, c, int(want[qi[k]]), first[c], pos)
    return fc


def case_ties(name, pkg, ob, oracle):
    """Identical best descriptors in one lane's sequence of a chunk, in two phases of a chunk, in different chunks and in
    different columns: the lowest bin-order position wins each time (16-bit keys; 64-bit with VH_FLOW_WIDE_KEYS=2)."""
    _check_ties(pkg, ob, oracle)


def case_ties_w19(name, pkg, ob, oracle):
    """The same ties in a class of 65 473 candidates: the 19-bit key, with all positions of interest above 2^16 - 200."""
    fc = _check_ties(pkg, ob, oracle, big_class=2)
    assert int((fc[:, 3] == 2).sum()) + 64 > 0x10000


CASES = {"one_trip": case_counts, "partial_chunk": case_counts, "chunk_crossing": case_counts, "ties": case_ties,
         "ties_w19": case_ties_w19}


@pytest.mark.parametrize("name", sorted(CASES))
def test_chunk_keys_case(name, pkg, ob, oracle, gpu):
    """Each case under the loops the environment selects: the speculative ones by default; the tests below run this test
    again with the tested loops and with the 64-bit keys."""
    CASES[name](name, pkg, ob, oracle)


def _rerun(env_over, skip=()):
    env = dict(os.environ, **env_over)
    expr = "chunk_keys_case" + "".join(" and not " + s for s in skip)
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-q", "-x", "-m", "gpu", "-k", expr],
                       env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "%d passed" % (len(CASES) - len(skip)) in r.stdout, r.stdout[-500:]


def test_chunk_keys_tested_loops(gpu):
    """VH_FLOW_TESTED=1: match_kernel<false> -- full tests, v tests and the three-range interior column over the same
    chunks, 16-bit and 19-bit keys (the switch is read once per process: a subprocess)."""
    _rerun({"VH_FLOW_TESTED": "1"})


@pytest.mark.parametrize("tested", ["0", "1"])
def test_chunk_keys_wide_keys(tested, gpu):
    """VH_FLOW_WIDE_KEYS=2: the 64-bit key, speculative and tested loops (without the large class: its size would select
    nothing here, the switch overrides it)."""
    _rerun({"VH_FLOW_WIDE_KEYS": "2", "VH_FLOW_TESTED": tested}, skip=("ties_w19",))


def test_chunk_keys_second_searches(pkg, ob, oracle, gpu, monkeypatch):
    """Noise frames under the speculative loops: more than 1 % of the queries are searched again (finish_tile's second
    searches take the winners of the new loop as their input), and the matches are the oracle's."""
    monkeypatch.setenv("VH_FLOW_TESTED", "0")
    w, h = 320, 128
    dims = [w, h, pkg.synth.bytes_per_line(w)]
    p, po = pkg.Params.default(), ob.Params.default()
    rng = np.random.default_rng(11)
    frames = [rng.integers(0, 256, (h, dims[2]), dtype=np.uint8) for _ in range(4)]
    g = pkg.StreamGroup(1, p)
    prev = None
    for left in frames:
        g.pushBack(left[None], left[None], dims, False)
        if prev is not None:
            g.matchFeatures(pkg.METHOD_FLOW)
            fp, fc = [oracle.compute_features(po, im, dims)[1] for im in (prev, left)]
            assert g.getMatches(0).tobytes() == oracle.matching(po, dims, 0, m1p=fp, m1c=fc).tobytes()
        prev = left
    spec, rate = g.searchStats()
    g.close()
    assert spec and rate > 0.01, (spec, rate)
