"""vote_select_kernel's bucketing (csrc/kernels_vote.hip: Matcher::bucketFeatures on the device -- a stable radix sort
by bucket, three wave scans over the grid in chunks of 64 buckets, one serial shuffle per bucket, a gather) at the
edges of its grid, its sort, its buckets and its capacities, through vh_remove_outliers_device and the group's device
post chain.  Everything is byte-exact against oracle.bucket_features(oracle.remove_outliers(pm)[0], ...), which
tests/test_oracle.py pins to the reference inside the reference's own bounds (tests/golden/bucket_edges.npz).

As in tests/test_match_tile_paths.py every case builds its input and asserts that it is the shape it claims -- from
the ORACLE's survivors, never from the device's output.  A batch holds lists of different shapes under one pair of
bucket sizes (the sizes belong to the call), so that a kernel reading a neighbour's grid or sort buffer shows.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

from oracle import bucket_edges as be
from test_outliers import random_matches

MF_ALL = 2 ** 30
CHUNK = 64  # buckets per step of the kernel's scan and shuffle loops (one per lane)


# ---------------------------------------------------------------------------------------------- building blocks
def smooth_flow(pm):
    pm["u1p"], pm["v1p"] = pm["u1c"] + 3, pm["v1c"] - 1  # (random_matches' flow before it disturbs some of it)


def move_points(pm, u, v):
    """Other coordinates for the current-frame points, every record keeping its flow."""
    du, dv = pm["u1p"] - pm["u1c"], pm["v1p"] - pm["v1c"]
    pm["u1c"], pm["v1c"] = u, v
    pm["u1p"], pm["v1p"] = pm["u1c"] + du, pm["v1c"] + dv
    return pm


def without_buckets(pm, bw, bh, holes):
    """The list without the records of the buckets `holes` (of the INPUT's grid; the case asserts what the vote left)."""
    _, _, ids, _ = be.shape(pm, bw, bh)
    return pm[~np.isin(ids, holes)].copy()


def list_with_survivors(pkg, oracle, target, seed):
    """A random_matches list of which the vote keeps exactly `target` records."""
    for n in range(target + 1, target + 300):
        pm = random_matches(pkg, np.random.default_rng([seed, n]), n, W=160, H=120)
        if len(oracle.remove_outliers(pm)[0]) == target:
            return pm
    raise AssertionError(f"no list with {target} survivors")


def digits_of(ids):
    """Radix digits (of 8 bits) the largest occupied bucket id has: the passes wave_radix_sort cannot all skip."""
    top = int(ids.max())
    return 1 + (top >= 1 << 8) + (top >= 1 << 16) + (top >= 1 << 24)


class Case:
    """Lists of one batch, the oracle's survivors of each, and the (max_features, bw, bh) calls to compare."""

    def __init__(self, oracle, lists, calls):
        self.lists, self.calls = lists, calls
        self.surv = [oracle.remove_outliers(pm)[0] for pm in lists]
        self.want = {c: [oracle.bucket_features(s, c[0], c[1], c[2]) if c[0] >= 1 else s for s in self.surv] for c in calls}

    def shapes(self, bw, bh):
        return [be.shape(s, bw, bh) for s in self.surv]


# ---------------------------------------------------------------------------------------------- the cases
def case_grid_around_the_chunks(pkg, oracle):
    """Survivor grids of 1, 2, 63, 64, 65, 127 and 129 buckets of 10 x 10 pixels: no chunk at all beyond the first, a
    last chunk of 63 and of 1 lanes (the `b < nb` guard of the scans and of the shuffle), a full lane 63 and an empty
    one behind the carry, and the count rewrite across a chunk boundary.  Every grid beyond 2 has empty buckets."""
    rng = np.random.default_rng(101)
    fields = {1: (10, 10, 40), 2: (20, 10, 70), 63: (90, 70, 700), 64: (80, 80, 700), 65: (130, 50, 700), 127: (1270, 10, 1500), 129: (430, 30, 1400)}
    lists = []
    for grid, (W, H, n) in fields.items():
        pm = random_matches(pkg, rng, n, W=W, H=H)
        lists.append(without_buckets(pm, 10.0, 10.0, [1, grid // 2, grid - 3]) if grid > 2 else pm)
    c = Case(oracle, lists, [(2, 10.0, 10.0), (MF_ALL, 10.0, 10.0)])
    for grid, (cols, rows, ids, lens) in zip(fields, c.shapes(10.0, 10.0)):
        assert cols * rows == grid and lens[-1] > 0, (grid, cols, rows, lens[-1])
        assert grid <= 2 or (lens == 0).any(), grid
    assert c.shapes(10.0, 10.0)[4][3][CHUNK - 1] > 0  # (65 buckets: lane 63 of the first chunk carries a non-empty bucket)
    return c


def case_radix_two_digits_at_the_boundary(pkg, oracle):
    """255, 256 and 257 buckets: the largest occupied bucket id is 254, 255 (one digit: pass 1 is skipped) and 256 (two:
    pass 1 sorts, and the result comes back from the other ping-pong buffer)."""
    rng = np.random.default_rng(102)
    fields = {255: (170, 150), 256: (160, 160), 257: (2570, 10)}
    lists = [random_matches(pkg, rng, 2500, W=W, H=H) for W, H in fields.values()]
    c = Case(oracle, lists, [(2, 10.0, 10.0)])
    for grid, (cols, rows, ids, lens) in zip(fields, c.shapes(10.0, 10.0)):
        assert cols * rows == grid and ids.max() == grid - 1 and digits_of(ids) == (2 if grid == 257 else 1), (grid, cols, rows, ids.max())
    return c


def case_radix_two_and_three_digits(pkg, oracle):
    """Buckets of 2 x 2 pixels and of one pixel on 640 x 240: about 38 400 buckets (two digits) and more than 65 536 (three),
    next to a list on a small field that needs one digit fewer under the same sizes."""
    rng = np.random.default_rng(103)
    lists = [random_matches(pkg, rng, 3000), random_matches(pkg, rng, 300), random_matches(pkg, rng, 600, W=100, H=50)]
    c = Case(oracle, lists, [(2, 2.0, 2.0), (1, 1.0, 1.0), (5, 1.0, 1.0)])
    two, one = c.shapes(2.0, 2.0), c.shapes(1.0, 1.0)
    assert 38000 < two[0][0] * two[0][1] <= 38400 and [digits_of(s[2]) for s in two] == [2, 2, 2], [s[:2] for s in two]
    assert 150000 < one[0][0] * one[0][1] <= 153600 and one[0][2].max() > 65536
    assert [digits_of(s[2]) for s in one] == [3, 3, 2], [int(s[2].max()) for s in one]
    assert max(s[3].max() for s in two) >= 2  # (some bucket of 2 x 2 pixels holds more than one record)
    return c


def case_single_bucket_occupancy(pkg, oracle):
    """Bucket sizes beyond the field: one bucket holds all survivors -- 1, 2, 63, 64, 65 and some 2 500 of them, so one
    lane shuffles the whole list -- with max_features of 1, len - 1, len, len + 1 (for len = 64 and the long list) and 2**30."""
    rng = np.random.default_rng(104)
    lists = [random_matches(pkg, rng, 40)[:1], random_matches(pkg, rng, 40)[:2]]
    lists += [list_with_survivors(pkg, oracle, k, 104) for k in (63, 64, 65)]
    lists.append(random_matches(pkg, rng, 3000))
    surv = [len(oracle.remove_outliers(pm)[0]) for pm in lists]
    assert surv[:5] == [1, 2, 63, 64, 65] and 2300 < surv[5] < 2800, surv
    L = surv[5]
    c = Case(oracle, lists, [(mf, 4000.0, 4000.0) for mf in (1, 63, 64, 65, L - 1, L, L + 1, MF_ALL)])
    assert all(cols * rows == 1 for cols, rows, _, _ in c.shapes(4000.0, 4000.0))
    assert [len(w) for w in c.want[(64, 4000.0, 4000.0)]] == [1, 2, 63, 64, 64, 64]
    assert len(c.want[(L - 1, 4000.0, 4000.0)][5]) == L - 1 and len(c.want[(L + 1, 4000.0, 4000.0)][5]) == L
    return c


def case_crowded_bucket_among_sparse_ones(pkg, oracle):
    """4 x 2 buckets of 50 x 50 pixels: the first holds more than 256 survivors (beyond what the reference's
    buckets[126][256] can hold), every other one 0 or 1."""
    rng = np.random.default_rng(105)
    dense = random_matches(pkg, rng, 600, W=48, H=48)
    far = random_matches(pkg, rng, 60, W=200, H=100)
    smooth_flow(far)
    _, _, ids, _ = be.shape(far, 50.0, 50.0)
    pick = [np.flatnonzero(ids == b)[0] for b in (1, 2, 5, 6, 7)]  # one record in five of the other seven buckets
    pm = np.concatenate([dense, far[pick]])
    pm["i1c"] = pm["i1p"] = np.arange(len(pm))
    c = Case(oracle, [pm, random_matches(pkg, rng, 500, W=200, H=100)], [(1, 50.0, 50.0), (300, 50.0, 50.0), (MF_ALL, 50.0, 50.0)])
    cols, rows, _, lens = c.shapes(50.0, 50.0)[0]
    assert (cols, rows) == (4, 2) and lens[0] > 256 and set(lens[1:]) == {0, 1} and lens[-1] == 1, lens
    return c


SIZES = (33.3, 1.5, 49.999996, 1.0)


def case_fractional_sizes_and_coordinates(pkg, oracle):
    """Bucket sizes of 33.3, 1.5, 49.999996 and 1.0 on lists with integer, quarter-pixel and arbitrary float32
    coordinates, and on lists a third of whose coordinates lie exactly on float32(k * size): floorf(u / size) next to
    an integer.  The vote itself runs on these coordinates."""
    rng = np.random.default_rng(106)
    lists = [random_matches(pkg, rng, 1200)]
    pm = random_matches(pkg, rng, 900)
    lists.append(move_points(pm, pm["u1c"] + rng.integers(0, 4, 900).astype(np.float32) / 4, pm["v1c"] + rng.integers(0, 4, 900).astype(np.float32) / 4))
    pm = random_matches(pkg, rng, 900)
    lists.append(move_points(pm, pm["u1c"] + np.minimum(rng.random(900, np.float32), np.float32(0.99)),
                             pm["v1c"] + np.minimum(rng.random(900, np.float32), np.float32(0.99))))
    for size in SIZES[:3]:
        pm = random_matches(pkg, rng, 700)
        s = np.float32(size)
        u, v = pm["u1c"].copy(), pm["v1c"].copy()
        k = rng.permutation(700)
        u[k[:250]] = np.round(u[k[:250]] / s).astype(np.float32) * s  # (products rounded to float32)
        v[k[150:400]] = np.round(v[k[150:400]] / s).astype(np.float32) * s
        lists.append(move_points(pm, u, v))
    c = Case(oracle, lists, [(2, s, s) for s in SIZES] + [(MF_ALL, 33.3, 1.5)])
    frac = [float(np.mean(s["u1c"] != np.floor(s["u1c"]))) for s in c.surv]
    assert frac[0] == 0 and frac[1] > 0.5 and frac[2] > 0.9, frac
    for size, s in zip(SIZES[:3], c.surv[3:]):
        q = s["u1c"] / np.float32(size)
        on_edge = (np.round(q).astype(np.float32) * np.float32(size) == s["u1c"]) & (s["u1c"] > 0)
        assert on_edge.sum() > 50, (size, int(on_edge.sum()))
    for size in SIZES:
        assert all(cols * rows > 8 for cols, rows, _, _ in c.shapes(size, size))
    return c


def case_compaction_steps(pkg, oracle):
    """Lists of 64 * 4 - 1 and 64 * 4 + 1 records in which the vote drops all of records 64..127 and keeps all of
    128..191: a 64-record step of the in-place compaction that stores nothing, followed by one in which every lane
    stores, 64 positions further down than it loaded."""
    lists = []
    for n, seed in ((255, 1071), (257, 1072)):
        rng = np.random.default_rng(seed)
        pm = random_matches(pkg, rng, n, W=200, H=120)
        # records 128..191 take the 64 positions farthest from the field's border: each other's neighbours, away from the hull
        inner = np.argsort(-np.minimum(np.minimum(pm["u1c"], 199 - pm["u1c"]), np.minimum(pm["v1c"], 119 - pm["v1c"])), kind="stable")[:64]
        rest = np.setdiff1d(np.arange(n), inner)
        at = np.concatenate([rest[:128], inner, rest[128:]])
        move_points(pm, pm["u1c"][at], pm["v1c"][at])
        smooth_flow(pm[64:192])
        # garbage: flows that differ from the smooth one and from each other by far more than the vote's tolerance of 5
        pm["u1p"][64:128] = pm["u1c"][64:128] + 40 + 11 * rng.permutation(64).astype(np.float32)
        pm["v1p"][64:128] = pm["v1c"][64:128] - 40 - 11 * rng.permutation(64).astype(np.float32)
        lists.append(pm)
    lists.append(random_matches(pkg, np.random.default_rng(1073), 320, W=200, H=120))
    c = Case(oracle, lists, [(0, 50.0, 50.0), (2, 50.0, 50.0)])
    for pm, s in zip(lists[:2], c.surv[:2]):
        kept = np.isin(pm["i1c"], s["i1c"])
        assert not kept[64:128].any() and kept[128:192].all(), (int(kept[64:128].sum()), int(kept[128:192].sum()))
        assert 0 < kept[:64].sum() and kept[192:].any()
    return c


CASES = {f.__name__[5:]: f for f in (case_grid_around_the_chunks, case_radix_two_digits_at_the_boundary, case_radix_two_and_three_digits,
                                      case_single_bucket_occupancy, case_crowded_bucket_among_sparse_ones,
                                      case_fractional_sizes_and_coordinates, case_compaction_steps)}
_built = {}


def built(name, pkg, oracle):
    """(the reference answers of a case are computed once and shared by its parameter sets)"""
    if name not in _built:
        _built[name] = CASES[name](pkg, oracle)
    return _built[name]


# ---------------------------------------------------------------------------------------------- the device against them
@pytest.mark.gpu
@pytest.mark.parametrize("lanes", [1, 16])
@pytest.mark.parametrize("name", sorted(CASES))
def test_bucketing_case(name, lanes, pkg, oracle, gpu):
    """Each case's batch under each of its calls, and once more with the lists in reverse order: the same buffer sizes, so
    that a slot's scratch -- where the allocation comes back -- still holds what a list of another grid left there."""
    c = built(name, pkg, oracle)
    for call in c.calls:
        mf, bw, bh = call
        for order in (slice(None), slice(None, None, -1)):
            got, _, _ = pkg.remove_outliers_device(c.lists[order], lanes_per_wave=lanes, max_features=mf, bucket_width=bw, bucket_height=bh)
            for k, (g, w) in enumerate(zip(got, c.want[call][order])):
                assert g.tobytes() == w.tobytes(), (name, call, order, k, len(g), len(w))


@pytest.mark.gpu
@pytest.mark.parametrize("lanes", [1, 16])
def test_bucketing_statuses(lanes, pkg, oracle, gpu):
    """Lists of 0, 1 and 3 records (VH_VOTE_SKIP: untouched, then bucketed), a collinear list and one of identical points
    (every record loses: no survivors, nothing out, no error), and a list with negative coordinates -- VH_ERR_UNSUPPORTED
    for it alone -- between healthy lists of the same wave."""
    rng = np.random.default_rng(108)
    base = random_matches(pkg, rng, 40)
    line = random_matches(pkg, rng, 12)
    line["v1c"] = 50
    line["u1c"] = np.arange(12) * 7
    same = random_matches(pkg, rng, 9)
    same["u1c"] = 33
    same["v1c"] = 44
    neg = random_matches(pkg, rng, 50)
    neg["u1c"] -= 1000
    neg["u1p"] -= 1000
    lists = [base[:0], base[:1], random_matches(pkg, rng, 300), base[:3], line, neg, same, random_matches(pkg, rng, 700)]
    surv = [oracle.remove_outliers(pm)[0] for pm in lists]
    assert [len(s) for s in surv[:2]] == [0, 1] and len(surv[3]) == 3 and len(surv[4]) == 0 and len(surv[6]) == 0
    assert 20 < len(surv[5]) and (surv[5]["u1c"] < 0).all()  # (the vote is defined on them; their bucket grid is not)
    healthy = [k for k in range(len(lists)) if k != 5]
    got, _, _, rc, counts = pkg.remove_outliers_device(lists, lanes_per_wave=lanes, max_features=2, bucket_width=50.0, bucket_height=50.0,
                                                       strict=False, with_counts=True)
    assert rc == pkg.VH_ERR_UNSUPPORTED and counts[5] == 0 and len(got[5]) == 0
    for k in healthy:
        assert got[k].tobytes() == oracle.bucket_features(surv[k], 2, 50.0, 50.0).tobytes(), k
    assert counts[4] == 0 and counts[6] == 0
    got, _, _ = pkg.remove_outliers_device([lists[k] for k in healthy], lanes_per_wave=lanes, max_features=1, bucket_width=7.5, bucket_height=7.5)
    for g, k in zip(got, healthy):  # without the refused list: no error at all
        assert g.tobytes() == oracle.bucket_features(surv[k], 1, 7.5, 7.5).tobytes(), k


@pytest.mark.gpu
@pytest.mark.parametrize("lanes", [1, 16])
def test_bucketing_capacity_boundary(lanes, pkg, oracle, gpu):
    """out_cap equal to a list's bucketed length delivers it; one less refuses that list alone -- VH_ERR_CAPACITY, its
    out_counts the length it needs -- and the other lists of the batch are delivered."""
    rng = np.random.default_rng(109)
    lists = [random_matches(pkg, rng, n) for n in (400, 900, 150)]
    want = [oracle.bucket_features(oracle.remove_outliers(pm)[0], 3, 40.0, 30.0) for pm in lists]
    L = [len(w) for w in want]
    assert L[1] > L[0] + 1 and L[0] > L[2] + 1 and L[2] > 20, L
    for cap, refused in ((L[1], ()), (L[1] - 1, (1,)), (L[0], (1,)), (L[0] - 1, (1, 0)), (L[2], (1, 0)), (L[2] - 1, (1, 0, 2))):
        got, _, _, rc, counts = pkg.remove_outliers_device(lists, lanes_per_wave=lanes, max_features=3, bucket_width=40.0, bucket_height=30.0,
                                                           out_cap=cap, strict=False, with_counts=True)
        assert rc == (pkg.VH_ERR_CAPACITY if refused else pkg.VH_OK), (cap, rc)
        assert list(counts) == L, (cap, list(counts), L)  # (delivered or not: the length the list has)
        for k in range(3):
            assert got[k].tobytes() == (b"" if k in refused else want[k].tobytes()), (cap, k)


@pytest.mark.gpu
@pytest.mark.parametrize("lanes", [1, 16])
@pytest.mark.parametrize("longest", [16384, 16385])
def test_vote_tally_switch(longest, lanes, pkg, oracle, gpu):
    """The longest list of a batch has exactly 16 384 records -- the last size whose vote counters live in LDS, all
    64 KB of it -- and 16 385, the first size of the tally with global counters."""
    rng = np.random.default_rng(110)
    lists = [random_matches(pkg, rng, 700), random_matches(pkg, rng, longest, W=1920, H=1080)]
    got, _, _ = pkg.remove_outliers_device(lists, lanes_per_wave=lanes)
    for g, pm in zip(got, lists):
        assert g.tobytes() == oracle.remove_outliers(pm)[0].tobytes(), len(pm)
    assert 4000 < len(got[1]) < longest


@pytest.mark.gpu
def test_list_limit_of_16_bit_links(pkg, oracle, gpu):
    """VH_VOTE_LIST_MAX = 65 535 records (16-bit hull links) in one list, voted and bucketed into a single bucket that
    one lane shuffles and gathers whole.  Measured on the MI355X: the sweep of the 65 535 points takes 503 ms (130 840
    triangles, 55 944 survivors), the whole test 1.0 s with the oracle's second on the host -- so it runs like the others."""
    rng = np.random.default_rng(111)
    pm = random_matches(pkg, rng, 65535, W=1920, H=1080)
    surv = oracle.remove_outliers(pm)[0]
    assert 20000 < len(surv) < 65535 and be.shape(surv, 4000.0, 4000.0)[:2] == (1, 1)
    got, ntri, ms = pkg.remove_outliers_device([pm], lanes_per_wave=1, max_features=MF_ALL, bucket_width=4000.0, bucket_height=4000.0)
    print(f"65 535 records: sweep {ms:.1f} ms, {ntri[0]} triangles, {len(surv)} survivors")
    assert got[0].tobytes() == oracle.bucket_features(surv, MF_ALL, 4000.0, 4000.0).tobytes()


def test_list_beyond_the_limit_is_refused_without_a_device(pkg):
    """65 536 records: VH_ERR_UNSUPPORTED before any device is touched (csrc/engine_api.hip)."""
    pm = np.zeros(65536, pkg.P_MATCH_DTYPE)
    with pytest.raises(pkg.VisoHipError) as ex:
        pkg.remove_outliers_device([pm], max_features=2)
    assert ex.value.code == pkg.VH_ERR_UNSUPPORTED


# ---------------------------------------------------------------------------------------------- the group's post chain
_chain = {}
FRAMES = 7  # of the scene the group tests share: stream s is at frame s + t in step t


@pytest.mark.gpu
@pytest.mark.parametrize("mf,bw,bh", [(1, 17.5, 23.0), (1000, 1000.0, 1000.0), (5, 1.0, 1.0)])
def test_group_post_chain_bucket_grids(mf, bw, bh, pkg, ob, oracle, gpu):
    """Group::bucket_need (csrc/engine_post.hip) sizes the batch's grid scratch and output slots from the image
    dimensions: a grid of one bucket, of 19 x 7, and of 320 x 160 = 51 200 one-pixel buckets whose 256 000 output slots
    are clamped to the match capacity.  S = 3 streams, two steps, refinement = 2; the bucketed lists equal the oracle's
    chain on the same quad matches bit for bit.  Refinement moves the three partners of a match and leaves (u1c, v1c),
    the point that is bucketed, on its pixel (tests/refine_oracle.py, as the reference): the flows the vote compares
    are sub-pixel, the bucketed coordinates are not, and the grid of the dimensions bounds every list's grid exactly.
    (Sub-pixel bucket coordinates: case_fractional_sizes_and_coordinates.)"""
    from test_refinement import H, W, expected, scene
    S, T = 3, 3
    dims = [W, H, pkg.synth.bytes_per_line(W)]
    fr = scene(pkg, FRAMES, seed=61)
    p, po = pkg.Params.default(refinement=2), ob.Params.default(refinement=2)
    # the grid bucket_need computes from the dimensions, restated: it must bound every list's own grid (an nb_max
    # below it would refuse a list that the reference's formula accepts)
    cols_d = int(np.floor(np.float32(W - 1) / np.float32(bw))) + 1
    rows_d = int(np.floor(np.float32(H - 1) / np.float32(bh))) + 1
    g = pkg.StreamGroup(S, p)
    g.postDeviceConfig(1, 2, 16)
    for t in range(T):
        g.pushBack(np.stack([fr[s + t][0] for s in range(S)]), np.stack([fr[s + t][1] for s in range(S)]), dims)
        if t == 0:
            continue
        g.matchFeatures(pkg.METHOD_QUAD)
        g.postBeginDevice(4096, mf, bw, bh, want_lists=True)
        res = g.postFinishDevice(0, want_lists=True, estimator=False)
        for s in range(S):
            if s + t not in _chain:  # (the oracle's refined list of a frame pair: once for all three parameter sets)
                _chain[s + t] = expected(oracle, po, dims, 2, fr[s + t - 1], fr[s + t], 2)[0]
            refined = _chain[s + t]
            assert g.getMatches(s).tobytes() == refined.tobytes()
            surv = oracle.remove_outliers(refined)[0]
            cols, rows, _, lens = be.shape(surv, bw, bh)
            assert len(surv) > 40 and (surv["u1p"] != np.floor(surv["u1p"])).mean() > 0.5, (t, s, len(surv))
            assert cols <= cols_d and rows <= rows_d and surv["u1c"].max() <= W - 1 and surv["v1c"].max() <= H - 1, (cols, rows, cols_d, rows_d)
            want = oracle.bucket_features(surv, mf, bw, bh)
            assert res["counts"][s] == len(want) and res["lists"][s].tobytes() == want.tobytes(), (t, s, res["counts"][s], len(want))
            if bw == 1000.0:
                assert cols * rows == 1 and len(want) == 1000 < len(surv)
            elif bw == 1.0:
                assert cols_d * rows_d == 51200 and cols * rows > 65536 // 2 and len(want) == len(surv)
            else:
                assert (cols_d, rows_d) == (19, 7) and (lens > 1).any() and len(want) < len(surv)
    g.close()


@pytest.mark.gpu
def test_group_post_chain_grid_shrinks_on_a_reused_batch(pkg, ob, oracle, gpu):
    """A batch of the ring keeps its grid scratch from step to step: two steps with a grid of up to 19 x 7 buckets fill
    both batches, then two steps with 9 x 1 buckets run on them.  The word behind the shorter grid's last count still
    holds the first position of the old grid's bucket 10 -- not zero, asserted below -- and is not this grid's to read."""
    from test_refinement import H, W, expected, scene
    S, T = 3, 5
    dims = [W, H, pkg.synth.bytes_per_line(W)]
    fr = scene(pkg, FRAMES, seed=61)
    p, po = pkg.Params.default(refinement=2), ob.Params.default(refinement=2)
    g = pkg.StreamGroup(S, p)
    g.postDeviceConfig(1, 2, 16)
    before = {}
    for t in range(T):
        g.pushBack(np.stack([fr[s + t][0] for s in range(S)]), np.stack([fr[s + t][1] for s in range(S)]), dims)
        if t == 0:
            continue
        g.matchFeatures(pkg.METHOD_QUAD)
        mf, bw, bh = (1, 17.5, 23.0) if t <= 2 else (1, 35.0, 160.0)
        g.postBeginDevice(4096, mf, bw, bh, want_lists=True)
        res = g.postFinishDevice(0, want_lists=True, estimator=False)
        for s in range(S):
            if s + t not in _chain:
                _chain[s + t] = expected(oracle, po, dims, 2, fr[s + t - 1], fr[s + t], 2)[0]
            surv = oracle.remove_outliers(_chain[s + t])[0]
            cols, rows, _, lens = be.shape(surv, bw, bh)
            if t <= 2:
                assert cols * rows > 100
                before[(t, s)] = np.concatenate([[0], np.cumsum(lens)])  # (what the scan leaves: every bucket's first position)
            else:  # (batches alternate: step t runs where step t - 2 ran)
                assert cols * rows == 9 and before[(t - 2, s)][cols * rows + 1] > 0, (cols, rows)
            want = oracle.bucket_features(surv, mf, bw, bh)
            assert res["counts"][s] == len(want) and res["lists"][s].tobytes() == want.tobytes(), (t, s, res["counts"][s], len(want))
    g.close()


# ---------------------------------------------------------------------------------------------- the checking build
@pytest.mark.gpu
def test_bucketing_checking_build(pkg, gpu):
    """This file's device tests once more on libviso_hip_check.so (every index invariant the kernels trust is verified)."""
    assert os.path.exists(pkg.CHECK_LIB_PATH), "build() makes it"
    env = dict(os.environ, VISO_HIP_LIB=pkg.CHECK_LIB_PATH)
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-q", "-x", "-m", "gpu", "-k", "not checking_build"],
                       env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert " passed" in r.stdout and "skipped" not in r.stdout, r.stdout[-500:]
