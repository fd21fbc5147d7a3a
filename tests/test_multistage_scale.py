"""Multi-stage matching at full size, on odd ranges and on its failure paths (tests/test_multistage.py runs 320 x 160).

Stateless vh_match_ranged on constructed feature sets: more drivers than one pass of ranged_circle_kernel's grid,
fractional / extreme / empty ranges, ties across lanes, v-bins and u-bins, degenerate sets.  Stateful: KITTI-size
frames on a lone matcher, mono handles, failed lazy allocations, frames with nothing to learn from, the epoch of the
pixel mask.  Every list is compared byte for byte (float fields bit for bit) with tests/multistage_oracle.py's
restatement; large sets go through its C form (oracle/viso_ranged.c), which a not-gpu test ties to the numpy form.
Every condition that keeps a case from being vacuous is asserted on the oracle's output before the GPU is asked.

tests/golden/multistage_answers.npz pins the restatement itself: the answers in it come from the restatement as of
the commit that added it (oracle/gen_golden_multistage.py), NOT from the reference -- the reference has nothing
behind use_prior."""
import ctypes as C
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import multistage_oracle as mo
from conftest import GOLDEN, ROOT
from test_multistage import CONFIGS, W, H, check_not_vacuous, images_of, scene

F32 = np.float32
DRIVER = {0: "i1c", 1: "i1c", 2: "i1p"}
#: displacement (du, dv) of the candidate against the query in every stage of the constructed circles
FLOW_D, DISP = (7, -4), 9
STAGE_D = {0: ((7, -4), (-7, 4)), 1: ((-DISP, 0), (DISP, 0)), 2: ((-DISP, 0), (7, -4), (DISP, 0), (-7, 4))}


# ------------------------------------------------------------------ constructed feature sets
def records(u, v, cls, desc):
    a = np.zeros((len(u), 12), np.int32)
    a[:, 0], a[:, 1], a[:, 3] = u, v, cls
    a[:, 4:] = np.ascontiguousarray(desc, np.uint8).view(np.int32).reshape(len(u), 8)
    return a


def descriptors(a):
    return a[:, 4:].copy().view(np.uint8).reshape(-1, 32)


def partner(rng, a, dims, d, jitter=(3, 3), far=0.0, leftward=False, medium=0.0):
    """A set that holds one partner per feature of a -- moved by d plus a jitter, the descriptor slightly changed -- in
    a shuffled order.  far: fraction of partners placed anywhere in the image (leftward: anywhere to the left on the
    same row, for a stereo stage); medium: fraction moved by 205..250 pixels in u (beyond the default radius)."""
    n = len(a)
    u = a[:, 0] + d[0] + rng.integers(-jitter[0], jitter[0] + 1, n)
    v = a[:, 1] + d[1] + rng.integers(-jitter[1], jitter[1] + 1, n)
    kind = rng.random(n)
    med = kind < medium
    u = np.where(med, a[:, 0] + np.sign(d[0] if d[0] else 1) * rng.integers(205, 251, n), u)
    is_far = (kind >= medium) & (kind < medium + far)
    if leftward:
        u = np.where(is_far, (rng.random(n) * (a[:, 0] + 1)).astype(np.int64), u)
    else:
        u = np.where(is_far, rng.integers(0, dims[0], n), u)
        v = np.where(is_far, rng.integers(0, dims[1], n), v)
    desc = np.clip(descriptors(a).astype(np.int32) + rng.integers(-2, 3, (n, 32)), 0, 255).astype(np.uint8)
    b = records(np.clip(u, 0, dims[0] - 1), np.clip(v, 0, dims[1] - 1), a[:, 3], desc)
    return b[rng.permutation(n)]


def circle_sets(rng, method, base, dims, **kw):
    """The four roles (None where the method reads none) around `base` as the driving set."""
    st = dict(kw, jitter=(3, 1), leftward=True)
    if method == 0:
        return [partner(rng, base, dims, FLOW_D, **kw), None, base, None]
    if method == 1:
        return [None, None, base, partner(rng, base, dims, (-DISP, 0), **st)]
    m2p = partner(rng, base, dims, (-DISP, 0), **st)
    m1c = partner(rng, base, dims, (-FLOW_D[0], -FLOW_D[1]), **kw)
    return [base, m2p, m1c, partner(rng, m1c, dims, (-DISP, 0), **st)]


def learned_like_ranges(rng, po, dims, method, quarter=True):
    """A window of a few pixels around every stage's displacement, with bounds that are multiples of 0.25."""
    nb = int(np.prod(mo.bin_grid(po, dims)))
    rg = mo.full_ranges(po, dims)
    for st, d in enumerate(STAGE_D[method]):
        for ax in range(2):
            q = 4.0 if quarter else 1.0
            rg[:, st, 2 * ax] = d[ax] - rng.integers(8, 33, nb) / q
            rg[:, st, 2 * ax + 1] = d[ax] + rng.integers(8, 33, nb) / q
    return rg


def raw_match_ranged(pkg, p, dims, method, ranges, sets, cap):
    """vh_match_ranged without the wrapper's error check -> (code, *n, records)."""
    z = np.zeros((0, 12), np.int32)
    s = [np.ascontiguousarray(z if m is None else m, np.int32) for m in sets]
    out = np.zeros(max(cap, 1), pkg.P_MATCH_DTYPE)
    n = C.c_int32(-7)
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)
    rc = pkg._lib().vh_match_ranged(C.byref(p), 0, (C.c_int32 * 3)(*dims), method, ptr(s[0]), len(s[0]), ptr(s[1]), len(s[1]),
                                    ptr(s[2]), len(s[2]), ptr(s[3]), len(s[3]), ptr(np.ascontiguousarray(ranges, F32)), ptr(out), cap,
                                    C.byref(n))
    return rc, n.value, out[:cap]


# ------------------------------------------------------------------ 1. more drivers than one pass of the grid
RANGED_G = 8              # VH_RANGED_G, lanes per driver
GRID_DRIVERS = 2048 * 32  # vh_launch_ranged_circle: at most 2048 workgroups of 256 / VH_RANGED_G = 32 drivers
BIG_DIMS = [6000, 3000, 6000]
BIG_N = 70000


@functools.lru_cache(maxsize=None)
def big_case(ob, oracle, method):
    rng = np.random.default_rng(100 + method)
    po = ob.Params.default()
    dims, n = BIG_DIMS, BIG_N
    base = records(rng.integers(20, dims[0] - 20, n), rng.integers(20, dims[1] - 20, n), rng.integers(0, 4, n),
                   rng.integers(0, 256, (n, 32), dtype=np.uint8))
    # pixels that two drivers of different classes bid for, one below and one above the first pass of the grid
    lo, hi = rng.permutation(GRID_DRIVERS)[:400], GRID_DRIVERS + rng.permutation(n - GRID_DRIVERS)[:400]
    base[hi, 0:2] = base[lo, 0:2]
    base[hi, 3] = (base[lo, 3] + 1) % 4
    sets = circle_sets(rng, method, base, dims)
    rg = learned_like_ranges(rng, po, dims, method)
    nb = len(rg)
    rg[rng.random(nb) < 0.03] = mo.full_ranges(po, dims)[0]           # bins that learned nothing
    gone = rng.random(nb) < 0.03
    rg[gone, :, 1] = rg[gone, :, 0] - 0.75                             # bins whose u window is empty
    want, det = oracle.ranged_matching(po, dims, method, *sets, rg, detail=True)
    drv = want[DRIVER[method]]
    assert len(base) > GRID_DRIVERS, "ndrive does not exceed one pass of the grid"
    assert len(want) > 1000 and (drv >= GRID_DRIVERS).any(), "no emitted match is driven from a later trip of the loop"
    assert (drv >> 8 == 0).any() and (drv >> 8 == (n - 1) >> 8).any(), "first or last emission chunk of 256 without a match"
    assert 0 < (det["state"] == 0).sum() < n, "every circle closes / none does"
    if method == 0:
        closed = np.flatnonzero(det["state"] > 0)
        pix = base[closed, 1].astype(np.int64) * dims[0] + base[closed, 0]
        low, high = set(pix[closed < GRID_DRIVERS].tolist()), set(pix[closed >= GRID_DRIVERS].tolist())
        assert len(low & high) > 20, "no pixel is bid for by drivers on both sides of index 65 536"
        assert (det["state"][GRID_DRIVERS:] == 2).sum() > 20, "the first-writer mask drops nothing in a later trip"
    return po, dims, sets, rg, want


@pytest.mark.gpu
@pytest.mark.parametrize("method", (0, 1, 2))
def test_more_drivers_than_one_grid_pass(pkg, ob, oracle, gpu, method):
    po, dims, sets, rg, want = big_case(ob, oracle, method)
    got = pkg.match_ranged(pkg.Params.default(), dims, method, rg, *sets)
    assert got.tobytes() == want.tobytes(), (method, len(got), len(want))


# ------------------------------------------------------------------ 2. fractional and extreme ranges
FRAC_DIMS = [2600, 300, 2600]
BIG = float(2 ** 20)
#: (min, max) an axis of a bin may get instead of a window around the displacement
MENU = ((-0.5, 0.5), (0.75, 0.25), (-2.0 * BIG, 2.0 * BIG), (-3e9, 3e9), (BIG + 4.25, 3e9), (-3e9, -BIG - 0.5),
        (-2700.25, -2650.5), (2650.5, 2700.25), (-250.5, 250.25), (-0.25, 0.25))


@functools.lru_cache(maxsize=None)
def fractional_case(ob, oracle, method):
    rng = np.random.default_rng(200 + method)
    po = ob.Params.default()  # binsize 50, radius 200
    dims, n = FRAC_DIMS, 6000
    base = records(rng.integers(0, dims[0], n), rng.integers(0, dims[1], n), rng.integers(0, 4, n),
                   rng.integers(0, 256, (n, 32), dtype=np.uint8))
    sets = circle_sets(rng, method, base, dims, far=0.25, medium=0.1)
    rg = learned_like_ranges(rng, po, dims, method)
    nb = len(rg)
    pick = rng.integers(0, 2 * len(MENU), (nb, 2))  # per bin and axis, the same in every stage; half keep their window
    for k, (lo, hi) in enumerate(MENU):
        for ax in range(2):
            rows = pick[:, ax] == k
            rg[rows, :, 2 * ax], rg[rows, :, 2 * ax + 1] = lo, hi
            assert rows.any(), ("menu entry unused", k, ax)
    assert (rg * 4 == np.round(rg * 4)).all() and (rg != np.round(rg)).any() and (rg < 0).any() and (rg > 0).any()
    assert (np.abs(rg) > BIG).any() and (rg[:, :, 0] > rg[:, :, 1]).any() and (np.abs(rg) > po.match_radius).any()
    want, det = oracle.ranged_matching(po, dims, method, *sets, rg, detail=True)
    assert len(want) > 300, len(want)
    # a bound that falls within +-1 of a bin border, for some query of some stage
    bs = po.match_binsize
    ubn, vbn = mo.bin_grid(po, dims)
    sb = np.minimum(base[:, 1] // bs, vbn - 1) * ubn + np.minimum(base[:, 0] // bs, ubn - 1)
    near = 0
    for st, (qr, _, _) in enumerate(mo.STAGES[method]):
        q = np.arange(n) if st == 0 else det["stage_idx"][:, st - 1]
        x = sets[qr][q, 0][:, None].astype(np.float64) + rg[sb, st, 0:2]
        r = np.mod(x, bs)
        near += int((((r <= 1) | (r >= bs - 1)) & (x > 0) & (x < dims[0])).sum())
    assert near > 50, "no query + bound within +-1 of a multiple of match_binsize"
    # a kernel that rounded the bounds any other way would give another list
    for how in ("nearest", "trunc", "outward"):
        alt = oracle.ranged_matching(po, dims, method, *sets, mo.misrounded(rg, how))
        assert alt.tobytes() != want.tobytes(), "bounds rounded '%s' give the same list: the case shows nothing" % how
    # ... and so would one that clamped the bounds too early, or held the window to +-match_radius
    a, b = {0: ("u1c", "u1p"), 1: ("u1c", "u2c"), 2: ("u1p", "u2p")}[method]
    du = np.abs(want[a] - want[b])
    assert (du > 1100).any(), "no match further away than 1100 pixels: the clamp at +-2^20 is not exercised"
    assert ((du > po.match_radius) & (du <= 250)).any(), "no match between match_radius and 250 pixels away"
    return po, dims, sets, rg, want


@pytest.mark.gpu
@pytest.mark.parametrize("method", (0, 1, 2))
def test_fractional_and_extreme_ranges(pkg, ob, oracle, gpu, method):
    po, dims, sets, rg, want = fractional_case(ob, oracle, method)
    got = pkg.match_ranged(pkg.Params.default(), dims, method, rg, *sets)
    assert got.tobytes() == want.tobytes(), (method, len(got), len(want))


# ------------------------------------------------------------------ 3. ties
TIE_DIMS = [400, 200, 400]


@functools.lru_cache(maxsize=None)
def tie_case(ob, oracle, method):
    """Few distinct descriptors, all four classes: most minima are attained several times, and the winner is the first
    in the reference's visiting order (u-bin, v-bin, list position), which is neither index order nor arrival order.
    The conditions are counted over stage 0 of the first 300 drivers."""
    rng = np.random.default_rng(300 + method)
    po = ob.Params.default(match_disp_tolerance=12)  # (several v-bins in the 1-d stages too)
    dims, n = TIE_DIMS, 1500
    palette = rng.integers(0, 256, (6, 32), dtype=np.uint8)
    a = records(rng.integers(0, dims[0], n), rng.integers(0, dims[1], n), rng.integers(0, 4, n), palette[rng.integers(0, 6, n)])
    shuffled = lambda: a[rng.permutation(n)]
    sets = {0: [shuffled(), None, a, None], 1: [None, None, a, shuffled()], 2: [a, shuffled(), shuffled(), shuffled()]}[method]
    nb = int(np.prod(mo.bin_grid(po, dims)))
    rg = np.empty((nb, 4, 4), F32)
    rg[:, :, 0::2] = -rng.integers(120, 321, (nb, 4, 2)) / 4.0
    rg[:, :, 1::2] = rng.integers(120, 321, (nb, 4, 2)) / 4.0
    want = oracle.ranged_matching(po, dims, method, *sets, rg)
    assert len(want) > 50, len(want)
    for rec in want:  # classes never match across each other
        cls = {int(sets[r][rec[f], 3]) for r, f in enumerate(("i1p", "i2p", "i1c", "i2c")) if rec[f] >= 0}
        assert len(cls) == 1
    # what decides the first stage of 300 drivers
    qr, cr, flow = mo.STAGES[method][0]
    q, c = mo.Index(po, dims, sets[qr]), mo.Index(po, dims, sets[cr])
    bs, ubn, vbn = po.match_binsize, *mo.bin_grid(po, dims)
    seen = dict(lanes=0, one_bin=0, v_bins=0, u_bins=0, not_smallest=0, not_last=0, later_u_bin_smaller_index=0)
    for i in range(300):
        sb = min(int(a[i, 1]) // bs, vbn - 1) * ubn + min(int(a[i, 0]) // bs, ubn - 1)
        ind, cost = mo.candidates_in_order(po, q, i, c, rg[sb, 0], flow)
        if len(ind) == 0:
            continue
        best = ind[cost == cost.min()]
        win = mo.find_match(po, q, i, c, rg[sb, 0], flow)
        assert win == best[0]
        ub = np.minimum(c.m[best, 0] // bs, ubn - 1)
        vb = np.minimum(c.m[best, 1] // bs, vbn - 1)
        cell = list(zip(ub.tolist(), vb.tolist()))
        seen["one_bin"] += len(set(cell)) < len(cell)
        # find_ranged: lane g of the driver's group takes positions g, g + 8, ... of the run of v-bins of one u-bin
        for u0 in set(ub.tolist()):
            run = [int(j) for vb_ in range(vbn) for j in c.bins.get((int(q.m[i, 3]) * vbn + vb_) * ubn + u0, ())]
            if len({run.index(int(j)) % RANGED_G for j, u in zip(best, ub) if u == u0}) > 1:
                seen["lanes"] += 1
                break
        seen["v_bins"] += any(len({v for u, v in cell if u == u0}) > 1 for u0 in set(ub.tolist()))
        seen["u_bins"] += len(set(ub.tolist())) > 1
        seen["not_smallest"] += win != best.min()
        seen["not_last"] += win != best[-1]
        seen["later_u_bin_smaller_index"] += bool((best[ub > ub[0]] < win).any())
    assert all(v > 5 for v in seen.values()), seen
    return po, dims, sets, rg, want


@pytest.mark.gpu
@pytest.mark.parametrize("method", (0, 1, 2))
def test_ties_across_lanes_v_bins_and_u_bins(pkg, ob, oracle, gpu, method):
    po, dims, sets, rg, want = tie_case(ob, oracle, method)
    got = pkg.match_ranged(pkg.Params.default(match_disp_tolerance=12), dims, method, rg, *sets)
    assert got.tobytes() == want.tobytes(), (method, len(got), len(want))


# ------------------------------------------------------------------ 4. degenerate sets
def degenerate_cases(ob, oracle):
    """-> list of (name, method, dims, sets, ranges, want)."""
    rng = np.random.default_rng(400)
    po = ob.Params.default()
    dims = [357, 169, 357]
    full = mo.full_ranges(po, dims)
    one = records([100], [60], [2], rng.integers(0, 256, (1, 32), dtype=np.uint8))
    out = []
    for method in (0, 1, 2):
        sets = [one if r in mo.NEED[method] else None for r in range(4)]
        want = oracle.ranged_matching(po, dims, method, *sets, full)
        assert len(want) == 1
        out.append(("one feature", method, dims, sets, full, want))
        # every window empty: nothing is accepted, min_ind stays 0 in every stage, and 0 is where the circle started
        none = full.copy()
        none[:, :, 1::2] = -500.25
        want, det = oracle.ranged_matching(po, dims, method, *sets, none, detail=True)
        assert not det["stage_hit"].any() and len(want) == 1, "the circle of defaults must close on feature 0"
        out.append(("one feature, empty windows", method, dims, sets, none, want))
    n = 1500
    base = records(rng.integers(20, 337, n), rng.integers(20, 149, n), rng.integers(0, 4, n), rng.integers(0, 256, (n, 32), dtype=np.uint8))
    for method in (0, 1, 2):
        sets = circle_sets(rng, method, base, dims)
        rg = learned_like_ranges(rng, po, dims, method)
        blind = rng.random(len(rg)) < 0.3
        rg[blind, 0, 0], rg[blind, 0, 1] = 0.75, 0.25  # stage 1 of these bins' drivers accepts nothing
        want, det = oracle.ranged_matching(po, dims, method, *sets, rg, detail=True)
        went_on = (det["stage_hit"][1:, 0] == 0) & (det["stage_idx"][1:, 0] == 0) & (det["stage_hit"][1:, 1] == 1)
        assert went_on.sum() > 20, "no driver whose stage 1 answers the default min_ind = 0 and goes on from feature 0"
        assert len(want) > 100
        out.append(("default min_ind", method, dims, sets, rg, want))
    sets = circle_sets(rng, 2, base, dims)
    for role in (1, 2, 3):  # a quad circle with one role empty
        hole = list(sets)
        hole[role] = None
        want = oracle.ranged_matching(po, dims, 2, *hole, full)
        assert len(want) == 0
        out.append(("role %d empty" % role, 2, dims, hole, full, want))
    return out


@pytest.mark.gpu
def test_degenerate_sets_and_capacity(pkg, ob, oracle, gpu):
    p = pkg.Params.default()
    for name, method, dims, sets, rg, want in degenerate_cases(ob, oracle):
        got = pkg.match_ranged(p, dims, method, rg, *sets)
        assert got.tobytes() == want.tobytes(), (name, method, len(got), len(want))
        if len(want) > 100:  # cap smaller than the list: the first cap records, the true count, VH_ERR_CAPACITY
            cap = len(want) // 2
            rc, cnt, part = raw_match_ranged(pkg, p, dims, method, rg, sets, cap)
            assert rc == pkg.VH_ERR_CAPACITY and cnt == len(want), (name, method, rc, cnt)
            assert part.tobytes() == want[:cap].tobytes(), (name, method)
            rc, cnt, part = raw_match_ranged(pkg, p, dims, method, rg, sets, len(want))
            assert rc == pkg.VH_OK and cnt == len(want) and part.tobytes() == want.tobytes()


# ------------------------------------------------------------------ the C form against the numpy form (no GPU)
def test_c_form_of_ranged_matching_equals_the_numpy_form(pkg, ob, oracle):
    """oracle.ranged_matching (oracle/viso_ranged.c) against mo.ranged_matching byte for byte: the scenes of
    tests/test_multistage.py with learned, full, perturbed fractional and extreme ranges, and a part of the tie case."""
    dims = [W, H, pkg.synth.bytes_per_line(W)]
    rng = np.random.default_rng(31)
    total = 0
    for seed, kw in CONFIGS:
        po = ob.Params.default(multi_stage=1, **kw)
        fr = scene(pkg, 2, seed=seed)
        for method in (0, 1, 2):
            r = mo.multistage(ob, oracle, po, dims, method, images_of(method, fr[0], fr[1]))
            assert oracle.ranged_matching(po, dims, method, *r["dense_sets"], r["ranges"]).tobytes() == r["dense"].tobytes(), (kw, method)
            nb = len(r["ranges"])
            odd = r["ranges"].copy()
            odd[:, :, 0::2] += rng.integers(-36, 24, (nb, 4, 2)) / F32(4)
            odd[:, :, 1::2] += rng.integers(-24, 36, (nb, 4, 2)) / F32(4)
            for k, (lo, hi) in enumerate(MENU):
                rows = rng.random(nb) < 0.04
                odd[rows, :, 2 * (k & 1)], odd[rows, :, 2 * (k & 1) + 1] = lo, hi
            for rg in (mo.full_ranges(po, dims), odd):
                trace = {}
                want = mo.ranged_matching(po, dims, method, *r["dense_sets"], rg, trace)
                got, det = oracle.ranged_matching(po, dims, method, *r["dense_sets"], rg, detail=True)
                assert got.tobytes() == want.tobytes(), (kw, method, len(got), len(want))
                assert det["n"] == len(want) and (det["state"] == 1).sum() == len(want)
                # the per-driver detail is the numpy form's trace
                for st in range(1, len(mo.STAGES[method])):
                    assert {int(x) for x in det["stage_idx"][:, st - 1]} == {q for (s, q) in trace if s == st}
                total += len(want)
    assert total > 2000
    # a crop of the KITTI-size dense sets, with the ranges learned at full size
    kdims = [KW, KH, pkg.synth.bytes_per_line(KW)]
    po = ob.Params.default(multi_stage=1)
    fr = kitti_frames(pkg, 2)
    for method in (0, 1, 2):
        r = mo.multistage(ob, oracle, po, kdims, method, images_of(method, fr[0], fr[1]), fast=True)
        crop = [None if m is None else m[(m[:, 0] > 350) & (m[:, 0] < 800) & (m[:, 1] < 200)] for m in r["dense_sets"]]
        want = mo.ranged_matching(po, kdims, method, *crop, r["ranges"])
        assert len(want) > 500 and oracle.ranged_matching(po, kdims, method, *crop, r["ranges"]).tobytes() == want.tobytes(), method
    for method in (0, 1, 2):
        po, tdims, sets, rg, want = tie_case(ob, oracle, method)
        cut = [None if s is None else s[:400] for s in sets]
        assert oracle.ranged_matching(po, tdims, method, *cut, rg).tobytes() == mo.ranged_matching(po, tdims, method, *cut, rg).tobytes()


def test_constructed_cases_meet_their_conditions(ob, oracle):
    """The conditions of the constructed cases hold (they are asserted again inside every GPU test): checked where
    there is no GPU, so that a change of a seed or a size cannot make a GPU test vacuous unnoticed."""
    for method in (0, 1, 2):
        big_case(ob, oracle, method)
        fractional_case(ob, oracle, method)
        tie_case(ob, oracle, method)
    assert len(degenerate_cases(ob, oracle)) == 12


# ------------------------------------------------------------------ 14. the restatement's recorded answers (no GPU)
def answer_cases(pkg):
    """The cases of tests/golden/multistage_answers.npz: the four CONFIGS of tests/test_multistage.py at 320 x 160 (numpy
    form throughout) and the first pair of the KITTI-size frames (pass 2 by the C form, which
    test_c_form_of_ranged_matching_equals_the_numpy_form ties to the numpy form on a crop of these very sets)."""
    cases = []
    for k, (seed, kw) in enumerate(CONFIGS):
        fr = scene(pkg, 2, seed=seed)
        cases.append(("cfg%d" % k, [W, H, pkg.synth.bytes_per_line(W)], kw, False, fr[0], fr[1]))
    fr = kitti_frames(pkg, 2)
    cases.append(("kitti", [KW, KH, pkg.synth.bytes_per_line(KW)], {}, True, fr[0], fr[1]))
    return cases


def test_restatement_reproduces_its_recorded_answers(pkg, ob, oracle):
    """tests/golden/multistage_answers.npz: counts and SHA-256 of sparse, ranges and dense as the restatement gave them
    when the file was recorded (oracle/gen_golden_multistage.py) -- not the reference's answers, it has none."""
    z = np.load(os.path.join(GOLDEN, "multistage_answers.npz"))
    names = [str(x) for x in z["names"]]
    now = mo.recorded_answers(ob, oracle, answer_cases(pkg))
    assert sorted(now) == sorted(names) and len(names) == 4 * 3 + 3
    for k, name in enumerate(names):
        counts, sha = now[name]
        assert counts == z["counts"][k].tolist(), (name, counts, z["counts"][k].tolist())
        assert sha == [str(x) for x in z["sha256"][k]], name


# ------------------------------------------------------------------ 5. KITTI size, a lone matcher
KW, KH = 1241, 376


def kitti_frames(pkg, T, seed=11):
    return scene(pkg, T, KW, KH, seed=seed, disparity=9, blur=3, blank=0.6)


def kitti_expected(pkg, ob, oracle, po, dims, method, prev, cur):
    r = mo.multistage(ob, oracle, po, dims, method, images_of(method, prev, cur), fast=True)
    check_not_vacuous(po, method, r)
    single = oracle.matching(po, dims, method, *r["dense_sets"])
    assert r["dense"].tobytes() != single.tobytes(), "pass 2 equals the single-stage list: the ranges change nothing"
    return r


@pytest.mark.gpu
@pytest.mark.parametrize("kw", ({}, dict(half_resolution=1), dict(nms_n=1), dict(nms_n=2)), ids=("default", "half", "nms1", "nms2"))
def test_kitti_size_lone_matcher(pkg, ob, oracle, gpu, kw):
    """1241 x 376, three pushes, methods 1, 0, 2 after each pair; nms_n = 1 / 2: sparse nms_n 4 (detect_nms<4>) / 8 (generic)."""
    dims = [KW, KH, pkg.synth.bytes_per_line(KW)]
    fr = kitti_frames(pkg, 3)
    p, po = pkg.Params.default(multi_stage=1, **kw), ob.Params.default(multi_stage=1, **kw)
    m = pkg.Matcher(p, outlier_removal=False)
    m.setMultiStageMatching(True)
    for t in range(3):
        m.pushBack(fr[t][0], fr[t][1], dims)
        if t == 0:
            continue
        for method in (1, 0, 2):
            r = kitti_expected(pkg, ob, oracle, po, dims, method, fr[t - 1], fr[t])
            m.matchFeatures(method)
            got = m.getMatches()
            assert got.tobytes() == r["dense"].tobytes(), (kw, t, method, len(got), len(r["dense"]))
            assert m.getSparseMatches().tobytes() == r["sparse"].tobytes(), (kw, t, method)
    m.close()


# ------------------------------------------------------------------ 8. mono handles
@pytest.mark.gpu
def test_mono_handles_with_the_switch_on(pkg, ob, oracle, gpu):
    """I2 = None, flow: a lone matcher and a group; stereo and quad on such a handle do what they do without the switch."""
    dims = [W, H, pkg.synth.bytes_per_line(W)]
    fr = scene(pkg, 4, seed=13)
    p, po = pkg.Params.default(multi_stage=1), ob.Params.default(multi_stage=1)
    want = {}
    for t in (1, 2, 3):
        r = mo.multistage(ob, oracle, po, dims, 0, (fr[t - 1][0], None, fr[t][0], None))
        check_not_vacuous(po, 0, r)
        want[t] = r
    outcome = {}
    for on in (False, True):
        m = pkg.Matcher(p, outlier_removal=False)
        if on:
            m.setMultiStageMatching(True)
        for t in range(3):
            m.pushBack(fr[t][0], None, dims)
            if t == 0:
                continue
            m.matchFeatures(0)
            if on:
                assert m.getMatches().tobytes() == want[t]["dense"].tobytes(), t
                assert m.getSparseMatches().tobytes() == want[t]["sparse"].tobytes(), t
        seen = []
        for method in (1, 2):
            rc = pkg._lib().vh_match_features(m._h, method, None)
            seen.append((rc, len(m.getMatches()) if rc == pkg.VH_OK else -1))
        outcome[on] = seen
        m.matchFeatures(0)  # the handle is still good
        if on:
            assert m.getMatches().tobytes() == want[2]["dense"].tobytes()
        m.close()
    assert outcome[True] == outcome[False], outcome
    S = 3
    g = pkg.StreamGroup(S, p)
    g.setMultiStageMatching(True)
    for step in range(2):
        g.pushBack(np.stack([fr[s + step][0] for s in range(S)]), None, dims)
    g.matchFeatures(0)
    for s in range(S):
        assert g.getMatches(s).tobytes() == want[s + 1]["dense"].tobytes(), s
        assert g.getSparseMatches(s).tobytes() == want[s + 1]["sparse"].tobytes(), s
    g.close()


# ------------------------------------------------------------------ 11. a failed lazy allocation
@pytest.mark.gpu
@pytest.mark.parametrize("method", (0, 2), ids=("pixel_mask", "range_table"))
def test_failed_allocation_leaves_the_handle_usable(pkg, ob, oracle, gpu, method):
    """The first flow match allocates the pixel mask, the first quad match the range table: the call that fails says
    VH_ERR_HIP, the next one succeeds and equals the oracle, and the handle ends with the memory of an undisturbed one."""
    dims = [W, H, pkg.synth.bytes_per_line(W)]
    S = 2
    fr = scene(pkg, 3, seed=7)
    p, po = pkg.Params.default(multi_stage=1), ob.Params.default(multi_stage=1)
    want = []
    for s in range(S):
        r = mo.multistage(ob, oracle, po, dims, method, images_of(method, fr[s], fr[s + 1]))
        check_not_vacuous(po, method, r)
        want.append(r)
    size = {}
    for disturbed in (False, True):
        g = pkg.StreamGroup(S, p)
        g.setMultiStageMatching(True)
        for step in range(2):
            g.pushBack(np.stack([fr[s + step][0] for s in range(S)]), np.stack([fr[s + step][1] for s in range(S)]), dims)
        if disturbed:
            g.debugFailNextAlloc()
            with pytest.raises(pkg.VisoHipError) as e:
                g.matchFeatures(method)
            assert e.value.code == pkg.VH_ERR_HIP
        for again in range(2):
            g.matchFeatures(method)
            for s in range(S):
                assert g.getMatches(s).tobytes() == want[s]["dense"].tobytes(), (disturbed, again, s)
                assert g.getSparseMatches(s).tobytes() == want[s]["sparse"].tobytes(), (disturbed, again, s)
        size[disturbed] = g.deviceBytes()
        g.close()
    assert size[True] == size[False], size


# ------------------------------------------------------------------ 12. nothing to learn from
#: textured squares on a flat frame, sizes found on the CPU.  10 pixels: a handful of raw sparse matches none of which
#: survives the vote, so every bin reads +-R, and a dozen dense matches; 12 pixels: 7 raw sparse matches, fewer than the
#: vote usually sees, of which 3 survive.  patch_kind() asserts both on the oracle's output.
PATCHES = (("no survivor", 10), ("short list", 12))


def patch_frames(pkg, size, w=W, h=H):
    out = []
    for l, r in pkg.synth.stereo_sequence(w, h, 2, disparity=4, blur=3, seed=17):
        a, b = np.full_like(l, 90), np.full_like(r, 90)
        a[60:60 + size, 120:120 + size] = l[60:60 + size, 120:120 + size]
        b[60:60 + size, 116:116 + size] = l[60:60 + size, 120:120 + size]
        out.append((a, b))
    return out


def patch_kind(po, dims, method, r, oracle):
    """What a frame pair teaches, from the oracle's output."""
    if len(r["sparse_raw"]) == 0 and len(r["dense"]) == 0 and all(s is None or len(s) == 0 for s in r["dense_sets"]):
        return "nothing at all"
    if len(r["sparse"]) == 0 and len(r["dense"]) > 0:
        # every bin +-R: the single-stage list
        assert r["ranges"].tobytes() == mo.full_ranges(po, dims).tobytes()
        assert r["dense"].tobytes() == oracle.matching(po, dims, method, *r["dense_sets"]).tobytes()
        return "no sparse match, dense matches"
    if method != 1 and 0 < len(r["sparse_raw"]) < 8:
        return "short sparse list"
    return "other"


@pytest.mark.gpu
def test_frames_with_nothing_to_learn_from(pkg, ob, oracle, gpu):
    dims = [W, H, pkg.synth.bytes_per_line(W)]
    p, po = pkg.Params.default(multi_stage=1), ob.Params.default(multi_stage=1)
    flat = np.full((H, dims[2]), 90, np.uint8)
    cases = [("constant", [(flat, flat), (flat, flat)])]
    cases += [(name, patch_frames(pkg, size)) for name, size in PATCHES]
    kinds = set()
    for name, fr in cases:
        m = pkg.Matcher(p, outlier_removal=False)
        m.setMultiStageMatching(True)
        for l, r in fr:
            m.pushBack(l, r, dims)
        for method in (0, 1, 2):
            r = mo.multistage(ob, oracle, po, dims, method, images_of(method, fr[0], fr[1]))
            kinds.add(patch_kind(po, dims, method, r, oracle))
            m.matchFeatures(method)  # VH_OK
            got = m.getMatches()
            assert got.tobytes() == r["dense"].tobytes(), (name, method, len(got), len(r["dense"]))
            assert m.getSparseMatches().tobytes() == r["sparse"].tobytes(), (name, method)
        m.close()
    assert kinds >= {"nothing at all", "no sparse match, dense matches", "short sparse list"}, kinds


# ------------------------------------------------------------------ 13. the epoch of the pixel mask
@pytest.mark.gpu
def test_repeated_flow_matches_never_see_a_stale_bid(pkg, ob, oracle, gpu):
    """Six flow matches without a push, then across pushes: pass 1 and pass 2 each keep a first-writer mask whose bids
    of the previous match must never win.  Duplicated pixels make sure the mask decides something."""
    dims = [W, H, pkg.synth.bytes_per_line(W)]
    fr = scene(pkg, 4, seed=19)
    p, po = pkg.Params.default(multi_stage=1), ob.Params.default(multi_stage=1)
    m = pkg.Matcher(p, outlier_removal=False)
    m.setMultiStageMatching(True)
    m.pushBack(fr[0][0], fr[0][1], dims)
    for t in (1, 2, 3):
        m.pushBack(fr[t][0], fr[t][1], dims)
        r = mo.multistage(ob, oracle, po, dims, 0, images_of(0, fr[t - 1], fr[t]))
        check_not_vacuous(po, 0, r)
        rq = mo.multistage(ob, oracle, po, dims, 2, images_of(2, fr[t - 1], fr[t]))
        for k in range(6):
            m.matchFeatures(0)
            assert m.getMatches().tobytes() == r["dense"].tobytes(), (t, k)
            assert m.getSparseMatches().tobytes() == r["sparse"].tobytes(), (t, k)
            if k % 2:  # another method in between leaves the masks alone
                m.matchFeatures(2)
                assert m.getMatches().tobytes() == rq["dense"].tobytes(), (t, k)
    m.close()


# ------------------------------------------------------------------ 6. a KITTI-size group in sub-batches (child)
HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.mark.gpu
def test_child_kitti_group_in_sub_batches(pkg, gpu):
    """tests/multistage_group_case.py under VH_SUBBATCH=3: six streams at 1241 x 376, rows against the lone matcher,
    vh_group_remove_outliers, the host post chain with the stereo and the monocular estimator."""
    r = subprocess.run([sys.executable, os.path.join(HERE, "multistage_group_case.py")], env=dict(os.environ, VH_SUBBATCH="3"),
                       capture_output=True, text=True, timeout=900, cwd=ROOT)
    assert r.returncode == 0 and "multistage group ok" in r.stdout, r.stdout[-2000:] + r.stderr[-3000:]


# ------------------------------------------------------------------ 7. a frame that needs the grid-stride loop
@pytest.mark.gpu
def test_full_hd_frames_need_the_grid_stride_loop(pkg, ob, oracle, gpu):
    """1920 x 1080 at nms_n = 1: more than 65 536 dense features per image, so the workgroups of ranged_circle_kernel
    walk several drivers with real bin indices, masks and emission chunks.  One quad and one flow step."""
    w, h = 1920, 1080
    dims = [w, h, pkg.synth.bytes_per_line(w)]
    fr = scene(pkg, 2, w, h, seed=5, disparity=9, blur=3, blank=0.7)
    p, po = pkg.Params.default(multi_stage=1, nms_n=1), ob.Params.default(multi_stage=1, nms_n=1)
    # include/viso_hip.h: worst-case capacity 4 per NMS block; a block is nms_n + 1 = 2 pixels wide
    assert 4 * (w // 2) * (h // 2) > GRID_DRIVERS
    want = {}
    for method in (2, 0):
        r = mo.multistage(ob, oracle, po, dims, method, images_of(method, fr[0], fr[1]), fast=True)
        check_not_vacuous(po, method, r)
        assert all(len(r["dense_sets"][k]) > GRID_DRIVERS for k in mo.NEED[method]), "a dense set fits one pass of the grid"
        assert (r["dense"][DRIVER[method]] >= GRID_DRIVERS).any(), "no match driven from a later trip of the loop"
        want[method] = r
    g = pkg.StreamGroup(1, p)
    g.setMultiStageMatching(True)
    for l, r_ in fr:
        g.pushBack(l[None], r_[None], dims)
    for method in (2, 0):
        g.matchFeatures(method)
        nf, nm = g.getCounts()
        assert nf[0].tolist() == [len(x) for x in want[2]["dense_sets"]] and nf[0].min() > GRID_DRIVERS, nf
        assert nm[0] == len(want[method]["dense"]), (method, nm)
        assert g.getMatches(0).tobytes() == want[method]["dense"].tobytes(), method
        assert g.getSparseMatches(0).tobytes() == want[method]["sparse"].tobytes(), method
    g.close()


# ------------------------------------------------------------------ 9. device images on a producer stream (child)
@pytest.mark.gpu
def test_child_device_images_on_a_producer_stream(pkg, gpu):
    """tests/multistage_stream_order_case.py (a process of its own: torch loads its HIP runtime first)."""
    r = subprocess.run([sys.executable, os.path.join(HERE, "multistage_stream_order_case.py")], capture_output=True, text=True,
                       timeout=600, cwd=ROOT)
    assert r.returncode == 0 and "multistage stream-order ok" in r.stdout, r.stdout[-2000:] + r.stderr[-3000:]


# ------------------------------------------------------------------ 10. truncated dense sets, short match lists
def raw_get_matches(pkg, m, cap=8192):
    buf = np.zeros(cap, pkg.P_MATCH_DTYPE)
    n = C.c_int32(0)
    rc = pkg._lib().vh_get_matches(m._h, buf.ctypes.data_as(C.c_void_p), cap, C.byref(n))
    return rc, n.value, buf


@pytest.mark.gpu
def test_truncated_dense_sets_and_short_match_lists(pkg, ob, oracle, gpu):
    """max_features below the dense count: VH_ERR_CAPACITY, and the records are the restatement's on the first
    max_features records of every dense set with the ranges of the UNtruncated sparse sets (the sparse group has the
    worst-case capacity).  max_matches below the pass-2 count: VH_ERR_CAPACITY, the true count, the first records."""
    dims = [W, H, pkg.synth.bytes_per_line(W)]
    fr = scene(pkg, 2, seed=7)
    p, po = pkg.Params.default(multi_stage=1), ob.Params.default(multi_stage=1)
    MF, MM = 256, 100
    for S in (1, 2):
        lone = pkg.Matcher(p, max_features=MF, max_matches=4096, outlier_removal=False) if S == 1 else None
        grp = pkg.StreamGroup(S, p, max_features=MF, max_matches=4096) if S > 1 else None
        h = lone or grp
        h.setMultiStageMatching(True)
        for l, r_ in fr:
            if lone:
                h.pushBack(l, r_, dims)
            else:
                h.pushBack(np.stack([l] * S), np.stack([r_] * S), dims)
        for method in (1, 0, 2):
            r = mo.multistage(ob, oracle, po, dims, method, images_of(method, fr[0], fr[1]))
            check_not_vacuous(po, method, r)
            assert all(len(r["dense_sets"][k]) > MF + 100 for k in mo.NEED[method])
            cut = [None if m is None else m[:MF] for m in r["dense_sets"]]
            want = mo.ranged_matching(po, dims, method, *cut, r["ranges"])
            assert 20 < len(want) < len(r["dense"]), "the truncation changes nothing"
            h.matchFeatures(method)
            if lone:
                rc, n, buf = raw_get_matches(pkg, h)
                assert rc == pkg.VH_ERR_CAPACITY and n == len(want), (method, rc, n, len(want))
                assert buf[:n].tobytes() == want.tobytes(), method
                with pytest.raises(pkg.VisoHipError) as e:
                    h.getMatches()
                assert e.value.code == pkg.VH_ERR_CAPACITY
                assert h.getSparseMatches().tobytes() == r["sparse"].tobytes(), method
            else:
                with pytest.raises(pkg.VisoHipError) as e:
                    h.getMatchesAll(cap_per_stream=4096)
                assert e.value.code == pkg.VH_ERR_CAPACITY
                for s in range(S):
                    assert h.getSparseMatches(s).tobytes() == r["sparse"].tobytes(), (method, s)
        h.close()
    m = pkg.Matcher(p, max_matches=MM, outlier_removal=False)
    m.setMultiStageMatching(True)
    for l, r_ in fr:
        m.pushBack(l, r_, dims)
    for method in (1, 0, 2):
        r = mo.multistage(ob, oracle, po, dims, method, images_of(method, fr[0], fr[1]))
        assert len(r["dense"]) > 4 * MM
        m.matchFeatures(method)
        rc, n, buf = raw_get_matches(pkg, m)
        assert rc == pkg.VH_ERR_CAPACITY and n == len(r["dense"]), (method, rc, n)
        assert buf[:MM].tobytes() == r["dense"][:MM].tobytes(), method
        assert m.getSparseMatches().tobytes() == r["sparse"].tobytes(), method
    m.close()


# ------------------------------------------------------------------ 15. the checking build
@pytest.mark.gpu
def test_child_scale_tests_on_the_checking_build(pkg, gpu):
    """The stateless and lone-matcher tests of this module on libviso_hip_check.so (-DVH_CHECK)."""
    assert os.path.exists(pkg.CHECK_LIB_PATH), "build() makes it"
    env = dict(os.environ, VISO_HIP_LIB=pkg.CHECK_LIB_PATH)
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-q", "-x", "-m", "gpu", "-k",
                        "grid_pass or fractional or ties or degenerate or kitti_size or mono_handles or stale_bid"],
                       env=env, capture_output=True, text=True, timeout=1500, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "16 passed" in r.stdout and " skipped" not in r.stdout, r.stdout[-2000:]
    assert "VH_CHECK" not in r.stderr
