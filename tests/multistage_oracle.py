"""numpy restatement of multi-stage matching ("Multi-stage contract") -- TEST INFRASTRUCTURE.

Stock libviso2 with multi_stage = 1 [upstream-recollection]: pass 1 matches the sparse feature sets and votes, the
surviving sparse matches give every statistics bin a search range per stage (computePriorStatistics), pass 2 matches the
dense sets with use_prior = true.  The primitives under it are the pinned oracle's (oracle.compute_features,
oracle.matching, oracle.remove_outliers); what is restated here is the statistics and findMatch / matching with a range
per (statistics bin, stage).  With every range at +-match_radius ranged_matching equals oracle.matching byte for byte
(tests/test_multistage.py), which ties the restatement to the pinned code."""
import math

import numpy as np

F32 = np.float32

P_MATCH_DTYPE = np.dtype([
    ("u1p", "<f4"), ("v1p", "<f4"), ("i1p", "<i4"), ("u2p", "<f4"), ("v2p", "<f4"), ("i2p", "<i4"),
    ("u1c", "<f4"), ("v1c", "<f4"), ("i1c", "<i4"), ("u2c", "<f4"), ("v2c", "<f4"), ("i2c", "<i4")])

#: roles a method reads (0 = 1p, 1 = 2p, 2 = 1c, 3 = 2c)
NEED = {0: (0, 2), 1: (2, 3), 2: (0, 1, 2, 3)}

#: stages of a method's circle: (query role, candidate role, flow?) with roles 0 = 1p, 1 = 2p, 2 = 1c, 3 = 2c
STAGES = {
    0: ((2, 0, True), (0, 2, True)),
    1: ((2, 3, False), (3, 2, False)),
    2: ((0, 1, False), (1, 3, True), (3, 2, False), (2, 0, True)),
}


def bin_grid(params, dims):
    bs = F32(params.match_binsize)
    return int(math.ceil(F32(dims[0]) / bs)), int(math.ceil(F32(dims[1]) / bs))  # src/matcher.cpp:282-283


def full_ranges(params, dims):
    """Every bin and stage at +-match_radius: use_prior changes nothing."""
    ubn, vbn = bin_grid(params, dims)
    r = np.empty((ubn * vbn, 4, 4), F32)
    r[:, :, 0::2] = -params.match_radius
    r[:, :, 1::2] = params.match_radius
    return r


# ------------------------------------------------------------------ statistics
def deltas(method, m):
    """delta[8] of one match and its reference point."""
    if method == 0:
        return [m["u1p"] - m["u1c"], m["v1p"] - m["v1c"], m["u1c"] - m["u1p"], m["v1c"] - m["v1p"]], (m["u1c"], m["v1c"])
    if method == 1:
        return [m["u2c"] - m["u1c"], F32(0), m["u1c"] - m["u2c"], F32(0)], (m["u1c"], m["v1c"])
    return [m["u2p"] - m["u1p"], F32(0), m["u2c"] - m["u2p"], m["v2c"] - m["v2p"],
            m["u1c"] - m["u2c"], F32(0), m["u1p"] - m["u1c"], m["v1p"] - m["v1c"]], (m["u1p"], m["v1p"])


def statistics(params, dims, method, pm):
    """computePriorStatistics -> ranges [nb, 4, 4] float32 (bin = v_bin * ubn + u_bin; stage; u_min, u_max, v_min, v_max).
    Stages the method does not have read +-match_radius."""
    ubn, vbn = bin_grid(params, dims)
    bs, R = F32(params.match_binsize), F32(params.match_radius)
    nst = len(STAGES[method])
    obs = [[] for _ in range(ubn * vbn)]
    clamp = lambda x, n: min(max(x, 0), n - 1)
    for m in pm:
        d, (u, v) = deltas(method, m)
        ub, vb = int(math.floor(F32(u) / bs)), int(math.floor(F32(v) / bs))
        for y in range(clamp(vb - 1, vbn), clamp(vb + 1, vbn) + 1):
            for x in range(clamp(ub - 1, ubn), clamp(ub + 1, ubn) + 1):
                obs[y * ubn + x].append(d)
    out = np.empty((ubn * vbn, 4, 4), F32)
    out[:, :, 0::2] = -R
    out[:, :, 1::2] = R
    for b, lst in enumerate(obs):
        if not lst:
            continue  # an empty bin: +-R, not widened
        a = np.array(lst, F32)
        for st in range(nst):
            for ax in range(2):
                lo, hi = F32(a[:, 2 * st + ax].min()), F32(a[:, 2 * st + ax].max())
                d = F32(hi - lo)
                if d < 20:
                    h = F32(math.ceil(F32(F32(20) - d) / F32(2)))
                    lo, hi = F32(lo - h), F32(hi + h)
                out[b, st, 2 * ax], out[b, st, 2 * ax + 1] = lo, hi
    return out


# ------------------------------------------------------------------ ranged findMatch / matching
class Index:
    """createIndexVector (src/matcher.cpp:194-214): ascending indices per bin (c * vbn + v_bin) * ubn + u_bin."""

    def __init__(self, params, dims, m):
        self.m = np.ascontiguousarray(m, np.int32).reshape(-1, 12)
        self.ubn, self.vbn = bin_grid(params, dims)
        bs = F32(params.match_binsize)
        self.desc = self.m[:, 4:12].copy().view(np.uint8).reshape(-1, 32).astype(np.int32)
        self.bins = {}
        for i, r in enumerate(self.m):
            ub = min(int(math.floor(F32(r[0]) / bs)), self.ubn - 1)
            vb = min(int(math.floor(F32(r[1]) / bs)), self.vbn - 1)
            self.bins.setdefault((int(r[3]) * self.vbn + vb) * self.ubn + ub, []).append(i)
        self.bins = {k: np.array(v, np.int64) for k, v in self.bins.items()}


def find_match(params, q, i1, c, rng, flow):
    """findMatch (src/matcher.cpp:216-272) with use_prior = true: query i1 of index q in index c inside rng =
    (u_min, u_max, v_min, v_max) relative to the query -> min_ind (0 when nothing is accepted)."""
    bs = F32(params.match_binsize)
    u1, v1, cls = int(q.m[i1, 0]), int(q.m[i1, 1]), int(q.m[i1, 3])
    u_min, u_max = F32(F32(u1) + rng[0]), F32(F32(u1) + rng[1])
    v_min, v_max = F32(F32(v1) + rng[2]), F32(F32(v1) + rng[3])
    if not flow:
        v_min, v_max = F32(v1 - params.match_disp_tolerance), F32(v1 + params.match_disp_tolerance)
    cl = lambda x, n: min(max(int(math.floor(x / bs)), 0), n - 1)
    ub0, ub1, vb0, vb1 = cl(u_min, c.ubn), cl(u_max, c.ubn), cl(v_min, c.vbn), cl(v_max, c.vbn)
    d1 = q.desc[i1]
    min_ind, min_cost = 0, 10000000
    for ub in range(ub0, ub1 + 1):
        for vb in range(vb0, vb1 + 1):
            idx = c.bins.get((cls * c.vbn + vb) * c.ubn + ub)
            if idx is None:
                continue
            u2, v2 = c.m[idx, 0].astype(F32), c.m[idx, 1].astype(F32)
            ok = (u2 >= u_min) & (u2 <= u_max) & (v2 >= v_min) & (v2 <= v_max)
            if not ok.any():
                continue
            idx = idx[ok]
            cost = np.abs(c.desc[idx] - d1).sum(axis=1)
            j = int(np.argmin(cost))  # the first minimum of the bin, in list order
            if cost[j] < min_cost:    # strict: an earlier bin keeps a tie
                min_ind, min_cost = int(idx[j]), int(cost[j])
    return min_ind


def ranged_matching(params, dims, method, m1p, m2p, m1c, m2c, ranges, trace=None):
    """Matcher::matching (src/matcher.cpp:274-344 and the stereo / quad compositions of SURVEY App. A.7) with
    use_prior = true -> p_match records.  trace (a dict, optional): (stage, query index) -> set of statistics bins whose
    drivers searched that query."""
    z = np.zeros((0, 12), np.int32)
    sets = [Index(params, dims, z if m is None else m) for m in (m1p, m2p, m1c, m2c)]
    n = [len(s.m) for s in sets]
    ubn, vbn = bin_grid(params, dims)
    bs = F32(params.match_binsize)
    ranges = np.asarray(ranges, F32).reshape(ubn * vbn, 4, 4)
    need = NEED[method]
    out = []
    if any(n[r] <= 0 for r in need):
        return np.zeros(0, P_MATCH_DTYPE)
    drive = sets[0] if method == 2 else sets[2]
    seen = set()  # the first-writer pixel mask M (flow)
    rec = lambda s, i: (F32(s.m[i, 0]), F32(s.m[i, 1]), i)
    none = (F32(-1), F32(-1), -1)
    for i in range(len(drive.m)):
        u, v = int(drive.m[i, 0]), int(drive.m[i, 1])
        sb = min(int(math.floor(F32(v) / bs)), vbn - 1) * ubn + min(int(math.floor(F32(u) / bs)), ubn - 1)  # :314-317
        idx = [i]
        for st, (qr, cr, flow) in enumerate(STAGES[method]):
            if trace is not None:
                trace.setdefault((st, idx[-1]), set()).add(sb)
            idx.append(find_match(params, sets[qr], idx[-1], sets[cr], ranges[sb, st], flow))
        if idx[-1] != i:
            continue
        if method == 0:
            i1p = idx[1]
            if (u, v) in seen:
                continue
            seen.add((u, v))
            out.append(rec(sets[0], i1p) + none + rec(sets[2], i) + none)
        elif method == 1:
            i2c = idx[1]
            if sets[2].m[i, 0] >= sets[3].m[i2c, 0]:
                out.append(none + none + rec(sets[2], i) + rec(sets[3], i2c))
        else:
            i2p, i2c, i1c = idx[1], idx[2], idx[3]
            if sets[0].m[i, 0] >= sets[1].m[i2p, 0] and sets[2].m[i1c, 0] >= sets[3].m[i2c, 0]:
                out.append(rec(sets[0], i) + rec(sets[1], i2p) + rec(sets[2], i1c) + rec(sets[3], i2c))
    return np.array(out, P_MATCH_DTYPE) if out else np.zeros(0, P_MATCH_DTYPE)


def candidates_in_order(params, q, i1, c, rng, flow):
    """The candidates findMatch accepts for query i1, in its visiting order (u-bin outer, v-bin inner, list order)
    -> (indices, costs).  find_match's answer is the first strict minimum of this sequence."""
    bs = F32(params.match_binsize)
    u1, v1, cls = int(q.m[i1, 0]), int(q.m[i1, 1]), int(q.m[i1, 3])
    u_min, u_max = F32(F32(u1) + rng[0]), F32(F32(u1) + rng[1])
    v_min, v_max = F32(F32(v1) + rng[2]), F32(F32(v1) + rng[3])
    if not flow:
        v_min, v_max = F32(v1 - params.match_disp_tolerance), F32(v1 + params.match_disp_tolerance)
    cl = lambda x, n: min(max(int(math.floor(x / bs)), 0), n - 1)
    ind, cost = [], []
    for ub in range(cl(u_min, c.ubn), cl(u_max, c.ubn) + 1):
        for vb in range(cl(v_min, c.vbn), cl(v_max, c.vbn) + 1):
            for j in c.bins.get((cls * c.vbn + vb) * c.ubn + ub, ()):
                u2, v2 = F32(c.m[j, 0]), F32(c.m[j, 1])
                if u_min <= u2 <= u_max and v_min <= v2 <= v_max:
                    ind.append(int(j))
                    cost.append(int(np.abs(c.desc[j] - q.desc[i1]).sum()))
    return np.array(ind, np.int64), np.array(cost, np.int64)


def misrounded(ranges, how):
    """ranges with the bounds turned into integers the WRONG way (the right way is ceil(min), floor(max)): what a kernel
    with that rounding would search.  how: "nearest" (halves away from zero), "trunc" (toward zero), "outward"
    (floor(min), ceil(max))."""
    r = np.asarray(ranges, np.float64).copy()
    if how == "nearest":
        r = np.sign(r) * np.floor(np.abs(r) + 0.5)
    elif how == "trunc":
        r = np.trunc(r)
    elif how == "outward":
        r[..., 0::2] = np.floor(r[..., 0::2])
        r[..., 1::2] = np.ceil(r[..., 1::2])
    else:
        raise ValueError(how)
    return r.astype(F32)


# ------------------------------------------------------------------ the composition
def sparse_params(ob, po):
    q = ob.Params.default(**{n: getattr(po, n) for n, _ in ob.Params._fields_})
    q.multi_stage = 1
    return q


def multistage(ob, oracle, po, dims, method, images, fast=False):
    """Both passes for one pair.  images = (I1p, I2p, I1c, I2c), None where the method reads none.
    -> dict(sparse_sets, dense_sets, sparse_raw, sparse, ranges, dense).  fast: pass 2 by the C form of ranged_matching
    (oracle.ranged_matching, tied to the numpy form by tests/test_multistage_scale.py) -- full-size frames."""
    q = sparse_params(ob, po)
    feats = [None if I is None else oracle.compute_features(q, I, dims) for I in images]
    need = NEED[method]
    sp = [feats[r][0] if r in need and feats[r] is not None else None for r in range(4)]
    de = [feats[r][1] if r in need and feats[r] is not None else None for r in range(4)]
    raw = oracle.matching(po, dims, method, *sp)
    voted = raw if method == 1 else oracle.remove_outliers(raw)[0]  # (stereo lists carry no flow: left alone)
    ranges = statistics(po, dims, method, voted)
    dense = oracle.ranged_matching(po, dims, method, *de, ranges) if fast else ranged_matching(po, dims, method, *de, ranges)
    return {"sparse_sets": sp, "dense_sets": de, "sparse_raw": raw, "sparse": voted, "ranges": ranges, "dense": dense}


# ------------------------------------------------------------------ recorded answers
def recorded_answers(ob, oracle, cases):
    """What tests/golden/multistage_answers.npz records.  cases: (name, dims, parameter overrides, fast, previous pair,
    current pair), see answer_cases() of tests/test_multistage_scale.py -> name_m<method> -> ([n sparse, n range values,
    n dense], [SHA-256 of sparse, ranges, dense])."""
    import hashlib
    out = {}
    for name, dims, kw, fast, prev, cur in cases:
        po = ob.Params.default(multi_stage=1, **kw)
        imgs = (prev[0], prev[1], cur[0], cur[1])
        for method in (0, 1, 2):
            r = multistage(ob, oracle, po, dims, method, [imgs[k] if k in NEED[method] else None for k in range(4)], fast=fast)
            parts = [np.ascontiguousarray(r[k]) for k in ("sparse", "ranges", "dense")]
            out["%s_m%d" % (name, method)] = ([len(parts[0]), int(parts[1].size), len(parts[2])],
                                             [hashlib.sha256(x.tobytes()).hexdigest() for x in parts])
    return out
