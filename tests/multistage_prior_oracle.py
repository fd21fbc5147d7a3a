"""numpy restatement of multi-stage matching with the motion prior ("Prior contract") -- TEST
INFRASTRUCTURE.

Stock matchFeatures hands Tr_delta to both passes [upstream-recollection].  Pass 1 is the pinned oracle's
matching_quad_prior on the sparse sets; what is restated here is pass 2: multistage_oracle.ranged_matching for the quad
method whose stage 1 (previous right -> current right) is findMatch with the distance term (src/matcher.cpp:257-264)
around the prediction of the circle's driving feature.  Doubles, one operation at a time, in the order of the kernels
(csrc/vh_prior.h); the compares are the literal ones.  With every range at +-match_radius ranged_matching_prior equals
oracle.matching_quad_prior byte for byte (tests/test_multistage_prior.py), which ties it to the pinned code."""
import math

import numpy as np

import multistage_oracle as mo

F32 = np.float32
F64 = np.float64


def predict(params, tr, u1p, v1p, u2p):
    """(u_, v_) of driver (u1p, v1p) whose hop 0 found u2p, under tr (16 doubles, row-major 4x4)."""
    t = np.asarray(tr, F64).reshape(16)
    f, cu, cv, base = F64(params.f), F64(params.cu), F64(params.cv), F64(params.base)
    with np.errstate(all="ignore"):
        d = F64(u1p) - F64(u2p)
        if d < 1.0:
            d = F64(1.0)
        x1p, y1p, z1p = (F64(u1p) - cu) * base / d, (F64(v1p) - cv) * base / d, f * base / d
        x2c = t[0] * x1p + t[1] * y1p + t[2] * z1p + t[3] - base
        y2c = t[4] * x1p + t[5] * y1p + t[6] * z1p + t[7]
        z2c = t[8] * x1p + t[9] * y1p + t[10] * z1p + t[11]
        return f * x2c / z2c + cu, f * y2c / z2c + cv


def costs_in_order(params, q, i1, c, rng, u_, v_):
    """The candidates the flow stage accepts for query i1 in visiting order -> (indices, double costs)."""
    ind, sad = mo.candidates_in_order(params, q, i1, c, rng, True)
    cost = sad.astype(F64)
    if len(ind) and u_ >= 0 and v_ >= 0:  # (false for a NaN)
        with np.errstate(all="ignore"):
            du, dv = c.m[ind, 0].astype(F64) - u_, c.m[ind, 1].astype(F64) - v_
            cost = cost + 4 * np.sqrt(du * du + dv * dv)
    return ind, cost


def find_match_prior(params, q, i1, c, rng, u_, v_):
    ind, cost = costs_in_order(params, q, i1, c, rng, u_, v_)
    min_ind, min_cost = 0, F64(10000000)
    for j, x in zip(ind, cost):
        if x < min_cost:
            min_ind, min_cost = int(j), x
    return min_ind


def ranged_matching_prior(params, dims, m1p, m2p, m1c, m2c, ranges, tr, trace=None):
    """Quad matching with use_prior = true and Tr_delta -> p_match records.  trace (a dict, optional): driver ->
    (u_, v_, indices, costs) of its stage 1."""
    z = np.zeros((0, 12), np.int32)
    sets = [mo.Index(params, dims, z if m is None else m) for m in (m1p, m2p, m1c, m2c)]
    if any(len(s.m) <= 0 for s in sets[1:]):
        return np.zeros(0, mo.P_MATCH_DTYPE)
    ubn, vbn = mo.bin_grid(params, dims)
    bs = F32(params.match_binsize)
    ranges = np.asarray(ranges, F32).reshape(ubn * vbn, 4, 4)
    rec = lambda s, i: (F32(s.m[i, 0]), F32(s.m[i, 1]), i)
    out = []
    for i in range(len(sets[0].m)):
        u, v = int(sets[0].m[i, 0]), int(sets[0].m[i, 1])
        sb = min(int(math.floor(F32(v) / bs)), vbn - 1) * ubn + min(int(math.floor(F32(u) / bs)), ubn - 1)
        i2p = mo.find_match(params, sets[0], i, sets[1], ranges[sb, 0], False)
        u_, v_ = predict(params, tr, u, v, int(sets[1].m[i2p, 0]))
        if trace is not None:
            trace[i] = (u_, v_) + costs_in_order(params, sets[1], i2p, sets[3], ranges[sb, 1], u_, v_)
        i2c = find_match_prior(params, sets[1], i2p, sets[3], ranges[sb, 1], u_, v_)
        i1c = mo.find_match(params, sets[3], i2c, sets[2], ranges[sb, 2], False)
        if mo.find_match(params, sets[2], i1c, sets[0], ranges[sb, 3], True) != i:
            continue
        if sets[0].m[i, 0] >= sets[1].m[i2p, 0] and sets[2].m[i1c, 0] >= sets[3].m[i2c, 0]:
            out.append(rec(sets[0], i) + rec(sets[1], i2p) + rec(sets[2], i1c) + rec(sets[3], i2c))
    return np.array(out, mo.P_MATCH_DTYPE) if out else np.zeros(0, mo.P_MATCH_DTYPE)


def multistage_prior(ob, oracle, po, dims, images, tr, trace=None):
    """Both passes of the quad method for one pair under tr; po carries the intrinsics.  -> dict as mo.multistage."""
    q = mo.sparse_params(ob, po)
    feats = [oracle.compute_features(q, I, dims) for I in images]
    sp, de = [f[0] for f in feats], [f[1] for f in feats]
    raw = oracle.matching_quad_prior(po, dims, tr, *sp)
    voted = oracle.remove_outliers(raw)[0]
    ranges = mo.statistics(po, dims, 2, voted)
    dense = ranged_matching_prior(po, dims, *de, ranges, tr, trace)
    return {"sparse_sets": sp, "dense_sets": de, "sparse_raw": raw, "sparse": voted, "ranges": ranges, "dense": dense}
