"""Matcher::getGain on the GPU: vh_gain, vh_group_set_gain, vh_group_gain(_indices) and the
lone-matcher forms.  The stateless entry is held to tests/gain_oracle.py bit for bit, gain and num both -- no tolerance
band: every step is a single-precision operation and the sum runs in the order of the index list.  The handle entries are
held to the stateless entry on the downloaded lists, positions and the pushed images, byte for byte.  gain_oracle.mean is
pinned to the reference's own Matcher::mean by tests/golden/gain_reference.npz (tools/gen_golden_gain.py)."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import gain_oracle as go
from conftest import GOLDEN, ROOT

SYMBOLS = ("vh_gain", "vh_group_set_gain", "vh_set_gain", "vh_group_gain", "vh_match_gain", "vh_group_gain_indices", "vh_match_gain_indices")
SCOPES = ("gain_copy", "gain_ratio", "gain_sum")
FLOW, QUAD = 0, 2
W0, H0, BPL0 = 40, 24, 48         # the stateless cases
DIMS0 = (W0, H0, BPL0)
RING = 4                          # VH_RING


def expect(pkg, code, call):
    with pytest.raises(pkg.VisoHipError) as e:
        call()
    assert e.value.code == code, e.value


def p_dtype():
    import __graft_entry__ as entry
    return entry.load_package().P_MATCH_DTYPE


def records(coords):
    """[(u1p, v1p, u1c, v1c)] -> p_match records (the other fields -1)."""
    pm = np.zeros(len(coords), p_dtype())
    for name in pm.dtype.names:
        pm[name] = -1
    for k, c in enumerate(coords):
        pm[k]["u1p"], pm[k]["v1p"], pm[k]["u1c"], pm[k]["v1c"] = c
    return pm


# ---- the constructed inputs, and what the restatement says of them: computed once ---------------------------------
def edge_images():
    """Random bytes of 30 .. 255 (every mean above 10); in the previous image a 7 x 7 patch of tens around (10, 10) -- a mean
    of exactly 10.0 -- and one around (20, 10) with a single 11: 10 + 1/49; in the current image a patch of zeros around (30, 10)."""
    rng = np.random.default_rng(5)
    Ip = rng.integers(30, 256, (H0, BPL0), dtype=np.uint8)
    Ic = rng.integers(30, 256, (H0, BPL0), dtype=np.uint8)
    Ip[7:14, 7:14] = 10
    Ip[7:14, 17:24] = 10
    Ip[9, 21] = 11
    Ic[7:14, 27:34] = 0
    return Ip, Ic


INF, NAN, BIG = np.inf, np.nan, 16777216.0
EDGE_COORDS = [
    (20.0, 12.0, 21.0, 13.0),                                # 0 interior
    (1.0, 12.0, 2.0, 12.0), (38.0, 12.0, 37.0, 12.0),        # 1, 2 clamped left / right
    (20.0, 1.0, 20.0, 2.0), (20.0, 22.0, 20.0, 21.0),        # 3, 4 clamped top / bottom
    (0.0, 0.0, 39.0, 23.0), (39.0, 0.0, 0.0, 23.0),          # 5, 6 corners; exactly on W - 1 / H - 1
    (40.0, 24.0, 40.0, 12.0), (44.0, 30.0, 20.0, 27.0),      # 7, 8 one beyond the image, further beyond (a 1-column window)
    (-2.0, -5.0, -1.0, 3.0), (-100.0, 12.0, 20.0, -100.0),   # 9, 10 negative
    (10.0, 10.0, 20.0, 12.0),                                # 11 mean_prev exactly 10.0: excluded
    (20.0, 10.0, 20.0, 12.0),                                # 12 mean_prev 10 + 1/49: included
    (20.0, 12.0, 30.0, 10.0),                                # 13 current window all zeros: ratio 0, counted
    (NAN, 12.0, 20.0, 12.0), (20.0, 12.0, 20.0, INF), (20.0, 12.0, BIG, 12.0), (20.0, -BIG, 20.0, 12.0), (-INF, 1.0, 2.0, 3.0),  # 14 .. 18 skipped
    (12.99, 7.01, 22.5, 3.999), (-0.5, -0.99, 38.999, 22.001),  # 19, 20 truncation (toward zero)
    (16777215.0, 12.0, 20.0, 12.0),                          # 21 the largest magnitude that counts
]
EDGE_IDX = list(range(len(EDGE_COORDS))) + [0, 0, 13, 5, -1, len(EDGE_COORDS), 12, 11, -7, 2 ** 30, 13]   # duplicates, -1, n, far outside
EXCLUDED_IDX = [11, 14, 15, 16, 17, 18, -1, len(EDGE_COORDS), 11]


def order_case():
    """The order-sensitive list: previous means of about 12 or about 227, current means of about 1.5 or about 227 and the
    windows across the borders between them -- ratios from below 0.01 to about 19 -- over 3 000 entries."""
    rng = np.random.default_rng(9)
    Ip = np.zeros((H0, BPL0), np.uint8); Ic = np.zeros((H0, BPL0), np.uint8)
    Ip[:, :20] = rng.integers(11, 14, (H0, 20)); Ip[:, 20:W0] = rng.integers(200, 256, (H0, W0 - 20))
    Ic[:12, :W0] = rng.integers(0, 4, (12, W0)); Ic[12:, :W0] = rng.integers(200, 256, (H0 - 12, W0))
    n = 400
    pm = records(np.stack([rng.uniform(0, W0, n), rng.uniform(0, H0, n), rng.uniform(0, W0, n), rng.uniform(0, H0, n)], 1).astype(np.float32))
    idx = rng.integers(0, n, 3000).astype(np.int32)
    return pm, idx, Ip, Ic


def random_list(seed, n, k):
    rng = np.random.default_rng(seed)
    pm = records(np.stack([rng.uniform(-4, W0 + 4, n), rng.uniform(-4, H0 + 4, n), rng.uniform(-4, W0 + 4, n), rng.uniform(-4, H0 + 4, n)], 1).astype(np.float32))
    return pm, rng.integers(-1, n + 1, k).astype(np.int32)


_CASES = {}


def cases():
    """name -> (pm, idx, Ip, Ic, (gain, num) of the restatement)"""
    if not _CASES:
        Ip, Ic = edge_images()
        edge = records(EDGE_COORDS)
        c = {"edges": (edge, np.array(EDGE_IDX, np.int32), Ip, Ic), "excluded": (edge, np.array(EXCLUDED_IDX, np.int32), Ip, Ic),
             "order": order_case(), "no_records": (records([]), np.array([0, 1, -1], np.int32), Ip, Ic)}
        for k in (0, 1, 63, 64, 65, 257):
            c[f"k{k}"] = random_list(100 + k, 50, k) + (Ip, Ic)
        rng = np.random.default_rng(17)
        for j in range(6):   # fillers of the 17-list call: other images, other lengths
            c[f"fill{j}"] = random_list(200 + j, 30 + 7 * j, 20 + 31 * j) + (rng.integers(0, 256, (H0, BPL0), dtype=np.uint8), rng.integers(0, 256, (H0, BPL0), dtype=np.uint8))
        for name, (pm, idx, a, b) in c.items():
            _CASES[name] = (pm, idx, a, b, go.gain(pm, idx, a, b, DIMS0))
    return _CASES


CALLS = {1: [["edges"], ["order"], ["excluded"], ["k257"]],
         2: [["k64", "k65"], ["k0", "edges"], ["order", "no_records"]],
         17: [["edges", "k0", "k1", "k63", "k64", "k65", "k257", "excluded", "order", "no_records", "fill0", "fill1", "fill2", "fill3", "fill4", "fill5", "edges"]]}


# ---- not GPU -----------------------------------------------------------------------------------------------------
def test_restatement_mean_equals_the_reference_fixture():
    z = np.load(os.path.join(GOLDEN, "gain_reference.npz"))
    W, H, bpl = (int(v) for v in z["dims"])
    assert len(z["windows"]) >= 300
    sizes = set()
    for (u0, u1, v0, v1), want in zip(z["windows"], z["means"]):
        got = go.mean(z["image"], bpl, int(u0), int(u1), int(v0), int(v1))
        assert np.float32(got).tobytes() == np.float32(want).tobytes(), (u0, u1, v0, v1, got, want)
        sizes.add((u1 - u0 + 1, v1 - v0 + 1))
    assert {(w, h) for w in range(1, 8) for h in range(1, 8)} <= sizes and any(w * h > 4096 for w, h in sizes)


def test_symbols_declared_exported_and_mirrored(pkg):
    header = open(os.path.join(ROOT, "include", "viso_hip.h")).read()
    lib = pkg._lib()
    for name in SYMBOLS:
        assert re.search(r"\b" + name + r"\(", header), name
        assert name in pkg.ABI_SYMBOLS and hasattr(lib, name), name
    assert all(hasattr(pkg.StreamGroup, n) for n in ("setGain", "gain")) and all(hasattr(pkg.Matcher, n) for n in ("setGain", "getGain"))
    assert hasattr(pkg.SequenceGroup, "gain") and callable(pkg.gain)
    # argument errors that need no device
    assert lib.vh_gain(0, -1, None, None, None, 0, None, None, None, None, None, None) == pkg.VH_ERR_INVALID_ARG
    assert lib.vh_gain(0, 0, None, None, None, 0, None, None, None, None, None, None) == pkg.VH_OK
    assert lib.vh_group_set_gain(None, 1) == pkg.VH_ERR_INVALID_ARG and lib.vh_group_gain(None, None, None) == pkg.VH_ERR_INVALID_ARG
    g, n = pkg.gain([records([(3.0, 3.0, 3.0, 3.0)])], [[]], np.zeros((H0, BPL0), np.uint8), np.zeros((H0, BPL0), np.uint8), DIMS0)
    assert g[0] == 1.0 and n[0] == 0   # no index entries: nothing launched, no device needed


def test_shim_member_compiles_and_links(pkg, tmp_path):
    src = tmp_path / "gain_shim.cpp"
    src.write_text('#include "viso_hip_matcher.hpp"\n#include <cstdio>\n'
                   "int main() { if (vh_device_count() < 1) { std::puts(\"no device\"); return 0; }\n"
                   "  Matcher::parameters p; Matcher m(p); m.setGainImages(true);\n"
                   "  float g = m.getGain(std::vector<int32_t>()); std::printf(\"%f\\n\", g); return g == 1.0f ? 0 : 1; }\n")
    exe = str(tmp_path / "gain_shim")
    subprocess.check_call(["g++", "-std=c++17", "-I" + os.path.join(ROOT, "include"), str(src), "-L" + os.path.dirname(pkg.LIB_PATH),
                           "-lviso_hip", "-Wl,-rpath," + os.path.dirname(pkg.LIB_PATH), "-o", exe])


def test_order_sensitive_input_tells_a_reordered_sum():
    pm, idx, Ip, Ic, (gain, num) = cases()["order"]
    r = np.array(go.ratios(pm, idx, Ip, Ic, DIMS0), np.float32)
    assert num == len(r) >= 2000
    pos = r[r > 0]
    assert pos.max() / pos.min() >= 1000.0                             # three decades
    seq = np.float32(0)
    for x in r:
        seq = np.float32(seq + x)
    assert seq.tobytes() != np.sum(r, dtype=np.float32).tobytes()      # numpy adds pairwise: a tree
    assert np.float32(seq / np.float32(num)).tobytes() == gain.tobytes()


def test_constructed_cases_hold_their_premises():
    c = cases()
    edge, _, Ip, Ic, (gain, num) = c["edges"]
    assert go.mean(Ip, BPL0, 7, 13, 7, 13) == np.float32(10.0) and go.mean(Ip, BPL0, 17, 23, 7, 13) == np.float32(491.0) / np.float32(49.0) > 10
    assert go.mean(Ic, BPL0, 27, 33, 7, 13) == 0
    assert go.window(40.0, 24.0, W0, H0) == (37, 39, 21, 23) and go.window(44.0, 30.0, W0, H0) == (39, 39, 23, 23)
    assert go.window(-0.5, -0.99, W0, H0) == (0, 3, 0, 3) and go.window(12.99, 7.01, W0, H0) == (9, 15, 4, 10)
    counted = [len(go.ratios(edge, [i], Ip, Ic, DIMS0)) for i in range(len(edge))]
    assert counted == [1] * 11 + [0, 1, 1] + [0] * 5 + [1, 1, 1]
    assert go.ratios(edge, [13], Ip, Ic, DIMS0)[0] == 0 and num == sum(counted[i] for i in EDGE_IDX if 0 <= i < len(edge))
    assert c["excluded"][4] == (np.float32(1), 0) and c["no_records"][4] == (np.float32(1), 0) and c["k0"][4] == (np.float32(1), 0)


# ---- GPU, stateless ------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("n_lists", sorted(CALLS))
def test_gpu_stateless_parity(n_lists, pkg, gpu):
    c = cases()
    for names in CALLS[n_lists]:
        assert len(names) == n_lists
        gain, num = pkg.gain([c[k][0] for k in names], [c[k][1] for k in names], np.stack([c[k][2] for k in names]),
                             np.stack([c[k][3] for k in names]), DIMS0)
        for j, k in enumerate(names):
            want_gain, want_num = c[k][4]
            print(k, gain[j], num[j], want_gain, want_num)
            assert num[j] == want_num and gain[j].tobytes() == want_gain.tobytes(), (k, gain[j], num[j], want_gain, want_num)


@pytest.mark.gpu
def test_gpu_stateless_strided_images_and_offsets(pkg, gpu):
    """The raw entry: image pairs further apart than their size, and lists / index lists that begin past element 0."""
    c = cases()
    names = ["edges", "k65"]
    lib = pkg._lib()
    stride = H0 * BPL0 + 80
    Ip = np.zeros(2 * stride, np.uint8); Ic = np.zeros(2 * stride, np.uint8)
    for j, k in enumerate(names):
        Ip[j * stride: j * stride + H0 * BPL0] = c[k][2].reshape(-1); Ic[j * stride: j * stride + H0 * BPL0] = c[k][3].reshape(-1)
    pm = np.concatenate([records([(1.0, 1.0, 1.0, 1.0)] * 3)] + [c[k][0] for k in names])
    idx = np.concatenate([np.zeros(5, np.int32)] + [c[k][1] for k in names])
    off = np.array([3, 3 + len(c["edges"][0]), len(pm)], np.int32)
    ioff = np.array([5, 5 + len(c["edges"][1]), len(idx)], np.int32)
    gain = np.zeros(2, np.float32); num = np.zeros(2, np.int32)
    dims = np.array(DIMS0, np.int32)
    p = lambda a: a.ctypes.data  # noqa: E731
    rc = lib.vh_gain(0, 2, p(dims), p(Ip), p(Ic), stride, p(pm), p(off), p(idx), p(ioff), p(gain), p(num))
    assert rc == pkg.VH_OK
    for j, k in enumerate(names):
        assert num[j] == c[k][4][1] and gain[j].tobytes() == c[k][4][0].tobytes(), (k, gain[j], num[j], c[k][4])


@pytest.mark.gpu
def test_child_checking_build(pkg, gpu):
    """The stateless cases once more on libviso_hip_check.so (-DVH_CHECK): every plane address and list position verified."""
    assert os.path.exists(pkg.CHECK_LIB_PATH), "build() makes it"
    env = dict(os.environ, VISO_HIP_LIB=pkg.CHECK_LIB_PATH)
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-q", "-x", "-m", "gpu", "-k", "stateless"],
                       env=env, capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "4 passed" in r.stdout and " skipped" not in r.stdout, r.stdout[-2000:]
    assert "VH_CHECK" not in r.stderr


# ---- GPU, handles --------------------------------------------------------------------------------------------------
W, H, S = 240, 120, 3
CAL = dict(f=225.0, cu=120.0, cv=60.0, base=0.5)
# the synthetic frames pan by (5, 1) px per frame at a disparity of 6: a plane at Z = f base / 6 under a sideways translation;
# a small roll on top makes the far records outliers (tests/test_motion_inliers.py: TR2)
Z = CAL["f"] * CAL["base"] / 6
TR = (0.0, 0.0, 0.02, -5 * Z / CAL["f"], -1 * Z / CAL["f"], 0.0)
GAINS = (1.0, 1.15, 0.92, 1.06, 1.1, 0.97)   # applied to the pixels of frame t
_FRAMES = {}


def dims_of(pkg):
    return [W, H, pkg.synth.bytes_per_line(W)]


def scaled(img, k):
    return np.clip(np.rint(img.astype(np.float64) * k), 0, 255).astype(np.uint8)


def frames_of(pkg):
    """[stream][t] -> (left, right): test_post_dense.py's three streams (textured, constant, textured on the left 45 %), the
    pixels of frame t multiplied by GAINS[t]."""
    if "f" not in _FRAMES:
        fr = [pkg.synth.stereo_sequence(W, H, len(GAINS), disparity=6, blur=3, seed=seed) for seed in (71, 72, 73)]
        fr[1] = [(np.full_like(a, 90), np.full_like(b, 90)) for a, b in fr[1]]
        half = []
        for a, b in fr[2]:
            a, b = a.copy(), b.copy()
            a[:, int(0.45 * W):] = 90; b[:, int(0.45 * W):] = 90
            half.append((a, b))
        fr[2] = half
        _FRAMES["f"] = [[(scaled(a, GAINS[t]), scaled(b, GAINS[t])) for t, (a, b) in enumerate(f)] for f in fr]
    return _FRAMES["f"]


def push(g, fr, t, dims, replace=False):
    g.pushBack(np.stack([f[t][0] for f in fr]), np.stack([f[t][1] for f in fr]), dims, replace=replace)


def lefts(fr, t):
    return np.stack([f[t][0] for f in fr])


def same_as_stateless(pkg, got, lists, pos, Ip, Ic, dims, what):
    want = pkg.gain(lists, pos, Ip, Ic, dims)
    print(what, got[0], got[1], want[0], want[1])
    assert got[0].tobytes() == want[0].tobytes() and np.array_equal(got[1], want[1]), (what, got, want)


def check_inlier_gain(pkg, g, Ip, Ic, dims, what):
    """gain() over the current classification == the stateless entry on the downloaded lists, positions and images"""
    got = g.gain()
    lists = [g.getMatches(s) for s in range(g.S)]
    pos = [g.getInlierMatches(s)[1] for s in range(g.S)]
    same_as_stateless(pkg, got, lists, pos, Ip, Ic, dims, what)
    return got, lists, pos


def mono_models(pkg, ob, g):
    e = pkg.MonoParams.default(ransac_iters=50, f=CAL["f"], cu=CAL["cu"], cv=CAL["cv"], height=1.0)
    r = ob.glibc_rand_after_srand0(8 * e.ransac_iters).reshape(e.ransac_iters, 8)
    _, ok, _, model = g.estimateMotionMono(e, np.stack([r] * g.S), model=True)
    return e, model, ok.astype(np.int32)


@pytest.mark.gpu
def test_gpu_group_of_three(pkg, ob, gpu):
    """Stereo and mono classifications of a group with an empty and a short stream; the value lies near the applied gain.
    Near: the restatement on the TRUE correspondences of stream 0 (a grid of points under the known pan of (5, 1) px) gives
    the applied gain to within 0.01 (pixel rounding over windows of mean ~130; asserted); wrong matches and the minority of
    windows that clip at 255 move the mean of some thousand ratios by less than 0.03 more -- a sanity bound, not the contract."""
    fr, dims = frames_of(pkg), dims_of(pkg)
    g = pkg.StreamGroup(S, pkg.Params.default())
    g.setGain(True)
    e = pkg.EgoParams.default(ransac_iters=50, inlier_threshold=2.5, **CAL)
    push(g, fr, 0, dims)
    push(g, fr, 1, dims)
    Ip, Ic = lefts(fr, 0), lefts(fr, 1)
    grid = records([(u, v, u - 5.0, v - 1.0) for u in range(20, W - 20, 12) for v in range(15, H - 15, 10)])
    ideal, n_ideal = go.gain(grid, np.arange(len(grid)), Ip[0], Ic[0], dims)
    applied = GAINS[1] / GAINS[0]
    assert n_ideal == len(grid) and abs(float(ideal) - applied) < 0.01, (ideal, applied)
    g.matchFeatures(QUAD)
    counts = g.motionInliers(e, np.array([TR] * S), np.ones(S, np.int32))
    (gain, num), lists, pos = check_inlier_gain(pkg, g, Ip, Ic, dims, "quad")
    assert np.array_equal(num <= counts, [True] * S) and num[0] > 100 and num[1] == 0 and gain[1] == 1.0 and 0 < num[2] < num[0], (num, counts)
    assert abs(float(gain[0]) - float(ideal)) < 0.03 and abs(float(gain[2]) - float(ideal)) < 0.03, (gain, ideal)
    want0 = go.gain(lists[0], pos[0], Ip[0], Ic[0], dims)             # and the restatement itself, on the longest list
    assert gain[0].tobytes() == want0[0].tobytes() and num[0] == want0[1]
    g.motionInliers(e, np.array([TR] * S), np.array([0, 1, 1], np.int32))   # ok = 0: gain 1, num 0
    gain0, num0 = g.gain()
    assert gain0[0] == 1.0 and num0[0] == 0 and gain0[2].tobytes() == gain[2].tobytes() and num0[2] == num[2]
    # flow lists under the mono test
    push(g, fr, 2, dims)
    g.matchFeatures(FLOW)
    m, model, ok = mono_models(pkg, ob, g)
    counts = g.motionInliersMono(m, model, ok)
    (gain, num), _, _ = check_inlier_gain(pkg, g, lefts(fr, 1), lefts(fr, 2), dims, "flow mono")
    assert num[1] == 0 and (not ok[0] or (num[0] > 50 and abs(float(gain[0]) - GAINS[2] / GAINS[1]) < 0.04)), (gain, num, ok, counts)
    g.close()


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["replace", "half_resolution", "refinement2", "multi_stage"])
def test_gpu_group_variants(case, pkg, ob, gpu):
    """A replace push overwrites the current plane; half_resolution = 1 keeps the full-resolution images; refinement 2
    gives fractional coordinates; multi-stage matching: the lists are pass 2's."""
    fr, dims = frames_of(pkg), dims_of(pkg)
    over = {"half_resolution": dict(half_resolution=1), "refinement2": dict(refinement=2), "multi_stage": dict(multi_stage=1)}.get(case, {})
    g = pkg.StreamGroup(S, pkg.Params.default(**over))
    if case == "multi_stage":
        g.setMultiStageMatching(True)
    g.setGain(True)
    e = pkg.EgoParams.default(ransac_iters=50, inlier_threshold=2.5, **CAL)
    push(g, fr, 0, dims)
    push(g, fr, 2 if case == "replace" else 1, dims)
    t_cur = 1
    if case == "replace":
        push(g, fr, 1, dims, replace=True)
    g.matchFeatures(QUAD)
    g.motionInliers(e, np.array([TR] * S), np.ones(S, np.int32))
    (gain, num), lists, _ = check_inlier_gain(pkg, g, lefts(fr, 0), lefts(fr, t_cur), dims, case)
    assert num[0] > 50 and abs(float(gain[0]) - GAINS[1]) < 0.04, (gain, num)
    if case == "refinement2":
        u = lists[0]["u1p"]                                            # (the refined coordinates of the flow hop)
        assert np.any(u != np.trunc(u))
    g.close()


@pytest.mark.gpu
def test_gpu_sequence_handle(pkg, ob, gpu):
    """Chunks of 4 and 2 frames: row r reads the images of rows r - 1 and r, row 0 of the second chunk the previous chunk's last."""
    fr, dims = frames_of(pkg)[0], dims_of(pkg)
    g = pkg.SequenceGroup(4, pkg.Params.default())
    g.setGain(True)
    e = pkg.EgoParams.default(ransac_iters=50, inlier_threshold=2.5, **CAL)
    blank = np.zeros_like(fr[0][0])
    for F, n in ((0, 4), (4, 2)):
        g.pushBack(np.stack([fr[t][0] for t in range(F, F + n)]), np.stack([fr[t][1] for t in range(F, F + n)]), dims)
        g.matchFeatures(QUAD)
        g.motionInliers(e, np.array([TR] * 4), np.ones(4, np.int32))
        pairs = [(F + r - 1, F + r) if (r < n and F + r >= 1) else None for r in range(4)]
        Ip = np.stack([fr[p[0]][0] if p else blank for p in pairs]); Ic = np.stack([fr[p[1]][0] if p else blank for p in pairs])
        (gain, num), lists, _ = check_inlier_gain(pkg, g, Ip, Ic, dims, f"chunk at {F}")
        # and over every record of every row (the pan of the synthetic frames wraps between frames 3 and 4: TR fits no record
        # of row 0 of the second chunk, the row that reads the previous chunk's last image)
        idx = [np.arange(len(pm), dtype=np.int32) for pm in lists]
        every = g.gain(idx)
        same_as_stateless(pkg, every, lists, idx, Ip, Ic, dims, f"chunk at {F}, every record")
        for r, p in enumerate(pairs):
            if p is None:
                assert gain[r] == 1.0 and num[r] == 0 and every[0][r] == 1.0 and every[1][r] == 0, (F, r)
            else:
                assert num[r] <= every[1][r] and every[1][r] > 50 and abs(float(every[0][r]) - GAINS[p[1]] / GAINS[p[0]]) < 0.04, (F, r, every)
    g.close()


@pytest.mark.gpu
def test_gpu_indices_form_and_lone_matcher(pkg, ob, gpu):
    """The caller's index lists on a group; a lone matcher whose list removeOutliers and bucketFeatures replaced on the host."""
    fr, dims = frames_of(pkg), dims_of(pkg)
    g = pkg.StreamGroup(S, pkg.Params.default())
    g.setGain(True)
    push(g, fr, 0, dims)
    push(g, fr, 1, dims)
    g.matchFeatures(QUAD)
    lists = [g.getMatches(s) for s in range(S)]
    rng = np.random.default_rng(3)
    idx = [np.concatenate([rng.permutation(len(pm))[::3], [-1, len(pm)]]).astype(np.int32) for pm in lists]
    idx[2] = np.zeros(0, np.int32)
    got = g.gain(idx)                                                  # no classification needed
    same_as_stateless(pkg, got, lists, idx, lefts(fr, 0), lefts(fr, 1), dims, "indices")
    assert got[1][0] > 100 and got[1][1] == 0 and got[1][2] == 0
    g.removeOutliers()                                                 # the lists are host-side ones now
    lists = [g.getMatches(s) for s in range(S)]
    idx = [np.arange(len(pm), dtype=np.int32)[::-1] for pm in lists]
    same_as_stateless(pkg, g.gain(idx), lists, idx, lefts(fr, 0), lefts(fr, 1), dims, "indices after removeOutliers")
    g.close()
    m = pkg.Matcher(pkg.Params.default(), outlier_removal=True)
    m.setGain(True)
    for t in range(2):
        m.pushBack(fr[0][t][0], fr[0][t][1], dims)
    m.matchFeatures(QUAD)
    m.bucketFeatures(2, 50.0, 50.0)
    pm = m.getMatches()
    assert 10 < len(pm) < len(lists[0])
    gain, num = m.getGain(np.arange(len(pm)))
    want = pkg.gain([pm], [np.arange(len(pm))], fr[0][0][0], fr[0][1][0], dims)
    assert gain.tobytes() == want[0][0].tobytes() and num == want[1][0] > 10
    e = pkg.EgoParams.default(ransac_iters=50, inlier_threshold=2.5, **CAL)
    n = m.motionInliers(e, TR)
    gain, num = m.getGain()
    pos = m.getInlierMatches()[1]
    want = pkg.gain([pm], [pos], fr[0][0][0], fr[0][1][0], dims)
    assert n == len(pos) and gain.tobytes() == want[0][0].tobytes() and num == want[1][0]
    m.close()


@pytest.mark.gpu
def test_gpu_one_stream_replaced_on_the_host(pkg, ob, gpu):
    """The matcher form of removeOutliers on a group handle replaces stream 0's list alone: the classification, the gain over
    it and the gain over index lists read a staged copy in which stream 0 is the shorter host-side list and streams 1 and 2
    are still their device lists.  Each equals the stateless entry on the lists vh_group_get_matches_all returns, exactly."""
    fr, dims = frames_of(pkg), dims_of(pkg)
    g = pkg.StreamGroup(S, pkg.Params.default())
    g.setGain(True)
    e = pkg.EgoParams.default(ransac_iters=50, inlier_threshold=2.5, **CAL)
    push(g, fr, 0, dims)
    push(g, fr, 1, dims)
    Ip, Ic = lefts(fr, 0), lefts(fr, 1)
    g.matchFeatures(QUAD)
    device_lists = [g.getMatches(s) for s in range(S)]
    assert pkg._lib().vh_remove_outliers(g._h) == pkg.VH_OK
    rows, n_rows = g.getMatchesAll()
    lists = [rows[s, :n_rows[s]].copy() for s in range(S)]
    print("device", [len(pm) for pm in device_lists], "served", list(n_rows))
    # the premise: streams 1 and 2 still serve their device lists, stream 0 a shorter one (the test is void otherwise)
    assert 0 < len(lists[0]) < len(device_lists[0]) and len(lists[2]) > 0
    assert [lists[s].tobytes() for s in (1, 2)] == [device_lists[s].tobytes() for s in (1, 2)]
    tr, ok = np.array([TR] * S), np.ones(S, np.int32)
    counts = g.motionInliers(e, tr, ok)
    want_flags, want_n, want_pm, want_pos = pkg.motion_inliers(e, lists, tr, ok)
    print("inliers", counts, want_n)
    assert np.array_equal(counts, want_n) and counts[0] > 50 and counts[2] > 0
    for s in range(S):
        got_pm, got_pos = g.getInlierMatches(s)
        assert g.getInlierFlags(s).tobytes() == want_flags[s].tobytes(), s
        assert got_pm.tobytes() == want_pm[s].tobytes() and np.array_equal(got_pos, want_pos[s]), s
    same_as_stateless(pkg, g.gain(), lists, want_pos, Ip, Ic, dims, "inliers, stream 0 replaced")
    idx = [np.array([0, len(pm) - 1, len(pm) // 2, len(pm), -1, 0], np.int32) for pm in lists]   # a few positions per stream
    got = g.gain(idx)
    same_as_stateless(pkg, got, lists, idx, Ip, Ic, dims, "indices, stream 0 replaced")
    assert got[1][0] > 0 and got[1][1] == 0 and got[1][2] > 0
    same_as_stateless(pkg, g.gain(), lists, want_pos, Ip, Ic, dims, "inliers again: the classification's copy is its own")
    g.close()


@pytest.mark.gpu
def test_gpu_state_rules_and_failed_allocation(pkg, ob, gpu):
    fr, dims = frames_of(pkg), dims_of(pkg)
    state = pkg.VH_ERR_STATE
    e = pkg.EgoParams.default(ransac_iters=50, inlier_threshold=2.5, **CAL)
    g = pkg.StreamGroup(S, pkg.Params.default())
    push(g, fr, 0, dims)
    expect(pkg, state, lambda: g.setGain(True))                        # the switch after a push
    push(g, fr, 1, dims)
    g.matchFeatures(QUAD)
    g.motionInliers(e, np.array([TR] * S), np.ones(S, np.int32))
    expect(pkg, state, g.gain)                                         # the gain entries with the switch off
    expect(pkg, state, lambda: g.gain([[0]] * S))
    g.close()
    g = pkg.StreamGroup(S, pkg.Params.default())
    g.setGain(True)
    push(g, fr, 0, dims)
    expect(pkg, state, lambda: g.gain([[0]] * S))                      # before a match call
    push(g, fr, 1, dims)
    g.matchFeatures(QUAD)
    expect(pkg, state, g.gain)                                         # before a classification
    g.motionInliers(e, np.array([TR] * S), np.ones(S, np.int32))
    bytes0 = g.deviceBytes()
    g.debugFailNextAlloc()                                             # the first call's block: refused before any launch
    expect(pkg, pkg.VH_ERR_HIP, g.gain)
    g.synchronize()
    assert g.deviceBytes() == bytes0 and g.profileRead("gain_ratio")[1] == 0
    first = g.gain()
    assert first[1][0] > 100 and g.gain()[0].tobytes() == first[0].tobytes()
    g.matchFeatures(QUAD)
    expect(pkg, state, g.gain)                                         # after the next match: no classification of these lists
    g.motionInliers(e, np.array([TR] * S), np.ones(S, np.int32))
    assert g.gain()[0].tobytes() == first[0].tobytes()
    push(g, fr, 2, dims)
    expect(pkg, state, g.gain)                                         # after the next push
    expect(pkg, state, lambda: g.gain([[0]] * S))
    g.close()
    # the planes' allocation refused: the push releases what it made, and the next one succeeds
    n_alloc = {}   # allocations of a first push: the smallest skip at which it succeeds
    for on in (False, True):
        for skip in range(80):
            g = pkg.StreamGroup(S, pkg.Params.default())
            g.setGain(on)
            g.debugFailAllocAfter(skip)
            try:
                push(g, fr, 0, dims)
                n_alloc[on] = skip
            except pkg.VisoHipError as err:
                assert err.code == pkg.VH_ERR_HIP and g.deviceBytes() == 0, (on, skip)
                if on:                                                 # usable: the next push allocates everything
                    push(g, fr, 0, dims)
                    push(g, fr, 1, dims)
                    g.matchFeatures(QUAD)
                    g.motionInliers(e, np.array([TR] * S), np.ones(S, np.int32))
                    assert g.gain()[1][0] > 100
            g.close()
            if on in n_alloc:
                break
    assert n_alloc[True] == n_alloc[False] + 1, n_alloc


@pytest.mark.gpu
def test_gpu_off_state_is_untouched(pkg, ob, gpu):
    """Off (never switched, or switched off again): the same bytes, the same lists, no scope of the feature; on: the planes
    and nothing else until a gain entry is called."""
    fr, dims = frames_of(pkg), dims_of(pkg)
    seen = {}
    for name in ("never", "off", "on"):
        g = pkg.StreamGroup(S, pkg.Params.default())
        if name != "never":
            g.setGain(name == "on")
        g.profileEnable(True)
        for t in range(3):
            push(g, fr, t, dims)
            if t:
                g.matchFeatures(QUAD)
        g.synchronize()
        seen[name] = (g.deviceBytes(), [g.getMatches(s).tobytes() for s in range(S)], {k: g.profileRead(k)[1] for k in SCOPES})
        g.close()
    assert seen["never"] == seen["off"] and seen["never"][2] == {k: 0 for k in SCOPES}
    pitch = (W + 15) // 16 * 16
    assert seen["on"][0] - seen["never"][0] == RING * S * pitch * H
    assert seen["on"][1] == seen["never"][1]
    assert seen["on"][2]["gain_copy"] == 3 and seen["on"][2]["gain_ratio"] == 0 and seen["on"][2]["gain_sum"] == 0
