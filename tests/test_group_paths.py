"""Stream groups on the two paths the benchmarked shapes take and small groups do not:

* detection in SUB-BATCHES of streams (engine.hip: push_device_queued).  A group of S streams is detected in
  ceil(S / ceil(S / nsub)) launches, nsub = VH_SUBBATCH or, by default, min(4, detection workgroups / 12 000
  (stereo) or 40 000 (mono)); every launch after the first reads its images, records, chunk counters, half-resolution
  images and feature sets at offsets of its first stream.  The group cases below are exact parity tests in a plain
  run (one launch per push) and cover those offsets when VH_SUBBATCH is set (test_child_subbatch runs them so); each
  case checks from the profile that the push took the number of launches the rule gives.
* search waves that walk SEVERAL query tiles (kernels_match.hip: flow_pass / rows_pass, `tile += gridDim.x * 4`): forced
  with VH_FLOW_WGS=1 (test_child_flow_wgs), and reached as real video reaches it -- a grid sized by the statistics of
  a sparse step, then a dense one (test_tile_hint_sparse_to_dense).
* the benchmark's own outputs (bench.py --dump-outputs) at the benchmarked shapes, every stream's counts and a sample
  of streams' records against the oracle (test_bench_outputs_match_the_oracle).

Integer/byte work: the bar is exact equality everywhere."""
import os
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
TILE_Q = 32      # vh_dev.h: VH_TILE_Q, queries per search tile
MARGIN = 7       # vh_dev.h: VH_MARGIN
THREADS = 16     # oracle worker threads (its calls release the GIL)
EMPTY = np.zeros((0, 12), np.int32)


def env_int(name):
    v = os.environ.get(name, "")
    return int(v) if v.strip() else 0


def block_count(extent, n):
    """engine.hip: Group::block_count."""
    lo, hi = n + MARGIN, extent - n - MARGIN
    return (hi - lo + n) // (n + 1) if hi > lo else 0


def detect_launches(S, ncam, W, H, nms_n, half):
    """detect_nms launches one push of an S-stream group makes (engine.hip: push_device_queued)."""
    sub = env_int("VH_SUBBATCH")
    if sub <= 0:
        ser = os.environ.get("VH_SERIAL")
        serial = ser[:1] == "1" if ser is not None else S <= 2
        Wm, Hm = (W // 2, H // 2) if half else (W, H)
        nbx, nby = block_count(Wm, nms_n), block_count(Hm, nms_n)
        nblocks = nbx * nby if nbx and nby else 0
        det_wgs = S * ncam * ((nblocks + 255) // 256)
        sub = 1 if serial else min(4, det_wgs // (12000 if ncam == 2 else 40000))
    nsub = max(1, min(sub, S))
    ssub = -(-S // nsub)
    return -(-S // ssub)


def tiles(f):
    """Query tiles of a feature set (kernels_bin.hip: make_tiles; rows_pass counts the same per class)."""
    return int(sum(-(-int((f[:, 3] == c).sum()) // TILE_Q) for c in range(4)))


QUERY_SETS = {0: (2, 0), 1: (2, 3), 2: (0, 1, 3, 2)}  # engine_match.hip match_args: the query set of every pass


def pmap(fn, items):
    with ThreadPoolExecutor(THREADS) as ex:
        return list(ex.map(fn, items))


class Frames:
    """Per-stream image sequences and their oracle features, computed once per image on a thread pool."""

    def __init__(self, oracle, po, dims, seqs):
        self.seqs, self.dims = seqs, dims  # seqs[s][t] = (left, right or None)
        keys = [(s, t, c) for s in range(len(seqs)) for t in range(len(seqs[s])) for c in range(2)]
        feats = pmap(lambda k: EMPTY if seqs[k[0]][k[1]][k[2]] is None
                     else oracle.compute_features(po, seqs[k[0]][k[1]][k[2]], dims)[1], keys)
        self.F = dict(zip(keys, feats))

    def stack(self, t, c):
        if self.seqs[0][t][c] is None:
            return None
        return np.stack([self.seqs[s][t][c] for s in range(len(self.seqs))])

    def quad(self, s, tp, tc):
        return [self.F[(s, tp, 0)], self.F[(s, tp, 1)], self.F[(s, tc, 0)], self.F[(s, tc, 1)]]


def check_group(pkg, oracle, po, g, fr, tp, tc, method):
    """Every stream's four feature sets and (if method is not None) its match list equal the oracle's.
    tp is None after the first push of a sequence (the previous sets are empty).  -> max query tiles of a pass."""
    S = g.S
    sets = [fr.quad(s, tp, tc) if tp is not None else [EMPTY, EMPTY, fr.F[(s, tc, 0)], fr.F[(s, tc, 1)]]
            for s in range(S)]
    wants = pmap(lambda s: oracle.matching(po, fr.dims, method, *sets[s]), range(S)) if method is not None else None
    nf, nm = g.getCounts()
    for s in range(S):
        assert list(nf[s]) == [len(x) for x in sets[s]], (s, tp, tc)
        for k in range(4):
            assert np.array_equal(g.getFeatures(s, k), sets[s][k]), (s, tp, tc, k)
        if method is not None:
            assert nm[s] == len(wants[s]) and g.getMatches(s).tobytes() == wants[s].tobytes(), (s, tp, tc, method)
    if method is None:
        return 0, 0
    return max(tiles(sets[s][q]) for s in range(S) for q in QUERY_SETS[method]), sum(len(w) for w in wants)


def check_launches(g, pushes, per_push, half):
    _, n = g.profileRead("detect_nms")
    assert n == pushes * per_push, (n, pushes, per_push, os.environ.get("VH_SUBBATCH"))
    _, nh = g.profileRead("half_res")
    assert nh == (pushes * per_push if half else 0), (nh, pushes, per_push)


def check_waves_loop(max_tiles):
    """Under VH_FLOW_WGS=w every (pass, stream) has 4w waves: the sets must hold more tiles than that, so that a wave
    walks two tiles or more (otherwise the forced run proves nothing)."""
    wgs = env_int("VH_FLOW_WGS")
    if wgs > 0:
        assert max_tiles > 4 * wgs, (max_tiles, wgs)


# ------------------------------------------------------------------ A: group cases
# id: (S, W, H, stride, stereo, nms_n, half_resolution, methods of steps 1..)
#   stride "odd" = the image width (odd: rows not 4-byte aligned, the generic detector); None = bytes_per_line(W)
GROUP_CASES = {
    "S5_quad_stereo_n1": (5, 320, 160, None, True, 1, 0, [2, 1, 2]),
    "S7_quad_n2_half": (7, 480, 240, None, True, 2, 1, [2, 1]),
    "S5_stereo_n3_half": (5, 400, 220, None, True, 3, 1, [1, 2]),
    "S7_quad_n4": (7, 360, 170, None, True, 4, 0, [2, 2]),
    "S5_mono_flow_n2": (5, 360, 180, None, False, 2, 0, [0, 0]),
    "S7_mono_flow_n3_half": (7, 520, 260, None, False, 3, 1, [0, 0]),
    "S5_mono_flow_n4_half": (5, 480, 240, None, False, 4, 1, [0]),
    "S7_quad_n5_odd_stride": (7, 331, 150, "odd", True, 5, 0, [2, 1]),
    "S5_mono_flow_n5_odd_stride_half": (5, 423, 221, "odd", False, 5, 1, [0, 0]),
}


def group_frames(pkg, S, W, H, stride, stereo, T, seed):
    seqs = []
    for s in range(S):
        sq = pkg.synth.stereo_sequence(W, H, T, disparity=4 + s, blur=3 + s % 3, seed=seed + s)
        if stride == "odd":
            sq = [(l[:, :W].copy(), r[:, :W].copy()) for l, r in sq]
        seqs.append([(l, r if stereo else None) for l, r in sq])
    bpl = W if stride == "odd" else pkg.synth.bytes_per_line(W)
    return seqs, [W, H, bpl]


@pytest.mark.parametrize("case", sorted(GROUP_CASES))
def test_subbatch_group(case, pkg, ob, oracle, gpu):
    """pushBack from the host, every stream's sets and matches after every step; the launches per push."""
    S, W, H, stride, stereo, n, half, methods = GROUP_CASES[case]
    T = len(methods) + 1
    over = {"nms_n": n, "half_resolution": half}
    p, po = pkg.Params.default(**over), ob.Params.default(**over)
    seqs, dims = group_frames(pkg, S, W, H, stride, stereo, T, 300 + 10 * S + n)
    fr = Frames(oracle, po, dims, seqs)
    per_push = detect_launches(S, 2 if stereo else 1, W, H, n, half)
    g = pkg.StreamGroup(S, p)
    g.profileEnable()
    max_tiles = 0
    for t in range(T):
        g.pushBack(fr.stack(t, 0), fr.stack(t, 1), dims, False)
        if t == 0:
            check_group(pkg, oracle, po, g, fr, None, 0, None)
        else:
            g.matchFeatures(methods[t - 1])
            mt, nmatch = check_group(pkg, oracle, po, g, fr, t - 1, t, methods[t - 1])
            assert nmatch > 20 * S, (case, t, nmatch)
            max_tiles = max(max_tiles, mt)
        check_launches(g, t + 1, per_push, half)
    check_waves_loop(max_tiles)
    g.close()


def test_subbatch_pipelined(pkg, ob, oracle, gpu):
    """Steps queued without a host sync (test_gpu_parity.py: test_pipelined_steps_without_host_sync) on a group
    of 7 streams, ending with a replace=True, read back only at the end."""
    S, W, H, T = 7, 320, 160, 6
    po = ob.Params.default()
    seqs, dims = group_frames(pkg, S, W, H, None, True, T, 700)
    fr = Frames(oracle, po, dims, seqs)
    per_push = detect_launches(S, 2, W, H, po.nms_n, 0)
    g = pkg.StreamGroup(S, pkg.Params.default())
    g.profileEnable()
    methods = [2, 2, 0, 2, 1]
    for t in range(T):
        g.pushBack(fr.stack(t, 0), fr.stack(t, 1), dims, False)
        if t:
            g.matchFeatures(methods[t - 1])
    g.pushBack(fr.stack(2, 0), fr.stack(2, 1), dims, True)  # the newest pair replaced by an older one
    g.matchFeatures(2)
    for s in range(S):
        f = [fr.F[(s, T - 2, 0)], fr.F[(s, T - 2, 1)], fr.F[(s, 2, 0)], fr.F[(s, 2, 1)]]
        for k in range(4):
            assert np.array_equal(g.getFeatures(s, k), f[k]), (s, k)
        want = oracle.matching(po, dims, 2, *f)
        assert len(want) > 50 and g.getMatches(s).tobytes() == want.tobytes(), s
    check_launches(g, T + 1, per_push, False)
    g.close()


def test_subbatch_device_buffer(gpu):
    """pushBackDevice from a torch buffer whose stream stride exceeds H * bpl: tests/group_device_case.py, a process of
    its own (torch must load its HIP runtime before the product library, as in bench.py)."""
    r = subprocess.run([sys.executable, os.path.join(HERE, "group_device_case.py")], capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0 and "group-device ok" in r.stdout, r.stdout[-2000:] + r.stderr[-3000:]


# ------------------------------------------------------------------ B2: a grid sized by a sparse step
def sparse_frame(img, W, H):
    """A nearly flat frame: one 48 x 40 textured patch in a constant field."""
    out = np.zeros_like(img)
    out[:, :W] = 128
    out[60:100, 100:148] = img[60:100, 100:148]
    return out


@pytest.mark.parametrize("method", [2, 0, 1], ids=["quad", "flow", "stereo"])
def test_tile_hint_sparse_to_dense(method, pkg, ob, oracle, gpu):
    """engine_match.hip: match_queued sizes the searches' grid of a non-serial group (S >= 3, nms_n <= 4) from the tiles an
    earlier launch saw (tiles_hint).  After a read-back of a step on nearly flat frames, a step on densely textured
    frames holds many times the tiles of that grid: every wave walks several tiles.  Then back to sparse frames."""
    S, W, H = 4, 640, 240
    stereo = method != 0
    p, po = pkg.Params.default(), ob.Params.default()
    dims = [W, H, pkg.synth.bytes_per_line(W)]
    seqs = []
    for s in range(S):
        dense = pkg.synth.stereo_sequence(W, H, 2, disparity=5 + s, blur=2, gain=3, seed=800 + s)
        calm = pkg.synth.stereo_sequence(W, H, 4, disparity=5 + s, blur=3, seed=850 + s)
        seq = [tuple(sparse_frame(x, W, H) for x in calm[0]), tuple(sparse_frame(x, W, H) for x in calm[1])] + dense \
            + [tuple(sparse_frame(x, W, H) for x in calm[2]), tuple(sparse_frame(x, W, H) for x in calm[3])]
        seqs.append([(l, r if stereo else None) for l, r in seq])
    fr = Frames(oracle, po, dims, seqs)
    npass = 4 if method == 2 else 2
    g = pkg.StreamGroup(S, p)

    def hint(tp, tc):  # engine_match.hip: choose_loop -- tiles_hint from the fullest stream's query sets
        nq = max(sum(len(fr.quad(s, tp, tc)[q]) for q in QUERY_SETS[method]) for s in range(S))
        return nq // npass // TILE_Q + 4

    g.pushBack(fr.stack(0, 0), fr.stack(0, 1), dims, False)
    g.pushBack(fr.stack(1, 0), fr.stack(1, 1), dims, False)
    g.matchFeatures(method)
    check_group(pkg, oracle, po, g, fr, 0, 1, method)  # read back: the sparse step's statistics are in
    sparse_hint = hint(0, 1)
    g.pushBack(fr.stack(2, 0), fr.stack(2, 1), dims, False)
    g.pushBack(fr.stack(3, 0), fr.stack(3, 1), dims, False)
    g.matchFeatures(method)
    dense_tiles, nmatch = check_group(pkg, oracle, po, g, fr, 2, 3, method)
    gx = ((sparse_hint + 3) // 4) | 1  # vh_launch_match: workgroups per (pass, stream) row, 4 waves each
    assert dense_tiles >= 8 * sparse_hint and dense_tiles > 8 * gx, (dense_tiles, sparse_hint, gx)
    assert nmatch > 1000 * S
    for t in (4, 5):  # and back to sparse frames
        g.pushBack(fr.stack(t, 0), fr.stack(t, 1), dims, False)
        g.matchFeatures(method)
        check_group(pkg, oracle, po, g, fr, t - 1, t, method)
    g.close()


# ------------------------------------------------------------------ the same cases with the paths forced
A_SEL = "subbatch_group or subbatch_pipelined or subbatch_device or tile_hint"
GROUP_SEL = "stream_group or pipelined or group_get_matches_all or group_async or push_back_device"
SEARCH_SEL = "golden or random_configs or tie_break or ring_buffer or kitti or query_tiles"
NOT_SELF = "not child and not bench_outputs"
PARITY = os.path.join(HERE, "test_gpu_parity.py")


def run_child(env_over, files, sel, timeout=900):
    env = dict(os.environ, **env_over)
    r = subprocess.run([sys.executable, "-m", "pytest", *files, "-q", "-x", "-m", "gpu", "-k", f"({sel}) and {NOT_SELF}"],
                       env=env, capture_output=True, text=True, timeout=timeout, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert " passed" in r.stdout and " skipped" not in r.stdout, r.stdout[-2000:]
    return r


@pytest.mark.parametrize("n", ["3", "4"])
def test_child_subbatch(n, gpu):
    """VH_SUBBATCH=n (read once per process): the group cases above in sub-batches (S = 5 in 2 + 2 + 1 streams, S = 7 in
    3 + 3 + 1 or 2 + 2 + 2 + 1; every case asserts its launch count), and with n = 3 the group tests of test_gpu_parity.py."""
    files = [os.path.abspath(__file__)] + ([PARITY] if n == "3" else [])
    run_child({"VH_SUBBATCH": n}, files, A_SEL + (" or " + GROUP_SEL if n == "3" else ""))


@pytest.mark.parametrize("tested", ["adaptive", "tested"])
def test_child_flow_wgs(tested, gpu):
    """VH_FLOW_WGS=1: one workgroup per (pass, stream), so every search wave walks many tiles one after the other (the
    group cases assert that their sets hold more than 4 tiles per pass), with the adaptive and with the tested loops."""
    env = {"VH_FLOW_WGS": "1"}
    if tested == "tested":
        env["VH_FLOW_TESTED"] = "1"
    run_child(env, [os.path.abspath(__file__), PARITY], A_SEL + " or " + SEARCH_SEL)


def test_child_checking_build(pkg, gpu):
    """Sub-batches and multi-tile waves together on libviso_hip_check.so (-DVH_CHECK: every index the kernels use
    unclamped verified on the device): no violation."""
    assert os.path.exists(pkg.CHECK_LIB_PATH), "build() makes it"
    r = run_child({"VISO_HIP_LIB": pkg.CHECK_LIB_PATH, "VH_SUBBATCH": "3", "VH_FLOW_WGS": "1"},
                  [os.path.abspath(__file__), PARITY], " or ".join((A_SEL, GROUP_SEL, SEARCH_SEL)), timeout=1500)
    assert "VH_CHECK" not in r.stderr


# ------------------------------------------------------------------ C: the benchmark's outputs
@pytest.mark.parametrize("workload,nsub", [("kitti", 4), ("1080p", 4), ("4k", 3)])
def test_bench_outputs_match_the_oracle(workload, nsub, tmp_path, pkg, ob, oracle, gpu):
    """bench.py --dump-outputs at the workload's own stream count: every stream's feature and match counts, and the
    sampled streams' records (converted as dump_outputs converts them), equal the oracle's on the inputs the bench
    made (bench.make_frames: a function of the arguments alone).  The groups are detected in sub-batches; a group of
    the same shape confirms the launch count and checks the last stream of every sub-batch record for record."""
    import bench
    wl = bench.WORKLOADS[workload]
    S, W, H = wl["streams"], wl["W"], wl["H"]
    steps, warmup, T = 2, 2, 2
    out = tmp_path / "dump"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--workload", workload, "--steps",
                        str(steps), "--warmup", str(warmup), "--frames", str(T), "--dump-outputs", str(out)],
                       cwd=tmp_path, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-3000:]
    d = {f[:-4]: np.load(out / f) for f in os.listdir(out)}
    k = warmup + steps - 1
    tc, tp = k % T, (k - 1) % T
    over = wl["params"]
    p, po = pkg.Params.default(**over), ob.Params.default(**over)
    frames, bpl = bench.make_frames(pkg, S, T, 0, size=(W, H))
    dims = [W, H, bpl]
    # oracle features once per distinct image: stream s shows frame t of sequence `seed` at time t + phase
    assign = bench.stream_assignment(0, S)
    key = lambda s, t: (assign[s][1], t + assign[s][2])
    first = {}
    for s in range(S):
        for t in (tp, tc):
            first.setdefault(key(s, t), (s, t))
    imgs = sorted(first.items())
    feats = pmap(lambda kv: [oracle.compute_features(po, frames[kv[1][1], c, kv[1][0]], dims)[1] for c in (0, 1)], imgs)
    F = {kk: f for (kk, _), f in zip(imgs, feats)}
    sets = [F[key(s, tp)] + F[key(s, tc)] for s in range(S)]
    want = pmap(lambda s: oracle.matching(po, dims, 2, *sets[s]), range(S))

    nf_want = np.array([[len(x) for x in f] for f in sets], np.float64)
    nm_want = np.array([len(w) for w in want], np.float64)
    assert np.array_equal(d["feature_counts"], nf_want), np.flatnonzero((d["feature_counts"] != nf_want).any(axis=1))
    assert np.array_equal(d["match_counts"], nm_want), np.flatnonzero(d["match_counts"] != nm_want)
    assert min(len(w) for w in want) > 100
    sample = d["sample_streams"].astype(int)
    assert len(sample) >= 1
    conv = lambda m: np.stack([m[f].astype(np.float32) for f in m.dtype.names], axis=1).reshape(-1, 12)
    assert np.array_equal(d["matches"], np.concatenate([conv(want[s]) for s in sample]))
    assert np.array_equal(d["features_left"], np.concatenate([sets[s][2] for s in sample]).astype(np.float64))
    assert np.array_equal(d["features_right"], np.concatenate([sets[s][3] for s in sample]).astype(np.float64))

    # the launches of one push at this shape, and the last stream of every sub-batch
    per_push = detect_launches(S, 2, W, H, p.nms_n, p.half_resolution)
    if not os.environ.get("VH_SUBBATCH"):
        assert per_push == nsub, (workload, per_push)
    ssub = -(-S // per_push)
    g = pkg.StreamGroup(S, p, max_features=wl["cap"], max_matches=wl["cap"])
    g.profileEnable()
    g.pushBack(frames[tp, 0], frames[tp, 1], dims, False)
    g.pushBack(frames[tc, 0], frames[tc, 1], dims, False)
    g.matchFeatures(pkg.METHOD_QUAD)
    check_launches(g, 2, per_push, False)
    lasts = sorted({min(S, (b + 1) * ssub) - 1 for b in range(per_push)})
    nf, nm = g.getCounts()
    assert np.array_equal(nf.astype(np.float64), d["feature_counts"]) and np.array_equal(nm.astype(np.float64), d["match_counts"])
    for s in lasts:
        for kk in range(4):
            assert np.array_equal(g.getFeatures(s, kk), sets[s][kk]), (s, kk)
        assert g.getMatches(s).tobytes() == want[s].tobytes(), s
    g.close()
    # coverage: records checked in every sub-batch, by the dump's sample (more than one sub-batch where its budget
    # holds more than one sub-batch's streams) and by the group above
    assert len(set(sample // ssub) | set(np.array(lasts) // ssub)) == per_push
    if sample.max() >= ssub:
        assert len(set(sample // ssub)) > 1
