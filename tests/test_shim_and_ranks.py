"""Host-side integration: the C++ `Matcher` drop-in (include/viso_hip_matcher.hpp)
and the multi-rank launch path of bench.py."""
import json
import os
import shutil
import socket
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

PKG = os.path.join(ROOT, "hls-final-visual-odometry_amd")
LINK = ["-L" + PKG, "-lviso_hip", "-Wl,-rpath," + PKG, "-Wl,-rpath-link,/opt/rocm/lib"]


def build_shim_demo(tmp_path, pkg):
    exe = str(tmp_path / "shim_stereo_loop")
    subprocess.check_call(["g++", "-std=gnu++11", "-O1", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "shim_stereo_loop.cpp"), "-o", exe] + LINK)
    return exe


def test_shim_compiles_as_cxx11_and_links(tmp_path, pkg):
    """The reference is C++03/11 host code compiled with g++: the shim must be too."""
    assert os.path.exists(build_shim_demo(tmp_path, pkg))


def free_port():
    s = socket.socket(); s.bind(("127.0.0.1", 0)); p = s.getsockname()[1]; s.close()
    return p


def test_two_rank_launch_gloo(pkg):
    """N>1 path on CPU: launched exactly as the driver launches bench.py, 2 ranks, gloo.  --dist-selftest runs
    main()'s own multi-rank control flow (bench.RankProtocol: process group, gathered rank descriptions, fences,
    timed blocks with the MAX-reduced clock and the agreed block count, final barrier) around a stubbed step:
    rank r sleeps r + 1 ms per step, so rank 1 must set the clock."""
    env = dict(os.environ, MASTER_ADDR="127.0.0.1")
    out = subprocess.check_output(
        [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2",
         "--master-addr", "127.0.0.1", "--master-port", str(free_port()),
         os.path.join(ROOT, "bench.py"), "--gpus", "2", "--dist-selftest", "--streams", "3", "--steps", "7", "--warmup", "2",
         "--blocks", "0"],
        env=env, cwd=ROOT, stderr=subprocess.STDOUT, timeout=240).decode()
    lines = [ln for ln in out.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, out  # rank 0 only
    r = json.loads(lines[0])
    assert r["n_gpus"] == 2 and r["global_stream_ids"] == [0, 1, 2, 3, 4, 5]  # disjoint rank-major sharding
    assert r["distinct_data"] is True
    # both ranks described themselves through the process group
    assert sorted(x["rank"] for x in r["ranks_seen"]) == [0, 1] and len({x["uuid"] for x in r["ranks_seen"]}) == 2
    # the agreed number of blocks (>= 3), each at least as long as the SLOWEST rank's 7 steps of 2 ms
    assert r["blocks"]["count"] >= 3 and all(b >= 7 * 0.002 for b in r["blocks"]["seconds_each"])
    assert 2.0 <= r["ms_per_step"] < 100.0  # (rank 1 sleeps 2 ms per step; the upper bound only guards against a clock that stopped meaning anything)
    assert r["value"] == pytest.approx(2 * 3 * 7 / (r["ms_per_step"] * 7e-3))  # whole-job aggregate over the MAX-reduced clock


def test_bench_launches_itself_for_more_than_one_gpu():
    """`python3 bench.py --gpus 2 ...` from a clean environment (no RANK / WORLD_SIZE: not under a launcher) starts
    torch.distributed.run itself as a child process, relays exactly ONE JSON line -- rank 0's -- and returns the
    child's exit code."""
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--dist-selftest", "--streams", "3", "--steps", "4",
                        "--warmup", "1", "--blocks", "3"], env=env, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=240)
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    lines = r.stdout.decode().splitlines()
    assert len(lines) == 1 and lines[0].startswith("{"), r.stdout.decode()
    d = json.loads(lines[0])
    assert d["n_gpus"] == 2 and sorted(x["rank"] for x in d["ranks_seen"]) == [0, 1]
    assert d["global_stream_ids"] == [0, 1, 2, 3, 4, 5]
    # a failing child is reported through the exit code (here: an argument the ranks reject)
    bad = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--dist-selftest", "--steps", "x"],
                         env=env, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=240)
    assert bad.returncode != 0 and not bad.stdout.decode().strip()


def test_rank_protocol_single_process():
    """The same protocol object with one rank and no process group (what `python bench.py` uses at N = 1)."""
    sys.path.insert(0, ROOT)
    import bench
    proto = bench.RankProtocol("gloo", 0, 0, 1)
    assert proto.active is False and proto.gather({"rank": 0}) == [{"rank": 0}]
    calls = []
    blocks = proto.timed_blocks(lambda: calls.append(1), lambda: None, 5, 4)
    assert len(blocks) == 4 and len(calls) == 20
    proto.close()
    with pytest.raises(AssertionError):
        bench.check_ranks([{"rank": 0, "pci_bus_id": 1, "pci_device_id": 0, "uuid": "a"}, {"rank": 1, "pci_bus_id": 1, "pci_device_id": 0, "uuid": "a"}], 2)


@pytest.mark.gpu
@pytest.mark.parametrize("bucket", [0, 1])
def test_shim_stereo_loop_matches_oracle(bucket, tmp_path, pkg, ob, oracle, gpu):
    """The C++ drop-in, driven like VisualOdometryStereo::process drives the
    reference's Matcher, yields the oracle's quad matches frame after frame."""
    exe = build_shim_demo(tmp_path, pkg)
    W, H, nf = 640, 240, 4
    bpl = pkg.synth.bytes_per_line(W)
    seq = pkg.synth.stereo_sequence(W, H, nf, disparity=9, blur=5, seed=77)
    with open(tmp_path / "frames.bin", "wb") as f:
        for l, r in seq:
            f.write(l.tobytes()); f.write(r.tobytes())
    subprocess.check_call([exe, str(tmp_path / "frames.bin"), str(W), str(H), str(bpl), str(nf), str(bucket),
                           str(tmp_path / "out.bin")], timeout=120)
    raw = open(tmp_path / "out.bin", "rb").read()
    po = ob.Params.default()
    dims = [W, H, bpl]
    F = [[oracle.compute_features(po, im, dims)[1] for im in pair] for pair in seq]
    pos = 0
    for t in range(nf):
        n = int(np.frombuffer(raw, np.int32, 1, pos)[0]); pos += 4
        got = np.frombuffer(raw, pkg.P_MATCH_DTYPE, n, pos); pos += 48 * n
        if t == 0:
            assert n == 0  # no previous pair yet
            continue
        want = oracle.matching(po, dims, 2, F[t - 1][0], F[t - 1][1], F[t][0], F[t][1])
        want, _ = oracle.remove_outliers(want)  # the shim's matchFeatures ends with it (src/matcher.cpp:108)
        if bucket:
            want = oracle.bucket_features(want, 2, 50, 50)
        assert n == len(want) and n > 50 and got.tobytes() == want.tobytes()
    assert pos == len(raw)


@pytest.mark.gpu
def test_shim_mono_loop_matches_oracle(tmp_path, pkg, ob, oracle, gpu):
    """VisualOdometryMono::process pattern (src/viso_mono.cpp:33-39): the mono
    pushBack overload, flow matching, removeOutliers, bucketing."""
    exe = build_shim_demo(tmp_path, pkg)
    W, H, nf = 480, 200, 4
    bpl = pkg.synth.bytes_per_line(W)
    seq = pkg.synth.stereo_sequence(W, H, nf, disparity=9, blur=5, seed=78)
    with open(tmp_path / "frames.bin", "wb") as f:
        for l, r in seq:
            f.write(l.tobytes()); f.write(r.tobytes())
    subprocess.check_call([exe, str(tmp_path / "frames.bin"), str(W), str(H), str(bpl), str(nf), "1",
                           str(tmp_path / "out.bin"), "1"], timeout=120)
    raw = open(tmp_path / "out.bin", "rb").read()
    po = ob.Params.default()
    dims = [W, H, bpl]
    F = [oracle.compute_features(po, pair[0], dims)[1] for pair in seq]
    pos = 0
    for t in range(nf):
        n = int(np.frombuffer(raw, np.int32, 1, pos)[0]); pos += 4
        got = np.frombuffer(raw, pkg.P_MATCH_DTYPE, n, pos); pos += 48 * n
        if t == 0:
            assert n == 0
            continue
        want, _ = oracle.remove_outliers(oracle.matching(po, dims, 0, m1p=F[t - 1], m1c=F[t]))
        want = oracle.bucket_features(want, 2, 50, 50)
        assert n == len(want) and n > 20 and got.tobytes() == want.tobytes()
    assert pos == len(raw)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["small_default", "small_multi", "small_half", "small_multi_half_n3"])
def test_shim_compute_features_member(name, tmp_path, pkg, ob, oracle, gpu):
    """Matcher::computeFeatures of the drop-in header (src/matcher.h:209), called as oracle/ref_harness.cpp calls the
    reference's -- references to null pointers in, _mm_malloc blocks out -- against the reference-generated fixtures:
    sparse and dense records bit for bit, the Sobel planes on their valid interior (fixture hashes at matching
    resolution; the oracle's filters for the full-resolution planes that half_resolution adds)."""
    from conftest import load_golden
    exe = str(tmp_path / "shim_compute_features")
    subprocess.check_call(["g++", "-std=gnu++11", "-O1", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "shim_compute_features.cpp"), "-o", exe] + LINK)
    p, dims, Ip, Ic, z = load_golden(name, pkg, pkg.Params)
    W, H, bpl = dims
    Ic.tofile(tmp_path / "img.bin")
    subprocess.check_call([exe, str(tmp_path / "img.bin"), str(W), str(H), str(bpl), str(p.nms_n), str(p.nms_tau), str(p.multi_stage),
                           str(p.half_resolution), str(tmp_path / "out.bin")], timeout=120)
    raw = open(tmp_path / "out.bin", "rb").read()
    pos = 0

    def take(dtype, n):
        nonlocal pos
        a = np.frombuffer(raw, dtype, n, pos)
        pos += a.nbytes
        return a

    n1 = int(take(np.int32, 1)[0]); m1 = take(np.int32, 12 * n1).reshape(n1, 12)
    n2 = int(take(np.int32, 1)[0]); m2 = take(np.int32, 12 * n2).reshape(n2, 12)
    dm = take(np.int32, 3)
    du = take(np.uint8, int(dm[2]) * int(dm[1])).reshape(dm[1], dm[2]); dv = take(np.uint8, int(dm[2]) * int(dm[1])).reshape(dm[1], dm[2])
    has_full = int(take(np.int32, 1)[0])
    assert np.array_equal(m2, z["max2c"]) and np.array_equal(m1, z["max1c"]) and n2 > 100
    assert (n1 > 0) == bool(p.multi_stage) and has_full == int(bool(p.half_resolution))
    assert oracle.fnv(np.ascontiguousarray(du[2:-2, 2:du.shape[1] - 16])) == int(z["du_interior_fnv"])
    assert oracle.fnv(np.ascontiguousarray(dv[2:-2, 2:dv.shape[1] - 16])) == int(z["dv_interior_fnv"])
    if has_full:
        duf = take(np.uint8, bpl * H).reshape(H, bpl); dvf = take(np.uint8, bpl * H).reshape(H, bpl)
        odu, odv, _, _ = oracle.filters(Ic)
        assert np.array_equal(duf[2:-2, 2:W - 2], odu[2:-2, 2:W - 2]) and np.array_equal(dvf[2:-2, 2:W - 2], odv[2:-2, 2:W - 2])
    assert pos == len(raw)
