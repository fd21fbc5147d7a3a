#!/usr/bin/env python3
"""What the landmarks cost on a sequence handle: one KITTI-size (1241 x 376) stereo sequence
resident in HBM, pushed in chunks of 256 frames, quad-matched with track linking on.  Per chunk: the dense lists are
classified under the estimated motion, the scene points of the inliers are asked for in the world frame (one Tw per row:
the accumulated pose), and vh_group_landmarks walks the chunk's track chains.  Prints one JSON line per chunk -- the device
time of the "landmarks" scope with each launch's share (index, link, chain, count, scan, store; the memset is the rest),
track_rank's device time of the same chunk (the same chains with a lighter hop: the yardstick of the walk), the bytes the
call moves by the count below and a device-to-device hipMemcpyAsync of as many bytes timed in the same session -- then the
pairs/s of the loop push .. landmarks with landmarks on and off in alternating runs, and a summary line.
  bytes = 8 per record slot (the memset of the observation index and the links)
        + 36 per point (index) + 28 per record of the rows >= 1 (link: the record read, the link written where linked)
        + 80 per record (chain: track 24, link and index 8, state written 48) + 16 per point + 48 per carried state
        + 4 per record (count) + 128 per landmark (store)
  python tools/sequence_landmark_rate.py [--frames 256] [--chunks 6] [--warmup 1] [--rate-runs 2]"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402  (loads its HIP runtime before the product library, as bench.py does)
import __graft_entry__ as entry  # noqa: E402
import bench  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--frames", type=int, default=256)
ap.add_argument("--chunks", type=int, default=6)
ap.add_argument("--warmup", type=int, default=1)
ap.add_argument("--rate-runs", type=int, default=2)
args = ap.parse_args()
S = args.frames

pkg = entry.load_package()
ob = entry.load_oracle()
wl = bench.WORKLOADS["kitti"]
W, H, cap = wl["W"], wl["H"], wl["cap"]
params = pkg.Params.default(**wl["params"])
bpl = pkg.synth.bytes_per_line(W)
dims, isz = [W, H, bpl], H * bpl
dev = torch.device("cuda", 0)
HIP = C.CDLL("libamdhip64.so")  # the runtime already in the process

P = 20  # stereo_sequence's pan repeats every 20 frames: frame t of the sequence is frame t % P
base = pkg.synth.stereo_sequence(W, H, P, disparity=12)
uniq = torch.from_numpy(np.stack([np.stack(pr) for pr in base])).to(dev)
N = S * (args.warmup + args.chunks)
frames = uniq[torch.arange(N, device=dev) % P].contiguous()
left, right = frames[:, 0].contiguous(), frames[:, 1].contiguous()
torch.cuda.synchronize()

e = pkg.EgoParams.default(f=721.5, cu=609.6, cv=172.9, base=0.54)
r = ob.glibc_rand_after_srand0(3 * e.ransac_iters).reshape(e.ransac_iters, 3)
rand3 = np.stack([r] * S)
lp = pkg.LandmarkParams.default(min_obs=2, max_missed=3, max_dist=0.5, gate_sigma=3.0)
STAGES = ("landmark_index", "landmark_link", "landmark_chain", "landmark_count", "landmark_scan", "landmark_store")


def motion_matrix(tr):
    """tr[6] (rx, ry, rz, tx, ty, tz) -> the 4x4 the estimator means by it"""
    rx, ry, rz = tr[:3]
    sx, cx, sy, cy, sz, cz = np.sin(rx), np.cos(rx), np.sin(ry), np.cos(ry), np.sin(rz), np.cos(rz)
    T = np.eye(4)
    T[:3, :3] = [[cy * cz, -cy * sz, sy],
                 [sx * sy * cz + cx * sz, -sx * sy * sz + cx * cz, -sx * cy],
                 [-cx * sy * cz + sx * sz, cx * sy * sz + sx * cz, cx * cy]]
    T[:3, 3] = tr[3:]
    return T


def copy_ms(nbytes, reps=5):
    """A device-to-device copy of nbytes on the current stream: the median of `reps` event-timed copies after one untimed."""
    a = torch.zeros(nbytes, dtype=torch.uint8, device=dev); b = torch.empty_like(a)
    st = torch.cuda.current_stream().cuda_stream

    def copy():
        assert HIP.hipMemcpyAsync(C.c_void_p(b.data_ptr()), C.c_void_p(a.data_ptr()), C.c_size_t(nbytes), 3, C.c_void_p(st)) == 0
    copy()
    ms = []
    for _ in range(reps):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record(); copy(); t1.record(); t1.synchronize()
        ms.append(t0.elapsed_time(t1))
    return float(np.median(ms))


def handle(landmarks_on, profile):
    g = pkg.SequenceGroup(S, params, max_features=cap, max_matches=cap)
    g.setTrackLinking(True)
    if landmarks_on:
        g.setLandmarks(True)
    g.setStream(torch.cuda.current_stream().cuda_stream)
    g.profileEnable(profile)
    return g


def chunk(g, c, pose, landmarks_on):
    """push .. scene points (.. landmarks) of chunk c -> (points per row, landmarks per row or None); pose: the camera of the
    last frame -> world, carried from chunk to chunk"""
    F = c * S
    g.pushBackDevice(left[F].data_ptr(), right[F].data_ptr(), isz, dims, S)
    g.matchFeatures(pkg.METHOD_QUAD)
    tr, ok, _ = g.estimateMotion(e, rand3)
    g.motionInliers(e, tr, ok.astype(np.int32))
    Tw = np.zeros((S, 4, 4))
    for s in range(S):
        if ok[s]:
            pose = pose @ np.linalg.inv(motion_matrix(tr[s]))
        Tw[s] = pose
    n_pts = g.scenePoints(e, None, Tw)
    return pose, n_pts, (g.landmarks(lp) if landmarks_on else None)


# ---- the device time of the call, launch by launch
g = handle(True, True)
pose, rows, last_row = np.eye(4), [], 0
for c in range(args.warmup + args.chunks):
    g.synchronize()
    g.profileReset()
    w0 = time.perf_counter()
    pose, n_pts, n_lm = chunk(g, c, pose, True)
    g.synchronize()
    if c < args.warmup:
        last_row = int(g.getTracksAll()[1][S - 1])
        continue
    ms = g.profileRead("landmarks")[0]
    shares = {k: round(g.profileRead(k)[0], 4) for k in STAGES}
    rank_ms = g.profileRead("track_rank")[0]
    trk, counts = g.getTracksAll()
    _, stride = g.landmarksDevice()
    records = int(counts.sum())
    linked = int(sum((trk[s, :counts[s]]["prev"] >= 0).sum() for s in range(S)))
    # (the carry is read where prev lies inside the previous chunk's last row, and only once a call on that chunk has left states)
    p0 = trk[0, :counts[0]]["prev"]
    carried = int(((p0 >= 0) & (p0 < last_row)).sum()) if c > 0 else 0
    last_row = int(counts[S - 1])
    points, lms = int(n_pts.sum()), int(n_lm.sum())
    nbytes = 8 * S * stride + 36 * points + 28 * (records - int(counts[0])) + 80 * records + 16 * points + 48 * carried + 4 * records + 128 * lms
    row = {"chunk": c, "records": records, "linked": linked, "points": points, "landmarks": lms, "landmarks_ms": round(ms, 4)}
    row.update(shares)
    row.update({"memset_and_gaps_ms": round(ms - sum(shares.values()), 4), "track_rank_ms": round(rank_ms, 4), "bytes": nbytes,
                "copy_ms": round(copy_ms(max(nbytes, 1)), 4)})
    rows.append(row)
    print(json.dumps(row), flush=True)
deep = max(int(g.getLandmarks(s)["n_obs"].max(initial=0)) for s in range(S))
g.close()

# ---- pairs/s of the whole loop, landmarks on and off in alternating runs (profiling off)
rates = {True: [], False: []}
for run in range(2 * args.rate_runs):
    on = run % 2 == 0
    g = handle(on, False)
    pose = np.eye(4)
    for c in range(args.warmup + args.chunks):
        if c == args.warmup:
            g.synchronize(); t0 = time.perf_counter()
        pose, _, _ = chunk(g, c, pose, on)
    g.synchronize()
    rates[on].append(args.chunks * S / (time.perf_counter() - t0))
    g.close()
    print(json.dumps({"run": run, "landmarks": on, "pairs_per_s": round(rates[on][-1], 1)}), flush=True)

med = lambda f: round(float(np.median([f(x) for x in rows])), 6)  # noqa: E731
out = {"metric": "sequence_landmarks_device_time", "frames_per_chunk": S, "W": W, "H": H, "chunks": len(rows), "deepest_n_obs_last_chunk": deep}
out.update({k: med(lambda x, k=k: x[k]) for k in rows[0] if k != "chunk"})
out["landmarks_over_copy"] = round(out["landmarks_ms"] / out["copy_ms"], 3) if out["copy_ms"] else None
out["chain_over_track_rank"] = round(out["landmark_chain"] / out["track_rank_ms"], 3) if out["track_rank_ms"] else None
out["pairs_per_s_on"] = round(float(np.median(rates[True])), 1)
out["pairs_per_s_off"] = round(float(np.median(rates[False])), 1)
print(json.dumps(out), flush=True)
