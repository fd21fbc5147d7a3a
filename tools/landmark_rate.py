#!/usr/bin/env python3
"""What the landmarks cost: S KITTI-size (1241 x 376) stereo streams resident in HBM, stepped
together and quad-matched with track linking on.  Every step classifies the dense lists under the estimated motion, asks
for the scene points of the inliers in the world frame (Tw = the accumulated pose) and fuses them along the tracks
(vh_group_landmarks).  Prints one JSON line per step -- the device time of the "landmarks" scope (memset + index + fuse +
scan + store), the records, points, carried states and landmarks, the bytes the pass reads and writes by the count below,
and a device-to-device hipMemcpyAsync of the same number of bytes timed in the same session as the yardstick -- and a
summary line with the medians and the ratio landmarks time / copy time.
  bytes = 4 per record slot (the memset of the observation index)
        + 36 per point (index: the record read, the index written)
        + 80 per record (fuse: track 24, index 4 + 4, state written 48) + 16 per point (its first half) + 48 per carried state
        + 128 per landmark (store: index 4, state 48, track 24, i1c 4, landmark written 48)
  python tools/landmark_rate.py [--streams 256] [--steps 24] [--warmup 3]"""
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
ap.add_argument("--streams", type=int, default=256)
ap.add_argument("--steps", type=int, default=24)
ap.add_argument("--warmup", type=int, default=3)
args = ap.parse_args()
S = args.streams

pkg = entry.load_package()
ob = entry.load_oracle()
wl = bench.WORKLOADS["kitti"]
W, H, cap = wl["W"], wl["H"], wl["cap"]
params = pkg.Params.default(**wl["params"])
bpl = pkg.synth.bytes_per_line(W)
dims, isz = [W, H, bpl], H * bpl
dev = torch.device("cuda", 0)
HIP = C.CDLL("libamdhip64.so")  # the runtime already in the process

P = 20  # stereo_sequence's pan repeats every 20 frames: stream s sees frame (t + s) % P at step t
base = pkg.synth.stereo_sequence(W, H, P, disparity=12)
uniq = torch.from_numpy(np.stack([np.stack(pr) for pr in base])).to(dev)
frames = uniq[torch.arange(S + P, device=dev) % P].contiguous()
left, right = frames[:, 0].contiguous(), frames[:, 1].contiguous()
torch.cuda.synchronize()

e = pkg.EgoParams.default(f=721.5, cu=609.6, cv=172.9, base=0.54)
r = ob.glibc_rand_after_srand0(3 * e.ransac_iters).reshape(e.ransac_iters, 3)
rand3 = np.stack([r] * S)
lp = pkg.LandmarkParams.default(min_obs=2, max_missed=3, max_dist=0.5, gate_sigma=3.0)


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


g = pkg.StreamGroup(S, params, max_features=cap, max_matches=cap)
g.setTrackLinking(True)
g.setStream(torch.cuda.current_stream().cuda_stream)
g.profileEnable(True)
pose = np.stack([np.eye(4)] * S)  # camera of the current frame -> world, per stream
rows = []
for t in range(args.warmup + args.steps):
    g.pushBackDevice(left[t % P].data_ptr(), right[t % P].data_ptr(), isz, dims)
    if t == 0:
        continue
    g.matchFeatures(pkg.METHOD_QUAD)
    tr, ok, _ = g.estimateMotion(e, rand3)
    n_in = g.motionInliers(e, tr, ok.astype(np.int32))
    for s in range(S):
        if ok[s]:
            pose[s] = pose[s] @ np.linalg.inv(motion_matrix(tr[s]))
    n_pts = g.scenePoints(e, None, pose)
    g.synchronize()
    g.profileReset()
    w0 = time.perf_counter()
    n_lm = g.landmarks(lp)
    call_ms = (time.perf_counter() - w0) * 1e3
    ms = g.profileRead("landmarks")[0]
    if t < args.warmup:
        continue
    trk, counts = g.getTracksAll()
    _, stride = g.landmarksDevice()
    records = int(counts.sum())
    carried = int(sum((trk[s, :counts[s]]["prev"] >= 0).sum() for s in range(S)))
    points, lms = int(n_pts.sum()), int(n_lm.sum())
    nbytes = 4 * S * stride + 36 * points + 80 * records + 16 * points + 48 * carried + 128 * lms
    row = {"step": t, "records": records, "points": points, "carried": carried, "landmarks": lms, "inliers": int(n_in.sum()),
           "landmarks_ms": round(ms, 4), "bytes": nbytes, "copy_ms": round(copy_ms(max(nbytes, 1)), 4), "call_ms": round(call_ms, 4)}
    rows.append(row)
    print(json.dumps(row), flush=True)
deep = max(int(g.getLandmarks(s)["n_obs"].max(initial=0)) for s in range(S))
g.close()
med = lambda f: round(float(np.median([f(x) for x in rows])), 6)  # noqa: E731
out = {"metric": "landmarks_device_time", "streams": S, "W": W, "H": H, "steps": len(rows), "deepest_n_obs_last_step": deep}
out.update({k: med(lambda x, k=k: x[k]) for k in rows[0] if k != "step"})
out["landmarks_over_copy"] = round(out["landmarks_ms"] / out["copy_ms"], 3) if out["copy_ms"] else None
print(json.dumps(out), flush=True)
