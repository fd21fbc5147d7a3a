#!/usr/bin/env python3
"""What the dense stages of the device post chain cost: S KITTI-size (1241 x 376) stereo streams
resident in HBM, stepped together and quad-matched, every step through vh_group_post_begin_device / _finish_device_dense
in the default ring shape (64 steps per batch, 3 batches, 16 lists per wave), the dense mode 0 / 1 / 2 / 3 in turn,
`--rounds` times over (alternating, so that drift hits every mode alike).  Per mode and round one JSON line: pairs/s of the
as-shipped loop (the fill and the drain of the pipeline included, as bench.py's e2e_matchfeatures), the ring's bytes and
the steps per batch they imply (the library halves them until the ring fits 80 % of the free memory), and -- from one more
pass over the ring with profiling on -- the device time and launch count of the scopes the dense stages record on the
batches' streams.  A summary line gives each mode's median rate and its ratio to mode 0 of the same session.
  python tools/post_dense_rate.py [--streams 256] [--rounds 4] [--steps-per-batch 64] [--batches 3] [--lanes 16]"""
import argparse
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
ap.add_argument("--rounds", type=int, default=4)
ap.add_argument("--steps-per-batch", type=int, default=64)
ap.add_argument("--batches", type=int, default=3)
ap.add_argument("--lanes", type=int, default=16)
ap.add_argument("--modes", default="0,1,2,3")
args = ap.parse_args()
S, B, NB = args.streams, args.steps_per_batch, args.batches
MODES = [int(m) for m in args.modes.split(",")]
SCOPES = ("post_dense_gate", "inlier_flag", "inlier_compact", "motion_refit")

pkg = entry.load_package()
wl = bench.WORKLOADS["kitti"]
W, H, cap = wl["W"], wl["H"], wl["cap"]
params = pkg.Params.default(**wl["params"])
bpl = pkg.synth.bytes_per_line(W)
dims, isz = [W, H, bpl], H * bpl
dev = torch.device("cuda", 0)

P = 20  # stereo_sequence's pan repeats every 20 frames: stream s sees frame (t + s) % P at step t
base = pkg.synth.stereo_sequence(W, H, P, disparity=12)
uniq = torch.from_numpy(np.stack([np.stack(pr) for pr in base])).to(dev)
frames = uniq[torch.arange(S + P, device=dev) % P].contiguous()
left, right = frames[:, 0].contiguous(), frames[:, 1].contiguous()
torch.cuda.synchronize()

ego = pkg.EgoParams.default(f=721.5, cu=609.6, cv=172.9, base=0.54)
r3 = np.random.default_rng(7).integers(0, 2 ** 31 - 1, (S, ego.ransac_iters, 3)).astype(np.int32)

g = pkg.StreamGroup(S, params, max_features=cap, max_matches=cap)
g.setStream(torch.cuda.current_stream().cuda_stream)
k = 0


def step():
    global k
    g.pushBackDevice(left[k % P].data_ptr(), right[k % P].data_ptr(), isz, dims)
    if k:
        g.matchFeatures(pkg.METHOD_QUAD)
    k += 1


step(); step()
g.synchronize()
cap_ps = int(min(cap, max(1024, int(g.getCounts()[1].max() * 1.25))))   # as bench.py sizes the slots
bytes_matcher = g.deviceBytes()


def run(mode, rnd):
    g.postDeviceConfig(B, NB, args.lanes)
    g.postDeviceDense(mode)
    dense = ("counts",) if mode else None
    depth, n = B * (NB - 1), max(4 * B * NB, 48)
    for j in range(B * NB):  # untimed: every batch of the ring is allocated and used once
        step(); g.postBeginDevice(cap_ps, 2, 50.0, 50.0, ego=ego, rand3=r3)
    for j in range(B * NB):
        g.postFinishDevice(B * NB - 1 - j, dense=dense)
    g.synchronize()
    ring = g.deviceBytes() - bytes_matcher
    ok, ok_refit, inl = [], [], []
    t0 = time.perf_counter()
    for j in range(n + depth):
        if j < n:
            step(); g.postBeginDevice(cap_ps, 2, 50.0, 50.0, ego=ego, rand3=r3)
        if j >= depth:
            r = g.postFinishDevice(min(j, n - 1) - (j - depth), dense=dense)
            ok.append(float(r["ok"].mean()))
            if mode:
                inl.append(float(r["inlier_counts"].mean()))
            if mode >= 2:
                ok_refit.append(float(r["ok_refit"].mean()))
    g.synchronize()
    dt = time.perf_counter() - t0
    # one more pass over the ring with profiling on: the scopes of the batches' streams
    g.profileEnable(True); g.profileReset()
    for j in range(B * NB):
        step(); g.postBeginDevice(cap_ps, 2, 50.0, 50.0, ego=ego, rand3=r3)
    for j in range(B * NB):
        g.postFinishDevice(B * NB - 1 - j, dense=dense)
    g.synchronize()
    scopes = {s: dict(zip(("ms", "launches"), g.profileRead(s))) for s in SCOPES}
    g.profileEnable(False)
    per_step = S * cap_ps * (176.0 + (53.0 if mode else 0.0))
    row = {"mode": mode, "round": rnd, "pairs_per_s": round(S * n / dt, 1), "steps": n, "ring_bytes": int(ring),
           "steps_per_batch_asked": B, "steps_per_batch_implied": round(ring / (NB * per_step), 1), "slot_records": cap_ps,
           "pose_ok_share": round(float(np.mean(ok)), 4), "inliers_per_stream": round(float(np.mean(inl)), 1) if inl else None,
           "refit_ok_share": round(float(np.mean(ok_refit)), 4) if ok_refit else None, "scopes_one_ring_pass": scopes}
    print(json.dumps(row), flush=True)
    return row


rows = [run(m, rnd) for rnd in range(args.rounds) for m in MODES]
g.close()
med = {m: float(np.median([r["pairs_per_s"] for r in rows if r["mode"] == m])) for m in MODES}
print(json.dumps({"metric": "post_dense_rate", "streams": S, "W": W, "H": H, "rounds": args.rounds,
                  "pairs_per_s_median": med, "spread": {m: [min(r["pairs_per_s"] for r in rows if r["mode"] == m),
                                                           max(r["pairs_per_s"] for r in rows if r["mode"] == m)] for m in MODES},
                  "ratio_to_mode_0": {m: round(med[m] / med[0], 4) for m in MODES} if 0 in med else None}), flush=True)
