#!/usr/bin/env python3
"""What the tail stages of the device post chain cost, after tools/post_dense_rate.py: S KITTI-size
(1241 x 376) stereo streams resident in HBM, stepped together and matched, every step through vh_group_post_begin_device /
_finish_device_tail in the default ring shape (64 steps per batch, 3 batches, 16 lists per wave).  The configurations, each
beside its own mask 0 and `--rounds` times over (alternating, so that drift hits every one alike):
  stereo      quad lists, the stereo estimator, dense mode 3:  mask 0 | VH_POST_TAIL_COV
  mono        flow lists, the mono estimator, dense mode 1:    mask 0 | MONO_REFIT + MONO_POSE | the same + MONO_REFINE
Per configuration and round one JSON line: pairs/s of the as-shipped loop (the fill and the drain of the pipeline included,
as bench.py's e2e_matchfeatures), the ring's bytes (vh_group_device_bytes less the matcher's), the shape in effect
(vh_group_post_device_shape: the library halves the steps per batch until the ring fits 80 % of the free memory), and --
from one more pass over the ring with profiling on -- the device time and launch count of the scopes the tail records on
the batches' streams.  A summary line gives each configuration's median rate and its ratio to the mask 0 of its family.
  python tools/post_tail_rate.py [--streams 256] [--rounds 4] [--steps-per-batch 64] [--batches 3] [--lanes 16] [--mono-iters 200]"""
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
ap.add_argument("--mono-iters", type=int, default=200)
ap.add_argument("--configs", default="stereo_0,stereo_cov,mono_0,mono_pose,mono_refine")
args = ap.parse_args()
S, B, NB = args.streams, args.steps_per_batch, args.batches
SCOPES = ("motion_cov", "mono_refit", "mono_pose_head", "mono_pose_tri", "mono_pose_front", "mono_pose_rank", "mono_pose_vote",
          "mono_pose_finish", "mono_pose_refine", "inlier_flag", "inlier_flag_mono", "inlier_compact", "motion_refit")

pkg = entry.load_package()
# name -> (mono estimator?, dense mode, tail mask, the mask 0 it is held against)
CONFIGS = {"stereo_0": (False, 3, 0, "stereo_0"), "stereo_cov": (False, 3, pkg.POST_TAIL_COV, "stereo_0"),
           "mono_0": (True, 1, 0, "mono_0"),
           "mono_pose": (True, 1, pkg.POST_TAIL_MONO_REFIT | pkg.POST_TAIL_MONO_POSE, "mono_0"),
           "mono_refine": (True, 1, pkg.POST_TAIL_MONO_REFIT | pkg.POST_TAIL_MONO_POSE | pkg.POST_TAIL_MONO_REFINE, "mono_0")}
NAMES = [c for c in args.configs.split(",") if c]
assert all(c in CONFIGS for c in NAMES), NAMES

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
mono = pkg.MonoParams.default(ransac_iters=args.mono_iters, f=721.5, cu=609.6, cv=172.9, height=1.65, pitch=-0.08)
rng = np.random.default_rng(7)
r3 = rng.integers(0, 2 ** 31 - 1, (S, ego.ransac_iters, 3)).astype(np.int32)
r8 = rng.integers(0, 2 ** 31 - 1, (S, mono.ransac_iters, 8)).astype(np.int32)

g = pkg.StreamGroup(S, params, max_features=cap, max_matches=cap)
g.setStream(torch.cuda.current_stream().cuda_stream)
k = 0


def step(method):
    global k
    g.pushBackDevice(left[k % P].data_ptr(), right[k % P].data_ptr(), isz, dims)
    if k:
        g.matchFeatures(method)
    k += 1


step(pkg.METHOD_QUAD); step(pkg.METHOD_QUAD)
g.synchronize()
cap_ps = int(min(cap, max(1024, int(g.getCounts()[1].max() * 1.25))))   # as bench.py sizes the slots
step(pkg.METHOD_FLOW)
g.synchronize()
cap_ps = int(min(cap, max(cap_ps, int(g.getCounts()[1].max() * 1.25))))
bytes_matcher = g.deviceBytes()


def run(name, rnd):
    is_mono, mode, mask, _ = CONFIGS[name]
    method = pkg.METHOD_FLOW if is_mono else pkg.METHOD_QUAD
    g.postDeviceConfig(B, NB, args.lanes)
    g.postDeviceDense(mode)
    g.postDeviceTail(mask)
    tail = () if mask else None

    def begin():
        step(method)
        if is_mono:
            g.postBeginDevice(cap_ps, 2, 50.0, 50.0, mono=mono, rand8=r8)
        else:
            g.postBeginDevice(cap_ps, 2, 50.0, 50.0, ego=ego, rand3=r3)

    begin()                                   # the first begin call of the ring sizes it: the shape in effect from here on
    b_eff, nb_eff = g.postDeviceShape()
    ring_steps = b_eff * nb_eff
    for j in range(ring_steps - 1):           # untimed: every batch of the ring is allocated and used once
        begin()
    for j in range(ring_steps):
        g.postFinishDevice(ring_steps - 1 - j, dense=("counts",), tail=tail)
    g.synchronize()
    ring = g.deviceBytes() - bytes_matcher
    depth, n = b_eff * (nb_eff - 1), max(4 * ring_steps, 48)
    ok, extra = [], {"ok_cov": [], "ok_model": [], "ok_pose": [], "refine_converged": []}
    t0 = time.perf_counter()
    for j in range(n + depth):
        if j < n:
            begin()
        if j >= depth:
            r = g.postFinishDevice(min(j, n - 1) - (j - depth), dense=("counts",), tail=tail)
            ok.append(float(r["ok"].mean()))
            for q in ("ok_cov", "ok_model", "ok_pose"):
                if q in r:
                    extra[q].append(float(r[q].mean()))
            if "refine" in r:
                extra["refine_converged"].append(float(((r["refine"]["status"] == 0) & (r["refine"]["n_updates"] >= 1)).mean()))
    g.synchronize()
    dt = time.perf_counter() - t0
    # one more pass over the ring with profiling on: the scopes of the batches' streams
    g.profileEnable(True); g.profileReset()
    for j in range(ring_steps):
        begin()
    for j in range(ring_steps):
        g.postFinishDevice(ring_steps - 1 - j, dense=("counts",), tail=tail)
    g.synchronize()
    scopes = {s: dict(zip(("ms", "launches"), g.profileRead(s))) for s in SCOPES}
    scopes = {s: v for s, v in scopes.items() if v["launches"]}
    g.profileEnable(False)
    row = {"config": name, "mask": mask, "dense_mode": mode, "estimator": "mono" if is_mono else "stereo", "round": rnd,
           "pairs_per_s": round(S * n / dt, 1), "steps": n, "ring_bytes": int(ring), "shape_asked": [B, NB], "shape_in_effect": [b_eff, nb_eff],
           "slot_records": cap_ps, "estimator_ok_share": round(float(np.mean(ok)), 4),
           "shares": {q: round(float(np.mean(v)), 4) for q, v in extra.items() if v},
           "batches_in_profiled_pass": nb_eff, "scopes_one_ring_pass": scopes}
    print(json.dumps(row), flush=True)
    return row


rows = [run(c, rnd) for rnd in range(args.rounds) for c in NAMES]
g.close()
med = {c: float(np.median([r["pairs_per_s"] for r in rows if r["config"] == c])) for c in NAMES}
print(json.dumps({"metric": "post_tail_rate", "streams": S, "W": W, "H": H, "rounds": args.rounds, "mono_ransac_iters": mono.ransac_iters,
                  "pairs_per_s_median": med,
                  "spread": {c: [min(r["pairs_per_s"] for r in rows if r["config"] == c), max(r["pairs_per_s"] for r in rows if r["config"] == c)]
                             for c in NAMES},
                  "ratio_to_mask_0": {c: round(med[c] / med[CONFIGS[c][3]], 4) for c in NAMES if CONFIGS[c][3] in med}}), flush=True)
