#!/usr/bin/env python3
"""KITTI-size (1241 x 376) stereo quad matching on a group of S streams with refinement = 0 / 1 / 2 (match positions
refined on the GPU): pairs per second of each, their ratio to refinement = 0, and the per-scope
kernel times of a few profiled steps.  Prints one JSON line.
  python tools/refine_rate.py [--streams 256] [--steps 40] [--warmup 4] [--profile-steps 4] [--modes 0,1,2]"""
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
ap.add_argument("--steps", type=int, default=40, help="timed steps per refinement mode")
ap.add_argument("--warmup", type=int, default=4, help="untimed steps first")
ap.add_argument("--profile-steps", type=int, default=4, help="profiled steps after the timed ones")
ap.add_argument("--modes", default="0,1,2")
args = ap.parse_args()

pkg = entry.load_package()
wl = bench.WORKLOADS["kitti"]
W, H, cap = wl["W"], wl["H"], wl["cap"]
S = args.streams
bpl = pkg.synth.bytes_per_line(W)
dims, isz = [W, H, bpl], H * bpl
dev = torch.device("cuda", 0)
P = 20  # stereo_sequence's pan repeats every 20 frames
base = pkg.synth.stereo_sequence(W, H, P, disparity=12)
uniq = torch.from_numpy(np.stack([np.stack(pr) for pr in base])).to(dev)  # [20, 2, H, bpl]
# stream s at step t reads frame (s + t) % 20: S + 20 consecutive frames, one image stride apart
frames = uniq[torch.arange(S + P, device=dev) % P].contiguous()
left, right = frames[:, 0].contiguous(), frames[:, 1].contiguous()
torch.cuda.synchronize()
SCOPES = ("detect_nms", "emit_features", "bin_scan", "bin_sort", "match", "chain", "refine_planes", "refine", "emit_matches")

out = {"metric": "refine_quad_pairs_per_s", "W": W, "H": H, "streams": S, "steps": args.steps, "modes": {}}
for r in [int(x) for x in args.modes.split(",")]:
    params = pkg.Params.default(**dict(wl["params"], refinement=r))
    g = pkg.StreamGroup(S, params, max_features=cap, max_matches=cap)
    g.setStream(torch.cuda.current_stream().cuda_stream)

    def step(t):
        o = t % P
        g.pushBackDevice(left[o].data_ptr(), right[o].data_ptr(), isz, dims)
        g.matchFeatures(pkg.METHOD_QUAD)

    for t in range(args.warmup):
        step(t)
    g.synchronize()
    t0 = time.perf_counter()
    for t in range(args.warmup, args.warmup + args.steps):
        step(t)
    g.synchronize()
    rate = S * args.steps / (time.perf_counter() - t0)
    g.profileEnable(True)
    g.profileReset()
    for t in range(args.profile_steps):
        step(t)
    g.synchronize()
    scopes = {}
    for name in SCOPES:
        ms, n = g.profileRead(name)
        if n:
            scopes[name] = {"ms_per_step": round(ms / args.profile_steps, 4), "launches": int(n)}
    g.profileEnable(False)
    _, nm = g.getCounts()
    out["modes"][str(r)] = {"pairs_per_s": round(rate, 1), "matches_stream0": int(nm[0]),
                            "device_gb": round(g.deviceBytes() / 1e9, 2), "scopes": scopes}
    g.close()
    torch.cuda.synchronize()
if "0" in out["modes"]:
    r0 = out["modes"]["0"]["pairs_per_s"]
    for v in out["modes"].values():
        v["ratio_to_0"] = round(v["pairs_per_s"] / r0, 3)
print(json.dumps(out), flush=True)
