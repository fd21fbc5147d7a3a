#!/usr/bin/env python3
"""KITTI-size (1241 x 376) quad and flow matching on a group of S streams with multi-stage matching off, on with the
vote and the statistics on the host ("on") and on with both on the device ("device": vh_group_set_multi_stage_device;
DESIGN.md section 6 f-3): pairs per second in alternating runs, matches per pair and the per-scope times of a few
profiled steps (sparse detection, pass 1, vote, statistics, pass 2).  It prints one JSON line; it decides nothing.
  python tools/multistage_rate.py [--streams 256] [--steps 24] [--warmup 3] [--rounds 3] [--profile-steps 3] [--methods 2,0]"""
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
ap.add_argument("--steps", type=int, default=24, help="timed steps per run")
ap.add_argument("--warmup", type=int, default=3, help="untimed steps before the first run of a handle")
ap.add_argument("--rounds", type=int, default=3, help="alternating off / on / device runs")
ap.add_argument("--profile-steps", type=int, default=3, help="profiled steps after the timed ones")
ap.add_argument("--methods", default="2,0")
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
frames = uniq[torch.arange(S + P, device=dev) % P].contiguous()
left, right = frames[:, 0].contiguous(), frames[:, 1].contiguous()
torch.cuda.synchronize()
SCOPES = ("detect_nms", "emit_features", "bin_scan", "bin_sort", "match", "chain", "emit_matches",
          "sparse_detect_nms", "sparse_emit_features", "sparse_bin_scan", "sparse_bin_sort", "sparse_match", "sparse_chain",
          "sparse_emit_matches", "sparse_vote_host", "statistics_host", "sparse_vote", "prior_stats", "ranged")
STATES = ("off", "on", "device")

out = {"metric": "multistage_pairs_per_s", "W": W, "H": H, "streams": S, "steps": args.steps, "methods": {}}
for method in [int(x) for x in args.methods.split(",")]:
    stereo = method != pkg.METHOD_FLOW
    params = pkg.Params.default(**dict(wl["params"], multi_stage=1))
    groups = {}
    for state in STATES:
        g = pkg.StreamGroup(S, params, max_features=cap, max_matches=cap)
        if state != "off":
            g.setMultiStageMatching(True)
        if state == "device":
            g.setMultiStageDevice(True)
        g.setStream(torch.cuda.current_stream().cuda_stream)
        groups[state] = g

    def step(g, t):
        o = t % P
        g.pushBackDevice(left[o].data_ptr(), right[o].data_ptr() if stereo else None, isz, dims)
        g.matchFeatures(method)

    def run(g, t0_, n):
        for t in range(t0_, t0_ + n):
            step(g, t)
        g.synchronize()

    for state in STATES:
        run(groups[state], 0, args.warmup)
    rates = {state: [] for state in STATES}
    t_at = args.warmup
    for _ in range(args.rounds):  # off, on, device, off, ...: a drift of the box shows in all three
        for state in STATES:
            t0 = time.perf_counter()
            run(groups[state], t_at, args.steps)
            rates[state].append(S * args.steps / (time.perf_counter() - t0))
        t_at += args.steps
    res = {}
    for state in STATES:
        g = groups[state]
        on = state != "off"
        g.profileEnable(True)
        g.profileReset()
        run(g, t_at, args.profile_steps)
        scopes = {}
        for name in SCOPES:
            ms, n = g.profileRead(name)
            if n:
                scopes[name] = {"ms_per_step": round(ms / args.profile_steps, 4), "launches": int(n)}
        g.profileEnable(False)
        _, nm = g.getCounts()
        r = sorted(rates[state])
        res[state] = {
            "pairs_per_s_runs": [round(x, 1) for x in rates[state]], "pairs_per_s_median": round(r[len(r) // 2], 1),
            "matches_per_pair_mean": round(float(nm.mean()), 1), "matches_stream0": int(nm[0]),
            "sparse_matches_stream0": int(len(g.getSparseMatches(0))) if on else None,
            "device_gb": round(g.deviceBytes() / 1e9, 2), "scopes": scopes}
        g.close()
    res["ratio_on_to_off"] = round(res["on"]["pairs_per_s_median"] / res["off"]["pairs_per_s_median"], 4)
    res["ratio_device_to_on"] = round(res["device"]["pairs_per_s_median"] / res["on"]["pairs_per_s_median"], 4)
    out["methods"]["quad" if method == 2 else ("flow" if method == 0 else "stereo")] = res
    torch.cuda.synchronize()
print(json.dumps(out), flush=True)
