#!/usr/bin/env python3
"""What the stock rule of the outlier vote costs: S KITTI-size (1241 x 376) stereo streams
resident in HBM, stepped together and quad-matched, every step through the device post chain (vote -> bucketing -> stereo
estimator) in the default ring shape, once on a group under VH_VOTE_REFERENCE and once on a group under VH_VOTE_STOCK,
`--rounds` times over, alternating.  Per rule and round one JSON line: pairs/s of the as-shipped loop (fill and drain of the
pipeline included, as bench.py's e2e_matchfeatures) and -- from one more pass over the ring with profiling on -- the
device time and launch count of the tally's scope (vote_tally under the reference rule, vote_tally_quad under the stock
rule).  Before that, the outlier counts of both rules on the same quad lists (the first `--count-streams` streams of one
step, host form).  A summary line gives each rule's median rate and the ratio.
  python tools/vote_rule_rate.py [--streams 256] [--rounds 3] [--steps-per-batch 64] [--batches 3] [--lanes 16]
                                 [--order reference,stock]"""
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
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--steps-per-batch", type=int, default=64)
ap.add_argument("--batches", type=int, default=3)
ap.add_argument("--lanes", type=int, default=16)
ap.add_argument("--count-streams", type=int, default=8)
ap.add_argument("--order", default="reference,stock", help="the order the two groups are created and run in (a control: both stay alive)")
args = ap.parse_args()
S, B, NB = args.streams, args.steps_per_batch, args.batches

pkg = entry.load_package()
wl = bench.WORKLOADS["kitti"]
W, H, cap = wl["W"], wl["H"], wl["cap"]
params = pkg.Params.default(**wl["params"])
bpl = pkg.synth.bytes_per_line(W)
dims, isz = [W, H, bpl], H * bpl
dev = torch.device("cuda", 0)

P = 20  # stereo_sequence's pan repeats every 20 frames
base = pkg.synth.stereo_sequence(W, H, P, disparity=12)
uniq = torch.from_numpy(np.stack([np.stack(pr) for pr in base])).to(dev)
frames = uniq[torch.arange(S + P, device=dev) % P].contiguous()
left, right = frames[:, 0].contiguous(), frames[:, 1].contiguous()
torch.cuda.synchronize()

ego = pkg.EgoParams.default(f=721.5, cu=609.6, cv=172.9, base=0.54)
r3 = np.random.default_rng(7).integers(0, 2 ** 31 - 1, (S, ego.ransac_iters, 3)).astype(np.int32)
RULES = {"reference": (pkg.VOTE_REFERENCE, "vote_tally"), "stock": (pkg.VOTE_STOCK, "vote_tally_quad")}
RULES = {name: RULES[name] for name in args.order.split(",")}
assert set(RULES) == {"reference", "stock"}, args.order


class Runner:
    def __init__(self, name):
        self.name, (rule, self.scope) = name, RULES[name]
        self.g = pkg.StreamGroup(S, params, max_features=cap, max_matches=cap)
        self.g.setVoteRule(rule)
        self.g.setStream(torch.cuda.current_stream().cuda_stream)
        self.k = 0
        self.step(); self.step()
        self.g.synchronize()
        self.cap_ps = int(min(cap, max(1024, int(self.g.getCounts()[1].max() * 1.25))))   # as bench.py sizes the slots
        self.g.postDeviceConfig(B, NB, args.lanes)

    def step(self):
        self.g.pushBackDevice(left[self.k % P].data_ptr(), right[self.k % P].data_ptr(), isz, dims)
        if self.k:
            self.g.matchFeatures(pkg.METHOD_QUAD)
        self.k += 1

    def ring_pass(self):
        for j in range(B * NB):
            self.step(); self.g.postBeginDevice(self.cap_ps, 2, 50.0, 50.0, ego=ego, rand3=r3)
        for j in range(B * NB):
            self.g.postFinishDevice(B * NB - 1 - j)
        self.g.synchronize()

    def run(self, rnd):
        g = self.g
        depth, n = B * (NB - 1), max(2 * B * NB, 48)
        self.ring_pass()  # untimed: every batch of the ring is allocated and used once
        ok = []
        t0 = time.perf_counter()
        for j in range(n + depth):
            if j < n:
                self.step(); g.postBeginDevice(self.cap_ps, 2, 50.0, 50.0, ego=ego, rand3=r3)
            if j >= depth:
                ok.append(float(g.postFinishDevice(min(j, n - 1) - (j - depth))["ok"].mean()))
        g.synchronize()
        dt = time.perf_counter() - t0
        g.profileEnable(True); g.profileReset()
        self.ring_pass()
        scopes = {s: dict(zip(("ms", "launches"), g.profileRead(s))) for s in ("vote_tally", "vote_tally_flow", "vote_tally_disp", "vote_tally_quad")}
        g.profileEnable(False)
        tally = scopes[self.scope]
        row = {"rule": self.name, "round": rnd, "pairs_per_s": round(S * n / dt, 1), "steps": n, "slot_records": self.cap_ps,
               "pose_ok_share": round(float(np.mean(ok)), 4), "tally_scope": self.scope, "tally_ms_one_ring_pass": round(tally["ms"], 3),
               "tally_launches": tally["launches"], "tally_ms_per_launch": round(tally["ms"] / max(tally["launches"], 1), 4),
               "lists_per_launch": S * B, "scopes_one_ring_pass": scopes}
        print(json.dumps(row), flush=True)
        return row


runners = {name: Runner(name) for name in RULES}
# the outlier counts of both rules on the same lists
g = runners["reference"].g
n_in = n_ref = n_stock = 0
for s in range(min(args.count_streams, S)):
    pm = g.getMatches(s)
    n_in += len(pm)
    n_ref += len(pm) - len(pkg.remove_outliers(pm))
    n_stock += len(pm) - len(pkg.remove_outliers(pm, rule=pkg.VoteRule.stock(pkg.METHOD_QUAD, params.outlier_flow_tolerance, params.outlier_disp_tolerance)))
print(json.dumps({"metric": "vote_rule_outliers", "streams_counted": min(args.count_streams, S), "records": n_in,
                  "dropped_reference": n_ref, "dropped_stock": n_stock}), flush=True)
rows = [runners[name].run(rnd) for rnd in range(args.rounds) for name in RULES]
for r in runners.values():
    r.g.close()
med = {name: float(np.median([r["pairs_per_s"] for r in rows if r["rule"] == name])) for name in RULES}
tally = {name: float(np.median([r["tally_ms_per_launch"] for r in rows if r["rule"] == name])) for name in RULES}
print(json.dumps({"metric": "vote_rule_rate", "streams": S, "W": W, "H": H, "rounds": args.rounds, "pairs_per_s_median": med,
                  "spread": {name: [min(r["pairs_per_s"] for r in rows if r["rule"] == name), max(r["pairs_per_s"] for r in rows if r["rule"] == name)]
                             for name in RULES},
                  "stock_over_reference": round(med["stock"] / med["reference"], 4), "tally_ms_per_launch_median": tally}), flush=True)
