#!/usr/bin/env python3
"""What reconstruction on a group costs: S KITTI-size (1241 x 376) stereo streams resident in HBM,
stepped together and quad-matched, `--runs` alternating runs per state: linking off, linking on, linking plus
reconstruction with the call placed after the next push (push t+1, reconstruct t, match t+1) and constructed poses.
Prints one JSON line: the rates per state, the per-step times of the four recon scopes (a separate profiled pass), the
wall time of reconstruct(), the extra device bytes and the lost tracks of the last step.  `--states off,link` runs on a
library without the feature (the comparison point: the tracks-on state of the parent commit, same day).
  python tools/group_recon_rate.py [--streams 256] [--steps 40] [--warmup 5] [--runs 3] [--history 8] [--states off,link,recon]"""
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
ap.add_argument("--steps", type=int, default=40, help="timed steps per run")
ap.add_argument("--warmup", type=int, default=5, help="untimed steps first")
ap.add_argument("--runs", type=int, default=3, help="alternating runs per state")
ap.add_argument("--history", type=int, default=8)
ap.add_argument("--states", default="off,link,recon")
args = ap.parse_args()
STATES = tuple(args.states.split(","))
S = args.streams

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

# constructed poses: 0.5 m forward per step with a slight turn; the same motion for every stream
c, s_ = np.cos(-0.004), np.sin(-0.004)
TR = np.array([[c, 0, s_, -0.03], [0, 1, 0, 0], [-s_, 0, c, -0.5], [0, 0, 0, 1]], np.float64)
TRS = np.repeat(TR[None], S, 0)


def handle(state):
    g = pkg.StreamGroup(S, params, max_features=cap, max_matches=cap)
    if state == "link":
        g.setTrackLinking(True)
    elif state == "recon":
        g.setReconstruction(pkg.ReconParams.default(f=721.5, cu=609.6, cv=172.9), args.history)
    g.setStream(torch.cuda.current_stream().cuda_stream)
    return g


wall = []
lost = [0, 0]


def run(g, state, t0, n):
    """Steps t0 .. t0 + n - 1; with reconstruction: push t+1, reconstruct t, match t+1."""
    for t in range(t0, t0 + n):
        g.pushBackDevice(left[t % P].data_ptr(), right[t % P].data_ptr(), isz, dims)
        if state == "recon" and t > 0:
            w0 = time.perf_counter()
            nt, na = C.c_int32(0), C.c_int32(0)
            rc = pkg._lib().vh_group_reconstruct(g._h, TRS.ctypes.data_as(C.c_void_p), C.byref(nt), C.byref(na))
            assert rc == pkg.VH_OK, rc
            wall.append(time.perf_counter() - w0)
            lost[0], lost[1] = nt.value, na.value
        g.matchFeatures(pkg.METHOD_QUAD)
    g.synchronize()


gs = {st: handle(st) for st in STATES}
pos = {}
for st in STATES:
    run(gs[st], st, 0, args.warmup)
    pos[st] = args.warmup
wall.clear()
rates = {st: [] for st in STATES}
for _ in range(args.runs):
    for st in STATES:
        w0 = time.perf_counter()
        run(gs[st], st, pos[st], args.steps)
        rates[st].append(S * args.steps / (time.perf_counter() - w0))
        pos[st] += args.steps
out = {"metric": "group_quad_pairs_per_s_with_reconstruction", "streams": S, "steps": args.steps, "history": args.history,
       "runs": {st: [round(x, 1) for x in rates[st]] for st in STATES},
       "median": {st: round(float(np.median(rates[st])), 1) for st in STATES}, "W": W, "H": H}
if "recon" in gs:
    g = gs["recon"]
    out["reconstruct_wall_ms"] = round(1e3 * float(np.median(wall)), 4)
    out["lost_tracks_last_step"], out["accepted_last_step"] = lost
    if "link" in gs:
        out["extra_device_bytes"] = int(g.deviceBytes() - gs["link"].deviceBytes())
        out["ratio_to_link"] = round(out["median"]["recon"] / out["median"]["link"], 4)
    # the kernels' own time: a profiled pass (events around every launch) of a few steps
    g.profileEnable(True)
    g.profileReset()
    nprof = 16
    run(g, "recon", pos["recon"], nprof)
    names = ("recon_store", "recon_tails", "recon_gather", "recon_solve", "track_rank", "emit_matches")
    out["kernel_ms_per_step"] = {k: round(g.profileRead(k)[0] / nprof, 4) for k in names}
    g.profileEnable(False)
for h in gs.values():
    h.close()
print(json.dumps(out), flush=True)
