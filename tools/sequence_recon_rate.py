#!/usr/bin/env python3
"""What reconstruction on a sequence handle costs: one KITTI-size (1241 x 376) stereo sequence,
resident in HBM, quad-matched in chunks of consecutive frames (as tools/track_rate.py), `--runs` alternating runs in three
states: linking off, linking on, linking plus reconstruction with the call placed after the next push (push k+1,
reconstruct k, match k+1) and constructed poses.  Prints one JSON line: the three rates, the per-chunk times of the four new
scopes beside track_rank and emit_matches (a separate profiled pass), the wall time of reconstruct(), the extra device
bytes, and -- labelled as a ratio against interpreted Python -- the host path it replaces for one chunk (getMatchesAll plus
Reconstruction.updateMany on the same lists).
  python tools/sequence_recon_rate.py [--chunk 256] [--chunks 40] [--warmup 2] [--runs 3] [--history 64]"""
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
ap.add_argument("--chunk", type=int, default=256)
ap.add_argument("--chunks", type=int, default=40, help="timed chunks per run")
ap.add_argument("--warmup", type=int, default=2, help="untimed chunks first")
ap.add_argument("--runs", type=int, default=3, help="alternating runs per state")
ap.add_argument("--history", type=int, default=64)
args = ap.parse_args()

pkg = entry.load_package()
wl = bench.WORKLOADS["kitti"]
W, H, cap = wl["W"], wl["H"], wl["cap"]
params = pkg.Params.default(**wl["params"])
bpl = pkg.synth.bytes_per_line(W)
dims, isz = [W, H, bpl], H * bpl
dev = torch.device("cuda", 0)

P = 20  # stereo_sequence's pan repeats every 20 frames (tools/sequence_rate.py)
base = pkg.synth.stereo_sequence(W, H, P, disparity=12)
uniq = torch.from_numpy(np.stack([np.stack(pr) for pr in base])).to(dev)
frames = uniq[torch.arange(args.chunk + P, device=dev) % P].contiguous()
left, right = frames[:, 0].contiguous(), frames[:, 1].contiguous()
torch.cuda.synchronize()

# constructed poses: 0.5 m forward per frame with a slight turn; the same motion for every row
c, s = np.cos(-0.004), np.sin(-0.004)
TR = np.array([[c, 0, s, -0.03], [0, 1, 0, 0], [-s, 0, c, -0.5], [0, 0, 0, 1]], np.float64)
TRS = np.repeat(TR[None], args.chunk, 0)
RECON = pkg.ReconParams.default(f=721.5, cu=609.6, cv=172.9)
STATES = ("off", "link", "recon")


def handle(state):
    g = pkg.SequenceGroup(args.chunk, params, max_features=cap, max_matches=cap)
    if state == "link":
        g.setTrackLinking(True)
    elif state == "recon":
        g.setReconstruction(RECON, args.history)
    g.setStream(torch.cuda.current_stream().cuda_stream)
    return g


def push(g, k):
    t0 = (k * args.chunk) % P
    g.pushBackDevice(left[t0].data_ptr(), right[t0].data_ptr(), isz, dims, args.chunk)


wall = []


def run(g, state, k0, n):
    """Chunks k0 .. k0 + n - 1; with reconstruction: push k+1, reconstruct k, match k+1."""
    for k in range(k0, k0 + n):
        push(g, k)
        if state == "recon" and k > 0:
            t0 = time.perf_counter()
            g.reconstruct(TRS)
            wall.append(time.perf_counter() - t0)
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
        t0 = time.perf_counter()
        run(gs[st], st, pos[st], args.chunks)
        rates[st].append(args.chunk * args.chunks / (time.perf_counter() - t0))
        pos[st] += args.chunks
extra = gs["recon"].deviceBytes() - gs["link"].deviceBytes()
wall_ms = 1e3 * float(np.median(wall)) if wall else None

# the kernels' own time: a profiled pass (events around every launch) of a few chunks
g = gs["recon"]
g.profileEnable(True)
g.profileReset()
nprof = 8
run(g, "recon", pos["recon"], nprof)
names = ("recon_store", "recon_tails", "recon_gather", "recon_solve", "track_rank", "emit_matches")
kern = {k: round(g.profileRead(k)[0] / nprof, 4) for k in names}
g.profileEnable(False)

# the host path it replaces, one chunk, the same lists: a ratio against interpreted Python
t0 = time.perf_counter()
rec, counts = g.getMatchesAll()
lists = [rec[r, :counts[r]] for r in range(args.chunk)]
host = pkg.Reconstruction()
host.setCalibration(RECON.f, RECON.cu, RECON.cv)
host.updateMany(lists, TRS)
host_ms = 1e3 * (time.perf_counter() - t0)
last = g.reconstruct(TRS)
for h in gs.values():
    h.close()
med = {st: float(np.median(rates[st])) for st in STATES}
print(json.dumps({"metric": "sequence_quad_pairs_per_s_with_reconstruction", "chunk": args.chunk, "chunks": args.chunks, "history": args.history,
                  "runs": {st: [round(x, 1) for x in rates[st]] for st in STATES}, "median": {st: round(v, 1) for st, v in med.items()},
                  "value": round(med["recon"], 1), "ratio_to_link": round(med["recon"] / med["link"], 4),
                  "kernel_ms_per_chunk": kern, "reconstruct_wall_ms": wall_ms, "extra_device_bytes": int(extra),
                  "lost_tracks_last_chunk": int(len(last)), "history_tracks_last_chunk": int((last["status"] == pkg.RECON_HISTORY).sum()),
                  "host_path_ms_one_chunk_interpreted_python": round(host_ms, 1), "W": W, "H": H}), flush=True)
