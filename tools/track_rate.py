#!/usr/bin/env python3
"""What feature tracks cost: one KITTI-size (1241 x 376) stereo sequence, resident in HBM, quad-matched in chunks of
consecutive frames on a sequence handle (as tools/sequence_rate.py), `--runs` alternating runs with track linking off and
on.  Prints one JSON line: both rates, their ratio, the three track kernels' time per chunk (profile scopes, from a
separate profiled pass), the extra device bytes; afterwards checks the tracks of the last chunk's rows against a
sequential host restatement of the link rule.
  python tools/track_rate.py [--chunk 256] [--chunks 100] [--warmup 2] [--runs 3]"""
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
ap.add_argument("--chunks", type=int, default=100, help="timed chunks per run")
ap.add_argument("--warmup", type=int, default=2, help="untimed chunks first")
ap.add_argument("--runs", type=int, default=3, help="alternating runs per state")
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


def handle(on):
    g = pkg.SequenceGroup(args.chunk, params, max_features=cap, max_matches=cap)
    g.setTrackLinking(on)
    g.setStream(torch.cuda.current_stream().cuda_stream)
    return g


def chunk(g, k):
    t0 = (k * args.chunk) % P
    g.pushBackDevice(left[t0].data_ptr(), right[t0].data_ptr(), isz, dims, args.chunk)
    g.matchFeatures(pkg.METHOD_QUAD)


def run(g, k0, n):
    for k in range(k0, k0 + n):
        chunk(g, k)
    g.synchronize()


gs = {False: handle(False), True: handle(True)}
pos = {False: 0, True: 0}
for on in (False, True):
    run(gs[on], 0, args.warmup)
    pos[on] = args.warmup
rates = {False: [], True: []}
for _ in range(args.runs):
    for on in (False, True):
        t0 = time.perf_counter()
        run(gs[on], pos[on], args.chunks)
        rates[on].append(args.chunk * args.chunks / (time.perf_counter() - t0))
        pos[on] += args.chunks
extra = gs[True].deviceBytes() - gs[False].deviceBytes()

# the kernels' own time: a profiled pass (events around every launch) of a few chunks
g = gs[True]
g.profileEnable(True)
g.profileReset()
nprof = 8
run(g, pos[True], nprof)
pos[True] += nprof
kern = {k: round(g.profileRead(k)[0] / nprof, 4) for k in ("track_carry", "track_scatter", "track_link", "track_rank", "emit_matches")}
g.profileEnable(False)

# every 8th row of the last chunk against the link rule restated on the host, given the row before it
_, counts = g.getTracksAll()
bad, oldest = [], 0
records = int(counts.sum())
first, _n = g.position()
for r in range(1, args.chunk, 8):
    pm_prev, tr_prev = g.getMatches(r - 1), g.getTracks(r - 1)
    pm, tr = g.getMatches(r), g.getTracks(r)
    where = {int(c): q for q, c in reversed(list(enumerate(pm_prev["i1c"])))}
    ok = len(tr) == len(pm) == counts[r]
    for j in range(len(pm) if ok else 0):
        q = where.get(int(pm["i1p"][j]), -1)
        want = (first + r, j, 1, -1, 0) if q < 0 else (tr_prev["birth_frame"][q], tr_prev["birth_pos"][q], tr_prev["age"][q] + 1, q, 0)
        if tuple(int(x) for x in tr[j]) != tuple(int(x) for x in want):
            ok = False
            break
    if not ok:
        bad.append(r)
    oldest = max(oldest, int(tr["age"].max(initial=0)))
for h in gs.values():
    h.close()
off, on = float(np.median(rates[False])), float(np.median(rates[True]))
print(json.dumps({"metric": "sequence_quad_pairs_per_s_with_tracks", "chunk": args.chunk, "chunks": args.chunks,
                  "off": [round(x, 1) for x in rates[False]], "on": [round(x, 1) for x in rates[True]],
                  "value": round(on, 1), "off_median": round(off, 1), "ratio": round(on / off, 4),
                  "kernel_ms_per_chunk": kern, "extra_device_bytes": int(extra), "records_last_chunk": records,
                  "oldest_track": oldest, "rows_mismatched": bad, "W": W, "H": H}), flush=True)
sys.exit(1 if bad else 0)
