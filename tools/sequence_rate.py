#!/usr/bin/env python3
"""One KITTI-size (1241 x 376) stereo sequence, resident in HBM, quad-matched in chunks of consecutive frames on a
sequence handle (vh_sequence_*), against the same frames on one stream (a lone Matcher, pushBackDevice + matchFeatures
per pair).  Prints one JSON line; afterwards checks every row of the last chunk against a lone matcher.
  python tools/sequence_rate.py [--chunk 256] [--chunks 200] [--warmup 2] [--one-pairs 2000]"""
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
ap.add_argument("--chunks", type=int, default=200, help="timed chunks")
ap.add_argument("--warmup", type=int, default=2, help="untimed chunks first")
ap.add_argument("--one-pairs", type=int, default=2000, help="pairs timed on one stream")
args = ap.parse_args()

pkg = entry.load_package()
wl = bench.WORKLOADS["kitti"]
W, H, cap = wl["W"], wl["H"], wl["cap"]
params = pkg.Params.default(**wl["params"])
bpl = pkg.synth.bytes_per_line(W)
dims, isz = [W, H, bpl], H * bpl
dev = torch.device("cuda", 0)

# the sequence: stereo_sequence's pan repeats every 20 frames, so frame t of the sequence is buffer frame t % 20 and a chunk
# starting at frame t0 is the chunk + 20 buffered frames read from t0 % 20 on
base = pkg.synth.stereo_sequence(W, H, 20, disparity=12)
P = 20
uniq = torch.from_numpy(np.stack([np.stack(pr) for pr in base])).to(dev)        # [20, 2, H, bpl]
frames = uniq[torch.arange(args.chunk + P, device=dev) % P].contiguous()        # [chunk + 20, 2, H, bpl]
left, right = frames[:, 0].contiguous(), frames[:, 1].contiguous()
torch.cuda.synchronize()
stride = isz

g = pkg.SequenceGroup(args.chunk, params, max_features=cap, max_matches=cap)
g.setStream(torch.cuda.current_stream().cuda_stream)


def chunk(k):
    t0 = (k * args.chunk) % P
    g.pushBackDevice(left[t0].data_ptr(), right[t0].data_ptr(), stride, dims, args.chunk)
    g.matchFeatures(pkg.METHOD_QUAD)


for k in range(args.warmup):
    chunk(k)
g.synchronize()
t0 = time.perf_counter()
for k in range(args.warmup, args.warmup + args.chunks):
    chunk(k)
g.synchronize()
dt = time.perf_counter() - t0
seq_rate = args.chunk * args.chunks / dt
last_first, n = g.position()
nf, nm = g.getCounts()

# one stream over the same device frames
m = pkg.Matcher(params, max_features=cap, max_matches=cap, outlier_removal=False)
npairs = args.one_pairs
for t in range(8):
    m.pushBackDevice(left[t % P].data_ptr(), right[t % P].data_ptr(), dims)
    m.matchFeatures(2)
m.synchronize()
t1 = time.perf_counter()
for t in range(npairs):
    m.pushBackDevice(left[t % P].data_ptr(), right[t % P].data_ptr(), dims)
    m.matchFeatures(2)
m.synchronize()
one_rate = npairs / (time.perf_counter() - t1)

# the last chunk's rows against a lone matcher driven frame by frame
m.pushBackDevice(left[(last_first - 1) % P].data_ptr(), right[(last_first - 1) % P].data_ptr(), dims)
bad = []
for r in range(n):
    t = (last_first + r) % P
    m.pushBackDevice(left[t].data_ptr(), right[t].data_ptr(), dims)
    m.matchFeatures(2)
    want = m.getMatches()
    if nm[r] != len(want) or (r % 37 == 0 and g.getMatches(r).tobytes() != want.tobytes()):
        bad.append(r)
m.close()
g.close()
print(json.dumps({"metric": "sequence_quad_pairs_per_s", "chunk": args.chunk, "chunks": args.chunks,
                  "value": round(seq_rate, 1), "one_stream_pairs_per_s": round(one_rate, 1),
                  "speedup": round(seq_rate / one_rate, 2), "rows_checked": int(n), "rows_mismatched": bad,
                  "matches_row0": int(nm[0]), "W": W, "H": H}), flush=True)
sys.exit(1 if bad else 0)
