#!/usr/bin/env python3
"""One KITTI-size (1241 x 376) stereo sequence, resident in HBM, matched in chunks of consecutive frames on a sequence
handle with multi-stage matching off (mode 0), with the vote and the statistics on the host (mode 1) and on the device
(mode 2): vh_sequence_set_multi_stage.  Flow and quad; prints one JSON line with pairs/s per (method, mode).
  python tools/sequence_multistage_rate.py [--chunk 256] [--chunks 12] [--warmup 2]"""
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
ap.add_argument("--chunks", type=int, default=12, help="timed chunks per state")
ap.add_argument("--warmup", type=int, default=2, help="untimed chunks first")
args = ap.parse_args()

pkg = entry.load_package()
wl = bench.WORKLOADS["kitti"]
W, H, cap = wl["W"], wl["H"], wl["cap"]
kw = dict(wl["params"])
kw["multi_stage"] = 1
params = pkg.Params.default(**kw)
bpl = pkg.synth.bytes_per_line(W)
dims, isz = [W, H, bpl], H * bpl
dev = torch.device("cuda", 0)

# stereo_sequence's pan repeats every 20 frames: a chunk starting at frame t0 is read from t0 % 20 on (tools/sequence_rate.py)
P = 20
base = pkg.synth.stereo_sequence(W, H, P, disparity=12)
uniq = torch.from_numpy(np.stack([np.stack(pr) for pr in base])).to(dev)
frames = uniq[torch.arange(args.chunk + P, device=dev) % P].contiguous()
left, right = frames[:, 0].contiguous(), frames[:, 1].contiguous()
torch.cuda.synchronize()

out = {"tool": "sequence_multistage_rate", "chunk": args.chunk, "chunks": args.chunks, "pairs_per_s": {}, "matches_per_pair": {}}
for name, method in (("flow", pkg.METHOD_FLOW), ("quad", pkg.METHOD_QUAD)):
    for mode in (0, 1, 2):
        g = pkg.SequenceGroup(args.chunk, params, max_features=cap, max_matches=cap)
        g.setMultiStage(mode)
        g.setStream(torch.cuda.current_stream().cuda_stream)

        def chunk(k):
            t0 = (k * args.chunk) % P
            g.pushBackDevice(left[t0].data_ptr(), right[t0].data_ptr() if method == pkg.METHOD_QUAD else None, isz, dims, args.chunk)
            g.matchFeatures(method)

        for k in range(args.warmup):
            chunk(k)
        g.synchronize()
        t0 = time.perf_counter()
        for k in range(args.warmup, args.warmup + args.chunks):
            chunk(k)
        g.synchronize()
        dt = time.perf_counter() - t0
        _, nm = g.getCounts()
        out["pairs_per_s"]["%s_mode%d" % (name, mode)] = round(args.chunk * args.chunks / dt, 1)
        out["matches_per_pair"]["%s_mode%d" % (name, mode)] = round(float(np.mean(nm)), 1)
        g.close()
print(json.dumps(out))
