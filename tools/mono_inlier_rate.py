#!/usr/bin/env python3
"""What the mono motion inliers cost: S KITTI-size (1241 x 376) streams resident in HBM, stepped
together and flow- or quad-matched; every step estimates the motion with the mono estimator, takes its models
(vh_group_estimate_motion_mono_model) and classifies the dense lists under them (vh_group_motion_inliers_mono); on quad
lists the stereo classifier (vh_group_motion_inliers under vh_group_estimate_motion's tr) runs beside it.  Prints one JSON
line per step -- the device times of the scopes, the bytes they move and the achieved GB/s -- and a summary line with the
medians and, as the yardstick, a device-to-device hipMemcpyAsync of the same byte count timed in the same session (copy_ms;
it reads and writes every byte, so copy_GBps counts twice that).
  bytes: inlier_flag_mono reads 32 per record and writes 1 (inlier_flag: 48 and 1); inlier_compact reads 1 per record and 48
  per inlier, writes 52 per inlier (the tile counts and the models are a few KB).
  python tools/mono_inlier_rate.py [--method flow|quad] [--streams 256] [--steps 8] [--warmup 3] [--iters 200]"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402  (loads its HIP runtime before the product library, as bench.py does)
import __graft_entry__ as entry  # noqa: E402
import bench  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--streams", type=int, default=256)
ap.add_argument("--steps", type=int, default=8)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--method", choices=("flow", "quad"), default="flow")
ap.add_argument("--iters", type=int, default=200, help="RANSAC hypotheses of the mono estimator (it only supplies the models)")
args = ap.parse_args()
S = args.streams

pkg = entry.load_package()
ob = entry.load_oracle()
wl = bench.WORKLOADS["kitti"]
W, H, cap = wl["W"], wl["H"], wl["cap"]
params = pkg.Params.default(**wl["params"])
bpl = pkg.synth.bytes_per_line(W)
dims, isz = [W, H, bpl], H * bpl
dev = torch.device("cuda", 0)
HIP = C.CDLL("libamdhip64.so")  # the runtime already in the process

P = 20  # stereo_sequence's pan repeats every 20 frames: stream s sees frame (t + s) % P at step t
base = pkg.synth.stereo_sequence(W, H, P, disparity=12)
uniq = torch.from_numpy(np.stack([np.stack(pr) for pr in base])).to(dev)
frames = uniq[torch.arange(S + P, device=dev) % P].contiguous()
left, right = frames[:, 0].contiguous(), frames[:, 1].contiguous()
torch.cuda.synchronize()

e = pkg.EgoParams.default(f=721.5, cu=609.6, cv=172.9, base=0.54)
r = ob.glibc_rand_after_srand0(3 * e.ransac_iters).reshape(e.ransac_iters, 3)
rand3 = np.stack([r] * S)
mono = pkg.MonoParams.default(ransac_iters=args.iters, f=721.5, cu=609.6, cv=172.9, height=1.65)
rand8 = np.stack([ob.glibc_rand_after_srand0(8 * mono.ransac_iters).reshape(mono.ransac_iters, 8)] * S)
quad = args.method == "quad"


def copy_ms(nbytes, reps=5):
    """A device-to-device copy of nbytes on the current stream: the median of `reps` event-timed copies after one untimed."""
    a = torch.zeros(nbytes, dtype=torch.uint8, device=dev); b = torch.empty_like(a)
    st = torch.cuda.current_stream().cuda_stream

    def copy():
        assert HIP.hipMemcpyAsync(C.c_void_p(b.data_ptr()), C.c_void_p(a.data_ptr()), C.c_size_t(nbytes), 3, C.c_void_p(st)) == 0
    copy()
    ms = []
    for _ in range(reps):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record(); copy(); t1.record(); t1.synchronize()
        ms.append(t0.elapsed_time(t1))
    return float(np.median(ms))


g = pkg.StreamGroup(S, params, max_features=cap, max_matches=cap)
g.setStream(torch.cuda.current_stream().cuda_stream)
g.profileEnable(True)
rows = []
for t in range(args.warmup + args.steps):
    g.pushBackDevice(left[t % P].data_ptr(), right[t % P].data_ptr() if quad else None, isz, dims)
    if t == 0:
        continue
    g.matchFeatures(pkg.METHOD_QUAD if quad else pkg.METHOD_FLOW)
    _, mok, _, models = g.estimateMotionMono(mono, rand8, model=True)
    stereo_ms = None
    if quad:   # the stereo classifier of the same lists, in the same session
        tr, ok, _ = g.estimateMotion(e, rand3)
        g.profileReset()
        g.motionInliers(e, tr, ok.astype(np.int32))
        stereo_ms = g.profileRead("inlier_flag")[0]
    g.profileReset()
    counts = g.motionInliersMono(mono, models, models["valid"].astype(np.int32))
    if t < args.warmup:
        continue
    n = int(g.getCounts()[1].sum())
    k = int(counts.sum())
    ms = {name: g.profileRead(name)[0] for name in ("inlier_flag_mono", "inlier_compact")}
    by = {"inlier_flag_mono": 33 * n, "inlier_compact": n + 100 * k}
    total = sum(by.values())
    row = {"step": t, "method": args.method, "records": n, "inliers": k, "valid": int(models["valid"].sum()), "ok": int(mok.sum()),
           "ms": {q: round(v, 4) for q, v in ms.items()}, "bytes": by,
           "GBps": {q: round(by[q] / (ms[q] * 1e6), 1) if ms[q] > 0 else None for q in ms},
           "both_ms": round(sum(ms.values()), 4), "both_GBps": round(total / (sum(ms.values()) * 1e6), 1),
           "copy_ms": round(copy_ms(total), 4), "stereo_inlier_flag_ms": None if stereo_ms is None else round(stereo_ms, 4)}
    row["copy_GBps"] = round(2 * total / (row["copy_ms"] * 1e6), 1)   # a copy of b bytes moves 2 b: read and write
    rows.append(row)
    print(json.dumps(row), flush=True)
g.close()
med = lambda f: round(float(np.median([f(x) for x in rows])), 4)  # noqa: E731
print(json.dumps({"metric": "mono_motion_inliers_device_time", "method": args.method, "streams": S, "W": W, "H": H, "steps": len(rows),
                  "records_per_step": med(lambda x: x["records"]), "inliers_per_step": med(lambda x: x["inliers"]),
                  "inlier_flag_mono_ms": med(lambda x: x["ms"]["inlier_flag_mono"]), "inlier_compact_ms": med(lambda x: x["ms"]["inlier_compact"]),
                  "inlier_flag_mono_GBps": med(lambda x: x["GBps"]["inlier_flag_mono"] or 0.0),
                  "stereo_inlier_flag_ms": med(lambda x: x["stereo_inlier_flag_ms"]) if quad else None,
                  "both_ms": med(lambda x: x["both_ms"]), "both_GBps": med(lambda x: x["both_GBps"]),
                  "copy_ms": med(lambda x: x["copy_ms"]), "copy_GBps": med(lambda x: x["copy_GBps"]),
                  "ratio_to_copy": med(lambda x: x["both_ms"] / x["copy_ms"])}), flush=True)
