#!/usr/bin/env python3
"""What the motion covariance costs: S KITTI-size (1241 x 376) stereo streams resident in HBM,
stepped together and quad-matched; every step estimates the motion (vh_group_estimate_motion), classifies the dense lists
under it (vh_group_motion_inliers), refines the motion on all inliers and classifies again (vh_group_refit_motion,
reclassify = 1), then asks for the covariance of the refined motion over its inliers (vh_group_motion_covariance, tr =
NULL: nothing is uploaded).  Prints one JSON line per step -- the device time of the motion_cov scope beside the
motion_refit scope of the same step, the bytes the pass reads (48 per inlier record: three 16-byte loads), a
device-to-device hipMemcpyAsync of that byte count timed in the same session as the yardstick, the wall time of the
whole call, how many lists got a covariance, and the median one-sigma of tx -- and a summary line with the medians.
  python tools/cov_rate.py [--streams 256] [--steps 8] [--warmup 3]"""
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
ap.add_argument("--steps", type=int, default=8)
ap.add_argument("--warmup", type=int, default=3)
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
    g.pushBackDevice(left[t % P].data_ptr(), right[t % P].data_ptr(), isz, dims)
    if t == 0:
        continue
    g.matchFeatures(pkg.METHOD_QUAD)
    tr, ok, _ = g.estimateMotion(e, rand3)
    g.motionInliers(e, tr, ok.astype(np.int32))
    g.synchronize()
    g.profileReset()
    tr2, ok2, nupd, counts = g.refitMotion(e, reclassify=True)
    w0 = time.perf_counter()
    cov, ssr, okc, n = g.motionCovariance(e)
    call_ms = (time.perf_counter() - w0) * 1e3
    if t < args.warmup:
        continue
    k = int(n.sum())
    sig_tx = np.sqrt(cov[okc, 3, 3])
    row = {"step": t, "inliers": k, "ok_refit": int(ok2.sum()), "ok_cov": int(okc.sum()),
           "motion_cov_ms": round(g.profileRead("motion_cov")[0], 4), "motion_refit_ms": round(g.profileRead("motion_refit")[0], 4),
           "n_updates_max": int(nupd.max()), "bytes_read": 48 * k, "copy_ms": round(copy_ms(max(48 * k, 1)), 4),
           "call_ms": round(call_ms, 4), "sigma_tx_median": float(np.median(sig_tx)) if len(sig_tx) else None}
    rows.append(row)
    print(json.dumps(row), flush=True)
g.close()
med = lambda f: round(float(np.median([f(x) for x in rows])), 6)  # noqa: E731
print(json.dumps({"metric": "motion_cov_device_time", "streams": S, "W": W, "H": H, "steps": len(rows),
                  "inliers_per_step": med(lambda x: x["inliers"]), "motion_cov_ms": med(lambda x: x["motion_cov_ms"]),
                  "motion_refit_ms": med(lambda x: x["motion_refit_ms"]), "n_updates_max": int(max(x["n_updates_max"] for x in rows)),
                  "bytes_read": med(lambda x: x["bytes_read"]), "copy_ms": med(lambda x: x["copy_ms"]),
                  "call_ms": med(lambda x: x["call_ms"]), "ok_cov": med(lambda x: x["ok_cov"])}), flush=True)
