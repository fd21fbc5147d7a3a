#!/usr/bin/env python3
"""What the motion refit on the landmarks costs: S KITTI-size (1241 x 376) stereo streams resident
in HBM, stepped together and quad-matched with track linking and the trajectory on; every step runs match, estimateMotion,
motionInliers, refitMotion (reclassify = 0, for the motion_refit scope on the same lists in the same run),
groupRefitMotionLandmarks (reclassify = 1), trajectory, scenePointsWorld(frame = 1), landmarks.  Prints one JSON line per step --
the device time of the refit_prior, refit_prior_fit and motion_refit scopes, n_used / n, the updates per list of both
fits, the bytes ONE update of the work-buffer fit reads (32 of the two record words + 32 of the prior per inlier record) and
a device-to-device hipMemcpyAsync of that byte count timed in the same session -- and a summary line with the medians.
  python tools/landmark_refit_rate.py [--streams 256] [--steps 8] [--warmup 3]"""
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
import importlib  # noqa: E402
lrf = importlib.import_module(pkg.__name__ + "._lmk_refit")  # the feature's extension module
rp = lrf.LandmarkRefitParams.default()
lp = pkg.LandmarkParams.default()


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
g.setTrackLinking(True)
g.setTrajectory()
g.profileEnable(True)
rows = []
for t in range(args.warmup + args.steps):
    g.pushBackDevice(left[t % P].data_ptr(), right[t % P].data_ptr(), isz, dims)
    if t == 0:
        continue
    g.matchFeatures(pkg.METHOD_QUAD)
    tr, ok, _ = g.estimateMotion(e, rand3)
    counts = g.motionInliers(e, tr, ok.astype(np.int32))
    g.synchronize()
    g.profileReset()
    _, _, nupd_plain, _ = g.refitMotion(e, reclassify=False)
    tr2, ok2, nupd, used, counts2 = lrf.groupRefitMotionLandmarks(g, e, rp, reclassify=True)
    plain_ms, prior_ms, fit_ms = (g.profileRead(k)[0] for k in ("motion_refit", "refit_prior", "refit_prior_fit"))
    g.trajectory()
    g.scenePointsWorld(e, pkg.SceneParams.default(frame=1))
    g.landmarks(lp)
    if t < args.warmup:
        continue
    k = int(counts.sum())
    row = {"step": t, "inliers": k, "n_used": int(used.sum()), "used_share": round(int(used.sum()) / max(k, 1), 4),
           "motion_refit_ms": round(plain_ms, 4), "refit_prior_ms": round(prior_ms, 4), "refit_prior_fit_ms": round(fit_ms, 4),
           "n_updates_plain_max": int(nupd_plain.max()), "n_updates_max": int(nupd.max()),
           "n_updates_plain_mean": round(float(nupd_plain[nupd_plain > 0].mean()) if (nupd_plain > 0).any() else 0.0, 2),
           "n_updates_mean": round(float(nupd[nupd > 0].mean()) if (nupd > 0).any() else 0.0, 2),
           "ok_plain": int((nupd_plain > 0).sum()), "ok_out": int(ok2.sum()),
           "bytes_per_update": 64 * k, "copy_ms": round(copy_ms(max(64 * k, 1)), 4)}
    # a launch lasts as long as its slowest list
    row["plain_ms_per_update"] = round(plain_ms / max(float(nupd_plain.max()), 1.0), 4)
    row["fit_ms_per_update"] = round(fit_ms / max(float(nupd.max()), 1.0), 4)
    rows.append(row)
    print(json.dumps(row), flush=True)
g.close()
med = lambda f: round(float(np.median([f(x) for x in rows])), 6)  # noqa: E731
print(json.dumps({"metric": "landmark_refit_device_time", "streams": S, "W": W, "H": H, "steps": len(rows),
                  **{k: med(lambda x, k=k: x[k]) for k in ("inliers", "used_share", "motion_refit_ms", "refit_prior_ms", "refit_prior_fit_ms",
                                                           "n_updates_plain_mean", "n_updates_mean", "plain_ms_per_update", "fit_ms_per_update",
                                                           "bytes_per_update", "copy_ms")}}), flush=True)
