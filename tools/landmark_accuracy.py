#!/usr/bin/env python3
"""What fusing buys, on the restatement alone (tests/landmark_oracle.py, CPU): a static cloud seen
by a stereo camera (KITTI calibration) that moves forward, every point observed in each of `frames` frames with a depth
error drawn from N(0, (noise_px * sigma_z)^2) along its viewing ray -- sigma_z = z^2 / (f * base), the depth error per pixel
of disparity error, as vh_scene_point carries it -- and handed over in the world frame.  Prints one JSON line: the median
distance to the truth of the last frame's scene point and of the fused landmark.
  python tools/landmark_accuracy.py [--points 2000] [--frames 10] [--noise-px 0.5]"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import landmark_oracle as lo  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--points", type=int, default=2000)
ap.add_argument("--frames", type=int, default=10)
ap.add_argument("--noise-px", type=float, default=0.5)
ap.add_argument("--seed", type=int, default=1)
args = ap.parse_args()
f, base = 721.5, 0.54
rng = np.random.default_rng(args.seed)
n = args.points
world = np.stack([rng.uniform(-15, 15, n), rng.uniform(-2, 2, n), rng.uniform(15, 60, n)], 1)
lp = lo.params(min_obs=1, max_missed=-1)
state, lm, single = None, None, None
for t in range(args.frames):
    cam = np.array([0.0, 0.0, 0.8 * t])                     # the camera's position: 0.8 m forward per frame
    rel = world - cam
    sigma = rel[:, 2] ** 2 / (f * base)
    noisy = rel * (1.0 + (rng.normal(0, args.noise_px, n) * sigma / rel[:, 2]))[:, None] + cam
    trk = np.zeros(n, lo.TRACK)
    trk["prev"] = np.arange(n) if t else -1
    trk["age"] = t + 1
    pts = np.zeros(n, lo.POINT)
    pts["x"], pts["y"], pts["z"] = noisy.T
    pts["sigma_z"] = sigma
    pts["src_pos"] = np.arange(n)
    lm, state = lo.update(trk, pts, state, lp)
    single = noisy
fused = np.stack([lm["x"], lm["y"], lm["z"]], 1).astype(np.float64)
err_single = np.linalg.norm(single - world, axis=1)
err_fused = np.linalg.norm(fused - world, axis=1)
print(json.dumps({"metric": "landmark_accuracy_oracle", "points": n, "frames": args.frames, "noise_px": args.noise_px,
                  "median_err_last_scene_point_m": round(float(np.median(err_single)), 4),
                  "median_err_landmark_m": round(float(np.median(err_fused)), 4),
                  "ratio": round(float(np.median(err_single) / np.median(err_fused)), 3),
                  "median_sigma_reported_m": round(float(np.median(lm["sigma"])), 4)}))
