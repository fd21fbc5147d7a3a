#!/usr/bin/env python3
"""Kernel time and tracks/s of vh_reconstruct_tracks on a KITTI-like batch, against the host restatement on one core.

The batch: `--lists` updates x `--tracks` lost tracks each (default 256 x 9000), track lengths drawn from the distribution
of the lost tracks of tests/golden/reconstruction_reference.npz, pixel-rounded projections of static points along a
forward drive of `--frames` frames.  Timing: the kernel's own HIP events (vh_reconstruct_last_kernel_ms: transfers
excluded), `--warmup` untimed calls, then `--blocks` blocks of `--reps` calls; the figure is the median of the block
means, with the spread of the blocks beside it.  Baseline: tests/reconstruction_oracle.py's solve_track on `--sample`
tracks of the same batch on one core, scaled to the batch; only the ratio is meaningful (the restatement is Python).
Prints one JSON line."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import __graft_entry__ as entry  # noqa: E402
import recon_cases as rc  # noqa: E402
import reconstruction_oracle as ro  # noqa: E402


def fixture_lengths():
    z = np.load(os.path.join(ROOT, "tests", "golden", "reconstruction_reference.npz"))
    r = ro.Reconstruction(None)
    r.setCalibration(*z["calibration"])
    pos = 0
    for k, n in enumerate(z["list_counts"]):
        r.update(z["matches"][pos:pos + n], z["Trs"][k], solve=False)
        pos += n
    return np.array([len(px) for _, px in r.lost_log])


def batch(n_tracks, n_frames, lengths, seed=1):
    rng = np.random.default_rng(seed)
    centres = np.cumsum(np.column_stack([rng.normal(0.01, 0.005, n_frames), rng.normal(0, 0.003, n_frames), 0.8 + rng.normal(0, 0.03, n_frames)]), 0)
    yaw = np.cumsum(rng.normal(-0.003, 0.002, n_frames))
    poses = [rc.pose(0.0, yaw[k], 0.0, centres[k]) for k in range(n_frames)]
    R = np.stack([p[:3, :3] for p in poses]); t = np.stack([p[:3, 3] for p in poses])
    length = np.minimum(rng.choice(lengths, n_tracks), n_frames)
    first = rng.integers(0, n_frames - length + 1).astype(np.int32)
    Z = rng.uniform(4, 45, n_tracks)
    Pc = np.column_stack([rng.uniform(-0.5, 0.5, n_tracks) * Z * 0.8, rng.uniform(-0.25, 0.2, n_tracks) * Z, Z])
    Pw = np.einsum("nji,nj->ni", R[first], Pc - t[first])   # R^T (Pc - t)
    offsets = np.zeros(n_tracks + 1, np.int32)
    offsets[1:] = np.cumsum(length)
    tid = np.repeat(np.arange(n_tracks), length)
    frame = first[tid] + (np.arange(offsets[-1]) - offsets[tid])
    q = np.einsum("nij,nj->ni", R[frame], Pw[tid]) + t[frame]
    px = np.column_stack([np.round(rc.F * q[:, 0] / q[:, 2] + rc.CU), np.round(rc.F * q[:, 1] / q[:, 2] + rc.CV)]).astype(np.float32)
    return rc.trs_of(poses), first, offsets, px


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lists", type=int, default=256); ap.add_argument("--tracks", type=int, default=9000)
    ap.add_argument("--frames", type=int, default=257); ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--blocks", type=int, default=7); ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--sample", type=int, default=2000)
    a = ap.parse_args()
    pkg, ob = entry.load_package(), entry.load_oracle()
    lengths = fixture_lengths()
    n = a.lists * a.tracks
    Trs, first, offsets, px = batch(n, a.frames, lengths)
    r = pkg.ReconParams.default(f=rc.F, cu=rc.CU, cv=rc.CV)
    for _ in range(a.warmup):
        pts, st, _ = pkg.reconstruct_tracks(r, Trs, first, offsets, px, metrics=False)
    blocks = []
    for _ in range(a.blocks):
        ms = []
        for _ in range(a.reps):
            pkg.reconstruct_tracks(r, Trs, first, offsets, px, metrics=False)
            ms.append(pkg.reconstruct_last_kernel_ms())
        blocks.append(float(np.mean(ms)))
    t0 = time.perf_counter()
    pkg.reconstruct_tracks(r, Trs, first, offsets, px, metrics=False)
    call_ms = (time.perf_counter() - t0) * 1e3
    kernel_ms = float(np.median(blocks))
    # the restatement on a sample, one core
    o = ob.Oracle()
    tab = ro.Tables(rc.F, rc.CU, rc.CV)
    for T in Trs:
        tab.push(T)
    idx = np.random.default_rng(2).choice(n, min(a.sample, n), replace=False)
    t0 = time.perf_counter()
    want = [ro.solve_track(tab, o.svd, int(first[i]), px[offsets[i]:offsets[i + 1]]) for i in idx]
    host_s = (time.perf_counter() - t0) * n / len(idx)
    same = all(pts[i].tobytes() == w[0].tobytes() and st[i] == w[1] for i, w in zip(idx, want))
    print(json.dumps(dict(tracks=n, lists=a.lists, frames=a.frames, mean_length=round(float(offsets[-1]) / n, 2),
                          kernel_ms=round(kernel_ms, 3), kernel_ms_blocks=[round(b, 3) for b in blocks],
                          tracks_per_s=round(n / kernel_ms * 1e3), warmup=a.warmup, blocks=a.blocks, reps=a.reps, call_ms=round(call_ms, 1),
                          accepted=int((st == 0).sum()), status_counts=np.bincount(st, minlength=6).tolist(),
                          host_restatement_s_one_core=round(host_s, 1), kernel_over_host=round(host_s * 1e3 / kernel_ms),
                          sample_equal=bool(same))))


if __name__ == "__main__":
    main()
