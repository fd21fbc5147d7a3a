#!/usr/bin/env python3
"""Records tests/golden/gain_reference.npz: a random image, windows on it and what the REFERENCE's own Matcher::mean
(src/matcher.cpp:347-354, the helper of getGain) returns for each.  Test infrastructure: compiles
tools/gain_ref_harness.cpp against the reference tree (oracle.binding.REFERENCE_ROOT) into the ignored oracle/_ref/ and
runs it; only the data is kept.

The windows: every extent 1 x 1 .. 7 x 7 seven times at random places (343 windows, the sizes a clamped getGain window
can have), and six large ones (up to the whole image) whose float sums pass 2^16 -- still exact integers, below 2^24."""
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import binding as ob  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "gain_reference.npz")
W, H, BPL = 200, 120, 208


def windows(rng):
    win = []
    for w in range(1, 8):
        for h in range(1, 8):
            for _ in range(7):
                u, v = int(rng.integers(0, W - w + 1)), int(rng.integers(0, H - h + 1))
                win.append((u, u + w - 1, v, v + h - 1))
    win += [(0, W - 1, 0, H - 1), (0, 63, 0, 63), (17, 180, 5, 99), (0, W - 1, 60, 60), (199, 199, 0, H - 1), (30, 129, 10, 109)]
    return np.array(win, np.int32)


def main():
    rng = np.random.default_rng(347)
    img = rng.integers(0, 256, (H, BPL), dtype=np.uint8)
    win = windows(rng)
    ref_dir = os.path.join(ROOT, "oracle", "_ref")
    os.makedirs(ref_dir, exist_ok=True)
    exe = os.path.join(ref_dir, "gain_ref_harness")
    src = os.path.join(ob.REFERENCE_ROOT, "src")
    units = ["filter", "myComputeFeature", "myMatch", "remove_outliers", "delaunator", "matrix"]
    subprocess.check_call(["g++", "-std=gnu++11", "-O2", "-msse3", "-w", "-I" + src, os.path.join(ROOT, "tools", "gain_ref_harness.cpp")]
                          + [os.path.join(src, u + ".cpp") for u in units] + ["-o", exe])
    din, dout = os.path.join(ref_dir, "gain_windows.bin"), os.path.join(ref_dir, "gain_means.bin")
    with open(din, "wb") as fh:
        fh.write(np.array([W, H, BPL], np.int32).tobytes())
        fh.write(img.tobytes())
        fh.write(np.int32(len(win)).tobytes())
        fh.write(win.tobytes())
    subprocess.check_call([exe, din, dout])
    means = np.fromfile(dout, np.float32)
    assert len(means) == len(win)
    np.savez_compressed(OUT, dims=np.array([W, H, BPL], np.int32), image=img, windows=win, means=means)
    print(f"{OUT}: {len(win)} windows, {os.path.getsize(OUT)} bytes")


if __name__ == "__main__":
    main()
