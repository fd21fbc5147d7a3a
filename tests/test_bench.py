"""bench.py's plain line and --dump-outputs: a plain run times exactly --steps steps and carries the headline keys;
the dumped outputs of the last timed step are float arrays and identical from run to run with the same arguments."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

ARGS = ["--steps", "3", "--warmup", "2", "--streams", "8", "--frames", "4"]


def run_bench(extra, tmp_path):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1"] + ARGS + extra, cwd=tmp_path,
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    assert r.returncode == 0, r.stderr.decode()[-3000:]
    lines = r.stdout.decode().splitlines()
    assert len(lines) == 1, r.stdout.decode()
    return json.loads(lines[0])


def test_bench_options_are_documented():
    out = subprocess.check_output([sys.executable, os.path.join(ROOT, "bench.py"), "--help"], timeout=60).decode()
    assert "--full" in out and "--dump-outputs" in out


@pytest.mark.gpu
def test_bench_plain_line_and_dump_outputs(tmp_path, pkg, gpu):
    dumps = []
    for i in range(2):
        d = tmp_path / f"dump{i}"
        line = run_bench(["--dump-outputs", str(d)], tmp_path)
        for key in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
            assert key in line, key
        assert line["unit"] == "pairs/s" and line["higher_is_better"] is True and line["dtype"] == "u8"
        assert line["steps"] == 3 and line["blocks"]["count"] == 1 and line["blocks"]["steps_each"] == 3
        assert line["ms_per_step"] > 0 and line["value"] == pytest.approx(8 * 3 / (line["ms_per_step"] * 3e-3))
        assert "cpu_baseline" not in line and "roofline" not in line  # what only --full measures
        files = sorted(os.listdir(d))
        assert files == sorted(n + ".npy" for n in ("feature_counts", "match_counts", "sample_streams", "matches",
                                                    "features_left", "features_right")), files
        arrays = {f: np.load(d / f) for f in files}
        assert all(a.dtype in (np.float32, np.float64) for a in arrays.values())
        assert sum(a.nbytes for a in arrays.values()) <= 64 << 20
        nm = arrays["match_counts.npy"]
        assert nm.shape == (8,) and nm.sum() > 0
        sample = arrays["sample_streams.npy"].astype(int)
        assert len(sample) == 8 and arrays["matches.npy"].shape == (int(nm[sample].sum()), 12)
        nf = arrays["feature_counts.npy"]
        assert arrays["features_left.npy"].shape == (int(nf[sample, 2].sum()), 12)
        assert arrays["features_right.npy"].shape == (int(nf[sample, 3].sum()), 12)
        dumps.append(arrays)
    for f in dumps[0]:
        assert dumps[0][f].tobytes() == dumps[1][f].tobytes(), f
