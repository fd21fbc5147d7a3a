"""Helper of test_group_paths.py::test_subbatch_device_buffer (run as a script: `python tests/group_device_case.py`).

vh_group_push_back_device from a torch buffer whose stream stride is larger than one image (H * bpl + a gap), as a
caller with padded per-stream slots would pass it: every stream's sets and matches after every step equal the
oracle's, and each push takes the number of detection launches the sub-batch rule gives."""
import os
import sys

import numpy as np
import torch  # before the product library: both then share torch's HIP runtime

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from test_group_paths import Frames, check_group, check_launches, detect_launches, group_frames  # noqa: E402
import __graft_entry__ as entry  # noqa: E402  (conftest put the repository root on sys.path)


def main() -> None:
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(0)
    pkg, ob = entry.load_package(), entry.load_oracle()
    oracle = ob.Oracle()
    S, W, H, T = 5, 320, 160, 3
    po = ob.Params.default()
    seqs, dims = group_frames(pkg, S, W, H, None, True, T, 900)
    fr = Frames(oracle, po, dims, seqs)
    isz = H * dims[2]
    stride = isz + 4608  # a gap after every image
    host = np.full((T, 2, S, stride), 0xA5, np.uint8)
    for t in range(T):
        for c in range(2):
            host[t, c, :, :isz] = fr.stack(t, c).reshape(S, isz)
    frames = torch.from_numpy(host).to(dev)
    torch.cuda.synchronize()
    per_push = detect_launches(S, 2, W, H, po.nms_n, 0)
    g = pkg.StreamGroup(S, pkg.Params.default())
    g.profileEnable()
    methods = [2, 1]
    for t in range(T):
        g.pushBackDevice(frames[t, 0].data_ptr(), frames[t, 1].data_ptr(), stride, dims, False)
        if t == 0:
            check_group(pkg, oracle, po, g, fr, None, 0, None)
        else:
            g.matchFeatures(methods[t - 1])
            _, nmatch = check_group(pkg, oracle, po, g, fr, t - 1, t, methods[t - 1])
            assert nmatch > 50 * S, nmatch
        check_launches(g, t + 1, per_push, False)
    g.close()
    print("group-device ok", per_push, "launches per push")


if __name__ == "__main__":
    main()
