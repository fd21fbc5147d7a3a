"""Helper of test_multistage_scale.py::test_child_device_images_on_a_producer_stream (run as a script).

tests/stream_order_case.py with multi-stage matching on.  The images are produced on a torch side stream and the group
is only told the stream; after vh_group_push_back_device the producer waits with vh_group_stream_wait_images and
overwrites the buffers on its stream.  The SPARSE detection reads the images after the dense one, so the wait must cover
it: the sparse list (and the pass-2 list) must equal the restatement's for the original images.  Every wait is on the
device and nothing is timed: a missing wait gives a wrong list, not a fault."""
import os
import sys

import numpy as np
import torch  # before the product library: both then share torch's HIP runtime

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import __graft_entry__ as entry  # noqa: E402
import multistage_oracle as mo  # noqa: E402
from test_multistage import check_not_vacuous, images_of, scene  # noqa: E402


def main() -> None:
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(0)
    pkg, ob = entry.load_package(), entry.load_oracle()
    oracle = ob.Oracle()
    S, W, H, T = 3, 1241, 376, 3
    bpl = pkg.synth.bytes_per_line(W)
    dims = [W, H, bpl]
    fr = scene(pkg, T + S - 1, W, H, seed=29, disparity=8, blur=3)
    host = np.zeros((T, 2, S, H, bpl), np.uint8)
    for s in range(S):
        for t in range(T):
            host[t, 0, s], host[t, 1, s] = fr[s + t]
    frames = torch.from_numpy(host).to(dev)
    p, po = pkg.Params.default(multi_stage=1), ob.Params.default(multi_stage=1)
    side = torch.cuda.Stream(device=dev)
    handle = side.cuda_stream
    live = torch.zeros((2, S, H, bpl), dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    g = pkg.StreamGroup(S, p)
    g.setMultiStageMatching(True)
    g.setStream(handle)
    for t in range(T):
        with torch.cuda.stream(side):
            torch.cuda._sleep(20_000_000)  # the copy below lags far behind the host
            live.copy_(frames[t])
        g.pushBackDevice(live[0].data_ptr(), live[1].data_ptr(), H * bpl, dims, False)
        with torch.cuda.stream(side):
            g.streamWaitImages(handle)     # both detections of this push have consumed `live` ...
            live.fill_(90)                 # ... before the producer wipes it
        if t:
            method = (2, 0)[t % 2]
            g.matchFeatures(method)
            for s in range(S):
                r = mo.multistage(ob, oracle, po, dims, method, images_of(method, fr[s + t - 1], fr[s + t]), fast=True)
                check_not_vacuous(po, method, r)
                assert g.getSparseMatches(s).tobytes() == r["sparse"].tobytes(), (t, s, "sparse")
                assert g.getMatches(s).tobytes() == r["dense"].tobytes(), (t, s, "dense")
    g.setStream(None)
    g.close()
    print("multistage stream-order ok")


if __name__ == "__main__":
    main()
