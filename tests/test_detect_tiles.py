"""detect_nms_fast<N> at the edges of its tile grid: byte parity of compute_features with the
oracle for nms_n = 1..4 where the last tile column / row holds 1 or TBX-1 / TBY-1 blocks, with
the candidate queues at their fullest (nms_tau = 0), on ties in scan order and on a full KITTI
frame.  Also checks that image rows end where the staged 16-byte chunks are clamped (stride ==
width, so the last chunk of a row reads into the next row)."""
import numpy as np
import pytest

TBX, TBY, MARGIN = 32, 8, 7  # DetTile<N> blocks per tile; VH_MARGIN


def extent_for(blocks, n):
    """Smallest image extent with `blocks` NMS blocks along it (engine.hip block_count)."""
    return 2 * n + 2 * MARGIN + (blocks - 1) * (n + 1) + 1


def parity(pkg, ob, oracle, img, dims, n, tau, min_feats):
    p, po = pkg.Params.default(nms_n=n, nms_tau=tau), ob.Params.default(nms_n=n, nms_tau=tau)
    got = pkg.compute_features(p, img, dims)
    want = oracle.compute_features(po, img, dims)
    assert len(want[1]) > min_feats, (n, dims, tau, len(want[1]))
    # [0]: the sparse pass (nms_n_sparse = 4n, max(n, 10) once 4n > 10: detect_nms_fast<4> at n = 1), [1]: the dense one
    assert np.array_equal(got[0], want[0]), (n, dims, tau, "sparse")
    assert np.array_equal(got[1], want[1]), (n, dims, tau, "dense")


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 2, 3, 4])
@pytest.mark.parametrize("bx_last,by_last", [(1, 1), (TBX - 1, TBY - 1), (1, TBY - 1), (TBX - 1, 1)])
def test_partial_edge_tiles(n, bx_last, by_last, pkg, ob, oracle, gpu):
    W = extent_for(TBX + bx_last, n)
    H = extent_for(2 * TBY + by_last, n)
    dims = [W, H, pkg.synth.bytes_per_line(W)]
    img = pkg.synth.frame(W, H, 2, 1, 3, 2, 70 + n, bpl=dims[2])
    parity(pkg, ob, oracle, img, dims, n, 30, 50)


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 2, 3, 4])
def test_full_queues_tau0(n, pkg, ob, oracle, gpu):
    """nms_tau = 0 on a textured image: nearly every block extremum is queued."""
    W, H = 513, 203
    dims = [W, H, pkg.synth.bytes_per_line(W)]
    img = pkg.synth.frame(W, H, 1, 2, 1, 3, 90 + n, bpl=dims[2])
    parity(pkg, ob, oracle, img, dims, n, 0, 1000)


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 2, 3, 4])
def test_ties_and_tight_stride(n, pkg, ob, oracle, gpu):
    """Flat and saturated patches (equal responses: the first position in scan order wins), on
    an image whose stride equals its width (a multiple of 4, so the fast kernel takes it)."""
    W, H = 600, 260
    dims = [W, H, W]
    img = pkg.synth.frame(W, H, 3, 1, 2, 3, 110 + n, bpl=W)
    img = img.copy()
    img[40:90, 100:260] = 255
    img[150:200, 300:520] = 17
    img[:, W - 30:] = 0
    img[H - 20:, :] = 255
    parity(pkg, ob, oracle, img, dims, n, 20, 200)


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 2, 3, 4])
def test_kitti_frame(n, pkg, ob, oracle, gpu):
    W, H = 1241, 376
    dims = [W, H, pkg.synth.bytes_per_line(W)]
    img = pkg.synth.frame(W, H, 4, 0, 4, 1, 130 + n, bpl=dims[2])
    parity(pkg, ob, oracle, img, dims, n, 50, 500)
