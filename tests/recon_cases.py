"""Inputs of tests/test_reconstruction.py (pure numpy, deterministic): a pool of tracks over a 41-frame drive, and a second
drive with one constructed track per outcome of Reconstruction::update (include/viso_hip.h: VH_RECON_*)."""
import math

import numpy as np

from egomotion_scene import KITTI, rot

F, CU, CV = KITTI["f"], KITTI["cu"], KITTI["cv"]
W, H = 1241, 376


def pose(rx=0.0, ry=0.0, rz=0.0, centre=(0.0, 0.0, 0.0)):
    """world -> camera for a camera at `centre` (world) turned by rot(rx, ry, rz)."""
    T = np.eye(4)
    T[:3, :3] = rot(rx, ry, rz)
    T[:3, 3] = -T[:3, :3] @ np.array(centre, float)
    return T


def trs_of(poses):
    """Tr of update k = motion frame k -> k + 1 (x_{k+1} = Tr x_k)."""
    return np.array([poses[k + 1] @ np.linalg.inv(poses[k]) for k in range(len(poses) - 1)])


def project(T, Pw):
    q = T @ np.append(Pw, 1.0)
    return F * q[0] / q[2] + CU, F * q[1] / q[2] + CV, q[2]


def track_of(poses, Pw, first, length, rng=None, noise=0.0, rounded=True):
    px = []
    for k in range(first, first + length):
        u, v, _ = project(poses[k], Pw)
        if rng is not None and noise:
            u, v = u + rng.normal(0, noise), v + rng.normal(0, noise)
        px.append((np.round(u), np.round(v)) if rounded else (u, v))
    return first, np.array(px, np.float32)


POOL_FRAMES = 41
POOL_LENGTHS = (2, 3, 7, 40)


def pool(n=257, seed=5):
    """-> (Trs [40, 4, 4], [(first_frame, pixels [len, 2] float32)] * n): lengths 2, 3, 7, 40 in turn, pixel-rounded
    positions of static points seen from a camera moving 0.3 m per frame with a slight turn.  Track 0 starts at frame 0,
    track 1 ends at the last frame, and so does every track of 40 frames that starts at frame 1 (the others start at 0)."""
    rng = np.random.default_rng(seed)
    poses, c, yaw = [], np.zeros(3), 0.0
    for k in range(POOL_FRAMES):
        poses.append(pose(rng.normal(0, 0.001), yaw, rng.normal(0, 0.001), c))
        yaw += -0.002 + rng.normal(0, 0.0005)
        c = c + np.array([rng.normal(0.005, 0.003), rng.normal(0, 0.002), 0.3 + rng.normal(0, 0.01)])
    tracks = []
    while len(tracks) < n:
        i = len(tracks)
        length = POOL_LENGTHS[i % 4]
        if i == 0:
            first = 0
        elif i == 1 or length == 40:
            first = POOL_FRAMES - length - (1 if length == 40 and i % 8 == 3 else 0)
        else:
            first = int(rng.integers(0, POOL_FRAMES - length + 1))
        Z = rng.uniform(14, 40) if length == 40 else rng.uniform(4, 40)
        Pc = np.array([rng.uniform(-0.5, 0.5) * Z * 0.8, rng.uniform(-0.25, 0.2) * Z, Z, 1.0])
        Pw = (np.linalg.inv(poses[first]) @ Pc)[:3]
        f, px = track_of(poses, Pw, first, length)
        if np.all((px[:, 0] >= 0) & (px[:, 0] < W) & (px[:, 1] >= 0) & (px[:, 1] < H)):
            tracks.append((f, px))
    return trs_of(poses), tracks


STATUS_NAMES = ("zero_motion", "infinity", "behind", "below_road", "road", "obstacle", "c_zero", "not_converged", "far", "narrow", "short")
#: seed of the noisy far track that is still moving after 22 updates (found with the restatement; the test asserts it)
NOT_CONVERGED_SEED = 8


def status_poses(theta):
    """Frames 0, 1: the same pose; 2: one metre to the side; 3 .. 10: 0.8 m forward each; 11: 0.8 m on and turned by theta
    about the vertical axis; 12: 0.8 m on, turned back."""
    poses = [pose(), pose(), pose(centre=(1, 0, 0))]
    for k in range(3, 11):
        poses.append(pose(centre=(1, 0, 0.8 * (k - 2))))
    poses.append(pose(ry=theta, centre=(1, 0, 0.8 * 9)))
    poses.append(pose(centre=(1, 0, 0.8 * 10)))
    return poses


C_ZERO_POINT = np.array([1.0 + 3.0, 0.0, 6.4 + 8.0])   # seen from frames 10, 11, 12


def c_zero_theta(p):
    """The turn of frame 11 that puts point p into its principal plane: row 2 of rot(0, t, 0) is (-sin t, 0, cos t)."""
    d = np.asarray(p, float) - np.array([1, 0, 0.8 * 9])
    return math.atan2(d[2], d[0])


def status_tracks(poses, not_converged_seed=NOT_CONVERGED_SEED):
    """name -> (first_frame, pixels)."""
    centre = lambda k: np.array([1.0, 0.0, 0.8 * (k - 2)])  # noqa: E731  (frames 2 .. 10)
    t = {}
    t["zero_motion"] = (0, np.array([(700, 200), (700, 200)], np.float32))
    t["infinity"] = (1, np.array([(700, 200), (700, 200)], np.float32))          # parallel rays one metre apart
    f, px = track_of(poses, centre(3) + (2, -1.5, 10), 3, 2)
    t["behind"] = (3, px[::-1].copy())                                          # the flow of a point BEHIND the camera
    t["below_road"] = track_of(poses, centre(3) + (1.5, 3.0, 10), 3, 5)
    t["road"] = track_of(poses, centre(3) + (1.5, 1.0, 10), 3, 5)
    t["obstacle"] = track_of(poses, centre(3) + (2, -1.5, 10), 3, 5)
    a, _, l = (project(poses[k], C_ZERO_POINT) for k in (10, 11, 12))
    t["c_zero"] = (10, np.array([a[:2], (600, 190), l[:2]], np.float32))
    rng = np.random.default_rng(not_converged_seed)
    # (hundreds of metres away and high above the road: the step along the ray stays above 1e-5 while float steps of p are 3e-5)
    Pw = centre(2) + (rng.uniform(-30, 30), rng.uniform(-60, -36), rng.uniform(210, 390))
    t["not_converged"] = track_of(poses, Pw, 2, 9, rng, 0.3, rounded=False)
    t["far"] = track_of(poses, centre(2) + (6, -2, 38), 2, 9)
    t["narrow"] = track_of(poses, centre(3) + (0.05, -1.2, 12), 3, 2, rounded=False)
    t["short"] = (5, np.array([(640, 190)], np.float32))
    return t


def flatten(tracks):
    first = np.array([f for f, _ in tracks], np.int32)
    offsets = np.zeros(len(tracks) + 1, np.int32)
    offsets[1:] = np.cumsum([len(px) for _, px in tracks])
    return first, offsets, np.concatenate([px for _, px in tracks]).astype(np.float32).reshape(-1, 2)
