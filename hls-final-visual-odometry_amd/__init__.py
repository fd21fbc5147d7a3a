"""viso-hip: MI355X-native feature detection + matching behind the libviso2
`Matcher` surface of Chang-Tun-Yu/HLS-final-Visual-Odometry.

This package is the thin Python host mirror over the C ABI of
`libviso_hip.so` (include/viso_hip.h).  All compute happens in the hand-written
HIP kernels under csrc/; there is no CPU or PyTorch fallback: importing works
without a GPU (so the library and its exported symbols can be checked), any
compute call without a usable GPU raises `VisoHipError(VH_ERR_NO_DEVICE)`, and a
missing shared library raises at import.

The directory name contains hyphens, so load it with
`__graft_entry__.load_package()` (importlib under the name
`hls_final_visual_odometry_amd`).

Three modules hold the code, and this one re-exports all of them: _abi (constants, structures, dtypes, the table of the
ABI's prototypes, loading and building the library, the call idioms every entry shares), _handles (Matcher, StreamGroup,
SequenceGroup) and _stateless (the functions that take their inputs and return their results in one call).
"""
from . import synth  # noqa: F401  (synthetic KITTI-shaped frames)
from ._abi import *  # noqa: F401,F403
from ._abi import _check, _dims, _feat, _lib, _models, _packed, _ptr, _rule, _scene_Tw, _traj_S0, _traj_T0  # noqa: F401
from ._handles import Matcher, SequenceGroup, StreamGroup  # noqa: F401
from ._stateless import *  # noqa: F401,F403
from ._stateless import _scene_points  # noqa: F401

