// vh_recon.h -- what engine_recon.hip (host) and kernels_recon.hip (device) share: the per-frame table and the launch.
#ifndef VH_RECON_H
#define VH_RECON_H

#include <hip/hip_runtime.h>
#include <stdint.h>

// One record per frame of the drive, built on the host exactly as Reconstruction's constructor, setCalibration and
// update build their three vectors (src/reconstruction.cpp:27-70):
//   [0, 12)   P_total[frame]       3 x 4, row-major
//   [12, 28)  Tr_inv_total[frame]  4 x 4, row-major
//   [28, 31)  Tr_total[frame].val[0..2][3]: the camera centre (all that pointDistance and rayAngle read of it)
//   [31]      unused
#define VH_RECON_FRAME_DOUBLES 32
#define VH_RECON_P 0
#define VH_RECON_TINV 12
#define VH_RECON_C 28

struct vh_recon_params;
// Lane i of the launch solves track order[i]; every output goes to the track's own index.
// road = rows 1 of Tr_cam_road (src/reconstruction.cpp:45-53): the only row pointType reads.
void vh_launch_recon(const vh_recon_params &r, const double road[4], const double *frames, int32_t n_tracks, const int32_t *order,
                     const int32_t *first_frame, const int32_t *offsets, const float *pixels, float *points, int32_t *status,
                     double *metrics, hipStream_t st);

#endif
