/* viso_hip_lmk_refit.h -- C ABI of libviso_hip.so, the motion refit on the landmarks.  An extension header beside
 * viso_hip.h, whose types it uses: the same library exports these entries, the same error codes and conventions hold. */
#ifndef VISO_HIP_LMK_REFIT_H
#define VISO_HIP_LMK_REFIT_H
#include "viso_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- motion refit on the landmarks: fused track points as the 3-d prior (csrc/kernels_lmk_refit.hip) ----
 * vh_refit_motion's Gauss-Newton loop with one difference: the 3-d point of a record whose track has a landmark is the
 * landmark -- the track's position averaged over every step that saw it -- brought into the previous camera's frame, in the
 * place of the point triangulated from the previous pair alone.  The rule has one copy, csrc/vh_refit_prior.h; all
 * arithmetic in double, every product and sum rounded on its own, sums added left to right.  Record i of a quad list,
 * p = prev_pos[i] (vh_track.prev of the record), the predecessor list's states st[0 .. n_prev), Tw_prev (row-major 4x4, the
 * previous camera to the world: what vh_traj_pose.Tw_prev holds for the pair):
 *   1. own = the point of the previous pair as vh_refit_motion forms it (max(u1p - u2p, 0.0001f)).
 *   2. the landmark point exists iff 0 <= p < n_prev (a p outside is never dereferenced) and st[p].n_obs >= min_obs:
 *      m = (swx / sw, swy / sw, swz / sw); d = m - (Tw[3], Tw[7], Tw[11]); L = R^T d with R the upper-left 3x3 of Tw_prev:
 *      L.x = R[0][0]*d.x + R[1][0]*d.y + R[2][0]*d.z, and so on.
 *   3. reason, the first that applies: 1 p outside the predecessor list or no predecessor; 2 n_obs < min_obs; 3 sw <= 0, or a
 *      value of m or L not finite; 4 L.z <= 0; 5 max_depth_ratio > 1 and L.z / own.Z outside [1 / max_depth_ratio,
 *      max_depth_ratio] or not finite; else 0.
 *   4. reason 0: (X, Y, Z) = L, source = 1.  Otherwise (X, Y, Z) = own, source = 0.
 * The fit is vh_refit_motion's contract word for word (updateParameters(.., 1, 1e-8), at most 102 updates, ok_in == 0 or
 * fewer than six records refused, reweighting read) over the points (X, Y, Z); the order of the sums is the same function
 * of the list's length, so a list whose records all fall back gives vh_refit_motion's bytes.  n_used[s]: the records of
 * list s with source == 1.  The same bytes from run to run, alone or among other lists, stateless and on a handle.
 * Not done: the covariance under prior points, the stage inside the device post chain, a mono form, sequence handles,
 * rows weighted by the landmark's sigma. */
typedef struct vh_refit_prior {      /* 32 bytes, one per record */
  double  X, Y, Z;                   /* the point the fit used, in the previous left camera's frame */
  int32_t source;                    /* 1: the landmark, 0: the record's own triangulation */
  int32_t reason;                    /* 0, or why the record fell back (1..5 above) */
} vh_refit_prior;
typedef struct vh_lmk_refit_params {
  int32_t min_obs;                   /* a landmark is used from this many accepted observations on; >= 1 */
  int32_t reserved;                  /* 0 */
  double  max_depth_ratio;           /* > 1: the gate on L.z / own.Z; else none */
} vh_lmk_refit_params;
void vh_default_lmk_refit_params(vh_lmk_refit_params *rp);   /* 2, 0, 0 */
/* Stateless, host pointers.  Lists, offsets and limits as vh_refit_motion's; prev_pos and prior (nullable: not wanted) are
 * indexed like pm; prev / prev_offsets as in vh_landmarks_update (both NULL: no list has a predecessor); Tw_prev
 * [n_sets][16]; tr_in / ok_in / tr_out / ok_out / n_updates as vh_refit_motion's; n_used [n_sets].
 * VH_ERR_INVALID_ARG: null pointers, min_obs < 1, reserved != 0, only one of prev / prev_offsets, what the offsets checks
 * refuse.  n_sets == 0 or no records at all: VH_OK (outputs zero), nothing is launched and no device is needed. */
int32_t vh_refit_motion_landmarks(const vh_ego_params *e, const vh_lmk_refit_params *rp, int32_t device, int32_t n_sets,
                                  const vh_p_match *pm, const int32_t *offsets, const int32_t *prev_pos,
                                  const vh_landmark_state *prev, const int32_t *prev_offsets, const double *Tw_prev,
                                  const double *tr_in, const int32_t *ok_in, double *tr_out, int32_t *ok_out, int32_t *n_updates,
                                  int32_t *n_used, vh_refit_prior *prior);
/* On a handle: the compacted inlier lists of the current STEREO classification, from the tr / ok it was made under, as
 * vh_group_refit_motion; prev_pos is vh_track.prev of the record in the current tracked list (through the inliers'
 * src_pos); the predecessor states are what the last vh_group_landmarks call wrote for the predecessor list as it stands,
 * under vh_group_landmarks' own validity rule -- without valid states every record has reason 1, n_used is 0 and the result
 * is vh_group_refit_motion's byte for byte (not an error).  Tw_prev [S][16] goes up; NULL: the trajectory's pose before this
 * pair's step (what vh_group_trajectory reports as Tw_prev for the pair), copied on the device.  reclassify, counts: as
 * vh_group_refit_motion.  Nothing else goes up; synchronous.
 * VH_ERR_UNSUPPORTED on a sequence handle (checked first).  VH_ERR_STATE wherever vh_group_refit_motion returns it; with
 * track linking off or without a tracked list of the current pair; where the classification read lists replaced on the
 * host; with Tw_prev == NULL and the trajectory off.
 * The first call adds one block, counted by vh_group_device_bytes: 32 bytes per record slot (S x max_matches), 128 + 4
 * bytes per stream (Tw_prev, n_used) and the refit's three arrays (48 + 4 + 4 bytes per stream), each of the six arrays
 * rounded up to 256 bytes; a handle that never calls these allocates and launches nothing.  A refused allocation is
 * VH_ERR_HIP before any launch and leaves the handle as it was.  Profile scopes: "refit_prior", "refit_prior_fit". */
int32_t vh_group_refit_motion_landmarks(vh_group *g, const vh_ego_params *e, const vh_lmk_refit_params *rp, const double *Tw_prev,
                                        int32_t reclassify, double *tr_out, int32_t *ok_out, int32_t *n_updates, int32_t *n_used,
                                        int32_t *counts);
int32_t vh_match_refit_motion_landmarks(vh_matcher *m, const vh_ego_params *e, const vh_lmk_refit_params *rp, const double *Tw_prev,
                                        int32_t reclassify, double *tr_out, int32_t *ok_out, int32_t *n_updates, int32_t *n_used,
                                        int32_t *count);
/* The priors of the last such call, one per record of the inlier list the fit read (before a reclassification), valid
 * until the next match call (VH_ERR_STATE otherwise), under the getters' capacity rule as vh_group_get_scene_points. */
int32_t vh_group_get_refit_priors(vh_group *g, int32_t stream, vh_refit_prior *out, int32_t cap, int32_t *n);

#ifdef __cplusplus
}
#endif
#endif
