/*
 * gridvision_hip_match.h -- [EXTENSION] X16: match the resident lidar scan to the resident costmap.
 *
 * A header of its own beside gridvision_hip.h (which it includes and which stays as it is: its 123 entry points and
 * ABI version 4).  libgridvision_hip.so exports the six functions declared here as well.  The reference has no such
 * step; this text is the definition, and the device call, the host twin and the tests' numpy reference all give its
 * bytes.
 *
 * What it is.  A correlative scan matcher (Olson's real-time correlative scan matching, Cartographer's and
 * Hector-SLAM's matchers, AMCL's likelihood field on the scoring side) over the two things a handle already holds:
 * the resident cloud and the costmap of the last gv_inflate, whose cost byte decays with the exact distance to the
 * nearest lethal cell -- a likelihood field.  Every pose of a window around a guess is scored by the sum of the cost
 * bytes under the scan's points; the best pose comes back, and gv_match_motion turns it into the `motion` of
 * gv_grid_move and gv_track_update: scan -> pose correction -> motion, without an outside odometry.
 *
 * Configuration.  gv_match_config:
 *   wx, wy      window half-widths in whole cells, 0..32 each
 *   wt          half the number of yaw candidates, 0..32
 *   yaw_step    rad, finite, >= 0; > 0 when wt > 0
 *   stride      1..1024
 *   min_points  >= 1
 *   flags       only GV_MATCH_USE_BAND
 * gv_set_match_config is handle configuration like gv_set_footprint: no device work, kept through gv_reset,
 * gv_set_log_odds and gv_grid_move; NULL turns it off (the state after gv_create); a call already enqueued keeps the
 * configuration it was enqueued with.  GV_ERR_BAD_ARG, configuration unchanged, for a null handle or a field out of
 * range.  The counts are NT = 2*wt+1, NY = 2*wy+1, NX = 2*wx+1.
 *
 * Guess.  gv_match_guess {x, y, yaw}: the pose of the current base frame in the grid's frame, the frame the poses of
 * gv_score_trajectories live in; typically the odometry increment since the last map update.  All three finite.
 *
 * Points.  Point i of the resident cloud is selected when i % stride == 0.  Its base-frame coordinates (bx, by, bz)
 * are the float32 transform by base_from_lidar, with the matrix and the operation order of the lidar map update:
 * x*c0 + (y*c1 + (z*c2 + c3)), every operation rounded on its own.  A selected point is USED when all three are
 * finite and, with GV_MATCH_USE_BAND and a height band set (gv_set_height_band), !(bz < z_ground) && !(bz > z_max),
 * the map update's own fp32 compares.  n_used counts the used points.
 *
 * Yaw candidates.  For t = 0..NT-1: theta_t = guess.yaw + (double)(t - wt) * yaw_step in fp64; c_t = (float)cos(theta_t),
 * s_t = (float)sin(theta_t) are evaluated ON THE HOST (libm, fp64, rounded once) and travel with the call as a table
 * of NT float pairs; the device evaluates no sine.  gv_match_rotations returns that table.
 *
 * Cells.  One float32 operation each, never contracted:  rx = (c_t*bx) - (s_t*by),  ry = (s_t*bx) + (c_t*by).  Then in
 * fp64:  gx = (double)rx + guess.x,  gy = (double)ry + guess.y,  vx = ((gx - off_x) - pos_x) / res  and vy likewise
 * (off = half the map's length, pos = its centre: grid_map's getIndex expression),  ux = floor(-vx),  uy = floor(-vy).
 * A used point whose ux or uy is not below 2^30 in magnitude contributes to no candidate; it still counts in n_used.
 * On the map these are getIndex's cells wherever its two range tests agree; at the map's border THIS text decides,
 * not getIndex: a cell is on the map iff 0 <= ux < nx and 0 <= uy < ny.
 *
 * Score.  Translation candidates are whole-cell index shifts (j, i), |j| <= wy, |i| <= wx:
 *   score[t][j][i] = sum over the used points of C(ux + i, uy + j),
 *   C(ix, iy) = cost[G - 1 - (iy*nx + ix)] on the map, 0 off it,
 * cost being the resident costmap of the last gv_inflate on whichever scale that ran.  The sums are uint32 (the call
 * requires ceil(n / stride) <= 2^24 selected points), so the result does not depend on scheduling.
 *
 * Candidate pose.  ix grows as x falls: shifting the points by +i cells is moving the vehicle by -i*res.  In fp64,
 * one operation each:  x = guess.x - (double)i * res,  y = guess.y - (double)j * res,  yaw = theta_t.  The pose is
 * nominal: the score is defined by the index shift, not by binning the shifted points again.
 *
 * Selection.  The best candidate has the largest score; ties go to the smallest Chebyshev distance
 * max(|t - wt|, |j|, |i|) (a flat field returns the guess), then to the smallest linear index
 * (t*NY + (j + wy))*NX + (i + wx).
 *
 * Result.  gv_match_result, 64 bytes, written by the device: the best candidate's offsets from the centre, n_used,
 * best_score, guess_score (the centre candidate's), valid = n_used >= min_points && best_score > 0, and the
 * candidate pose (no transcendental is involved: the bytes equal the host's).  With GV_MATCH_KEEP_SCORES, a flag of
 * the call, the whole volume scores[NT*NY*NX] (uint32, the linear index above) goes to the caller's buffer; a caller
 * derives a covariance from it.
 *
 * Calls.  gv_match_scan_async enqueues on gv_stream(h): a point pass, the score pass and the selection.  It reads the
 * resident cloud as the frames enqueued after the last upload would, and the costmap as the last enqueued gv_inflate
 * left it; ordered like gv_score_trajectories_async, allowed between gv_tick_enqueue and gv_tick_wait.  result and
 * scores may be pinned (gv_host_alloc: written in place by the device) or pageable (a copy command behind the
 * kernels); both are complete once the stream has been waited for.  gv_match_scan is the same call followed by the wait.
 *   GV_ERR_BAD_ARG, state unchanged: a null handle, guess or result, a non-finite guess, unknown flags,
 *     GV_MATCH_KEEP_SCORES with null scores.
 *   GV_ERR_TF: base_from_lidar was never set.
 *   GV_ERR_STATE: no configuration, no cloud, no gv_inflate since gv_create / gv_reset, more than 2^24 selected points,
 *     a communicator of more than one rank (ranks own row bands of the grid).
 * gv_match_scan_host is the host twin (no handle, no GPU): the same arithmetic text compiled for the host, over the
 * geometry gv_create gives grid_x, grid_y and resolution, a costmap of G bytes, SoA points, base_from_lidar, an
 * optional band (NULL: none), configuration, guess and flags.  GV_ERR_BAD_ARG for what the calls above refuse.
 * gv_match_rotations (host only): table[2*t] = c_t, table[2*t + 1] = s_t, NT pairs.
 * gv_match_motion (host only): the `motion` for gv_grid_move and gv_track_update when the map was last registered at
 * the previous base frame: (qx, qy, qz, qw; tx, ty, tz) = (0, 0, sin(yaw/2), cos(yaw/2); x, y, 0) of the result's pose.
 *
 * Not built: a multi-resolution branch-and-bound search, sub-cell refinement, a covariance, matching on a sharded
 * grid, FrameFlow wiring.
 */
#ifndef GRIDVISION_HIP_MATCH_H_
#define GRIDVISION_HIP_MATCH_H_

#include "gridvision_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define GV_MATCH_USE_BAND    (1u << 0)   /* gv_match_config.flags: the height band selects the points */
#define GV_MATCH_KEEP_SCORES (1u << 0)   /* flags of a call: the whole volume goes to `scores` */

typedef struct {
  int32_t wx, wy, wt;
  int32_t stride;
  double yaw_step;
  int32_t min_points;
  uint32_t flags;
} gv_match_config;       /* 32 bytes */

typedef struct {
  double x, y, yaw;
} gv_match_guess;        /* 24 bytes */

typedef struct {
  int32_t best_t, best_j, best_i;   /* signed offsets from the centre candidate */
  int32_t valid;
  uint32_t n_used, best_score, guess_score;
  uint32_t reserved;                /* 0 */
  double x, y, yaw;                 /* the best candidate's pose */
  uint64_t reserved2;               /* 0 */
} gv_match_result;       /* 64 bytes */

int gv_set_match_config(gv_handle h, const gv_match_config *cfg /* NULL: off */);
int gv_match_scan_async(gv_handle h, const gv_match_guess *guess, uint32_t flags, gv_match_result *result,
                        uint32_t *scores /* NT*NY*NX with GV_MATCH_KEEP_SCORES, else may be NULL */);
int gv_match_scan(gv_handle h, const gv_match_guess *guess, uint32_t flags, gv_match_result *result,
                  uint32_t *scores /* NT*NY*NX with GV_MATCH_KEEP_SCORES, else may be NULL */);
int gv_match_scan_host(uint8_t grid_x, uint8_t grid_y, double resolution, const uint8_t *cost, const float *x,
                       const float *y, const float *z, size_t n, const gv_transform *base_from_lidar,
                       const gv_height_band *band /* may be NULL */, const gv_match_config *cfg,
                       const gv_match_guess *guess, uint32_t flags, gv_match_result *result,
                       uint32_t *scores /* NT*NY*NX with GV_MATCH_KEEP_SCORES, else may be NULL */);
int gv_match_rotations(const gv_match_config *cfg, const gv_match_guess *guess, float *table /* 2 * NT floats */);
int gv_match_motion(const gv_match_result *result, gv_transform *out);

#ifdef __cplusplus
}
#endif
#endif /* GRIDVISION_HIP_MATCH_H_ */
