/*
 * gridvision_hip_search.h -- [EXTENSION] X18: wide-window scan matching, branch and bound over a pooled costmap.
 *
 * A header of its own beside gridvision_hip_match.h (which it includes and which stays as it is, like gridvision_hip.h
 * with its 123 entry points and ABI version 4).  libgridvision_hip.so exports the four functions declared here as well.
 * This text is the definition: the device call, the host twin and the tests' numpy reference all give its bytes.
 *
 * What it is.  gv_match_scan (X16) scores every pose of a window of at most 65 x 65 shifts.  A vehicle that lost its
 * pose needs tens of metres.  gv_match_search gives the answer of the exhaustive definition over a window of up to
 * 257 x 257 shifts x 65 yaws, and finds it the way Cartographer's matcher does, with one coarse level: an upper bound
 * for every S x S block of shifts from a max-pooled costmap, exact scores only for the blocks whose bound reaches the
 * best score of the most promising block.
 *
 * Configuration.  gv_search_config:
 *   wx, wy      window half-widths in whole cells, 0..128 each
 *   wt          half the number of yaw candidates, 0..32
 *   stride      1..1024
 *   yaw_step    rad, finite, >= 0; > 0 when wt > 0
 *   min_points  >= 1
 *   flags       only GV_SEARCH_USE_BAND
 *   block_log2  1..4: blocks of S x S shifts, S = 1 << block_log2
 *   reserved    0
 * gv_set_search_config is handle configuration like gv_set_match_config and independent of it: no device work, kept
 * through gv_reset, gv_set_log_odds and gv_grid_move; NULL turns it off (the state after gv_create); a call already
 * enqueued keeps the configuration it was enqueued with.  GV_ERR_BAD_ARG, configuration unchanged, for a null handle
 * or a field out of range.  NT = 2*wt+1, NY = 2*wy+1, NX = 2*wx+1.
 *
 * Result record.  The guess, the points and n_used, the yaw candidates, the cells (ux, uy), the cost C, the score
 * score[t][j][i], the candidate pose, the selection order and the record gv_match_result are word for word those of
 * gridvision_hip_match.h with wx, wy, wt, stride, yaw_step, min_points and the band flag of this configuration; only
 * the window is wider, |j| <= wy <= 128 and |i| <= wx <= 128.  The record, guess_score and valid included, is the one
 * the exhaustive definition gives.  There is no GV_MATCH_KEEP_SCORES: no dense volume exists.
 *
 * Search and stats.  The stats are deterministic and part of the definition.
 *   Blocks.  S = 1 << block_log2, NBX = ceil(NX / S), NBY = ceil(NY / S).  Block (t, J, I) has the origin
 *     jb = -wy + J*S, ib = -wx + I*S and holds the window's candidates (t, j, i) with jb <= j < jb + S and
 *     ib <= i < ib + S; NX and NY are odd, so the last row and column of blocks are clipped.  Its index is
 *     (t*NBY + J)*NBX + I.  n_blocks = NT*NBY*NBX.
 *   Pooled costmap.  M(ix, iy) = max of C(ix + dx, iy + dy) over 0 <= dx, dy < S: nonzero only for
 *     -(S-1) <= ix < nx and -(S-1) <= iy < ny.
 *   Bound.  B[t][J][I] = sum over the used points whose cell exists of M(ux + ib, uy + jb), a uint32 sum.  The pooling
 *     covers the whole S x S block even where the window clips it.  bound_max = the largest B; bound_sum = the sum of
 *     every B as uint64.
 *   Seed.  The block with the largest B; ties go to the smallest max(|t - wt|, |J - wy / S|, |I - wx / S|) (integer
 *     division: the distance from the block that holds the centre), then to the smallest block index.  seed_block is
 *     its index; lower_score = L, the largest score among the seed's candidates inside the window.
 *   Survivors.  A block survives iff B > 0 and B >= L.  n_survivors counts them, n_scored their candidates inside the
 *     window.
 *   Answer.  The best candidate, by X16's selection order, among the candidates of all survivors and the centre
 *     candidate (0, 0, 0), which is always scored and gives guess_score.
 * Why this is the exhaustive answer.  M(ux + ib, uy + jb) >= C(ux + i, uy + j) for every candidate of the block, point
 * by point, so B is not below any score in the block.  Let s* be the largest score of the window.  L is a score, so
 * s* >= L.  If s* > 0, every candidate that scores s* lies in a block with B >= s* >= L and B > 0: a survivor, so all
 * of them are compared, and the selection order picks among them as it does among all.  If s* = 0, every score is 0
 * and the order picks the smallest Chebyshev distance: the centre.  On a flat nonzero field every block survives: the
 * worst case, n_scored = NT*NY*NX.
 *
 * Calls.  gv_match_search_async enqueues on gv_stream(h): X16's point pass, the pool pass over the resident costmap,
 * the bound pass, the seed, the prune and the fine pass, no host wait between them.  It reads the resident cloud and
 * the costmap as gv_match_scan_async does and is ordered like it; allowed between gv_tick_enqueue and gv_tick_wait.
 * result and stats (may be NULL) may be pinned (gv_host_alloc: written in place by the device) or pageable (a copy
 * command behind the kernels); both are complete once the stream has been waited for.  gv_match_search is the same
 * call followed by the wait.
 *   GV_ERR_BAD_ARG, state unchanged, nothing written: a null handle, guess or result, a non-finite guess, flags != 0.
 *   GV_ERR_TF: base_from_lidar was never set.
 *   GV_ERR_STATE: no configuration, no cloud, no gv_inflate since gv_create / gv_reset, more than 2^24 selected points,
 *     a communicator of more than one rank.
 * gv_match_search_host is the host twin (no handle, no GPU), with gv_match_scan_host's arguments.  GV_ERR_BAD_ARG for
 * what the calls above refuse.  gv_match_rotations and gv_match_motion serve both matchers.
 *
 * Not built: more than one coarse level, sub-cell refinement, a covariance, matching on a sharded grid, FrameFlow wiring.
 */
#ifndef GRIDVISION_HIP_SEARCH_H_
#define GRIDVISION_HIP_SEARCH_H_

#include "gridvision_hip_match.h"

#ifdef __cplusplus
extern "C" {
#endif

#define GV_SEARCH_USE_BAND (1u << 0)   /* gv_search_config.flags: the height band selects the points */

typedef struct {
  int32_t wx, wy;        /* 0..128 */
  int32_t wt;            /* 0..32 */
  int32_t stride;        /* 1..1024 */
  double yaw_step;
  int32_t min_points;    /* >= 1 */
  uint32_t flags;
  int32_t block_log2;    /* 1..4 */
  int32_t reserved;      /* 0 */
} gv_search_config;      /* 40 bytes */

typedef struct {
  uint32_t n_blocks, n_survivors, n_scored, seed_block, lower_score, bound_max;
  uint64_t bound_sum;
} gv_search_stats;       /* 32 bytes */

int gv_set_search_config(gv_handle h, const gv_search_config *cfg /* NULL: off */);
int gv_match_search_async(gv_handle h, const gv_match_guess *guess, uint32_t flags /* 0 */, gv_match_result *result,
                          gv_search_stats *stats /* may be NULL */);
int gv_match_search(gv_handle h, const gv_match_guess *guess, uint32_t flags /* 0 */, gv_match_result *result,
                    gv_search_stats *stats /* may be NULL */);
int gv_match_search_host(uint8_t grid_x, uint8_t grid_y, double resolution, const uint8_t *cost, const float *x,
                         const float *y, const float *z, size_t n, const gv_transform *base_from_lidar,
                         const gv_height_band *band /* may be NULL */, const gv_search_config *cfg,
                         const gv_match_guess *guess, uint32_t flags /* 0 */, gv_match_result *result,
                         gv_search_stats *stats /* may be NULL */);

#ifdef __cplusplus
}
#endif
#endif /* GRIDVISION_HIP_SEARCH_H_ */
