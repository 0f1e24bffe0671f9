/*
 * gridvision_hip_gain.h -- [EXTENSION] X20: exploration goals ranked by the unknown cells they would reveal, on the
 * device.
 *
 * A header of its own that includes gridvision_hip_frontier.h and is NOT included by anything.  gridvision_hip.h, its
 * 123 entry points and ABI version 4 are frozen, and so are the seven gvx_ entry points of X19.  The rule from here on: A
 * HEADER ADDED AFTER ABI 4 OWNS ITS PREFIX.  gv_ is gridvision_hip.h's and its three companions', gvx_ is
 * gridvision_hip_frontier.h's, gvx2_ is this header's; a later header takes a prefix of its own, and no header adds a
 * symbol under another's.  The library exports the eight functions declared here.  The reference has no such step; this
 * text is the definition, and the device call, the host twin and the tests' plain reference all give its bytes.
 *
 * What it is.  X19 ranks frontier clusters by size or by distance.  What an exploration stack ranks by is how much
 * never-observed space a sensor would see from a goal, weighed against the way there.  gvx2_gain casts rays from every
 * candidate cell over the packed layer, counts the distinct unknown cells they pass, and scores the candidate by that
 * count against its value in X9's field; gvx2_frontier_gain takes the goal cells of the resident frontier records as
 * the candidates without a host wait in between; gvx2_nav_field_from_gain seeds the field with the chosen goal.
 *
 * Everything is integer arithmetic in entry coordinates, OccupancyGrid.data order as in X6, X9, X17 and X19: entry
 * e = y * nx + x, G = nx * ny.  Nothing wraps across a row end.  Grids with nx or ny above 65535 are refused.
 *
 * Classes, from the packed int8 layer v (what gv_to_occupancy_grid returns), by X19's class test over this
 * configuration's own bounds:
 *   FREE     iff 0 <= v <= free_max
 *   UNKNOWN  iff unknown_min <= v <= unknown_max
 *   OPAQUE   everything else: occupied cells, the band between free and unknown, the -1 of a NaN occupancy.
 * Candidate.  An entry c = (cx, cy), cx = c % nx, cy = c / nx.
 * Rays.  With the radius R there are 8 R rays per candidate, one to each cell of the square ring at Chebyshev distance
 *   R.  Ray r in 0 .. 8R-1 has side = r / (2R), j = r % (2R) and the offset (ox, oy)
 *     side 0  (-R + j, -R)      side 1  (R, -R + j)      side 2  (R - j, R)      side 3  (-R, R - j)
 *   and ends at (ex, ey) = (cx + ox, cy + oy), on the map or off it: the end is only arithmetic.
 * Line.  The cells of a ray are those of grid_map's LineIterator from (cx, cy) to (ex, ey) (gv_line.hpp has its closed
 *   form): ddx = |ox|, ddy = |oy|, the steps are the signs of ox and oy (+1 at 0); the major axis is x when ddx >= ddy,
 *   else y; major = max(ddx, ddy) = R, minor = min(ddx, ddy); num = major / 2 (integer division).  Cell 0 is (cx, cy).
 *   From one cell to the next: num += minor; if num >= major then num -= major and the minor coordinate takes its step;
 *   the major coordinate takes its step always.
 * Walk.  Ray r takes cells i = 1 .. R in order.  With (x, y) cell i:
 *   1. x or y off the map: rays_off_map += 1, the ray stops.
 *   2. d2 = (x - cx)^2 + (y - cy)^2; d2 > R^2: rays_range += 1, the ray stops.
 *   3. the cell is SEEN.
 *   4. the cell is OPAQUE: rays_opaque += 1, nearest_opaque_d2 = min(nearest_opaque_d2, d2), the ray stops.
 *   A ray that passes cell R without stopping adds 1 to rays_range.  FREE and UNKNOWN cells are both transparent.  The
 *   candidate's own cell is never tested or marked, whatever its class.
 * Counts.  n_unknown, n_free and n_opaque are the numbers of DISTINCT SEEN cells of each class.
 *   rays_opaque + rays_off_map + rays_range = 8 R.
 *
 * gvx2_gain_config, 32 bytes:
 *   free_max                   0..100
 *   unknown_min, unknown_max   0..100, free_max < unknown_min <= unknown_max   (the rule of gvx_frontier_config)
 *   radius                     1..255 cells
 *   min_gain                   0..2^20
 *   w_gain, w_dist             0..65535
 *   reserved                   0
 * gvx2_gain_record, one per candidate, 48 bytes, every byte defined:
 *    0  int32  entry              the candidate as given
 *    4  uint32 status             GVX2_GAIN_INVALID | GVX2_GAIN_UNREACHABLE | GVX2_GAIN_BELOW_MIN
 *    8  int32  n_unknown, n_free, n_opaque
 *   20  int32  rays_opaque, rays_off_map, rays_range
 *   32  uint32 nearest_opaque_d2  0xFFFFFFFF when no ray ended on an opaque cell
 *   36  uint32 dist               field[entry] with GVX2_GAIN_USE_FIELD, else 0; field is that of the last gv_nav_field*
 *   40  int64  score              (int64)w_gain * n_unknown - (int64)w_dist * dist; 0 when INVALID or UNREACHABLE
 *   status bits:
 *   GVX2_GAIN_INVALID      entry is outside 0..G-1.  status is exactly GVX2_GAIN_INVALID, every field behind it is zero
 *                          (nearest_opaque_d2 too), and no ray is cast.
 *   GVX2_GAIN_UNREACHABLE  with GVX2_GAIN_USE_FIELD, field[entry] >= GV_NAV_UNREACHABLE.  The rays are cast and counted
 *                          all the same; dist is the field's value; score is 0.
 *   GVX2_GAIN_BELOW_MIN    n_unknown < min_gain.  The score is what the formula gives.
 * gvx2_gain_info, 32 bytes:
 *    0  int32  n_candidates   of a list call n; of a frontier call the resident frontier's n_written
 *    4  int32  n_ranked       records among them with status == 0
 *    8  int32  best           the ranked record with the largest score, ties to the smaller index; -1 when there is none
 *   12  int32  best_entry     its entry, -1 when there is none
 *   16  int64  best_score     its score, 0 when there is none
 *   24  uint32 flags          the call's flags
 *   28  int32  radius         the configuration's
 * Every output is a count, a minimum or a maximum of integers: no schedule shows in any byte.
 *
 * Calls.
 * gvx2_set_gain_config is handle configuration like gvx_set_frontier_config: no device work, kept through gv_reset,
 *   gv_set_log_odds and gv_grid_move; NULL turns it off; GV_ERR_BAD_ARG, the configuration unchanged, outside the ranges.
 * gvx2_gain_async enqueues on gv_stream(h) with no host wait (the allocations of a first call excepted); gvx2_gain is
 *   the same call followed by the wait.  n in 1..4096; flags a subset of {GVX2_GAIN_USE_FIELD, GVX2_GAIN_DEVICE_ENTRIES}.
 *   entries follows the rule of X7's poses: host memory is copied before the call returns; with
 *   GVX2_GAIN_DEVICE_ENTRIES it is device memory that the kernel reads in place, behind what gv_stream(h) holds.  The
 *   call reads the packed layer as the last enqueued grid pass left it and the field as last made.  Ordering and
 *   permissions are as for gvx_frontier_async; the call is allowed between gv_tick_enqueue and gv_tick_wait.  info and
 *   out[n] follow gv_nav_path_async's destination rules: pinned 16-byte aligned memory is written by the kernel,
 *   anything else through a copy command; both are complete once the stream has been waited for.  Records and info stay
 *   RESIDENT until the next gain call or gv_reset.  GV_ERR_BAD_ARG for a null handle, entries, info or out, n out of
 *   range or unknown flags.  GV_ERR_STATE when no configuration is set, with USE_FIELD and no field, with a communicator
 *   of more than one rank, and on a grid side above 65535.
 * gvx2_frontier_gain_async / gvx2_frontier_gain: the candidates are the goal_entry of the resident frontier's written
 *   records, n_candidates is read from the resident frontier info on the device, and cap -- the length of out -- is the
 *   cap of the frontier call that made the records.  Records n_written .. cap-1 of out are all zero bytes.  flags a
 *   subset of {GVX2_GAIN_USE_FIELD}.  gvx_frontier_async followed by this call needs no wait in between.  GV_ERR_STATE
 *   with no resident frontier, plus the state errors above.
 * gvx2_gain_host is the host twin, plain C++ with no handle, over the geometry gv_create gives grid_x, grid_y and
 *   resolution.  field may be NULL without GVX2_GAIN_USE_FIELD; GVX2_GAIN_DEVICE_ENTRIES is refused.  GV_ERR_BAD_ARG
 *   for what the calls above refuse and for an invalid geometry.
 * gvx2_device_gain gives read-only device pointers to the resident records and info, and the length of the records (n of
 *   a list call, cap of a frontier call).  Each destination may be NULL.  GV_ERR_STATE with no resident result.
 * gvx2_nav_field_from_gain is the counterpart of gvx_nav_field_from_frontier: X9's solver seeded on the device with the
 *   cell of candidate k, k = -1 the resident `best`; the index is read on the device.  A missing best, an INVALID record
 *   and k >= n_candidates are "no usable seed", not an error.  Field bytes and n_seeds_used equal gv_nav_field over that
 *   cell's centre.  It waits on the host as gv_nav_field does and replaces the field; the resident records keep the dist
 *   of the field they were made with.  GV_ERR_BAD_ARG for a null handle or k outside -1 .. (resident length)-1; its
 *   state errors are those of gv_nav_field_from_path, plus "no resident gain".  Its use: gv_nav_path from the vehicle
 *   then ends on the chosen goal.
 *
 * Not built: sensor field-of-view cones, rays that end after a run of unknown cells, a per-cell seen layer returned to
 * the caller, one candidate split over several workgroups, the sharded grid, a FrameFlow switch.
 */
#ifndef GRIDVISION_HIP_GAIN_H_
#define GRIDVISION_HIP_GAIN_H_

#include "gridvision_hip_frontier.h"

#ifdef __cplusplus
extern "C" {
#endif

#define GVX2_GAIN_USE_FIELD (1u << 0)        /* flags of a call: dist and UNREACHABLE from the field of the last gv_nav_field* */
#define GVX2_GAIN_DEVICE_ENTRIES (1u << 1)   /* flags of a list call: entries is device memory, read in place */
#define GVX2_GAIN_INVALID (1u << 0)          /* status bits of a record */
#define GVX2_GAIN_UNREACHABLE (1u << 1)
#define GVX2_GAIN_BELOW_MIN (1u << 2)
#define GVX2_GAIN_MAX_N 4096
#define GVX2_GAIN_MAX_RADIUS 255
#define GVX2_GAIN_NO_OPAQUE 0xFFFFFFFFu      /* nearest_opaque_d2 when no ray ended on an opaque cell */

typedef struct {
  int32_t free_max;
  int32_t unknown_min, unknown_max;
  int32_t radius;
  int32_t min_gain;
  int32_t w_gain, w_dist;
  uint32_t reserved;      /* 0 */
} gvx2_gain_config;       /* 32 bytes */

typedef struct {
  int32_t entry;
  uint32_t status;
  int32_t n_unknown, n_free, n_opaque;
  int32_t rays_opaque, rays_off_map, rays_range;
  uint32_t nearest_opaque_d2;
  uint32_t dist;
  int64_t score;
} gvx2_gain_record;       /* 48 bytes */

typedef struct {
  int32_t n_candidates;
  int32_t n_ranked;
  int32_t best;
  int32_t best_entry;
  int64_t best_score;
  uint32_t flags;
  int32_t radius;
} gvx2_gain_info;         /* 32 bytes */

int gvx2_set_gain_config(gv_handle h, const gvx2_gain_config *cfg /* NULL: off */);
int gvx2_gain_async(gv_handle h, int32_t n, const int32_t *entries /* n */, uint32_t flags, gvx2_gain_info *info, gvx2_gain_record *out /* n */);
int gvx2_gain(gv_handle h, int32_t n, const int32_t *entries /* n */, uint32_t flags, gvx2_gain_info *info, gvx2_gain_record *out /* n */);
int gvx2_frontier_gain_async(gv_handle h, uint32_t flags, gvx2_gain_info *info, gvx2_gain_record *out /* cap of the resident frontier */);
int gvx2_frontier_gain(gv_handle h, uint32_t flags, gvx2_gain_info *info, gvx2_gain_record *out /* cap of the resident frontier */);
int gvx2_gain_host(uint8_t grid_x, uint8_t grid_y, double resolution, const int8_t *occ_i8, const uint32_t *field /* may be NULL */,
                   const gvx2_gain_config *cfg, int32_t n, const int32_t *entries /* n */, uint32_t flags, gvx2_gain_info *info,
                   gvx2_gain_record *out /* n */);
int gvx2_device_gain(gv_handle h, gvx2_gain_record **records, gvx2_gain_info **info, int32_t *n);
int gvx2_nav_field_from_gain(gv_handle h, int32_t k, gv_nav_info *nav_info /* may be NULL */);

#ifdef __cplusplus
}
#endif
#endif /* GRIDVISION_HIP_GAIN_H_ */
