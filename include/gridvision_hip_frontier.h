/*
 * gridvision_hip_frontier.h -- [EXTENSION] X19: frontier clusters and exploration goals from the resident grid, on the
 * device.
 *
 * A header of its own that includes gridvision_hip.h and is NOT included by it.  gridvision_hip.h, its 123 entry points
 * and ABI version 4 are frozen; entry points added after ABI 4 live in a second C namespace, gvx_, so that the frozen
 * gv_ export set of libgridvision_hip.so stays exactly what it was.  The library exports the seven functions declared
 * here.  The reference has no such step; this text is the definition, and the device call, the host twin and the tests'
 * plain reference all give its bytes.
 *
 * What it is.  The grid tells observed cells from never-observed ones: the constructor state (0.0, 0.5, 50) is the prior,
 * and gv_grid_move refills every cell that scrolls in with it.  Frontier exploration (Yamauchi; nav2's and explore_lite's
 * frontier search) finds the free cells that border unknown space, groups them into connected clusters and ranks one
 * as the goal.  gvx_frontier does that on the device and keeps the result there; gvx_nav_field_from_frontier seeds X9's
 * distance field with the clusters' cells, so that gv_nav_path from the vehicle ends on the nearest reachable frontier
 * cell and "where to go when nobody supplies a goal" never crosses the host.
 *
 * Everything is in OccupancyGrid.data order, like X6, X9 and X17: entry e = y * nx + x.  Nothing wraps across a row end.
 * Cells off the map do not exist: they are neither unknown nor free.  Grids with nx or ny above 65535 are refused.
 *
 * Classes, from the packed int8 layer v (what gv_to_occupancy_grid returns):
 *   FREE     iff 0 <= v <= free_max
 *   UNKNOWN  iff unknown_min <= v <= unknown_max
 *   everything else is neither, the -1 of a NaN occupancy included.
 * Frontier cell.  A FREE cell of which
 *   at least one of the four neighbours (x-1, y), (x+1, y), (x, y-1), (x, y+1) is on the map and UNKNOWN
 *     (4-connectivity is its own mirror image under the 180 degree turn between cell order and data order), and,
 *   when max_cost < 256, cost[e] < max_cost in the costmap of the last gv_inflate.  With max_cost == 256 the costmap is
 *     not read and need not exist.
 * Component.  A maximal set of frontier cells connected under 8-connectivity.  Its label is the smallest entry in it.
 * Cluster.  A component with n_cells >= min_cells.  Clusters are ordered by ascending label; the first `cap` of them are
 *   WRITTEN.
 * Labels layer.  labels[G], uint32: GVX_FRONTIER_NONE at a cell that is no frontier cell; at every frontier cell its
 *   component's label, whether or not the component passed min_cells or cap.
 *
 * gvx_frontier_config, 32 bytes:
 *   free_max                   0..100
 *   unknown_min, unknown_max   0..100, free_max < unknown_min <= unknown_max
 *   max_cost                   1..256
 *   min_cells                  1..2^20
 *   flags, reserved[2]         0
 * gvx_frontier_record, one record per written cluster, 64 bytes, every byte defined:
 *    0  int32  label          smallest entry of the cluster
 *    4  int32  n_cells
 *    8  int32  min_x, max_x, min_y, max_y   entry coordinates
 *   24  uint64 sum_x, sum_y   sums of the entry coordinates
 *   40  int32  centre_entry   the cluster cell with the smallest ((x-cx)^2 + (y-cy)^2, entry), cx = sum_x / n_cells and
 *                             cy = sum_y / n_cells by unsigned integer division
 *   44  int32  field_entry    with GVX_FRONTIER_USE_FIELD: over the cluster cells whose value in the field of the last
 *   48  uint32 field_min        gv_nav_field* is below GV_NAV_UNREACHABLE, (field_min, field_entry) is the smallest
 *                               (value, entry).  When no cell qualifies, or without the flag, field_min =
 *                               GV_NAV_UNREACHABLE and field_entry = -1.
 *   52  int32  goal_entry     field_entry when that is >= 0, else centre_entry
 *   56  float  goal_x, goal_y the cell centre of goal_entry by X17's formula (gridvision_hip_path.h): with ix = nx-1-x,
 *                             X = (float)((pos_x + off_x) - ((double)ix + 0.5) * res), Y likewise
 *   Records n_written .. cap-1 of out[cap] are all zero bytes.
 * gvx_frontier_info, 32 bytes:
 *   n_frontier_cells
 *   n_components   all components
 *   n_clusters     components passing min_cells
 *   n_written      min(n_clusters, cap)
 *   best           index into the written records: with USE_FIELD the record with the smallest field_min among those
 *                  with field_entry >= 0, without it the record with the largest n_cells; ties go to the smaller index;
 *                  -1 when there is none
 *   largest        largest n_cells over all components, 0 when none
 *   flags          the call's flags
 *   reserved       0
 * All outputs are integer minima, sums and counts: no order of execution shows in any byte.
 *
 * Calls.
 * gvx_set_frontier_config is handle configuration like gv_set_nav_config: no device work, kept through gv_reset,
 *   gv_set_log_odds and gv_grid_move; NULL turns it off; GV_ERR_BAD_ARG, the configuration unchanged, outside the ranges.
 * gvx_frontier_async enqueues on gv_stream(h) with no host wait (the allocations of a first or larger call excepted);
 *   gvx_frontier is the same call followed by the wait.  cap in 1..4096, flags a subset of {GVX_FRONTIER_USE_FIELD}.
 *   It reads the packed layer as the last enqueued grid pass left it, and the costmap or field as last made.  Ordering
 *   and permissions are as for gv_inflate; the call is allowed between gv_tick_enqueue and gv_tick_wait.  info and
 *   out[cap] follow gv_nav_path_async's destination rules: pinned 16-byte aligned memory is written by the kernel,
 *   anything else through a copy command; both are complete once the stream has been waited for.  Records, info and
 *   labels stay RESIDENT until the next call or gv_reset.  GV_ERR_BAD_ARG for a null handle, info or out, cap out of
 *   range or unknown flags.  GV_ERR_STATE when no configuration is set, when max_cost < 256 and there is no costmap,
 *   with USE_FIELD and no field, with a communicator of more than one rank, and on a grid side above 65535.
 * gvx_frontier_host is the host twin, plain C++ with no handle, over the geometry gv_create gives grid_x, grid_y and
 *   resolution.  cost may be NULL when max_cost == 256, field without USE_FIELD; out and labels may each be NULL.
 *   GV_ERR_BAD_ARG for what the calls above refuse and for an invalid geometry.
 * gvx_get_frontier_labels is a synchronous read-back of the G labels.  GV_ERR_STATE before the first call since
 *   gv_create or gv_reset.
 * gvx_device_frontier gives read-only device pointers to labels[G], records[cap] and the info record, and the cap of
 *   the call that made them, like gv_device_nav_path.  Each destination may be NULL.  GV_ERR_STATE with no resident
 *   frontier.
 * gvx_nav_field_from_frontier is the counterpart of gv_nav_field_from_path: X9's solver seeded on the device, with k in
 *   0..cap-1 by every cell of written cluster k, with k = -1 by every cell of every written cluster.  k >= n_written is
 *   "no usable seed", not an error: the device reads n_written.  Field bytes and n_seeds_used equal gv_nav_field over
 *   those cells' centres.  It waits on the host as gv_nav_field does and replaces the field.  GV_ERR_BAD_ARG for a null
 *   handle or k outside -1..cap-1; its state errors are those of gv_nav_field_from_path, plus "no resident frontier".
 *
 * Not built: frontiers on a sharded grid, a FrameFlow switch, information-gain ranking, incremental relabelling after
 * a map change, more than 4096 written clusters.
 */
#ifndef GRIDVISION_HIP_FRONTIER_H_
#define GRIDVISION_HIP_FRONTIER_H_

#include "gridvision_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define GVX_FRONTIER_USE_FIELD (1u << 0)   /* flags of a call: rank the clusters by the field of the last gv_nav_field* */
#define GVX_FRONTIER_NONE 0xFFFFFFFFu      /* labels[e] of a cell that is no frontier cell */
#define GVX_FRONTIER_MAX_CAP 4096

typedef struct {
  int32_t free_max;
  int32_t unknown_min, unknown_max;
  int32_t max_cost;
  int32_t min_cells;
  uint32_t flags;         /* 0 */
  uint32_t reserved[2];   /* 0 */
} gvx_frontier_config;    /* 32 bytes */

typedef struct {
  int32_t label;
  int32_t n_cells;
  int32_t min_x, max_x, min_y, max_y;
  uint64_t sum_x, sum_y;
  int32_t centre_entry;
  int32_t field_entry;
  uint32_t field_min;
  int32_t goal_entry;
  float goal_x, goal_y;
} gvx_frontier_record;           /* 64 bytes */

typedef struct {
  int32_t n_frontier_cells;
  int32_t n_components;
  int32_t n_clusters;
  int32_t n_written;
  int32_t best;
  int32_t largest;
  uint32_t flags;
  uint32_t reserved;      /* 0 */
} gvx_frontier_info;      /* 32 bytes */

int gvx_set_frontier_config(gv_handle h, const gvx_frontier_config *cfg /* NULL: off */);
int gvx_frontier_async(gv_handle h, int32_t cap, uint32_t flags, gvx_frontier_info *info, gvx_frontier_record *out /* cap */);
int gvx_frontier(gv_handle h, int32_t cap, uint32_t flags, gvx_frontier_info *info, gvx_frontier_record *out /* cap */);
int gvx_frontier_host(uint8_t grid_x, uint8_t grid_y, double resolution, const int8_t *occ_i8, const uint8_t *cost /* may be NULL */,
                      const uint32_t *field /* may be NULL */, const gvx_frontier_config *cfg, int32_t cap, uint32_t flags,
                      gvx_frontier_info *info, gvx_frontier_record *out /* cap, may be NULL */, uint32_t *labels /* G, may be NULL */);
int gvx_get_frontier_labels(gv_handle h, uint32_t *labels_out /* G */);
int gvx_device_frontier(gv_handle h, uint32_t **labels, gvx_frontier_record **records, gvx_frontier_info **info, int32_t *cap);
int gvx_nav_field_from_frontier(gv_handle h, int32_t k, gv_nav_info *nav_info /* may be NULL */);

#ifdef __cplusplus
}
#endif
#endif /* GRIDVISION_HIP_FRONTIER_H_ */
