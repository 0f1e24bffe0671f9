/*
 * gridvision_hip_shortcut.h -- [EXTENSION] X21: resident paths pulled tight by line-of-sight shortcuts and thinned to
 * waypoints, on the device.
 *
 * A header of its own that includes gridvision_hip.h and is NOT included by anything.  gridvision_hip.h, its 123 entry
 * points and ABI version 4 are frozen, and so are the gvx_ entry points of X19 and the gvx2_ ones of X20.  By the rule
 * written down with X20, A HEADER ADDED AFTER ABI 4 OWNS ITS PREFIX: this one takes gvx3_, and the library exports the
 * seven functions declared here.  The reference has no such step; this text is the definition, and the device call, the
 * host twin and the tests' plain reference all give its bytes.
 *
 * What it is.  gv_nav_path (X17) leaves a 4- or 8-connected staircase of cells per start.  Nobody follows that directly:
 * every user of a grid planner first pulls the string tight -- a later cell of the path that can be seen from an earlier
 * one is joined to it by a straight line -- and then thins the result to waypoints at a spacing.  gvx3_shortcut does both
 * for every resident path at once and keeps the waypoints resident; gvx3_nav_field_from_shortcut seeds X9's field with
 * them, so a controller scored against that field is pulled along the straightened path, not along the stairs.
 *
 * Everything is integer arithmetic in entry coordinates, OccupancyGrid.data order as in X6, X9 and X17: entry
 * e = y * nx + x, x = e % nx, y = e / nx.  The cell centres are the one exception.  Nothing wraps across a row end.
 *
 * Inputs on the device.
 *   The resident paths of the last gv_nav_path*: entries[S][cap] and the S records.  Path s has n = n_cells cells
 *   c[0 .. n-1]; a start that walked nowhere has n = 0.
 *   The costmap of the last gv_inflate: uint8, G entries.  It is read as it stands when the call runs on the stream, as
 *   gv_nav_field_from_path reads it: a gv_inflate enqueued between the path call and this one is the costmap seen.
 * gvx3_shortcut_config, 32 bytes:
 *   max_cost   0..254    a cell is CLEAR iff its cost byte <= max_cost
 *   window     1..4096   W: how many path cells ahead of an anchor a shortcut may reach
 *   spacing    0..65535  waypoints every `spacing` cells of a segment's line; 0: anchors only
 *   reserved   five words, all 0
 * Flags of a call: GVX3_SHORTCUT_NO_CORNER.
 *
 * Line.  L(p -> q) is the cells of grid_map's LineIterator from p = (px, py) to q = (qx, qy) (gv_line.hpp has its closed
 *   form): ddx = |qx - px|, ddy = |qy - py|, the steps are the signs of qx - px and qy - py (+1 at 0); the major axis is x
 *   when ddx >= ddy, else y; major = max(ddx, ddy), minor = min(ddx, ddy); num = major / 2 (integer division).  Cell 0 is
 *   p.  From one cell to the next: num += minor; if num >= major then num -= major and the minor coordinate takes its
 *   step; the major coordinate takes its step always.  major + 1 cells, cell major is q.  The line is directional:
 *   L(p -> q) need not be L(q -> p) reversed.  p == q is the one cell p, major 0.
 * VISIBLE(p, q).  Every cell of L(p -> q), both ends included, is CLEAR.  With GVX3_SHORTCUT_NO_CORNER, for every
 *   i >= 1 whose cell (x_i, y_i) differs from cell i-1 in both coordinates, the two flanking cells (x_{i-1}, y_i) and
 *   (x_i, y_{i-1}) must be CLEAR as well: X17's no-corner-cut rule.  All these cells lie in the bounding box of p and q,
 *   hence on the map.
 * Anchors (greedy, farthest visible).  a_0 = 0.  For an anchor a < n-1 the next anchor is the LARGEST j in
 *   a+2 .. min(a+W, n-1) with VISIBLE(c[a], c[j]); when there is none (or the range is empty) it is a+1.  The step to
 *   a+1 is never tested: a path's own step is always accepted, whatever its cost.  Visibility is not monotone in j (a
 *   pillar hides some j and not a larger one), so it is the largest j, not the one before the first failure.  The chain
 *   ends at the anchor n-1.  A pair of consecutive anchors (a, b) is a SEGMENT, its line L(c[a] -> c[b]).
 * Waypoints, in this order, slot k of the outputs for the k-th:
 *   for each segment (a, b) in order, with m the major of its line:
 *     1. the cell c[a], index a;
 *     2. with spacing > 0, the line's cells i = spacing, 2 * spacing, ... < m, each with index -1;
 *   3. after the last segment (with n == 1: there is none), the cell c[n-1], index n-1.
 *   Emission stops once wcap waypoints are written; the status is TRUNCATED iff some waypoint was not emitted, which is
 *   iff the last one, c[n-1], was not.  A segment is ENTERED when its first anchor c[a] is written; the anchors of the
 *   chain are not searched for beyond the last entered segment.
 * Output per path s.
 *   entries[s][wcap]  int32   the waypoints' data-order entries
 *   index[s][wcap]    int32   the path index of an anchor, -1 for a waypoint between anchors
 *   xy[s][wcap][2]    float32 cell centres by exactly gridvision_hip_path.h's expression: with ix = nx-1-x,
 *                     X = (float)((pos_x + off_x) - ((double)ix + 0.5) * res), Y likewise; fp64, rounded once.
 *   Slots of all three past n_waypoints hold unspecified values.
 *   gvx3_shortcut_info, 32 bytes, every byte defined:
 *      0  int32  status         GVX3_SHORTCUT_OK 0; GVX3_SHORTCUT_TRUNCATED 1; GVX3_SHORTCUT_EMPTY 2: the source path's
 *                               n_cells is 0 -- every other field is then 0 and end_entry is -1
 *      4  int32  n_waypoints    waypoints written
 *      8  int32  n_anchors      those of them with index >= 0
 *     12  int32  n_src          the source path's n_cells
 *     16  int32  n_steps        the sum of major over the entered segments
 *     20  int32  n_diag_steps   the sum of min(ddx, ddy) over the entered segments
 *     24  int32  max_cost_seen  the largest cost byte over all cells of the entered segments' lines, both ends included
 *                               (an untested a -> a+1 step is a segment like any other), and over c[n-1] when that last
 *                               waypoint is written (which matters for n == 1 alone)
 *     28  int32  end_entry      the entry of the last waypoint written
 *   Every value is an index maximum, a count, a sum or a maximum of integers: no schedule shows in any byte.
 *
 * Calls.
 * gvx3_set_shortcut_config is handle configuration like gvx2_set_gain_config: no device work, kept through gv_reset; NULL
 *   turns it off; GV_ERR_BAD_ARG, the configuration unchanged, outside the ranges above.
 * gvx3_shortcut_async enqueues one kernel on gv_stream(h) with no host wait (the allocations of a first or larger call
 *   excepted); gvx3_shortcut is the same call followed by the wait.  S is that of the resident paths.  wcap in 1..65536
 *   and S * wcap <= 2^20; flags a subset of {GVX3_SHORTCUT_NO_CORNER}.  Ordering and permissions are as for
 *   gv_nav_path_async; the call is allowed between gv_tick_enqueue and gv_tick_wait.  info[S] and, when not NULL,
 *   way_xy[S * wcap * 2] follow gv_nav_path_async's destination rules: pinned memory (info 16-byte, way_xy 8-byte
 *   aligned) is written by the kernel in place, anything else through a copy command behind it; both are complete once
 *   the stream has been waited for.  Waypoints and records stay RESIDENT, in buffers of their own, until the next shortcut
 *   call or gv_reset; the source paths survive the call unchanged.  GV_ERR_BAD_ARG for a null handle or info, wcap out of
 *   range or unknown flags, and -- once the state holds -- for S * wcap above 2^20.  GV_ERR_STATE when no configuration
 *   is set, with no resident path, with no costmap, and with a communicator of more than one rank.
 * gvx3_shortcut_host is the host twin, plain C++ with no handle, over the geometry gv_create gives grid_x, grid_y and
 *   resolution, ANY cost array of G bytes and ANY entry lists: src_entries[S * cap], path s at s * cap with src_n[s]
 *   cells (0 .. cap).  Lines between arbitrary on-map cells need no adjacency.  S in 1..256, cap in 1..65536,
 *   S * cap <= 2^20, wcap as above.  entries, index and xy may each be NULL.  GV_ERR_BAD_ARG for what the calls above
 *   refuse, for an invalid geometry, for src_n[s] outside 0 .. cap and for a source entry (among the first src_n[s] of a
 *   path) outside 0 .. G-1.
 * gvx3_get_shortcut is a synchronous read-back of resident shortcut s, modelled on gv_get_nav_path: the record into
 *   info, and the first min(n_waypoints, cap_out) waypoints into entries[cap_out], index[cap_out] and xy[cap_out * 2];
 *   each of the four may be NULL.  GV_ERR_BAD_ARG for a null handle, s outside 0..S-1 or cap_out < 0; GV_ERR_STATE with
 *   no resident shortcut.
 * gvx3_device_shortcut gives read-only device pointers to entries[S][wcap], index[S][wcap], xy[S][wcap][2] and info[S]
 *   and the S and wcap of the call that made them, valid until the next shortcut call or gv_destroy.  Each destination
 *   may be NULL.  GV_ERR_STATE with no resident shortcut.
 * gvx3_nav_field_from_shortcut solves X9's field seeded on the device with the written waypoints of resident shortcut
 *   s; their number is read on the device.  The field's bytes and n_seeds_used equal what
 *   gv_nav_field(h, <those waypoints' xy>, n_waypoints) gives; with spacing 1 this is the PathDist field of the
 *   straightened path.  A waypoint blocked in the costmap is skipped exactly as a seed is; n_waypoints == 0 is "no usable
 *   seed", not an error.  It waits on the host as gv_nav_field does and replaces the field as that does; the resident
 *   paths and shortcuts survive.  GV_ERR_BAD_ARG for a null handle or s out of range; GV_ERR_STATE with no resident
 *   shortcut, and the state errors of gv_nav_field_from_path.
 *
 * Not built: Euclidean or sub-cell smoothing, curvature limits, headings per waypoint, device-resident configuration,
 * the sharded grid, a FrameFlow switch.
 */
#ifndef GRIDVISION_HIP_SHORTCUT_H_
#define GRIDVISION_HIP_SHORTCUT_H_

#include "gridvision_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define GVX3_SHORTCUT_NO_CORNER (1u << 0)   /* flags of a call: a diagonal step of a line needs both flanking cells CLEAR */

#define GVX3_SHORTCUT_OK        0
#define GVX3_SHORTCUT_TRUNCATED 1
#define GVX3_SHORTCUT_EMPTY     2

#define GVX3_SHORTCUT_MAX_WINDOW  4096
#define GVX3_SHORTCUT_MAX_SPACING 65535
#define GVX3_SHORTCUT_MAX_WCAP    65536
#define GVX3_SHORTCUT_MAX_CELLS   (1 << 20)   /* S * wcap */

typedef struct {
  int32_t max_cost;
  int32_t window;
  int32_t spacing;
  uint32_t reserved[5];   /* 0 */
} gvx3_shortcut_config;   /* 32 bytes */

typedef struct {
  int32_t status;
  int32_t n_waypoints;
  int32_t n_anchors;
  int32_t n_src;
  int32_t n_steps;
  int32_t n_diag_steps;
  int32_t max_cost_seen;
  int32_t end_entry;
} gvx3_shortcut_info;     /* 32 bytes */

int gvx3_set_shortcut_config(gv_handle h, const gvx3_shortcut_config *cfg /* NULL: off */);
int gvx3_shortcut_async(gv_handle h, int32_t wcap, uint32_t flags, gvx3_shortcut_info *info /* S */,
                        float *way_xy /* S * wcap * 2, may be NULL */);
int gvx3_shortcut(gv_handle h, int32_t wcap, uint32_t flags, gvx3_shortcut_info *info /* S */,
                  float *way_xy /* S * wcap * 2, may be NULL */);
int gvx3_shortcut_host(uint8_t grid_x, uint8_t grid_y, double resolution, const uint8_t *cost, const gvx3_shortcut_config *cfg,
                       const int32_t *src_entries /* S * cap */, const int32_t *src_n /* S */, int32_t S, int32_t cap, int32_t wcap,
                       uint32_t flags, gvx3_shortcut_info *info /* S */, int32_t *entries /* S * wcap, may be NULL */,
                       int32_t *index /* S * wcap, may be NULL */, float *xy /* S * wcap * 2, may be NULL */);
int gvx3_get_shortcut(gv_handle h, int32_t s, int32_t *entries, int32_t *index, float *xy, int32_t cap_out, gvx3_shortcut_info *info);
int gvx3_device_shortcut(gv_handle h, int32_t **entries, int32_t **index, float **xy, gvx3_shortcut_info **info, int32_t *S,
                         int32_t *wcap);
int gvx3_nav_field_from_shortcut(gv_handle h, int32_t s, gv_nav_info *nav_info /* may be NULL */);

#ifdef __cplusplus
}
#endif
#endif /* GRIDVISION_HIP_SHORTCUT_H_ */
