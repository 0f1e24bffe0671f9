/*
 * gridvision_hip_path.h -- [EXTENSION] X17: extract paths from the distance field of X9, on the device.
 *
 * A header of its own beside gridvision_hip.h, like gridvision_hip_match.h.  gridvision_hip.h includes it at its end
 * and is otherwise as it was (its 123 entry points and ABI version 4); libgridvision_hip.so exports the six functions
 * declared here as well.  The reference has no such step; this text is the definition, and the device call, the host
 * twin and the tests' plain reference all give its bytes.
 *
 * What it is.  gv_nav_field (X9) leaves NavFn's potential on the device: the geodesic distance of every cell from the
 * seeds.  The step every user of such a field takes next is to walk it downhill from the vehicle to the goal: the path
 * (NavFn's and MapGridCritic's users do it on the host).  gv_nav_path walks it on the device for S starts at once and
 * keeps the paths there, and gv_nav_field_from_path seeds the next field with every cell of such a path -- the field
 * nav2's PathDist critic reads -- so that plan, then follow the plan, never crosses the host.
 *
 * Input field.  The field of the last gv_nav_field: uint32, G entries in OccupancyGrid.data order, entry e = y * nx + x,
 *   GV_NAV_BLOCKED and GV_NAV_UNREACHABLE as X9 defines them.  The path call reads only the field, never the costmap,
 *   so it is consistent with the snapshot the field is.
 * Starts.  starts_xy[S][2], float32 in the grid's frame, host memory, copied before the call returns.  Each goes through
 *   the grid's own getIndex on ((double)x, (double)y), exactly as a seed of gv_nav_field does.  S in 1..256, cap in
 *   1..65536 (the room of one path, in cells), S * cap <= 2^20.
 * Descent.  From the start cell: cur the current cell, (x, y) its entry coordinates, v its value.  While v != 0:
 *     the candidates are tried in this fixed order, in entry coordinates: (x-1, y), (x+1, y), (x, y-1), (x, y+1);
 *     with GV_PATH_DIAGONAL, a flag of the call, these follow: (x-1, y-1), (x+1, y-1), (x-1, y+1), (x+1, y+1);
 *     a candidate COUNTS when it is on the map (0 <= x < nx, 0 <= y < ny) and its value is STRICTLY SMALLER than the
 *       best so far; the best starts at v;
 *     a diagonal (x+dx, y+dy) counts only if both flanking cells, (x+dx, y) and (x, y+dy), are not GV_NAV_BLOCKED: no
 *       corner is cut;
 *     the last candidate that lowered the best is the next cell, so ties go to the earlier candidate.
 *   Nothing wraps across a row end.  On a field of gv_nav_field every reachable cell that is no seed has a 4-neighbour
 *   smaller by exactly step[cost], so the walk ends at a seed.  Values strictly decrease, so no input -- not even an
 *   arbitrary array handed to the host twin -- makes it loop without bound.
 * Output per start s.
 *   entries[s][cap]  int32 data-order entries, the start cell first, the seed cell last.
 *   xy[s][cap][2]    float32 cell centres.  With ix = nx-1-x and iy = ny-1-y:
 *                      X = (float)((pos_x + off_x) - ((double)ix + 0.5) * res),  Y likewise with iy, pos_y, off_y
 *                    (pos the map's centre, off half its length), each operation in fp64 and the result rounded once.
 *                    getIndex takes every such centre back to its own cell.
 *   Slots of both past n_cells hold unspecified values.
 *   gv_nav_path_info, 32 bytes, every byte defined:
 *     status       GV_PATH_REACHED      0  ended on a value-0 cell (also when that is cell number cap)
 *                  GV_PATH_TRUNCATED    1  cap cells written and the last one is no seed
 *                  GV_PATH_OFF_MAP      2  the start fails getIndex (non-finite included); n_cells 0
 *                  GV_PATH_BLOCKED      3  the start's cell is GV_NAV_BLOCKED; n_cells 0
 *                  GV_PATH_UNREACHABLE  4  the start's cell is GV_NAV_UNREACHABLE; n_cells 0
 *                  GV_PATH_STUCK        5  no candidate is smaller and v != 0.  A field of gv_nav_field never gives
 *                                          it; it exists for the arbitrary input of the host twin.
 *     n_cells      cells written
 *     start_value  the field at the start; GV_NAV_BLOCKED off the map
 *     end_value    the field at the last cell written, 0 when reached; start_value when n_cells == 0
 *     start_entry  -1 off the map
 *     end_entry    the last cell written; -1 when n_cells == 0
 *     n_diagonal   diagonal moves taken
 *     reserved     0
 *
 * Calls.  gv_nav_path_async enqueues on gv_stream(h): a copy of the start cells and one kernel, ordered like
 *   gv_score_nav_async and allowed wherever that is, between gv_tick_enqueue and gv_tick_wait too.  The paths stay
 *   RESIDENT in buffers of the handle's own (entries, xy and the S records) until the next path call or gv_reset.
 *   info[S] and, when not NULL, paths_xy[S * cap * 2] follow gv_score_nav_async's destination rules: pinned memory
 *   (gv_host_alloc; info 16-byte, paths_xy 8-byte aligned) is written by the kernel in place, anything else through
 *   a copy command behind it; both are complete once the stream has been waited for.  With paths_xy NULL the paths
 *   stay resident only.  GV_ERR_BAD_ARG, state unchanged, for a null handle, starts_xy or info, S, cap or S * cap out
 *   of range, flags other than GV_PATH_DIAGONAL.  GV_ERR_STATE before the first field since gv_create / gv_reset and
 *   with a communicator of more than one rank.  gv_nav_path is the same call followed by the wait.
 * gv_nav_path_host is the host twin (no handle, no GPU): the same arithmetic text compiled for the host over the
 *   geometry gv_create gives grid_x, grid_y and resolution (the arguments of gv_footprint_cells) and ANY field of G
 *   values.  entries[S * cap] and paths_xy[S * cap * 2] may each be NULL.  GV_ERR_BAD_ARG for what the call above
 *   refuses, a null field and an invalid geometry.
 * gv_get_nav_path is a synchronous read-back of resident path s: the record into info, and the first
 *   min(n_cells, cap_out) cells into entries[cap_out] and xy[cap_out * 2]; each of the three may be NULL.
 *   GV_ERR_BAD_ARG for a null handle, s outside 0..S-1 or cap_out < 0; GV_ERR_STATE with no resident path.
 * gv_device_nav_path gives the device pointers of entries[S][cap], xy[S][cap][2] and info[S] and the S and cap of the
 *   call that made them, for device-side consumers: read-only, valid until the next path call or gv_destroy.  Each
 *   destination may be NULL.  GV_ERR_STATE with no resident path.
 * gv_nav_field_from_path solves the field seeded by every cell of resident path s.  The field's bytes and
 *   n_seeds_used equal what gv_nav_field(h, <that path's xy>, n_cells) gives; neither the path nor its length crosses
 *   the host first.  It reads the costmap of the last gv_inflate and the configuration in force now, so a path cell
 *   blocked since then is skipped exactly as a seed is; n_cells == 0 is "no usable seed", not an error.  It waits on
 *   the host as gv_nav_field does and replaces the field as that does.  The resident paths survive it.
 *   GV_ERR_BAD_ARG for a null handle or s out of range; GV_ERR_STATE with no resident path, no configuration, no
 *   costmap, or a communicator of more than one rank.
 *
 * Not built: NavFn's interpolated gradient (sub-cell paths), path smoothing and a thinning stride, device-resident
 * starts, paths on a sharded grid.
 */
#ifndef GRIDVISION_HIP_PATH_H_
#define GRIDVISION_HIP_PATH_H_

#include "gridvision_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define GV_PATH_DIAGONAL (1u << 0)   /* flags of a call: the four diagonal candidates follow the four straight ones */

#define GV_PATH_REACHED     0
#define GV_PATH_TRUNCATED   1
#define GV_PATH_OFF_MAP     2
#define GV_PATH_BLOCKED     3
#define GV_PATH_UNREACHABLE 4
#define GV_PATH_STUCK       5

typedef struct {
  int32_t status;
  int32_t n_cells;
  uint32_t start_value, end_value;
  int32_t start_entry, end_entry;
  int32_t n_diagonal;
  uint32_t reserved;   /* 0 */
} gv_nav_path_info;    /* 32 bytes */

int gv_nav_path_async(gv_handle h, const float *starts_xy, int32_t S, int32_t cap, uint32_t flags, gv_nav_path_info *info,
                      float *paths_xy /* S * cap * 2, may be NULL */);
int gv_nav_path(gv_handle h, const float *starts_xy, int32_t S, int32_t cap, uint32_t flags, gv_nav_path_info *info,
                float *paths_xy /* S * cap * 2, may be NULL */);
int gv_nav_path_host(uint8_t grid_x, uint8_t grid_y, double resolution, const uint32_t *field, const float *starts_xy,
                     int32_t S, int32_t cap, uint32_t flags, gv_nav_path_info *info, int32_t *entries /* may be NULL */,
                     float *paths_xy /* may be NULL */);
int gv_get_nav_path(gv_handle h, int32_t s, int32_t *entries, float *xy, int32_t cap_out, gv_nav_path_info *info);
int gv_device_nav_path(gv_handle h, int32_t **entries, float **xy, gv_nav_path_info **info, int32_t *S, int32_t *cap);
int gv_nav_field_from_path(gv_handle h, int32_t s, gv_nav_info *info /* may be NULL */);

#ifdef __cplusplus
}
#endif
#endif /* GRIDVISION_HIP_PATH_H_ */
