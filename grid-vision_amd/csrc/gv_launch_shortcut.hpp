// gv_launch_shortcut.hpp -- launchers of the shortcut kernels (gv_shortcut.hip); gv_api_shortcut.hip calls them.
// Every launcher only enqueues work on `s`; none allocates or synchronises.
#pragma once

#include <hip/hip_runtime.h>

#include "gv_shortcut.hpp"
#include "gv_launch_planner.hpp"   // NavArgs: the seed kernel stands beside k_nav_seeds and k_nav_seeds_path

namespace gv {

// [EXTENSION] X21 shortcuts and waypoints.  Everything is in OccupancyGrid.data order.  One workgroup per resident path.
struct ShortcutArgs {
  GridParams g;
  ShortcutRule rule;
  int32_t S, cap, wcap;                // of the resident paths; the room of one shortcut, in waypoints
  const uint8_t *cost;                 // G: the costmap of the last gv_inflate
  const int32_t *src_entries;          // S * cap: the resident paths ...
  const gv_nav_path_info *src_info;    // ... and their records
  int32_t *entries, *index;            // S * wcap each (resident)
  float *xy;                           // S * wcap * 2 (resident)
  gvx3_shortcut_info *info;            // S (resident)
  float *xy_out;                       // the device view of a pinned way_xy, or null: written as well
  gvx3_shortcut_info *info_out;        // the device view of a pinned info, or null: written as well
};
void launch_shortcut(const ShortcutArgs &a, hipStream_t s);
// the seeds of gvx3_nav_field_from_shortcut: launch_nav_seeds with the waypoints of a resident shortcut (a.seeds),
// n_waypoints read from its record
void launch_nav_seeds_shortcut(const NavArgs &a, const gvx3_shortcut_info *rec, int32_t wcap, hipStream_t s);

}  // namespace gv
