// gv_launch_gain.hpp -- launchers of the gain kernels (gv_gain.hip); gv_api_gain.hip calls them.
// Every launcher only enqueues work on `s`; none allocates or synchronises.
#pragma once

#include <hip/hip_runtime.h>

#include "gv_gain.hpp"
#include "gv_launch_planner.hpp"   // NavArgs: the seed kernel stands beside k_nav_seeds, k_nav_seeds_path and k_nav_seeds_frontier

namespace gv {

// [EXTENSION] X20 information gain.  Everything is in OccupancyGrid.data order.  One workgroup per record slot: slot b of a
// list call is candidate entries[b]; of a frontier call the goal_entry of frontier record b while b < n_written (read on
// the device), a zero record behind that.
struct GainArgs {
  GridParams g;
  GainRule rule;
  int32_t n;                          // record slots: n of a list call, the frontier's cap of a frontier call
  uint32_t flags;                     // of the call
  const int8_t *i8;                   // the packed layer
  const uint32_t *field;              // G, read with GVX2_GAIN_USE_FIELD
  const int32_t *entries;             // n: a list call
  const gvx_frontier_record *frec;    // non-null: a frontier call; the resident frontier records ...
  const gvx_frontier_info *finfo;     // ... and info
  gvx2_gain_record *rec;              // n (resident)
  gvx2_gain_info *info;               // one (resident)
  gvx2_gain_record *rec_out;          // the device view of a pinned `out`, or null: written as well
  gvx2_gain_info *info_out;           // the device view of a pinned `info`, or null: written as well
};
// threads of a ray workgroup: a lane per ray, whole wavefronts, 1024 at the most
inline int32_t gain_threads(int32_t R)
{
  const int32_t t = (8 * R + 63) / 64 * 64;
  return t < 1024 ? t : 1024;
}
// the ray kernel and the finish kernel of a call, in order; false: the runtime refused the ray kernel's LDS size
// (hipGetLastError tells the caller)
bool launch_gain(const GainArgs &a, hipStream_t s);
// the seed of gvx2_nav_field_from_gain: launch_nav_seeds with the cell of resident record k (-1: of the resident best)
struct GainSeedArgs {
  const gvx2_gain_record *rec;
  const gvx2_gain_info *info;
  int32_t k;
};
void launch_nav_seeds_gain(const NavArgs &a, const GainSeedArgs &f, hipStream_t s);

}  // namespace gv
