// gv_types.hpp -- POD parameter blocks shared by the host side (gv_api*.hip)
// and the gfx950 kernels, passed by value as kernel arguments, and the few functions of the grid's
// geometry that host and device evaluate from one text (GV_HD, as gv_line.hpp does).
#pragma once

#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>   // float4 (BBoxTest)
#endif

#include "../../include/gridvision_hip.h"
#include "gv_line.hpp"   // GV_HD

namespace gv {

// Geometry of the resident grid (grid_map conventions, src/occupancy_grid.cpp:4-14).
// Layers are stored exactly like grid_map's column-major MatrixXf(size0,size1):
// linear cell = iy*nx + ix, ix = x index (fastest), (0,0) = +x,+y corner.
struct GridParams {
  int32_t nx, ny, G;
  double res;
  double len_x, len_y;   // size * res
  double pos_x, pos_y;   // map centre
  double off_x, off_y;   // 0.5 * len
  double inv_res;        // fl64(1 / res): quotient estimate of the points pass (never the result itself)
};

// grid_map::GridMap::getIndex (called at src/occupancy_grid.cpp:152), the one text of it for the kernels and for the
// host twins of gv_host_math.hpp (footprint_cells, nav_seed_entry, the sensor origin's cell):
//   indexVector = (position - 0.5*length - mapPosition) / resolution, index = (int)(-indexVector)
//   inside iff t = -(position - mapPosition - 0.5*length), 0 <= t < length
// Built with -ffp-contract=off everywhere: separate roundings, exact fp64 divisions.
GV_HD bool get_index(const GridParams &g, double x, double y, int &ix, int &iy)
{
  const double tx = -((x - g.pos_x) - g.off_x);
  const double ty = -((y - g.pos_y) - g.off_y);
  if (!(tx >= 0.0 && ty >= 0.0 && tx < g.len_x && ty < g.len_y)) return false;  // NaN/inf land here
  const double vx = ((x - g.off_x) - g.pos_x) / g.res;
  const double vy = ((y - g.off_y) - g.pos_y) / g.res;
  const int jx = (int)(-vx);
  const int jy = (int)(-vy);
  if (jx < 0 || jy < 0 || jx >= g.nx || jy >= g.ny) return false;
  ix = jx;
  iy = jy;
  return true;
}

// The OccupancyGrid.data order rule (toOccupancyGrid, src/occupancy_grid.cpp): cell (ix, iy) of a layer stored in that
// order -- the packed grid, the costmap, the distance field -- is entry G - 1 - (iy * nx + ix).
GV_HD int32_t data_entry(const GridParams &g, int ix, int iy) { return g.G - 1 - (iy * g.nx + ix); }

// Row-major 3x4 fp32 rigid transform (the top of PCL's 4x4).
struct Mat34f {
  float m[12];
};

// fp64 rigid transform as tf2 applies it (basis rows + origin).
struct Xform64 {
  double b[9];
  double o[3];
};

struct CamK {
  double k[9];   // row-major K
  int32_t W, H;  // image width / height
};

#if defined(__HIPCC__)   // (names a HIP vector type: the host twins that plain g++ compiles do not see it)
// exact fp32 form of the bbox test + per-16x16-pixel-tile candidate masks (built on the device by
// launch_bbox_prepare from the uploaded gv_bbox array)
struct BBoxTest {
  const float4 *bbox_f;                  // (x_min, y_min, x_max, y_max) as float thresholds
  const unsigned long long *tile_mask;   // [tiles_y][tiles_x][mask_words]
  int32_t tiles_x, tiles_y, mask_words;
};
#endif

// sensor origin for the X2 ray-march
struct RayOrigin {
  double ox, oy;      // base-frame position of the lidar origin
  int32_t cx, cy;     // its cell
  int32_t valid;      // 0: origin outside the map -> no rays this frame
};

// [EXTENSION] X4 height band of the lidar map update (gv_set_height_band).  Base-frame z < z_ground: ground return
// (the end of a free-space ray, own cell included, when clears; else dropped), z > z_max: dropped.  Off is
// {-inf, +inf, 0}: every finite point is an obstacle, as without the band.
struct HeightBand {
  float z_ground, z_max;
  int32_t clears;
};

// [EXTENSION] X9 distance field (gv_set_nav_config): what entering a cell of cost byte v costs, 0 for a blocked cell.
// The one text of the definition: gv_nav_step_table on the host, the kernels of gv_navfield.hip on the device.
struct NavStep {
  int32_t obstacle_cost, cost_weight;
};
GV_HD uint32_t nav_step(NavStep s, uint32_t v)
{
  return (int32_t)v >= s.obstacle_cost ? 0u : 1u + (uint32_t)s.cost_weight * v;
}

// [EXTENSION] X12 limits on MPPI's sampled controls (gv_set_mppi_limits) as the chain reads them: the largest step up
// and down of a channel (rate * dt), the control in force before step 0 (NaN: free), 1 / min_turn_radius (0: none).
struct MppiChain {
  float up[3], dn[3];
  float u_prev[3];
  float inv_r;
};

// ---- sector ray stage (gv_raysector.hip): what the kernel and the host's plan (host::SectorPlan) size LDS by
constexpr int kSecThreads = 512;   // 8 wavefronts per sector workgroup
// Ends of a slope bucket: the first kSlots in the bucket's own row of a table, in arrival order; what a crowded bucket
// holds beyond that (the buckets of the few rational slopes many ends share) goes to one overflow list.  No count /
// prefix / placement passes: an end is placed the moment its bucket is known.
constexpr int kSlotLog = 3, kSlots = 1 << kSlotLog;
#ifndef GV_SLOT_TOTAL
#define GV_SLOT_TOTAL 2048
#endif
constexpr int kSlotTotal = GV_SLOT_TOTAL;   // a wedge with more ends than this (4 per bucket: measured, config 3 and config 5) is placed by counting sort instead

// LDS layout of one sector workgroup (bytes), shared by the kernel and the plan
struct SectorLds {
  size_t tab, marks, cnt, bstart, bmax32, lvl, pfx, sfx, raw, over, total;
};
GV_HD SectorLds sector_lds_layout(int cap, int marks_words, int log2m)
{
  const size_t M = (size_t)1 << log2m;
  SectorLds L;
  size_t o = 0;
  L.tab = o;    o += (M * kSlots > (size_t)cap ? M * kSlots : (size_t)cap) * 4;   // [M][kSlots] packed ends (16-byte aligned rows); a crowded group: cap ends grouped by bucket
  L.raw = o;    o += (size_t)cap * 4;           // packed ends in scan order (staging list; the long-ray pass reads it too)
  L.over = o;   o += (size_t)(cap > 2 * kSlotTotal ? cap : 2 * kSlotTotal) * 4;   // overflow entries: bucket << 16 | index into raw -- two lists of
                                                // kSlotTotal (as placed / after the same-slope merge); a crowded group: cap bucket numbers (16 bit)
  L.marks = o;  o += (size_t)marks_words * 4;
  L.cnt = o;    o += M * 4;                     // ends per bucket (may exceed kSlots); a crowded group: the end of every bucket's run
  L.bstart = o; o += M * 4;                     // a crowded group: the start of every bucket's run
  L.bmax32 = o; o += 2 * M * 4;                 // bucket max reach; dead once the range-max tables are built: then the long-ray list (2M entries)
  L.lvl = o;
  L.pfx = L.lvl + 7 * M * 2;                    // in-block (64 buckets) sparse levels 0..6
  L.sfx = L.pfx + M * 2;
  o += 9 * M * 2;
  L.total = (o + 15) & ~(size_t)15;
  return L;
}

// Inclusive index rectangle of one object (updateGridCellsFast block).
struct Rect {
  int32_t x0, y0, x1, y1;
  int32_t valid;
};

// device-side result of the vision-orientation geometry for one bbox
struct VisionOut {
  float loc[3];
  float orient;     // alpha + theta_ray
  float err;
  float dims[3];    // length, width, height (fp32 sums, :474-476)
  int32_t valid;    // 0 for classes the reference skips (:496-499)
};

// Completion of a synchronous call without a copy command or a runtime wait: the call's last kernel stores its
// (small) results straight into pinned, device-mapped host memory, every workgroup then takes a ticket, and the
// one whose ticket comes last publishes the call's sequence number in the block's first word -- the host spins on
// that word (tools/micro/call_latency.hip: 8 us instead of 31 for copy + hipStreamSynchronize).  flag == nullptr:
// plain device outputs, nothing published.  (The device side, call_done, is gv_device.hpp's.)
struct CallDone {
  unsigned *ticket = nullptr;   // device memory, zero between calls
  unsigned *flag = nullptr;     // host-mapped
  unsigned seq = 0;
};

// reference constants, include/grid_vision/occupancy_grid.hpp:25-31, occupancy_grid.cpp:182
constexpr float kLogOddsFree = -0.4f;
constexpr float kLogOddsOccupied = 1.2f;
constexpr float kLogOddsPrior = 0.0f;
constexpr float kInitProbability = 0.5f;
constexpr float kLogOddsDecay = -0.2f;
constexpr float kMinLogOdds = -2.0f;
constexpr float kMaxLogOdds = 3.6f;
constexpr float kRectIncrement = 0.85f;

enum Stage : int {
  kStageDetections = 0,  // vision-orientation geometry + rectangles
  kStagePoints = 1,      // transform + bin + ray ends + bbox test
  kStageRayCompact = 2,
  kStageRayMarch = 3,
  kStageFinalize = 4,
  kNumStages = 5
};

}  // namespace gv
