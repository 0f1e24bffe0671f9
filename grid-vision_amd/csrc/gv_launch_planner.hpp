// gv_launch_planner.hpp -- launchers of the planner's and the controller's kernels: gv_inflate.hip, gv_trajscore.hip,
// gv_navfield.hip, gv_navpath.hip, gv_rollout.hip, gv_mppi.hip, gv_dynscore.hip and the tracker's update (gv_track.hip).
// gv_api_planner.hip, gv_api_control.hip and gv_api_path.hip call them.
// Every launcher only enqueues work on `s`; none allocates or synchronises.
#pragma once

#include <hip/hip_runtime.h>

#include "gv_types.hpp"
#include "gv_dyn.hpp"       // DynParams, DynObject
#include "gv_track.hpp"     // TrackParams, TrackEgo, TrackState
#include "gv_navpath.hpp"   // gv_nav_path_info
#include "gv_mppi.hpp"      // mppi_chunk_rows, mppi_tile_cols: the shapes MppiAverageArgs carries

namespace gv {

// [EXTENSION] X6 inflated costmap (gv_inflate.hip).  Everything is in OccupancyGrid.data order: "row" y, "column" x of
// byte y * nx + x of the packed layer (the cell order turned by 180 degrees; distances do not care).
// The lethal bitmap: one bit per cell along x, rows_words() 64-bit words per row = one zero guard word, the row's
// whole words (bits past nx zero), one zero guard word.  The guard words are zeroed once, when the buffer is made.
struct InflateArgs {
  int32_t nx, ny;
  int32_t row_words;            // words per bitmap row, guards included
  int32_t thr;                  // lethal iff (int8) v >= thr
  int32_t rc, d2max;            // search radius in cells, largest squared distance with a cost
  const int8_t *i8;             // the packed layer
  unsigned long long *bits;     // ny * row_words words
  const uint8_t *table;         // d2max + 1 costs (device)
  uint8_t *cost;                // G
  uint16_t *dist2;              // G or null
};
inline int32_t inflate_row_words(int32_t nx) { return (nx + 63) / 64 + 2; }
void launch_lethal_bits(const InflateArgs &a, hipStream_t s);
void launch_inflate_tiles(const InflateArgs &a, hipStream_t s);
// [EXTENSION] X7 trajectory scoring (gv_trajscore.hip): K trajectories of P poses against the costmap of gv_inflate.
// The footprint travels by value: a call already enqueued keeps the one it was enqueued with.
struct TrajArgs {
  GridParams g;
  gv_footprint fp;
  const float *poses;           // K * P * 3 (device)
  int32_t K, P;
  const uint8_t *cost;          // G, OccupancyGrid.data order: cell (ix, iy) is byte data_entry(g, ix, iy)
  gv_traj_score *scores;        // K records (device memory, or the device view of pinned host memory; 16-byte aligned)
  uint8_t *pose_cost;           // K * P, or null
};
void launch_score_trajectories(const TrajArgs &a, hipStream_t s);
// [EXTENSION] X9 goal / path distance field (gv_navfield.hip).  Everything is in OccupancyGrid.data order, as in X6.
// The field is relaxed tile by tile (kNavTile x kNavTile cells, one workgroup each) in rounds, one launch per round;
// flags_in[t] != 0: tile t has something to do this round (cleared by the tile), flags_out: the next round's.
constexpr int32_t kNavTile = 64;
constexpr int32_t kNavPassCap = 40;   // passes of a tile per round (gv_navfield.hip says where it comes from)
struct NavArgs {
  int32_t nx, ny, G;
  int32_t tiles_x, tiles_y;
  NavStep step;
  int32_t pass_cap;
  const uint8_t *cost;          // G (+ the costmap buffer's 16 bytes of slack)
  uint32_t *field;              // G rounded up to a multiple of 4
  const int32_t *seeds;         // n_seeds entries of the field (device)
  int32_t n_seeds;
  uint32_t *flags_in, *flags_out;   // tiles_x * tiles_y each
  uint32_t *counter;            // seeds: seeds used; a round: tiles that changed
};
void launch_nav_init(const NavArgs &a, hipStream_t s);    // BLOCKED / UNREACHABLE from the cost byte
void launch_nav_seeds(const NavArgs &a, hipStream_t s);   // 0 at the seeds, their tiles into flags_out
void launch_nav_relax(const NavArgs &a, hipStream_t s);   // one round
struct NavScoreArgs {
  GridParams g;
  const float *poses;           // K * P * 3 (device)
  int32_t K, P;
  const uint32_t *field;        // G
  gv_nav_score *scores;         // K records (device memory, or the device view of pinned host memory; 8-byte aligned)
};
void launch_score_nav(const NavScoreArgs &a, hipStream_t s);
// [EXTENSION] X17 path extraction from that field (gv_navpath.hip; the arithmetic is gv_navpath.hpp's): a wavefront
// per start walks the field downhill and leaves entries[S][cap], xy[S][cap][2] and S records in the handle's buffers.
struct PathArgs {
  GridParams g;
  const uint32_t *field;        // G
  const int32_t *starts;        // S data-order entries, -1: off the map (device)
  int32_t S, cap;
  uint32_t diagonal;            // GV_PATH_DIAGONAL of the call
  int32_t *entries;             // S * cap (resident)
  float *xy;                    // S * cap * 2 (resident)
  gv_nav_path_info *info;       // S (resident)
  float *xy_out;                // the device view of a pinned paths_xy, or null: written as well
  gv_nav_path_info *info_out;   // the device view of a pinned info, or null: written as well
};
void launch_nav_path(const PathArgs &a, hipStream_t s);
// the seeds of gv_nav_field_from_path: launch_nav_seeds with the cells of a resident path, n_cells read from its record
void launch_nav_seeds_path(const NavArgs &a, const gv_nav_path_info *rec, int32_t cap, hipStream_t s);
// [EXTENSION] X10 rollout and control step (gv_rollout.hip; the arithmetic is gv_motion.hpp's).  The motion model, the
// start and the weights travel by value: a call already enqueued keeps what it was enqueued with.
struct RolloutArgs {
  int32_t model;                // GV_MOTION_DIFF / GV_MOTION_OMNI
  double dt;
  double start[3];              // X, Y, T
  const float *controls;        // K * P * C floats, or K * C with `constant` (device)
  int32_t K, P;
  bool constant;
  float *poses;                 // K * P * 3 (device)
};
void launch_rollout(const RolloutArgs &a, hipStream_t s);
struct ControlSelectArgs {
  gv_critic_weights w;
  const gv_traj_score *traj;    // K records (device)
  const gv_nav_score *nav;      // K records (device), or null when no nav weight is set
  const gv_dyn_score *dyn;      // [EXTENSION] X13: K records (device), or null when no dyn configuration is set
  uint32_t w_dyn_sum, w_dyn_max;   // ... and its two weights
  int32_t K;
  gv_control_result *result;    // one record (device memory, or the device view of pinned host memory; 16-byte aligned)
  uint64_t *totals;             // K, or null (device memory, or the device view of pinned host memory)
};
void launch_control_select(const ControlSelectArgs &a, hipStream_t s);
// [EXTENSION] X11 MPPI sampling and softmax average (gv_mppi.hip; the arithmetic is gv_mppi.hpp's).  The configuration,
// the seed and the iteration travel by value; the nominal is read when the kernel runs.
struct MppiSampleArgs {
  gv_mppi_config cfg;
  int32_t C;                    // floats per step of the motion model in force
  int32_t K, P;
  uint64_t seed, iteration;
  bool shift;                   // GV_MPPI_SHIFT
  const float *nominal;         // P * C (device)
  float *controls;              // K * P * C (device)
};
void launch_mppi_sample(const MppiSampleArgs &a, hipStream_t s);
// The two launches of the average.  `result` and `totals` are what k_control_select left in device memory; the *_out
// pointers are device views of pinned host memory, or null (the caller then enqueues a copy command).
struct MppiAverageArgs {
  double lambda;
  int32_t K, J;                 // trajectories, columns P * C
  int32_t rows, tile;           // mppi_chunk_rows(K, J), mppi_tile_cols(J)
  const float *controls;        // K * J (device)
  const uint64_t *totals;       // K (device)
  const gv_control_result *result;   // one record (device)
  double *partial;              // chunks * J sums, then chunks weights: chunks = ceil(K / rows)
  float *nominal;               // J (device): rewritten unless no trajectory is admitted
  uint64_t *totals_out;         // K, or null
  gv_control_result *result_out;   // one record (16-byte aligned), or null
  float *nominal_out;           // J, or null
  const double *x;              // [EXTENSION] X12, with gamma > 0: x_k of the admitted (K, device), else null
  const uint64_t *x_min_key;    // ... and mppi_min_key of their minimum (device), else null
};
void launch_mppi_average(const MppiAverageArgs &a, hipStream_t s);
// [EXTENSION] X12 the chain over the sampled controls, in place, behind k_mppi_sample (gv_mppi.hip).
struct MppiConstrainArgs {
  MppiChain chain;
  int32_t C;
  int32_t K, P;
  float *controls;              // K * P * C (device)
};
void launch_mppi_constrain(const MppiConstrainArgs &a, hipStream_t s);
// [EXTENSION] X12 the control cost of every trajectory and the minimum of x over the admitted, behind k_control_select.
// The caller clears *x_min_key to all ones on the stream in front of the launch.
struct MppiCostArgs {
  double qc[3];                 // mppi_cost_scale per channel
  int32_t C;
  int32_t K, P;
  bool shift;                   // the GV_MPPI_SHIFT of the sampling that made the controls
  const float *nominal;         // P * C (device)
  const float *controls;        // K * P * C (device)
  const uint64_t *totals;       // K (device)
  const gv_control_result *result;   // one record (device)
  double *g;                    // K (device)
  double *x;                    // K (device): written for the admitted
  uint64_t *x_min_key;          // one (device)
};
void launch_mppi_control_cost(const MppiCostArgs &a, hipStream_t s);
// [EXTENSION] X13 scoring against predicted moving objects (gv_dynscore.hip; the arithmetic is gv_dyn.hpp's).  The
// configuration and the number of objects travel by value; the object table and the cost table are read when the
// kernel runs, behind the copy commands that filled them on the same stream.
struct DynArgs {
  DynParams p;
  const float *poses;           // K * P * 3 (device)
  int32_t K, P;
  const DynObject *objs;        // n_obj rows (device); not read when n_obj == 0
  int32_t n_obj;                // 0 .. kDynMaxObjects
  const uint8_t *table;         // p.T costs (device)
  gv_dyn_score *scores;         // K records (device memory, or the device view of pinned host memory; 8-byte aligned)
  uint8_t *pose_cost;           // K * P, or null
  const int32_t *n_obj_dev;     // [EXTENSION] X14: null, or the count of a set a fed gv_track_update wrote on the device;
                                // read once per workgroup, clamped to 0 .. kDynMaxObjects, and n_obj is not used
};
void launch_score_dynamic(const DynArgs &a, hipStream_t s);
// [EXTENSION] X14 one update of the tracker (gv_track.hip; the arithmetic is gv_track.hpp's).  The configuration, dt and
// the motion travel by value.  One workgroup rewrites `state` in place.
struct TrackArgs {
  TrackParams p;
  TrackEgo ego;                 // ego.on == 0: no motion given
  double dt;
  int32_t fresh;                // != 0: the state is the one after gv_create whatever the block holds
  int32_t n;                    // detections, 0 .. kTrackSlots
  const gv_lshape_pose *dets;   // n records (device); not read when n == 0
  TrackState *state;            // device
  gv_track_info *info;          // one record or null (device memory, or the device view of pinned host memory)
  gv_track *tracks;             // kTrackSlots records or null (likewise; 8-byte aligned)
  DynObject *feed_objs;         // kTrackSlots rows of X13's object table or null (device)
  int32_t *feed_n;              // their count, beside them; null with feed_objs
  const int32_t *n_dev;         // [EXTENSION] X15: null, or the count of a tick's detection list (device); read instead of n
};
void launch_track_update(const TrackArgs &a, hipStream_t s);

}  // namespace gv
