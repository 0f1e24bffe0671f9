// gv_kernels.hpp -- launchers of the gfx950 kernels (defined in gv_kernels.hip).
// Every launcher only enqueues work on `s`; none allocates or synchronises.
#pragma once

#include <hip/hip_runtime.h>

#include "gv_types.hpp"
#include "gv_dyn.hpp"
#include "gv_track.hpp"
#include "gv_match.hpp"
#include "gv_navpath.hpp"
#include "gv_search.hpp"
#include "gv_pose_math.hpp"

namespace gv {

// exact fp32 form of the bbox test + per-16x16-pixel-tile candidate masks (built on the device by
// launch_bbox_prepare from the uploaded gv_bbox array)
// Diagnostic build only (-DGV_DIAG, GV_TIMELINE=1): every workgroup of a launch reports the constant-rate clock when
// it starts and when it ends; min / max over the launch = the kernel's residence on the device, taken without any
// packet in the queues (tools/native_timeline.py).  Nothing in the shipped kernels.
#ifdef GV_DIAG
// (begin: the first workgroup of the launch only; end: every eighth workgroup -- one atomic per workgroup on one
//  address slowed the 1024-workgroup grid pass by a third)
#define GV_TL_LINEAR_ID (blockIdx.x + blockIdx.y * gridDim.x)
#define GV_TL_BEGIN(tl) do { if ((tl) && threadIdx.x == 0 && GV_TL_LINEAR_ID == 0) atomicMin(&(tl)[0], (unsigned long long)__builtin_amdgcn_s_memrealtime()); } while (0)
#define GV_TL_END(tl) do { if ((tl) && threadIdx.x == 0 && (GV_TL_LINEAR_ID & 7u) == 0) atomicMax(&(tl)[1], (unsigned long long)__builtin_amdgcn_s_memrealtime()); } while (0)
#else
#define GV_TL_BEGIN(tl) do { } while (0)
#define GV_TL_END(tl) do { } while (0)
#endif

struct BBoxTest {
  const float4 *bbox_f;                  // (x_min, y_min, x_max, y_max) as float thresholds
  const unsigned long long *tile_mask;   // [tiles_y][tiles_x][mask_words]
  int32_t tiles_x, tiles_y, mask_words;
};

struct PointsArgs {
  const float *x, *y, *z;
  uint32_t n;
  GridParams g;
  Mat34f m_base;     // base <- lidar   (X1/X2)
  Mat34f m_cam;      // camera <- lidar (A1/A5)
  CamK cam;
  RayOrigin org;
  BBoxTest bt;
  int32_t *hits;       // G   hits[cell] += 1
  uint8_t *clip_end;   // G
  int32_t *cell_idx;   // N or null
  int16_t *bbox_id;    // N or null
  bool do_bin, do_ray, do_bbox;
  HeightBand band;     // X4: which binned points count as hits / ray ends (off: {-inf, +inf, 0})
};
void launch_points(const PointsArgs &a, hipStream_t s);
// float thresholds + 16x16-pixel tile candidate masks of the bbox test, from the device copy of the bboxes
// copy_src / copy_dst / copy_bytes (optional): the kernel also copies that many bytes (rounded up to 16) first -- the
// detection block from its pinned, device-visible staging, `bboxes` then pointing into the staging
void launch_bbox_prepare(const gv_bbox *bboxes, int32_t nb, int32_t tiles_x, int32_t tiles_y, int32_t mask_words,
                         float4 *bbox_f, unsigned long long *tile_mask, hipStream_t s, const void *copy_src = nullptr,
                         void *copy_dst = nullptr, size_t copy_bytes = 0);

void launch_transform_cloud(const float *x, const float *y, const float *z, uint32_t n, const Mat34f &m,
                            float *ox, float *oy, float *oz, hipStream_t s);
void launch_deinterleave(const uint8_t *data, uint32_t n, uint32_t point_step, uint32_t off_x,
                         uint32_t off_y, uint32_t off_z, float *x, float *y, float *z, hipStream_t s);

// poses -> index rectangles (updateMap corners + updateGridCellsFast index part).
// from_cam: poses are camera-frame, apply `bc` (base <- camera) to the position first.
void launch_rects_from_poses(const gv_lshape_pose *poses, int32_t n, const GridParams &g, bool from_cam,
                             const Xform64 &bc, Rect *rects, hipStream_t s);
// dead-code overload: centre points + class depth (computeBoundingBox3D)
void launch_rects_from_points(const double *pts_xyz, const gv_bbox *bboxes, int32_t n,
                              const GridParams &g, Rect *rects, hipStream_t s);

// vision-orientation geometry, one wavefront per bbox; also emits camera-frame
// gv_lshape_pose (position + dims only; the quaternion is filled by the host).  sets: nullptr in the product; the
// test hook gv_test_vision_sets passes nb * 64 * 4 floats (loc0, loc1, loc2, err of every lane) + nb int32 (winner).
// out_dev: nullptr, or (a GV_TICK_KEEP_DETS tick, X15) device memory for a second copy of `out`, which is usually pinned
void launch_vision(const float *orient, const float *conf, const float *dims, const gv_bbox *bboxes,
                   int32_t nb, const gv_cam_params &cam, VisionOut *out, gv_lshape_pose *poses_cam, float *sets,
                   VisionOut *out_dev, hipStream_t s);

void launch_ray_compact(const int32_t *hits, const uint8_t *clip_end, const GridParams &g,
                        uint32_t *list, uint32_t *count, hipStream_t s);
void launch_ray_march(const uint32_t *list, const uint32_t *count, const GridParams &g,
                      const RayOrigin &org, uint8_t *miss, unsigned long long *stats, hipStream_t s);

struct FinalizeArgs {
  GridParams g;
  float *log_odds, *occupancy;
  int8_t *occ_i8;          // OccupancyGrid.data order (reversed linear)
  const Rect *rects;
  int32_t n_rects;
  int32_t *hits;           // null => no hit/miss rule (plain updateMap)
  uint8_t *miss;
  uint8_t *clip_end;
  bool zero_counts;        // clear hits/miss/clip_end for the next frame
  int64_t cell_begin, cell_end;   // band of cells to finalise ([0,G) on one GPU)
};
void launch_finalize(const FinalizeArgs &a, hipStream_t s);

void launch_fill_f32(float *p, float v, size_t n, hipStream_t s);

// [EXTENSION] X3 ego motion (gv_gridmove.hip): the three layers resampled under the planar transform S into a scratch
// copy, then copied back into place (the resident pointers stay the same)
struct GridMoveArgs {
  GridParams g;
  double c, s, tx, ty;        // S: cos / sin of its yaw, translation in metres
  float *lo, *occ;            // resident layers
  int8_t *i8;
  float *lo_out, *occ_out;    // scratch copy (16-byte aligned)
  int8_t *i8_out;
};
void launch_grid_move(const GridMoveArgs &a, hipStream_t s);             // resident -> scratch
void launch_grid_move_copy_back(const GridMoveArgs &a, hipStream_t s);   // scratch -> resident
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
struct RansacState;
// [EXTENSION] X15 the tick's detection list (gv_track.hip, k_tick_dets; the arithmetic is gv_pose_math.hpp's): the valid
// candidates of a tick's pose branch in order, in the base frame, into `out`.  One workgroup.
struct TickDetsArgs {
  int32_t mode;                 // kTickDetsNone: an empty list; kTickDetsVision: candidates are vout; kTickDetsPca: cam + valid
  int32_t n_cand;               // 0 .. kTickDetCandidates
  const VisionOut *vout;        // vision: n_cand records (device)
  const gv_lshape_pose *cam;    // PCA: n_cand camera-frame poses (device)
  const uint8_t *valid;         // PCA: n_cand flags (device)
  const RansacState *st;        // PCA: the ground plane's state (device): decides "empty segmented cloud"
  uint64_t n_cloud;             // PCA: points of the cloud the tick read
  gv_transform tf_bc;           // base <- camera
  TickDetList *out;             // device
};
enum : int32_t { kTickDetsNone = 0, kTickDetsVision = 1, kTickDetsPca = 2 };
void launch_tick_dets(const TickDetsArgs &a, hipStream_t s);
// [EXTENSION] X16 scan-to-costmap matching (gv_match.hip; the arithmetic is gv_match.hpp's).  The configuration, the
// guess and the host-built rotation table travel by value: a call already enqueued keeps what it was enqueued with.
// `head` is one zeroed block per call: word 0 counts the used points, the volume starts at word kMatchHeadWords.
// The point pass (k_match_points) is the one kernel that reads the cloud, and both matchers run it: it has an argument
// block of its own, over the calling matcher's `pts` and the counter word of its `head`.
struct MatchPointsArgs {
  Mat34f m_base;
  HeightBand band;
  const float *x, *y, *z;       // the resident cloud (device)
  uint32_t n;                   // its points
  uint32_t n_sel;               // ceil(n / stride): the selected ones, point sel * stride each
  int32_t stride;
  uint32_t use_band;
  float2 *pts;                  // n_sel pairs (device): the used points' (bx, by), in any order
  uint32_t *used;               // their count (device), zero when the pass starts
};
void launch_match_points(const MatchPointsArgs &a, hipStream_t s);
constexpr int32_t kMatchHeadWords = 4;
struct MatchArgs {
  GridParams g;
  MatchParams p;
  uint32_t n_sel;               // ceil(n / stride): the bound on the used points
  const float2 *pts;            // the used points' (bx, by) (device)
  uint32_t *head;               // kMatchHeadWords + NT*NY*NX words (device), zero when the point pass starts
  const uint8_t *cost;          // the resident costmap
  gv_match_result *result;      // one record (device memory, or the device view of pinned host memory; 8-byte aligned)
  uint32_t *scores_out;         // null, or the device view of a pinned destination of the volume
  float rot[2 * kMatchMaxSide]; // (c_t, s_t), NT pairs
};
void launch_match_score(const MatchArgs &a, hipStream_t s);
void launch_match_select(const MatchArgs &a, hipStream_t s);
// [EXTENSION] X18 wide-window matching by branch and bound (gv_search.hip; the arithmetic is gv_search.hpp's and
// gv_match.hpp's).  The point pass is X16's, given a MatchPointsArgs over this call's `head` and `pts`.  `head` is one zeroed
// block per call: the counters below, the two pre-slots (the seed block's exact scores, then the centre block's), then
// the bounds B[n_blocks].
enum : int32_t {
  kSearchUsed = 0,        // n_used (the point pass counts here)
  kSearchSurvivors = 1,   // n_survivors
  kSearchScored = 2,      // n_scored
  kSearchLower = 3,       // L
  kSearchSeedKey = 4,     // uint64: the largest search_seed_key
  kSearchBoundSum = 6,    // uint64
  kSearchBestKey = 8,     // uint64: the largest match_key over the survivors' candidates
  kSearchPre = 16,        // 2 * kSearchMaxS2 words
  kSearchBounds = kSearchPre + 2 * kSearchMaxS2,
};
struct SearchArgs {
  GridParams g;
  SearchParams sp;
  uint32_t n_sel;               // ceil(n / stride): the bound on the used points
  uint32_t n_blocks;
  const float2 *pts;            // the used points' (bx, by) (device)
  uint32_t *head;               // kSearchBounds + n_blocks words (device), zero when the point pass starts
  const uint8_t *cost;          // the resident costmap
  uint8_t *rows;                // ny rows of nx + S - 1: the costmap pooled along x
  uint8_t *pool;                // M: (ny + S - 1) rows of nx + S - 1 (search_pool_at)
  uint32_t *list;               // n_blocks words: the survivors' block indices, in any order
  uint32_t *slots;              // n_blocks * S * S words: slot k holds the exact scores of list[k]'s block
  gv_match_result *result;      // one record (device memory, or the device view of pinned host memory)
  gv_search_stats *stats;       // likewise
  float rot[2 * kMatchMaxSide]; // (c_t, s_t), NT pairs
};
void launch_search_pool(const SearchArgs &a, hipStream_t s);
void launch_search_bound(const SearchArgs &a, hipStream_t s);
void launch_search_seed(const SearchArgs &a, hipStream_t s);
void launch_search_fine(const SearchArgs &a, bool pre, hipStream_t s);   // pre: the seed's and the centre's block
void launch_search_prune(const SearchArgs &a, hipStream_t s);
void launch_search_select(const SearchArgs &a, hipStream_t s);
// bytes (a multiple of 16) from device memory to pinned, device-visible host memory by `blocks` workgroups
void launch_publish_grid(const int8_t *src, int8_t *dst_host, size_t bytes, int blocks, hipStream_t s);
void launch_hold(unsigned long long ticks_100mhz, hipStream_t s);   // one idle wavefront for that long (queue probe)
void launch_u8_to_i32(const uint8_t *in, int32_t *out, size_t n, hipStream_t s);
void launch_i16_to_i32(const int16_t *in, int32_t *out, size_t n, hipStream_t s);

// ---- tile-path binning: partition by 128x128-cell tile + per-tile LDS histogram (gv_binning.hip) ----
constexpr int kBinTileLog = 7;
constexpr int kBinTile = 1 << kBinTileLog;             // cells per tile side
constexpr int kBinTileCells = kBinTile * kBinTile;     // 16384: an int32 tile is 64 KB of LDS
constexpr int kBinSplitMax = 8;                        // workgroups that may share one crowded tile
constexpr uint32_t kBinSplitKeys = 32768;              // keys per share of a crowded tile

struct BinArgs {
  const float *x, *y, *z;
  uint32_t n;
  GridParams g;
  Mat34f m_base, m_cam;
  CamK cam;
  RayOrigin org;
  BBoxTest bt;
  int32_t nb, nb_pad;      // bboxes of the test (do_bbox); nb rounded up to a multiple of 4
  int16_t *bbox_id;        // N (do_bbox)
  int32_t *cell_idx;       // N or null
  bool do_ray, do_bbox;    // do_bbox needs bin_bbox_fits(): the test's tables are staged in LDS
  uint32_t chunk;          // points per partition workgroup (multiple of 256, <= 32768)
  uint32_t n_wg;           // ceil(n / chunk)
  int32_t tiles_x, tiles_y, n_tiles;
  uint16_t *keys;          // [n_wg][chunk]  keys of a chunk grouped by tile
  uint16_t *tab;           // [n_wg][n_tiles + 1]  start of every tile's run inside the chunk; [n_tiles] = count
  uint32_t *tile_total;    // [n_tiles]  keys per tile over all chunks (zero on entry)
  const gv_lshape_pose *rect_poses;   // optional rider: n_rect_poses base-frame poses -> rects_out (one extra workgroup)
  int32_t n_rect_poses;
  Rect *rects_out;
  unsigned long long *dbg; // diagnostic build: 16 clock stamps per workgroup (null in production)
  unsigned long long *tl;  // diagnostic build: {first workgroup in, last workgroup out} of this launch (GV_TIMELINE)
  HeightBand band;         // X4: runtime thresholds (GV_KARG), not a template parameter (off: {-inf, +inf, 0})
};
constexpr size_t kBinBBoxLdsMax = 24 * 1024;   // LDS the partition kernel may spend on the bbox-test tables
uint32_t bin_chunk_for(size_t n);
bool bin_bbox_fits(int nb, const BBoxTest &bt);
void launch_bin_partition(const BinArgs &a, hipStream_t s, hipEvent_t t0 = nullptr, hipEvent_t t1 = nullptr, bool any_order = false);

struct BinTileArgs {
  int32_t nx, ny, tiles_x, tiles_y, n_tiles;
  uint32_t n_wg, chunk;
  const uint16_t *keys;
  const uint16_t *tab;
  const uint32_t *tile_total;   // this frame's totals
  uint32_t *tile_total_next;    // cleared here for the next frame's partition
  uint32_t *done;               // [n_tiles] arrival tickets of shared tiles (zero between frames)
  uint32_t *scratch;            // [max_slots][kBinSplitMax][kBinTileCells + 512] partial tiles
  uint32_t split_keys, max_slots;
  int32_t *hits;                // G int32 (every cell written) or null
  uint32_t *hitN, *clipN, *hitT, *clipT;   // end bitmaps (layout: gv_raysector.hip), every word written
  uint32_t *freeN, *freeT;                 // free-cell bitmaps of the same buffer set: zeroed here (or null)
  int32_t nxw, nyw, nx_pad, ny_pad;
  unsigned long long *dbg;                 // diagnostic build: 16 clock stamps per workgroup (null in production)
  unsigned long long *tl;                  // diagnostic build: launch begin / end (GV_TIMELINE)
};
// n_helpers >= n / split_keys extra workgroups serve the shares 1.. of crowded tiles
void launch_bin_tiles(const BinTileArgs &a, uint32_t n_helpers, hipStream_t s, hipEvent_t t0 = nullptr, hipEvent_t t1 = nullptr);

// ---- sector/gather ray stage + tile grid pass (gv_raysector.hip) ----
struct SectorArgs {
  GridParams g;
  RayOrigin org;
  // from log2s_oct to flat_direct: host::SectorPlan's fields (gv_host_math.hpp), whose violations() lists their bounds
  uint8_t log2s_oct[8];   // sectors of octant o = 1 << log2s_oct[o]: short wedges get fewer, fatter sectors
  uint16_t wg_base[9];    // first workgroup of the k-th octant in dispatch order (oct_perm); [8] = grid size
  uint16_t rev_oct[8];    // octant o, bit c: the threads hold row c of the wedge's columns (512 per row) in descending order
  int32_t cap;            // ends per LDS chunk
  int32_t log2m;          // slope buckets per sector = 1 << log2m
  int32_t marks_words;    // LDS words of cell bits, one per wedge column
  uint32_t oct_perm;      // dispatch order of the octants, 3 bits each (longest wedge first); 0 = identity off
  int32_t reorder;        // 1: longest octants and the rational-gap sectors (0, S/2-1, S/2, S-1) first
  const uint32_t *hitN, *clipN, *hitT, *clipT;
  int32_t nxw, nyw, nx_pad, ny_pad;
  uint32_t *freeN;        // free-cell bitmap, bits along x (written for y-major octants); same layout as hitN
  uint32_t *freeT;        // free-cell bitmap, bits along y (written for x-major octants); same layout as hitT
  unsigned long long *stats;
  int32_t wg_first, wg_stride;   // this launch runs workgroups wg_first, wg_first + wg_stride, ... of the dispatch order
  int32_t n_helpers;      // 0 or 16: second workgroups for the first / last sector of every octant, first in the dispatch order
  uint32_t march_limit;   // most ray cells beyond the threshold column a sector will march (else: exact per cell)
  int32_t flat_k;         // cost ratio exact-cell evaluation : marched cell for the choice beyond T (0: always march when possible)
  uint32_t flat_direct;   // a tail of at most this many cells is evaluated exactly without looking at the long rays at all
  int32_t ablate;         // timing experiments only: 2 skip gather, 4 skip flush, 8/16/32 early exits
  unsigned long long *dbg; // diagnostic phase stamps, 16 per workgroup (null in production)
  unsigned long long *tl;  // diagnostic build: launch begin / end (GV_TIMELINE)
};
// what the launch takes from the plan beside the arguments: k_ray_sectors<ch>, dynamic LDS, workgroups of the whole dispatch
struct SectorLaunch {
  int ch;
  size_t lds_bytes;
  int total_workgroups;
};
bool launch_ray_sectors(const SectorArgs &a, const SectorLaunch &l, hipStream_t s, hipEvent_t done = nullptr, hipEvent_t t0 = nullptr);

struct FinalizeTileArgs {
  GridParams g;
  float *log_odds, *occupancy;
  int8_t *occ_i8;
  const Rect *rects;
  int32_t n_rects;
  const uint32_t *hitN;            // hit bitmap (bits along x)
  const uint32_t *freeN, *freeT;   // free-cell bitmaps of the ray stage (N | T)
  int32_t nx_pad, ny_pad;
  bool counts;            // apply the hit/miss rule
  bool dense;             // write every row; false: a tile row whose log-odds did not change by a bit is not written,
                          // right only while occupancy and the packed grid derive from the current log-odds
  int32_t y_begin, y_end; // rows to finalise ([0, ny) on one GPU)
  unsigned long long *tl; // diagnostic build: launch begin / end (GV_TIMELINE)
};
bool launch_finalize_tiles(const FinalizeTileArgs &a, hipStream_t s, hipEvent_t done = nullptr, hipEvent_t t0 = nullptr);
void launch_miss_to_i32(const uint32_t *freeN, const uint32_t *freeT, int nx, int ny, int nx_pad, int ny_pad,
                        int32_t *out, hipStream_t s);

// ---- frame sharded by points over several GPUs: OR-exchange helpers (gv_shard.hip) ----
void launch_or_slices(const uint32_t *src, uint32_t *dst, size_t count_words, int world, hipStream_t s);
// bands, chunk size and bitmap geometry come from the plan (host::ShardPlan, gv_host_math.hpp)
namespace host { struct ShardPlan; }
void launch_pack_free_bands(const uint32_t *fN, const uint32_t *fT, const host::ShardPlan &P, uint32_t *out, hipStream_t s);
void launch_unpack_free_band(const uint32_t *in, const host::ShardPlan &P, int rank, uint32_t *fN, uint32_t *fT, hipStream_t s);

// ---- kNN depth + radius outlier counts (gv_knn_pca.hip) ----
struct Cand2 {
  float d2;
  uint32_t idx;
};
size_t knn_partial_entries(int nb, int k);   // Cand2 entries of the stage-1 lists

// Completion of a synchronous call without a copy command or a runtime wait: the call's last kernel stores its
// (small) results straight into pinned, device-mapped host memory, every workgroup then takes a ticket, and the
// one whose ticket comes last publishes the call's sequence number in the block's first word -- the host spins on
// that word (tools/micro/call_latency.hip: 8 us instead of 31 for copy + hipStreamSynchronize).  flag == nullptr:
// plain device outputs, nothing published.
struct CallDone {
  unsigned *ticket = nullptr;   // device memory, zero between calls
  unsigned *flag = nullptr;     // host-mapped
  unsigned seq = 0;
};
#if defined(__HIPCC__)
// by ONE lane of every workgroup of the grid, after that lane's result stores (other lanes that stored: a system-scope
// fence of their own, then a barrier, first).  The system-scope fences stay: the results go to the HOST, and stores
// from different CUs reach it on different paths -- with only "my stores are acknowledged" (s_waitcnt vmcnt(0)) before
// the ticket the host saw the flag ahead of another workgroup's payload in 4 calls of 10 (tools/result_block_soak.py,
// profiles/r04/ticket_fence_ab.txt).  Tickets BETWEEN WORKGROUPS OF ONE KERNEL over device memory need no fence when
// the data goes through agent-scope atomics (k_ransac_moments, k_pca_extent, k_cell_scan).
__device__ __forceinline__ void call_done(const CallDone &d, unsigned n_wg)
{
  if (!d.flag) return;
  __threadfence_system();
  const unsigned t = __hip_atomic_fetch_add(d.ticket, 1u, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT);
  if (t == n_wg - 1u) {
    __hip_atomic_store(d.ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __threadfence_system();
    __hip_atomic_store(d.flag, d.seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
  }
}
// Such a ticket, by one lane of every workgroup once its stores have been acknowledged (s_waitcnt vmcnt(0) at the site):
// true in the workgroup that arrives last, which leaves the counter zero for the next call
__device__ __forceinline__ bool take_last_ticket(unsigned *ticket)
{
  const unsigned t = __hip_atomic_fetch_add(ticket, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  const bool last = t == gridDim.x - 1u;
  if (last) __hip_atomic_store(ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  return last;
}
#endif

// buildKDTree projection, then the exact k nearest of every box centre and the median depth of each
struct KnnArgs {
  const float *x, *y, *z;   // the resident cloud (lidar frame), n each
  uint32_t n;
  Mat34f m_cam;             // camera <- lidar
  CamK cam;
  float *pu, *pv, *pd;      // n each: (u, v, depth) of every point, NaN where skipped; written by launch_project_uvd
  const gv_bbox *bboxes;    // nb (device): only the centres are read
  int nb, k;                // k in [1, 32]
  Cand2 *partial;           // knn_partial_entries(nb, k)
  float *depths;            // nb; may be host-mapped (then done.flag is set)
  float *knn_d2;            // nb * k sorted squared distances behind it, or null
};
void launch_project_uvd(const KnnArgs &a, hipStream_t s);
void launch_knn(const KnnArgs &a, const CallDone &done, hipStream_t s);

// ---- device-resident RANSAC ground plane + per-bbox clouds / radius filter / PCA (gv_cloudops.hip) ----
struct RansacState {
  float4 plane;             // best sampled plane
  float4 refined;           // least-squares plane of its inliers (= plane when fewer than 3)
  unsigned long long m;         // inliers of `plane`
  unsigned long long n_inliers; // inliers of `refined` (the mask / the ground points the classify pass dropped)
  unsigned best_count;          // 0: could not estimate a planar model
  unsigned ticket;              // arrival counter of the moments pass (zero between calls)
};
size_t ransac_scratch_doubles(size_t n);
// The inlier counters of the hypotheses are kept in kRansacCountSlices copies (workgroup w adds to copy w % slices,
// the selection sums them): every workgroup ends with one atomic per hypothesis, and 245 workgroups on the same
// 50 words queue up in two L2 channels otherwise.  counts holds kRansacCountSlices * iters words.
constexpr int kRansacCountSlices = 16;
struct RansacArgs {
  const float *x, *y, *z;   // the resident cloud (lidar frame), n each: transformed on the fly
  uint32_t n;
  Mat34f m_cam;
  float thr_f;              // smallest float >= the fp64 threshold
  int iters;                // hypotheses (launch_ransac_plane)
  unsigned long long seed;
  unsigned *counts;         // kRansacCountSlices * iters, zero on entry (the pass leaves them zero)
  double *scratch;          // ransac_scratch_doubles(n): tree-sum partials of the refinement
  RansacState *st;          // device; stays there
  uint8_t *mask;            // n: inliers of the refined plane (launch_ransac_mask)
  RansacState *st_copy;     // optional, may be host-mapped: the final *st, stored by the workgroup that finishes last
};
// hypotheses, inlier counts of all of them, selection + refinement into *st
void launch_ransac_plane(const RansacArgs &a, hipStream_t s);
// mask[n] of the refined plane's inliers + st->n_inliers
void launch_ransac_mask(const RansacArgs &a, const CallDone &done, hipStream_t s);
// one selected point of the radius filter, in bucket order
struct CellNode {
  float x, y, z;    // camera frame
  int32_t id;       // bbox
};
static_assert(sizeof(CellNode) == 16, "one node = one 16-byte access");
// The bucket table of the radius filter: n_buckets (a power of two >= 4096 that only grows) counting-sort buckets.
// k_cell_scan writes pre[0 .. n_buckets] and blk_off[0 .. n_buckets / 4096], the last of which is the number of
// selected points.  The host allocates n_buckets + 4 and n_buckets / 4096 + 4 words: blk_off's slack holds the scan's
// ticket, two words behind the number of selected points (one zeroed allocation for both); pre's is slack only.
struct BucketTable {
  uint32_t *cnt;            // n_buckets, zero on entry (every call counts them back to zero)
  uint32_t *pre;            // pre_words(n_buckets): a bucket's first slot inside its scan block
  uint32_t *blk_off;        // off_words(n_buckets), zero when allocated: block offsets | n_selected | - | ticket
  uint32_t n_buckets;
  static size_t pre_words(size_t nb) { return nb + 4; }
  static size_t off_words(size_t nb) { return nb / 4096 + 4; }
  // the table three allocations of these sizes hold: the smallest of what each has room for
  static size_t held(size_t cnt_cap, size_t pre_cap, size_t off_cap)
  {
    const size_t p = pre_cap < 4 ? 0 : pre_cap - 4, o = off_cap < 4 ? 0 : (off_cap - 4) * 4096;
    return cnt_cap < p ? (cnt_cap < o ? cnt_cap : o) : (p < o ? p : o);
  }
  uint32_t *n_selected() const { return blk_off + n_buckets / 4096; }
  unsigned *scan_ticket() const { return blk_off + n_buckets / 4096 + 2; }   // zero between calls
};
// extractCloudPerBBox + RadiusOutlierRemoval: the first-match box of every point (ground points of st->refined dropped
// when use_plane), the selected points in bucket order, and which of them survive the filter
struct RadiusFilterArgs {
  const float *x, *y, *z;   // the resident cloud (lidar frame), n each
  uint32_t n;
  Mat34f m_cam;
  CamK cam;
  BBoxTest bt;
  int nb;
  bool use_plane;
  float thr_f;              // ground test (use_plane)
  RansacState *st;          // device: the plane; n_inliers is counted here when use_plane
  int16_t *ids;             // n
  BucketTable tab;
  CellNode *sorted;         // n nodes: the selected points in bucket order
  uint8_t *keep;            // n: keep[t] = 1 where sorted point t survives the filter
  uint32_t *ticket_of;      // n: a selected point's slot inside its bucket
  long long *acc;           // pca_acc_words(nb), zero on entry: the kept points' coordinate sums
  float r2f;                // largest float <= radius^2
  int min_pts;
};
void launch_radius_filter(const RadiusFilterArgs &a, hipStream_t s);
size_t pca_acc_words(int nb);   // 64-bit words of acc
size_t pca_ext_words(int nb);   // 32-bit words of ext
// centroid + PCA rectangle of every bbox's kept points (bboxPoseEstimation :156-181, computePCABoundingBox :187-247)
// from order-independent integer sums: covariance pass, extents pass, poses by the last workgroup
struct PcaRectArgs {
  const CellNode *sorted;   // launch_radius_filter's
  const uint32_t *n_sel;    // device: the number of selected points (BucketTable::n_selected)
  uint32_t n;               // points of the cloud
  const uint8_t *keep;
  long long *acc;           // pca_acc_words(nb): launch_radius_filter's sums; left zero
  unsigned *ext;            // pca_ext_words(nb), zero on entry and left zero
  unsigned *ticket;         // zero on entry and left zero
  int nb;
  const RansacState *st;
  bool use_plane;           // an empty segmented cloud (no plane, or all ground) gives no poses
  gv_lshape_pose *poses;    // nb, 16-byte aligned (stored as double2); may be host-mapped
  uint8_t *valid;           // nb
  RansacState *st_copy;     // optional, 8-byte aligned: *st rides home in the same block (64-bit words)
  gv_lshape_pose *poses_dev;   // optional, device memory: a second copy with a NaN length where valid[b] == 0 (no pose:
                               // its corners fail getIndex, so k_rects_from_poses gives no cells)
  uint8_t *valid_dev;          // optional, device memory: a second copy of `valid` (X15: k_tick_dets reads it)
};
void launch_pca_rect(const PcaRectArgs &a, const CallDone &done, hipStream_t s);

}  // namespace gv
