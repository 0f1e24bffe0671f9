// gv_launch_frame.hpp -- launchers of the frame path's kernels: the generic path (gv_generic.hip), the rectangles
// (gv_detections.hip), the tile path (gv_binning.hip, gv_raysector.hip), the grid pass of both (gv_gridpass.hip), ego motion
// (gv_gridmove.hip), the shard helpers (gv_shard.hip) and the cloud / layer movers (gv_cloudio.hip).  gv_api.hip,
// gv_api_frame.hip and gv_api_shard.hip call them.
// Every launcher only enqueues work on `s`; none allocates or synchronises.
#pragma once

#include <hip/hip_runtime.h>

#include "gv_types.hpp"

namespace gv {

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
struct BBoxPrepareArgs {
  const gv_bbox *bboxes;           // nb boxes (device, or inside the staging with the copy rider)
  int32_t nb;
  int32_t tiles_x, tiles_y;        // 16x16-pixel tiles of the image
  int32_t mask_words;              // 64-box words per tile
  float4 *bbox_f;                  // nb thresholds (BBoxTest::bbox_f)
  unsigned long long *tile_mask;   // tiles_y * tiles_x * mask_words (BBoxTest::tile_mask)
  const void *copy_src = nullptr;  // optional rider: the pinned staging ...
  void *copy_dst = nullptr;        // ... the device block it goes to ...
  size_t copy_bytes = 0;           // ... and how much of it
};
void launch_bbox_prepare(const BBoxPrepareArgs &a, hipStream_t s);

// A1 standalone: camera-frame copy of the cloud (gv_cloudio.hip)
struct TransformCloudArgs {
  const float *x, *y, *z;   // n each (device)
  uint32_t n;
  Mat34f m;                 // the transform applied
  float *ox, *oy, *oz;      // n each (device)
};
void launch_transform_cloud(const TransformCloudArgs &a, hipStream_t s);
// PointCloud2 bytes -> SoA (gv_cloudio.hip)
struct DeinterleaveArgs {
  const uint8_t *data;      // n * point_step bytes (device)
  uint32_t n;
  uint32_t point_step;      // bytes per point
  uint32_t off_x, off_y, off_z;   // byte offsets of the three float fields inside a point
  float *x, *y, *z;         // n each (device)
};
void launch_deinterleave(const DeinterleaveArgs &a, hipStream_t s);

// poses -> index rectangles (updateMap corners + updateGridCellsFast index part).
// from_cam: poses are camera-frame, apply `bc` (base <- camera) to the position first.
struct RectsFromPosesArgs {
  const gv_lshape_pose *poses;   // n (device)
  int32_t n;
  GridParams g;
  bool from_cam;
  Xform64 bc;                    // base <- camera; read with from_cam only
  Rect *rects;                   // n (device)
};
void launch_rects_from_poses(const RectsFromPosesArgs &a, hipStream_t s);
// dead-code overload: centre points + class depth (computeBoundingBox3D)
struct RectsFromPointsArgs {
  const double *pts_xyz;    // n * 3 (device)
  const gv_bbox *bboxes;    // n (device): only the labels are read
  int32_t n;
  GridParams g;
  Rect *rects;              // n (device)
};
void launch_rects_from_points(const RectsFromPointsArgs &a, hipStream_t s);
// generic ray stage (gv_generic.hip): the ends of the frame's rays into a list, then the cells of every ray
struct RayCompactArgs {
  const int32_t *hits;      // G
  const uint8_t *clip_end;  // G
  GridParams g;
  uint32_t *list;           // G entries: cell | include_end << 31
  uint32_t *count;          // their number (device), zero on entry
};
void launch_ray_compact(const RayCompactArgs &a, hipStream_t s);
struct RayMarchArgs {
  const uint32_t *list;     // launch_ray_compact's
  const uint32_t *count;
  GridParams g;
  RayOrigin org;            // !org.valid: nothing is launched
  uint8_t *miss;            // G: 1 where a ray passes
  unsigned long long *stats;   // {rays, cells visited} added here, or null
};
void launch_ray_march(const RayMarchArgs &a, hipStream_t s);

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

// ---- cloud / layer movers (gv_cloudio.hip; launch_fill_f32 above is one of them) ----
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

// ---- sector/gather ray stage (gv_raysector.hip) ----
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

// ---- grid pass: the map update rule over the cells, generic and tile form (gv_gridpass.hip) ----
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
// the ray stage's free-cell bitmaps as one int32 per cell (the test hooks that read the miss layer)
struct MissToI32Args {
  const uint32_t *freeN, *freeT;   // the two bitmaps (N | T)
  int nx, ny;                      // cells
  int nx_pad, ny_pad;              // the bitmaps' padded sizes
  int32_t *out;                    // G
};
void launch_miss_to_i32(const MissToI32Args &a, hipStream_t s);

// ---- frame sharded by points over several GPUs: OR-exchange helpers (gv_shard.hip) ----
void launch_or_slices(const uint32_t *src, uint32_t *dst, size_t count_words, int world, hipStream_t s);
// bands, chunk size and bitmap geometry come from the plan (host::ShardPlan, gv_host_math.hpp)
namespace host { struct ShardPlan; }
void launch_pack_free_bands(const uint32_t *fN, const uint32_t *fT, const host::ShardPlan &P, uint32_t *out, hipStream_t s);
void launch_unpack_free_band(const uint32_t *in, const host::ShardPlan &P, int rank, uint32_t *fN, uint32_t *fT, hipStream_t s);

}  // namespace gv
