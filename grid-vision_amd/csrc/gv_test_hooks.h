/* gv_test_hooks.h -- entry points the library exports for tests/ only.  NOT part of the ABI: include/gridvision_hip.h
 * does not declare them, INTEGRATION.md does not list them, a maintainer's binding never sees them; they may change or
 * go without an ABI version step. */
#ifndef GV_TEST_HOOKS_H
#define GV_TEST_HOOKS_H
#include "../../include/gridvision_hip.h"
#ifdef __cplusplus
extern "C" {
#endif
/* No RCCL, one device: runs the sharded frame (gv_frame_enqueue_sharded's kernels, bands and slices) for EVERY rank of
 * a `world`-GPU job on this handle -- the resident cloud is the whole cloud, rank r takes points
 * [n*r/world, n*(r+1)/world) -- with the exchanges done by device copies; the result must equal gv_process_frame's
 * (tests/test_gpu_parity.py::test_sharded_frame_every_rank_emulated). */
int gv_test_frame_sharded_emulated(gv_handle h, const gv_frame_desc *desc, int32_t world);
/* gv_vision_post_process's kernel (k_vision, through the same launch_vision) with its one test-only output switched on:
 * sets[(i * 64 + lane) * 4 ..] = loc0, loc1, loc2, err of constraint set `lane` = ((l*4+t)*2+r)*4+b of box i, and
 * winner[i] = the set the arg-min chose, 64 when no residual is below FLT_MAX.  The product's call sites pass a null
 * pointer there and store nothing (tests/test_gpu_vision.py). */
int gv_test_vision_sets(gv_handle h, const float *orient, const float *conf, const float *dims, const gv_bbox *bboxes,
                        int32_t nb, float *sets /* nb*64*4 */, int32_t *winner /* nb */);
/* gv_compute_bbox_pose (with_ground == 0) or gv_compute_bbox_pose_ground_removed (with_ground != 0), the product's own
 * call unchanged, and then what that call left resident on the device: *n_sel = the number of selected points (the
 * bucket scan's total), nodes[4 * t ..] = the 16 bytes of CellNode t (camera x, y, z as floats, the box id as an int32)
 * in bucket order, keep[t] = 1 where point t survived the radius filter.  nodes and keep have room for the resident
 * cloud's n points.  A call that launches nothing (no boxes, no points) reports *n_sel = 0.  No kernel of its own
 * (tests/test_gpu_pose.py). */
int gv_test_bbox_pose_nodes(gv_handle h, const gv_bbox *bboxes, int32_t nb, int32_t with_ground, gv_lshape_pose *poses_out,
                            uint8_t *valid, int32_t *n_poses_or_fail, float *nodes /* n*4 */, uint8_t *keep /* n */,
                            int64_t *n_sel);
/* gv_segment_ground_plane(threshold, iterations, seed, is_ground) (pose_path == 0; bboxes .. n_poses_or_fail unused), or
 * gv_compute_bbox_pose_ground_removed(bboxes, nb, poses_out, valid, n_poses_or_fail) with its fixed 0.04 / 50 / 12345
 * (pose_path != 0; threshold .. is_ground unused): the product's own call through the same function, and the RansacState
 * that call brings home anyway -- the sampled plane, the refined plane, m = the sampled plane's inliers as the moments pass
 * counted them, n_inliers = the refined plane's as the mask / classify pass counted them, best_count = the winner's count as
 * the counting pass left it (0: no plane, everything else zero).  No kernel of its own (tests/test_gpu_ransac.py). */
typedef struct gv_test_ransac_state_t {
  float plane[4], refined[4];
  uint64_t m, n_inliers;
  uint32_t best_count, pad;
} gv_test_ransac_state_t;
int gv_test_ransac_state(gv_handle h, double threshold, int32_t iterations, uint64_t seed, int32_t pose_path,
                         const gv_bbox *bboxes, int32_t nb, uint8_t *is_ground /* n */, gv_lshape_pose *poses_out,
                         uint8_t *valid, int32_t *n_poses_or_fail, gv_test_ransac_state_t *out);
/* Host only, no handle and no device: the plan of the sharded frame (host::ShardPlan, csrc/gv_host_math.hpp) that a handle
 * over an nx x ny grid keeps for a communicator of `world` ranks: words of one end-bitmap slice and of one packed free-cell
 * band, whether one ncclReduceScatter of *cnt0 cells per rank serves the hit counts (else one ncclReduce per band: the
 * choice no one-GPU run can take), and rows[2 * r], rows[2 * r + 1] = band [y0, y1) of rank r
 * (tests/test_oracle_properties.py). */
int gv_test_shard_plan(int32_t nx, int32_t ny, int32_t world, int64_t *slice, int64_t *chunk, int32_t *equal_bands,
                       int64_t *cnt0, int32_t *rows /* 2 * world */);
/* Host only, no handle and no device: the plan of the sector ray stage (host::SectorPlan, csrc/gv_host_math.hpp) that a
 * handle over an nx x ny grid builds for origin cell (cx, cy) and a cloud of n_points, with the knobs read from the
 * environment by the function gv_create reads them with.  wg[7 * b ..] = octant, sector, helper, part, nparts, stat slot,
 * idle of workgroup b of the dispatch order, for b < min(total_workgroups, wg_cap) (tests/test_sector_plan_host.py). */
typedef struct gv_test_sector_plan_t {
  int32_t len[8], imax;
  int32_t log2s_oct[8], rev_oct[8];
  int32_t cap, log2m, marks_words;
  uint32_t oct_perm;
  int32_t reorder;
  uint32_t wg_base[9];
  int32_t n_helpers;
  int32_t flat_k;
  uint32_t march_limit, flat_direct;
  int32_t ch;
  int64_t lds_bytes;
  uint32_t total_workgroups;
  int64_t stat_slots;
  uint32_t violations;          /* host::SectorPlan::violations(), bits in the order of its enum */
} gv_test_sector_plan_t;
int gv_test_sector_plan(int32_t nx, int32_t ny, int32_t cx, int32_t cy, int64_t n_points, gv_test_sector_plan_t *plan,
                        int32_t *wg /* 7 * wg_cap */, int64_t wg_cap);
/* [EXTENSION] X15.  gv_test_tick_dets: a synchronous read-back (it waits for gv_stream(h)) of the detection list the last
 * GV_TICK_KEEP_DETS tick left on the device: the 128 records as they lie there, *n = records used, *n_total = poses found.
 * GV_ERR_STATE when the last tick enqueued did not carry the flag.  No kernel of its own.
 * gv_test_tick_dets_host: host only, no handle and no device: the selection and the camera->base transform of k_tick_dets
 * (csrc/gv_pose_math.hpp: the same text) over n_cand camera-frame poses and their valid flags; empty != 0 is the "empty
 * segmented cloud" outcome (tests/test_tick_track_host.py, tests/test_gpu_tick_track.py). */
int gv_test_tick_dets(gv_handle h, gv_lshape_pose *out /* 128 */, int32_t *n, int32_t *n_total);
int gv_test_tick_dets_host(const gv_lshape_pose *cam, const uint8_t *valid, int32_t n_cand, int32_t empty, const gv_transform *tf_bc,
                           gv_lshape_pose *out /* 128 */, int32_t *n, int32_t *n_total);
/* gv_test_end_bitmaps: a synchronous copy of the four end bitmaps the tile pass (k_bin_tiles) wrote for the ray stage, of
 * the buffer set of the last frame, as the last synchronous gv_process_frame on the tile path left them.  Words, not cells:
 *   N (hitN, clipN): *nxw * *ny_pad words, bit x & 31 of word (x >> 5) * ny_pad + y;
 *   T (hitT, clipT): *nyw * *nx_pad words, bit y & 31 of word (y >> 5) * nx_pad + x.
 * All four array pointers null and the four size pointers set: the sizes only.  GV_ERR_STATE when the handle is not on the
 * tile path or no binned frame has run.  No kernel of its own (tests/test_gpu_tile_pass.py). */
int gv_test_end_bitmaps(gv_handle h, uint32_t *hitN, uint32_t *clipN, uint32_t *hitT, uint32_t *clipT,
                        int32_t *nxw, int32_t *nyw, int32_t *nx_pad, int32_t *ny_pad);
/* gv_test_wave: one helper of csrc/gv_wave.hpp on the device, lane by lane (k_test_wave, csrc/gv_test_wave.hip: the one
 * kernel that exists for a test).  One wavefront per 64 inputs, `threads` (64, 256 or 1024) to a workgroup: lane l of wave
 * w reads in[w * 64 + l], runs helper `op` inside `if ((active[w] >> l) & 1)` and stores its own result to
 * out[w * 64 + l]; an inactive lane stores GV_TEST_WAVE_INACTIVE.  No result is ever an address or an index.  Synchronous
 * on gv_stream(h), buffers of its own, freed before it returns; 1 <= n_waves <= 4096.  *counter_out: the final value of
 * the one uint32 counter the append ops add to (zeroed before the launch; 0 for every other op).
 * 32-bit ops take the low word of `in` and store their result zero-extended; fp64 ops take and store the bits.  The ops:
 *   SCAN_ADD / _MAX / _MIN, REDUCE_ADD / _MAX / _MIN   wave_scan<Op>, wave_reduce<Op>
 *   SHIFT_DOWN_1 / _2 / _4 / _8      wave_shift_down<H>(v, fill = (unsigned)arg)
 *   GROUP_SUM_8 / _16                group_sum<LANES>((int)v); whole aligned groups of LANES lanes may be inactive
 *   MIN_KEY, MAX64, SUM64            wave_min_key, wave_max64, wave_sum64 over the 64 bits
 *   SUM_I32 / _U32, MAX_I32 / _U32   wave_sum<T>, wave_max<T>
 *   SHFL_XOR64                       shfl_xor64(v, o = arg), 1 <= arg <= 63
 *   BUTTERFLY, TREE_SHFL             wave_butterfly, wave_tree_sum_shfl: every lane's bits (the header promises lane 0's)
 *   DPP_F64_SHL_1 / _2 / _4 / _8     dpp_f64<row_shl:k>
 *   RANK_LEADER                      m = __ballot(in & 1): wave_leader(m) in the high word, wave_rank(m, l) in the low one;
 *                                    GV_TEST_WAVE_SKIPPED in the active lanes of a wave whose m is 0
 *   BCAST_U64 / _I32 / _F64          wave_bcast<T>(v, lane = arg), 0 <= arg <= 63: unsigned long long, int, double
 *   APPEND, APPEND_ALL               m = __ballot(in & 1); a wave whose m is 0 skips the call (GV_TEST_WAVE_SKIPPED), else
 *                                    base = wave_append / wave_append_all(counter, m, l) and every active lane stores base
 *                                    in the high word, base + wave_rank(m, l) in the low one
 * GV_ERR_BAD_ARG, and nothing launched: a null pointer, n_waves, threads, op or arg out of range; an active mask other
 * than all 64 lanes for any op but GROUP_SUM_*, RANK_LEADER, BCAST_* and APPEND* (gv_wave.hpp defines the DPP scans, the
 * butterflies and the trees for a full wavefront only); GROUP_SUM_* with a group of LANES lanes partly active; BCAST_* with lane `arg` inactive in some wave; APPEND_ALL with lane 0 inactive
 * in some wave (tests/test_gpu_wave.py). */
typedef enum gv_test_wave_op {
  GV_TEST_WAVE_SCAN_ADD = 0, GV_TEST_WAVE_SCAN_MAX, GV_TEST_WAVE_SCAN_MIN,
  GV_TEST_WAVE_REDUCE_ADD, GV_TEST_WAVE_REDUCE_MAX, GV_TEST_WAVE_REDUCE_MIN,
  GV_TEST_WAVE_SHIFT_DOWN_1, GV_TEST_WAVE_SHIFT_DOWN_2, GV_TEST_WAVE_SHIFT_DOWN_4, GV_TEST_WAVE_SHIFT_DOWN_8,
  GV_TEST_WAVE_GROUP_SUM_8, GV_TEST_WAVE_GROUP_SUM_16,
  GV_TEST_WAVE_MIN_KEY,
  GV_TEST_WAVE_SUM_I32, GV_TEST_WAVE_SUM_U32, GV_TEST_WAVE_MAX_I32, GV_TEST_WAVE_MAX_U32,
  GV_TEST_WAVE_MAX64, GV_TEST_WAVE_SUM64, GV_TEST_WAVE_SHFL_XOR64,
  GV_TEST_WAVE_BUTTERFLY, GV_TEST_WAVE_TREE_SHFL,
  GV_TEST_WAVE_DPP_F64_SHL_1, GV_TEST_WAVE_DPP_F64_SHL_2, GV_TEST_WAVE_DPP_F64_SHL_4, GV_TEST_WAVE_DPP_F64_SHL_8,
  GV_TEST_WAVE_RANK_LEADER,
  GV_TEST_WAVE_BCAST_U64, GV_TEST_WAVE_BCAST_I32, GV_TEST_WAVE_BCAST_F64,
  GV_TEST_WAVE_APPEND, GV_TEST_WAVE_APPEND_ALL,
  GV_TEST_WAVE_OPS
} gv_test_wave_op;
#define GV_TEST_WAVE_INACTIVE 0xA5A5A5A5A5A5A5A5ull
#define GV_TEST_WAVE_SKIPPED 0x5A5A5A5A5A5A5A5Aull
int gv_test_wave(gv_handle h, int32_t op, int32_t arg, int32_t threads /* 64, 256 or 1024 */,
                 const uint64_t *in /* n_waves*64 */, const uint64_t *active /* n_waves */, int64_t n_waves,
                 uint64_t *out /* n_waves*64 */, uint32_t *counter_out);
#ifdef __cplusplus
}
#endif
#endif
