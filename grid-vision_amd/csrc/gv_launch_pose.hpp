// gv_launch_pose.hpp -- launchers of the pose calls' kernels: the vision-orientation solver (gv_detections.hip), the
// kNN depth (gv_knn_pca.hip), the RANSAC ground plane (gv_ransac.hip), the per-box cloud path (gv_cloudops.hip) and the
// tick's detection list (k_tick_dets, gv_track.hip).  gv_api_pose.hip and gv_api_frame.hip call them.
// Every launcher only enqueues work on `s`; none allocates or synchronises.
#pragma once

#include <hip/hip_runtime.h>

#include "gv_types.hpp"
#include "gv_pose_math.hpp"   // TickDetList

namespace gv {

// vision-orientation geometry, one wavefront per bbox; also emits camera-frame
// gv_lshape_pose (position + dims only; the quaternion is filled by the host).  sets: nullptr in the product; the
// test hook gv_test_vision_sets passes nb * 64 * 4 floats (loc0, loc1, loc2, err of every lane) + nb int32 (winner).
// out_dev: nullptr, or (a GV_TICK_KEEP_DETS tick, X15) device memory for a second copy of `out`, which is usually pinned
struct VisionArgs {
  const float *orient;          // nb * 4 network outputs (device)
  const float *conf;            // nb * 2
  const float *dims;            // nb * 3
  const gv_bbox *bboxes;        // nb (device)
  int32_t nb;
  gv_cam_params cam;
  VisionOut *out;               // nb records
  gv_lshape_pose *poses_cam;    // nb camera-frame poses (device)
  float *sets = nullptr;        // the test hook's per-lane sets
  VisionOut *out_dev = nullptr; // the second copy of `out`
};
void launch_vision(const VisionArgs &a, hipStream_t s);
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
// ---- kNN depth + radius outlier counts (gv_knn_pca.hip) ----
struct Cand2 {
  float d2;
  uint32_t idx;
};
size_t knn_partial_entries(int nb, int k);   // Cand2 entries of the stage-1 lists

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

// ---- device-resident RANSAC ground plane (gv_ransac.hip) + per-bbox clouds / radius filter / PCA (gv_cloudops.hip) ----
// The sweep geometry both files assume: a workgroup of the kernels that sweep the cloud takes kCoBlock points.
constexpr int kCoThreads = 1024;          // workgroup of the sweep kernels
constexpr int kCoPts = 4;                 // points per thread
constexpr int kCoBlock = kCoThreads * kCoPts;   // 4096 points = 64 level-0 groups of the sum tree
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
