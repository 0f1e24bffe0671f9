// gv_api_pose.hip -- the result block, kNN depth, RANSAC ground plane, per-box PCA poses, the vision
// post-processing and the node's tick (gv_tick_*).
#include <atomic>
#include <algorithm>
#include <cassert>
#include <cstdint>
#include <cstring>
#include <vector>

#include "gv_context.hpp"

extern "C" {

// camera-frame pose of one VisionOut (vision_orientation.cpp:432-444)
static gv_lshape_pose pose_of_vision_out(const VisionOut &vo)
{
  gv_lshape_pose p;
  p.px = vo.loc[0]; p.py = vo.loc[1]; p.pz = vo.loc[2];     // :434-436
  const host::Quat q = host::quat_from_rpy(0, -vo.orient, 0);   // :440
  p.qx = q.x; p.qy = q.y; p.qz = q.z; p.qw = q.w;
  p.length = vo.dims[0]; p.width = vo.dims[1]; p.height = vo.dims[2];
  return p;
}

// the valid VisionOuts' poses, compacted (vision_orientation.cpp:496-499); tf: into that frame (transformLShapeObjects);
// out null: counted only
static int32_t collect_vision_poses(const VisionOut *vo, int32_t n, const gv_transform *tf, gv_lshape_pose *out)
{
  int32_t m = 0;
  for (int32_t i = 0; i < n; ++i) {
    if (!vo[i].valid) continue;
    gv_lshape_pose p = pose_of_vision_out(vo[i]);
    if (tf) host::transform_pose(*tf, p);
    if (out) out[m] = p;
    ++m;
  }
  return m;
}

// boxes and the network's outputs for them, for kernels that read them raw (no bbox-test tables)
static DetUpload vision_upload(const gv_bbox *bboxes, int32_t nb, const float *orient, const float *conf, const float *dims,
                               hipStream_t s)
{
  DetUpload u;
  u.bboxes = bboxes; u.nb = nb;
  u.orient = orient; u.conf = conf; u.dims = dims;
  u.stream = s;
  u.masks = false;
  return u;
}

// the solver over the first nb boxes of such an upload, its records into the standalone scratch (sets, out_dev: null)
static VisionArgs scratch_vision_args(gv_context *h, const DetSet &d, int32_t nb)
{
  VisionArgs a;
  a.orient = d.orient; a.conf = d.conf; a.dims = d.dims; a.bboxes = d.bboxes; a.nb = nb;
  a.cam = h->cam;
  a.out = h->sb[0].vout; a.poses_cam = d.poses;
  return a;
}

int gv_vision_post_process(gv_handle h, const float *orient, const float *conf, const float *dims,
                           const gv_bbox *bboxes, int32_t nb, gv_lshape_pose *poses_out, int32_t *n_out)
{
  if (!h || nb < 0 || !n_out || (nb && (!orient || !conf || !dims || !bboxes || !poses_out))) return GV_ERR_BAD_ARG;
  GV_TRY
  *n_out = 0;
  if (nb == 0) return GV_OK;
  int rc = use_device(h);
  if (rc) return rc;
  DetSet &d = h->det[2];
  if ((rc = upload_det(h, d, vision_upload(bboxes, nb, orient, conf, dims, h->stream)))) return rc;
  GV_HIP(hipEventRecord(d.ready, h->stream));
  launch_vision(scratch_vision_args(h, d, nb), h->stream);
  GV_HIP(hipGetLastError());
  std::vector<VisionOut> vo((size_t)nb);
  GV_HIP(hipMemcpyAsync(vo.data(), h->sb[0].vout, (size_t)nb * sizeof(VisionOut), hipMemcpyDeviceToHost, h->stream));
  GV_HIP(hipStreamSynchronize(h->stream));
  *n_out = collect_vision_poses(vo.data(), nb, nullptr, poses_out);
  return GV_OK;
  GV_CATCH
}

// test hook (gv_test_hooks.h): gv_vision_post_process's upload and launch with the kernel's `sets` output switched on
int gv_test_vision_sets(gv_handle h, const float *orient, const float *conf, const float *dims, const gv_bbox *bboxes,
                        int32_t nb, float *sets, int32_t *winner)
{
  if (!h || nb < 0 || (nb && (!orient || !conf || !dims || !bboxes || !sets || !winner))) return GV_ERR_BAD_ARG;
  GV_TRY
  if (nb == 0) return GV_OK;
  int rc = use_device(h);
  if (rc) return rc;
  DetSet &d = h->det[2];
  if ((rc = upload_det(h, d, vision_upload(bboxes, nb, orient, conf, dims, h->stream)))) return rc;
  GV_HIP(hipEventRecord(d.ready, h->stream));
  DevBuf<float> dsets;   // nb * 64 * (loc0, loc1, loc2, err), then nb winners
  if ((rc = dsets.reserve(h, (size_t)nb * 257))) return rc;
  VisionArgs va = scratch_vision_args(h, d, nb);
  va.sets = dsets;
  launch_vision(va, h->stream);
  GV_HIP(hipGetLastError());
  GV_HIP(hipMemcpyAsync(sets, dsets, (size_t)nb * 256 * sizeof(float), hipMemcpyDeviceToHost, h->stream));
  GV_HIP(hipMemcpyAsync(winner, dsets + (size_t)nb * 256, (size_t)nb * sizeof(int32_t), hipMemcpyDeviceToHost, h->stream));
  GV_HIP(hipStreamSynchronize(h->stream));
  return GV_OK;
  GV_CATCH
}

// ---- the result block (ResultBlock, gv_context.hpp) ----
int ResultBlock::begin(gv_context *h, size_t bytes, CallDone &done)
{
  // a tick between gv_tick_enqueue and gv_tick_wait owns the result block (and the standalone detection set): the
  // calls that would reuse them are refused until the tick has been waited for
  if (h->tick.pending) { h->err = "a tick is pending: call gv_tick_wait first"; return GV_ERR_STATE; }
  int rc;
  if (bytes + kHeader > host.cap()) {
    GV_HIP(hipStreamSynchronize(h->stream));   // nothing in flight writes the old block
    const size_t want = std::max<size_t>(2 * (bytes + kHeader), 16384);
    // coherent (fine-grained) explicitly: the host must see the payload and the flag while the kernel that stores them
    // is still running, whatever HIP_HOST_COHERENT says
    if ((rc = host.reserve(h, want, hipHostMallocCoherent | hipHostMallocMapped))) return rc;
    std::memset(host, 0, want);
  }
  if ((rc = ticket.reserve_zeroed(h, 16, h->stream))) return rc;   // 64 bytes
  if (++seq == 0u) seq = 1u;   // 0 = "nothing published yet"
  done.ticket = ticket;
  done.flag = reinterpret_cast<unsigned *>(host.get());
  done.seq = seq;
  return GV_OK;
}

static inline void cpu_relax()
{
#if !defined(__HIP_DEVICE_COMPILE__) && (defined(__x86_64__) || defined(__i386__))
  __builtin_ia32_pause();
#endif
}

// Host side of CallDone: spin on the block's first word.  The stream is looked at now and then so that a call
// whose kernels failed ends in an error instead of a hang.
int ResultBlock::wait(gv_context *h)
{
  volatile unsigned *flag = reinterpret_cast<volatile unsigned *>(host.get());
  for (unsigned spins = 1;; ++spins) {
    if (*flag == seq) break;
    cpu_relax();   // the calls take 80-400 us: leave the core's other thread its issue slots
    if ((spins & 0xfffu) == 0u) {
      const hipError_t q = hipStreamQuery(h->stream);
      if (q == hipErrorNotReady) continue;
      if (q == hipSuccess && *flag == seq) break;
      h->err = q == hipSuccess ? "result block never published" : hipGetErrorString(q);
      return GV_ERR_HIP;
    }
  }
  std::atomic_thread_fence(std::memory_order_acquire);
  return GV_OK;
}

// buildKDTree projection (cloud_detections.cpp:8-33) into the transformed-cloud buffers, then the exact k nearest (:43-87)
// of nb boxes; depths | knn_d2 (or null) may lie in the result block
static KnnArgs knn_args(const gv_context *h, const gv_bbox *boxes, int32_t nb, int32_t k, float *depths, float *knn_d2)
{
  KnnArgs a{};
  a.x = h->cx; a.y = h->cy; a.z = h->cz; a.n = (uint32_t)h->n;
  a.m_cam = h->m_cam; a.cam = h->camk;
  a.pu = h->tx; a.pv = h->ty; a.pd = h->tz;
  a.bboxes = boxes; a.nb = nb; a.k = k;
  a.partial = h->pose.knn_partial;
  a.depths = depths; a.knn_d2 = knn_d2;
  return a;
}

int gv_compute_depth_for_bboxes(gv_handle h, const gv_bbox *bboxes, int32_t nb, int32_t k, float *depths,
                                float *knn_d2)
{
  if (!h || nb < 0 || (nb && (!bboxes || !depths)) || k < 1 || k > 32) return GV_ERR_BAD_ARG;
  if (!h->has_cl) return GV_ERR_TF;
  GV_TRY
  if (nb == 0) return GV_OK;
  int rc = use_device(h);
  if (rc) return rc;
  if ((rc = upload_scratch_bboxes(h, bboxes, nb, false))) return rc;   // the kNN reads the boxes' centres only
  if ((rc = ensure_tbuf(h, std::max<size_t>(h->n, 1)))) return rc;
  if ((rc = h->pose.knn_partial.reserve(h, knn_partial_entries(nb, k)))) return rc;
  // depths | sorted squared distances, stored by the merge kernel straight into the result block
  ResultBlock &R = h->pose.res;
  CallDone done;
  if ((rc = R.begin(h, (size_t)nb * (1 + (size_t)k) * sizeof(float), done))) return rc;
  float *r_depths = reinterpret_cast<float *>(R.payload()), *r_d2 = r_depths + nb;
  const KnnArgs ka = knn_args(h, h->det[2].bboxes, nb, k, r_depths, knn_d2 ? r_d2 : nullptr);
  launch_project_uvd(ka, h->stream);
  launch_knn(ka, done, h->stream);
  GV_HIP(hipGetLastError());
  if ((rc = R.wait(h))) return rc;
  std::memcpy(depths, r_depths, (size_t)nb * sizeof(float));
  if (knn_d2) std::memcpy(knn_d2, r_d2, (size_t)nb * k * sizeof(float));
  return GV_OK;
  GV_CATCH
}

// segmentGroundPlane(0.04, 50 hypotheses) as computeBBoxPose calls it (grid_vision_node.cpp:215-216)
constexpr int32_t kPoseRansacIters = 50;
constexpr uint64_t kPoseRansacSeed = 12345ull;

static int ensure_ransac_buffers(gv_context *h, size_t n, int32_t iterations)
{
  gv_context::Pose &P = h->pose;
  int rc;
  if ((rc = P.plane_counts.reserve_zeroed(h, (size_t)iterations * kRansacCountSlices, h->stream)) ||   // every pass leaves them zero
      (rc = P.rscratch.reserve(h, ransac_scratch_doubles(n))))
    return rc;
  return P.rstate.reserve_zeroed(h, 1, h->stream);
}

// plane fit and mask pass over the camera-frame cloud (the reference segments transformed_cloud: transformed on the fly);
// st_copy: where the mask pass hands the final state out
static RansacArgs ransac_args(const gv_context *h, float thr_f, int32_t iterations, uint64_t seed, RansacState *st_copy = nullptr)
{
  const gv_context::Pose &P = h->pose;
  RansacArgs a{};
  a.x = h->cx; a.y = h->cy; a.z = h->cz; a.n = (uint32_t)h->n;
  a.m_cam = h->m_cam;
  a.thr_f = thr_f; a.iters = iterations; a.seed = seed;
  a.counts = P.plane_counts; a.scratch = P.rscratch; a.st = P.rstate;
  a.mask = P.ground; a.st_copy = st_copy;
  return a;
}

// poses | RansacState | valid of nb boxes, as k_pca_extent stores them behind `base` (in the result block).  The kernel
// stores the poses as double2 and the state as 64-bit words: base is 16-byte aligned, and so is then the state.
struct PoseBlock {
  static_assert(sizeof(gv_lshape_pose) % 16 == 0 && alignof(RansacState) <= 16 && sizeof(RansacState) % 8 == 0, "PoseBlock alignment");
  uint8_t *base;
  int32_t nb;
  PoseBlock(uint8_t *base_, int32_t nb_) : base(base_), nb(nb_) { assert((reinterpret_cast<uintptr_t>(base) & 15u) == 0); }
  gv_lshape_pose *poses() const { return reinterpret_cast<gv_lshape_pose *>(base); }
  RansacState *state() const { return reinterpret_cast<RansacState *>(base + (size_t)nb * sizeof(gv_lshape_pose)); }
  uint8_t *valid() const { return base + (size_t)nb * sizeof(gv_lshape_pose) + sizeof(RansacState); }
  static size_t bytes(int32_t nb) { return (size_t)nb * (sizeof(gv_lshape_pose) + 1) + sizeof(RansacState); }
};

// "empty segmented cloud": no plane, no ground point, or nothing but ground among the n points -> the reference returns {}
// (cloud_detections.cpp:307-309)
static bool segmented_cloud_empty(const RansacState &st, size_t n)
{
  return tick_dets_empty(st.best_count, st.n_inliers, (uint64_t)n);   // (gv_pose_math.hpp: k_tick_dets decides the same)
}

// The scratch of enqueue_bbox_pose, group by group; a group has room for what its smallest member has room for.
// Per point, with n / 8 + 1024 of slack:
static int reserve_pose_points(gv_context *h, size_t n)
{
  gv_context::Pose &P = h->pose;
  if (n <= std::min({P.nodes.cap(), P.keep.cap(), P.ticket_of.cap()})) return GV_OK;
  const size_t want = n + n / 8 + 1024;
  int rc;
  if ((rc = P.nodes.reserve(h, want)) || (rc = P.keep.reserve(h, want))) return rc;
  return P.ticket_of.reserve(h, want);
}
// per box, with nb / 4 + 64 of slack (every call leaves them zero)
static int reserve_pose_boxes(gv_context *h, int32_t nb)
{
  gv_context::Pose &P = h->pose;
  if (pca_acc_words(nb) <= P.pca_acc.cap() && pca_ext_words(nb) <= P.pca_ext.cap()) return GV_OK;
  const int want = nb + nb / 4 + 64;
  if (int rc = P.pca_acc.reserve_zeroed(h, pca_acc_words(want), h->stream)) return rc;
  return P.pca_ext.reserve_zeroed(h, pca_ext_words(want), h->stream);
}
// cell buckets: a power of two, about one per two points, that only grows (the three arrays stay L2 resident at config-3
// size; cells that share a bucket only add candidates that fail the id or distance test)
static int reserve_pose_buckets(gv_context *h, size_t n)
{
  gv_context::Pose &P = h->pose;
  size_t n_buckets = 4096;
  while (n_buckets < n / 2 && n_buckets < ((size_t)1 << 25)) n_buckets <<= 1;
  if (n_buckets <= P.buckets().n_buckets) return GV_OK;
  int rc;
  if ((rc = P.cellcnt.reserve_zeroed(h, n_buckets, h->stream)) ||   // every call counts them back to zero
      (rc = P.cellpre.reserve(h, BucketTable::pre_words(n_buckets))))
    return rc;
  return P.celloff.reserve_zeroed(h, BucketTable::off_words(n_buckets), h->stream);   // the scan's ticket is in there
}

// extractCloudPerBBox + RadiusOutlierRemoval(0.4, 10)  (cloud_detections.cpp:250-298, 150-154)
static RadiusFilterArgs radius_filter_args(const gv_context *h, int32_t nb, bool with_ground, float thr_f)
{
  const gv_context::Pose &P = h->pose;
  const double radius = 0.4;
  RadiusFilterArgs a{};
  a.x = h->cx; a.y = h->cy; a.z = h->cz; a.n = (uint32_t)h->n;
  a.m_cam = h->m_cam; a.cam = h->camk;
  a.bt = bbox_test_of(h, h->det[2]); a.nb = nb;
  a.use_plane = with_ground; a.thr_f = thr_f; a.st = P.rstate;
  a.ids = h->sb[h->last.points].bbox_id;
  a.tab = P.buckets();
  a.sorted = P.nodes; a.keep = P.keep; a.ticket_of = P.ticket_of;
  a.acc = P.pca_acc;
  a.r2f = host::floor_to_float(radius * radius); a.min_pts = 10;
  return a;
}

// centroid + PCA rectangle per bbox from order-independent integer sums over the kept points (:156-247), into `out`
static PcaRectArgs pca_rect_args(const gv_context *h, int32_t nb, bool with_ground, const PoseBlock &out, gv_lshape_pose *poses_dev,
                                 uint8_t *valid_dev)
{
  const gv_context::Pose &P = h->pose;
  PcaRectArgs a{};
  a.sorted = P.nodes; a.n_sel = P.buckets().n_selected(); a.n = (uint32_t)h->n; a.keep = P.keep;
  a.acc = P.pca_acc; a.ext = P.pca_ext; a.ticket = P.pca_ticket; a.nb = nb;
  a.st = P.rstate; a.use_plane = with_ground;
  a.poses = out.poses(); a.valid = out.valid(); a.st_copy = out.state(); a.poses_dev = poses_dev;
  a.valid_dev = valid_dev;
  return a;
}

// extractCloudPerBBox -> RadiusOutlierRemoval -> centroid + PCA rectangle, all on the device and all enqueued
// without a host wait in between; only the nb poses come back.  with_ground: the points of the refined RANSAC
// plane in *rstate are dropped first (computeBBoxPose, cloud_detections.cpp:300-321), and the "empty segmented
// cloud" outcomes (:307-309) are decided on the device.
// poses_dev (optional): the camera-frame poses also go to device memory (a NaN length marks "no pose": its
// corners fail getIndex, so k_rects_from_poses gives it no cells), for a map update enqueued right behind this without a trip to the host.
static int enqueue_bbox_pose(gv_context *h, int32_t nb, bool with_ground, float thr_f, const PoseBlock &out, const CallDone &done,
                             gv_lshape_pose *poses_dev = nullptr, uint8_t *valid_dev = nullptr)
{
  gv_context::Pose &P = h->pose;
  int rc;
  if ((rc = reserve_pose_points(h, h->n)) || (rc = reserve_pose_boxes(h, nb)) ||
      (rc = P.pca_ticket.reserve_zeroed(h, 16, h->stream)) ||   // 64 bytes
      (rc = reserve_pose_buckets(h, h->n)) || (rc = P.rstate.reserve_zeroed(h, 1, h->stream)))
    return rc;
  launch_radius_filter(radius_filter_args(h, nb, with_ground, thr_f), h->stream);
  h->last.bbox_id = true;
  launch_pca_rect(pca_rect_args(h, nb, with_ground, out, poses_dev, valid_dev), done, h->stream);
  GV_HIP(hipGetLastError());
  return GV_OK;
}

static int compute_bbox_pose_impl(gv_handle h, const gv_bbox *bboxes, int32_t nb, gv_lshape_pose *poses_out,
                                  uint8_t *valid, bool with_ground, RansacState *st_out)
{
  if (!h || nb < 0 || nb > 32767 || (nb && (!bboxes || !poses_out || !valid))) return GV_ERR_BAD_ARG;
  if (!h->has_cl) return GV_ERR_TF;
  GV_TRY
  int rc = use_device(h);
  if (rc) return rc;
  const size_t n = h->n;
  for (int32_t b = 0; b < nb; ++b) { valid[b] = 0; poses_out[b] = gv_lshape_pose{}; }
  if (st_out) *st_out = RansacState{};
  if (n == 0 || (with_ground && n < 3)) return GV_OK;
  if (nb && (rc = upload_scratch_bboxes(h, bboxes, nb))) return rc;
  const float thr_f = host::ceil_to_float(0.04);   // for a float f: f < thr_f <=> (double)f < 0.04
  ResultBlock &R = h->pose.res;
  CallDone done;
  if (with_ground) {
    if ((rc = ensure_ransac_buffers(h, n, kPoseRansacIters))) return rc;
    launch_ransac_plane(ransac_args(h, thr_f, kPoseRansacIters, kPoseRansacSeed), h->stream);
    GV_HIP(hipGetLastError());
    h->pose.ground_n = 0;   // the mask itself is not materialised on this path
  }
  if (nb) {
    // poses | state | flags: stored by the PCA kernel straight into the result block, no copy, no runtime wait
    if ((rc = R.begin(h, PoseBlock::bytes(nb), done))) return rc;
    const PoseBlock out(R.payload(), nb);
    if ((rc = enqueue_bbox_pose(h, nb, with_ground, thr_f, out, done))) return rc;
    if ((rc = R.wait(h))) return rc;
    std::memcpy(poses_out, out.poses(), (size_t)nb * sizeof(gv_lshape_pose));
    std::memcpy(valid, out.valid(), (size_t)nb);
    if (st_out) std::memcpy(st_out, out.state(), sizeof(RansacState));
    return GV_OK;
  }
  if (with_ground) {   // no boxes: the ground count still decides the return value
    if ((rc = h->pose.ground.reserve(h, n))) return rc;
    if ((rc = R.begin(h, sizeof(RansacState), done))) return rc;
    launch_ransac_mask(ransac_args(h, thr_f, kPoseRansacIters, kPoseRansacSeed, reinterpret_cast<RansacState *>(R.payload())), done,
                       h->stream);
    GV_HIP(hipGetLastError());
    if ((rc = R.wait(h))) return rc;
    if (st_out) std::memcpy(st_out, R.payload(), sizeof(RansacState));
    return GV_OK;
  }
  GV_HIP(hipStreamSynchronize(h->stream));
  return GV_OK;
  GV_CATCH
}

int gv_compute_bbox_pose(gv_handle h, const gv_bbox *bboxes, int32_t nb, gv_lshape_pose *poses_out, uint8_t *valid)
{
  return compute_bbox_pose_impl(h, bboxes, nb, poses_out, valid, false, nullptr);
}

// segmentGroundPlane on the device; state (plane, inlier count) comes back, the mask stays resident
static int segment_ground_device(gv_context *h, double threshold, int32_t iterations, uint64_t seed, RansacState &st)
{
  const size_t n = h->n;
  ResultBlock &R = h->pose.res;
  st = RansacState{};
  h->pose.ground_n = 0;
  if (n < 3) return GV_OK;
  int rc;
  if ((rc = ensure_ransac_buffers(h, n, iterations))) return rc;
  if ((rc = h->pose.ground.reserve(h, n))) return rc;
  const float thr_f = host::ceil_to_float(threshold);
  launch_ransac_plane(ransac_args(h, thr_f, iterations, seed), h->stream);
  CallDone done;
  if ((rc = R.begin(h, sizeof(RansacState), done))) return rc;
  launch_ransac_mask(ransac_args(h, thr_f, iterations, seed, reinterpret_cast<RansacState *>(R.payload())), done, h->stream);
  GV_HIP(hipGetLastError());
  if ((rc = R.wait(h))) return rc;
  std::memcpy(&st, R.payload(), sizeof(RansacState));
  h->pose.ground_n = n;
  return GV_OK;
}

// gv_segment_ground_plane; st: the state the call brings home anyway (handed on by gv_test_ransac_state only)
static int segment_ground_plane_impl(gv_handle h, double threshold, int32_t iterations, uint64_t seed, uint8_t *is_ground,
                                     float coeff[4], int64_t *n_inliers, RansacState &st)
{
  st = RansacState{};
  if (!h || !(threshold > 0.0) || iterations < 1 || iterations > 4096) return GV_ERR_BAD_ARG;
  if (!h->has_cl) return GV_ERR_TF;
  GV_TRY
  int rc = use_device(h);
  if (rc) return rc;
  if (coeff) coeff[0] = coeff[1] = coeff[2] = coeff[3] = 0.0f;
  if (n_inliers) *n_inliers = 0;
  if (is_ground && h->n) std::memset(is_ground, 0, h->n);
  if ((rc = segment_ground_device(h, threshold, iterations, seed, st))) return rc;
  if (!st.best_count) return GV_OK;   // "Could not estimate a planar model" (:122-126)
  if (is_ground) {   // the caller asked for the per-point mask: the only O(N) transfer of this call
    GV_HIP(hipMemcpyAsync(is_ground, h->pose.ground, h->n, hipMemcpyDeviceToHost, h->stream));
    GV_HIP(hipStreamSynchronize(h->stream));
  }
  if (coeff) { coeff[0] = st.refined.x; coeff[1] = st.refined.y; coeff[2] = st.refined.z; coeff[3] = st.refined.w; }
  if (n_inliers) *n_inliers = (int64_t)st.n_inliers;
  return GV_OK;
  GV_CATCH
}

int gv_segment_ground_plane(gv_handle h, double threshold, int32_t iterations, uint64_t seed, uint8_t *is_ground,
                            float coeff[4], int64_t *n_inliers)
{
  RansacState st;
  return segment_ground_plane_impl(h, threshold, iterations, seed, is_ground, coeff, n_inliers, st);
}

// gv_compute_bbox_pose_ground_removed; st: as above
static int bbox_pose_ground_removed_impl(gv_handle h, const gv_bbox *bboxes, int32_t nb, gv_lshape_pose *poses_out,
                                         uint8_t *valid, int32_t *n_poses_or_fail, RansacState &st)
{
  st = RansacState{};
  if (!h || nb < 0 || (nb && (!bboxes || !poses_out || !valid))) return GV_ERR_BAD_ARG;
  if (!h->has_cl) return GV_ERR_TF;
  // computeBBoxPose (cloud_detections.cpp:300-321): segmentGroundPlane -> extractCloudPerBBox -> PCA, enqueued as
  // one batch: the device decides the "empty segmented cloud" cases, the host reads 56 bytes of state + the poses
  if (n_poses_or_fail) *n_poses_or_fail = 0;
  int rc = compute_bbox_pose_impl(h, bboxes, nb, poses_out, valid, true, &st);
  if (rc) return rc;
  if (segmented_cloud_empty(st, h->n)) {
    for (int32_t b = 0; b < nb; ++b) valid[b] = 0;
    if (n_poses_or_fail) *n_poses_or_fail = -1;
    return GV_OK;
  }
  if (n_poses_or_fail)
    for (int32_t b = 0; b < nb; ++b) *n_poses_or_fail += valid[b];
  return GV_OK;
}

int gv_compute_bbox_pose_ground_removed(gv_handle h, const gv_bbox *bboxes, int32_t nb, gv_lshape_pose *poses_out,
                                        uint8_t *valid, int32_t *n_poses_or_fail)
{
  RansacState st;
  return bbox_pose_ground_removed_impl(h, bboxes, nb, poses_out, valid, n_poses_or_fail, st);
}

// test hook (gv_test_hooks.h): one of the two public calls above, and the RansacState it brought home
int gv_test_ransac_state(gv_handle h, double threshold, int32_t iterations, uint64_t seed, int32_t pose_path,
                         const gv_bbox *bboxes, int32_t nb, uint8_t *is_ground, gv_lshape_pose *poses_out, uint8_t *valid,
                         int32_t *n_poses_or_fail, gv_test_ransac_state_t *out)
{
  if (!out) return GV_ERR_BAD_ARG;
  RansacState st;
  const int rc = pose_path ? bbox_pose_ground_removed_impl(h, bboxes, nb, poses_out, valid, n_poses_or_fail, st)
                           : segment_ground_plane_impl(h, threshold, iterations, seed, is_ground, nullptr, nullptr, st);
  const float4 pl = st.plane, rf = st.refined;
  out->plane[0] = pl.x; out->plane[1] = pl.y; out->plane[2] = pl.z; out->plane[3] = pl.w;
  out->refined[0] = rf.x; out->refined[1] = rf.y; out->refined[2] = rf.z; out->refined[3] = rf.w;
  out->m = st.m; out->n_inliers = st.n_inliers; out->best_count = st.best_count; out->pad = 0u;
  return rc;
}

// test hook (gv_test_hooks.h): the public call, then the selected points and their keep flags as it left them
int gv_test_bbox_pose_nodes(gv_handle h, const gv_bbox *bboxes, int32_t nb, int32_t with_ground, gv_lshape_pose *poses_out,
                            uint8_t *valid, int32_t *n_poses_or_fail, float *nodes, uint8_t *keep, int64_t *n_sel)
{
  if (!h || !n_sel || !nodes || !keep) return GV_ERR_BAD_ARG;
  *n_sel = 0;
  int rc = with_ground ? gv_compute_bbox_pose_ground_removed(h, bboxes, nb, poses_out, valid, n_poses_or_fail)
                       : gv_compute_bbox_pose(h, bboxes, nb, poses_out, valid);
  if (rc) return rc;
  GV_TRY
  if (nb == 0 || h->n == 0 || (with_ground && h->n < 3)) return GV_OK;   // nothing was launched
  if ((rc = set_device_only(h))) return rc;
  uint32_t m = 0;
  GV_HIP(hipMemcpyAsync(&m, h->pose.buckets().n_selected(), sizeof(m), hipMemcpyDeviceToHost, h->stream));
  GV_HIP(hipStreamSynchronize(h->stream));
  if ((size_t)m > h->n) { h->err = "more selected points than points"; return GV_ERR_STATE; }
  if (m) {
    GV_HIP(hipMemcpyAsync(nodes, h->pose.nodes, (size_t)m * sizeof(CellNode), hipMemcpyDeviceToHost, h->stream));
    GV_HIP(hipMemcpyAsync(keep, h->pose.keep, (size_t)m, hipMemcpyDeviceToHost, h->stream));
    GV_HIP(hipStreamSynchronize(h->stream));
  }
  *n_sel = (int64_t)m;
  return GV_OK;
  GV_CATCH
}

/* ------------------------------------------------------------ the node's tick -- */
// GridVision::timerCallback from filterBBoxes on (grid_vision_node.cpp:153-244) as ONE batch of device work: the
// static boxes' kNN depth (:168-184), the dynamic boxes' poses -- orientation-network geometry (:190-209) or ground
// removal + per-box clouds + radius filter + PCA rectangle (:210-231) --, their rectangles in the base frame, the
// map update with the int8 pack, and the packed grid's way home.  The poses never leave the device on their way
// into the grid (k_pca_bbox / k_vision -> k_rects_from_poses(from_cam) -> grid pass); what the markers need comes
// back through the pinned result block.  gv_tick_wait is the tick's only host wait.
int gv_tick_enqueue(gv_handle h, const gv_tick_desc *d)
{
  if (!h || !d || d->n_bboxes < 0 || d->n_bboxes > 16383 || (d->n_bboxes && !d->bboxes)) return GV_ERR_BAD_ARG;
  if (d->n_net < 0 || (d->n_net && (!d->orient || !d->conf || !d->dims))) return GV_ERR_BAD_ARG;
  const bool vision = d->flags & GV_TICK_VISION_ORIENT;
  const bool lidar = d->flags & GV_TICK_LIDAR_BIN, lidar_ray = d->flags & GV_TICK_LIDAR_RAYMARCH;
  if (lidar_ray && !lidar) return GV_ERR_BAD_ARG;
  GV_TRY
  gv_context::Tick &T = h->tick;
  if (T.pending) return GV_ERR_STATE;   // one tick at a time (the node's timer is single threaded, grid_vision_node.cpp:49-50)
  const bool keep_dets = d->flags & GV_TICK_KEEP_DETS;   // [EXTENSION] X15
  T.dets_live = false;
  const int32_t n_all = d->n_bboxes;
  // filterBBoxes (:384-403), order preserving
  std::vector<gv_bbox> cat((size_t)2 * n_all + 1);
  int32_t ns = 0, nd = 0;
  if (n_all) {
    std::memcpy(cat.data(), d->bboxes, (size_t)n_all * sizeof(gv_bbox));
    std::vector<gv_bbox> dy((size_t)n_all);
    int rcf = gv_filter_bboxes(d->bboxes, n_all, cat.data() + n_all, &ns, dy.data(), &nd);
    if (rcf) return rcf;
    std::memcpy(cat.data() + n_all + ns, dy.data(), (size_t)nd * sizeof(gv_bbox));
  }
  const int32_t k = d->k_near;
  if (ns && (k < 1 || k > 32)) return GV_ERR_BAD_ARG;
  if (vision && d->n_net && d->n_net != nd) return GV_ERR_BAD_ARG;
  if (n_all && (!h->has_cl || !h->has_bc)) return GV_ERR_TF;   // transformLidarToCamera / transformPoseToBaseFrame
  if (lidar && !h->has_bl) return GV_ERR_TF;
  if (lidar && !sector_path(h)) { h->err = "the lidar extension inside the tick needs the tile path (nx % 4 == 0)"; return GV_ERR_STATE; }
  int rc = use_device(h);   // frames in flight finish first: the tick's work is one sequence on the public stream
  if (rc) return rc;
  hipStream_t s = h->stream;
  const size_t n = h->n;
  const bool pca = !vision && nd > 0 && n >= 3;              // computeBBoxPose on ALL boxes (:215-216)
  const bool net = vision && nd > 0 && d->n_net == nd;       // poses only when the network ran for every dynamic box
  DetSet &D = h->det[2];
  if (n_all) {
    DetUpload u;   // [all | static | dynamic] boxes in one block; the bbox test (the PCA branch's) covers the first n_all
    u.bboxes = cat.data(); u.nb = 2 * n_all;
    if (net) { u.orient = d->orient; u.conf = d->conf; u.dims = d->dims; }
    u.stream = s;
    u.masks = pca;
    u.n_net = net ? nd : 0; u.nb_test = n_all;
    u.fused = true;
    if ((rc = upload_det(h, D, u))) return rc;
    GV_HIP(hipEventRecord(D.ready, s));
  }
  // result block: depths | poses, state, valid (the PCA call's layout) | VisionOut
  T.off_depth = 0;
  T.off_pose = ((size_t)ns * sizeof(float) + 15) & ~(size_t)15;
  T.off_vout = (T.off_pose + PoseBlock::bytes(n_all) + 15) & ~(size_t)15;
  CallDone none;   // nothing published: the tick ends with an event on the public stream
  if ((rc = h->pose.res.begin(h, T.off_vout + (size_t)nd * sizeof(VisionOut) + 16, none))) return rc;
  none = CallDone{};
  uint8_t *blk = h->pose.res.payload();
  // --- static boxes: buildKDTree + computeDepthForBoundingBoxes (:168-184).  Independent of the pose branch: it
  // runs on a lane beside it and joins the public stream before the tick's last event.
  T.knn_ran = ns > 0;
  bool knn_forked = false;
  if (ns > 0) {
    if ((rc = ensure_tbuf(h, std::max<size_t>(n, 1)))) return rc;
    if ((rc = h->pose.knn_partial.reserve(h, knn_partial_entries(ns, k)))) return rc;
    hipStream_t sk = s;
    if (h->tune.tick_knn_lane && nd > 0) {
      sk = h->streams[1];
      GV_HIP(hipEventRecord(T.fork, s));
      GV_HIP(hipStreamWaitEvent(sk, T.fork, 0));
      h->sb[1].lane_clean = false;
      knn_forked = true;
    }
    const KnnArgs ka = knn_args(h, D.bboxes + n_all, ns, k, reinterpret_cast<float *>(blk + T.off_depth), nullptr);
    launch_project_uvd(ka, sk);
    launch_knn(ka, none, sk);
    GV_HIP(hipGetLastError());
    if (knn_forked) GV_HIP(hipEventRecord(T.join, sk));
  }
  // --- dynamic boxes -> camera-frame poses on the device -> rectangles
  int32_t n_rects = 0;
  Rect *rects = h->fs[0].rects;
  T.pca_ran = T.vision_ran = false;
  TickDetsArgs da{};   // what k_tick_dets reads of the branch that ran (kTickDetsNone: an empty list)
  if (keep_dets) {
    if ((rc = T.dets.reserve(h, 1)) || (net && (rc = T.dets_vout.reserve(h, (size_t)nd + (size_t)nd / 4))) ||
        (pca && (rc = T.dets_valid.reserve(h, (size_t)n_all + (size_t)n_all / 4))))
      return rc;
    da.tf_bc = h->tf_bc;
    da.out = T.dets;
  }
  RectsFromPosesArgs ra;   // either branch's camera-frame poses -> rectangles
  ra.poses = D.poses; ra.g = h->g; ra.from_cam = true; ra.bc = h->x_bc; ra.rects = rects;
  if (net) {   // VisionOrientation::postProcessOutputs (:190-209)
    VisionArgs va;
    va.orient = D.orient; va.conf = D.conf; va.dims = D.dims; va.bboxes = D.bboxes + n_all + ns; va.nb = nd;
    va.cam = h->cam;
    va.out = reinterpret_cast<VisionOut *>(blk + T.off_vout); va.poses_cam = D.poses;
    va.out_dev = keep_dets ? T.dets_vout.get() : nullptr;
    launch_vision(va, s);
    ra.n = nd;
    launch_rects_from_poses(ra, s);
    n_rects = nd;
    T.vision_ran = true;
    da.mode = kTickDetsVision; da.n_cand = nd; da.vout = T.dets_vout;
  } else if (pca) {   // cloud_detections::computeBBoxPose (:210-231)
    const float thr_f = host::ceil_to_float(0.04);
    if ((rc = ensure_ransac_buffers(h, n, kPoseRansacIters))) return rc;
    launch_ransac_plane(ransac_args(h, thr_f, kPoseRansacIters, kPoseRansacSeed), s);
    h->pose.ground_n = 0;
    if ((rc = enqueue_bbox_pose(h, n_all, true, thr_f, PoseBlock(blk + T.off_pose, n_all), none, D.poses,
                                keep_dets ? T.dets_valid.get() : nullptr)))
      return rc;
    ra.n = n_all;
    launch_rects_from_poses(ra, s);
    n_rects = n_all;
    T.pca_ran = true;
    da.mode = kTickDetsPca; da.n_cand = n_all; da.cam = D.poses; da.valid = T.dets_valid;
    da.st = h->pose.rstate; da.n_cloud = (uint64_t)n;
  }
  if (keep_dets) launch_tick_dets(da, s);   // behind the pose kernels, inside `done`
  GV_HIP(hipGetLastError());
  // --- map update (:145, :206, :230, :235) + int8 pack (:265-278)
  if (lidar && n > 0) {   // [EXTENSION] the fused frame's kernels, serial on the public stream
    if ((rc = ensure_point_buffers(h, n))) return rc;
    BinningJob bin{D};   // buffer set 0 and the public stream throughout
    bin.n = n;
    bin.do_ray = lidar_ray; bin.write_hits = true;
    if ((rc = enqueue_binning(h, bin))) return rc;
    SectorsJob sec;
    sec.stream = s;
    if (lidar_ray && (rc = enqueue_sectors(h, sec))) return rc;
    GridPassJob grid;
    grid.rects = rects; grid.n_rects = n_rects;
    grid.counts = true;
    grid.y1 = h->g.ny;
    grid.stream = s;
    if ((rc = enqueue_grid_pass(h, grid))) return rc;
    // a tick writes no per-point output: those of the call before it stay where they are
    set_last_frame(h, 0, 0, h->last.points, true, true, h->last.cell_idx, h->last.bbox_id);
  } else if ((rc = enqueue_plain_update(h, n_rects)))
    return rc;
  // a copy command, not gv_publish_grid_async's kernel: no upload competes for the copy engines inside a tick, and the
  // kernel measured no faster here (0.326 vs 0.321 ms PCA tick, 0.167 vs 0.161 ms vision tick)
  if (d->grid_out) GV_HIP(hipMemcpyAsync(d->grid_out, h->occ_i8, (size_t)h->g.G, hipMemcpyDeviceToHost, s));
  if (knn_forked) GV_HIP(hipStreamWaitEvent(s, T.join, 0));
  GV_HIP(hipEventRecord(T.done, s));
  T.flags = d->flags;
  T.n_all = n_all; T.n_static = ns; T.n_dynamic = nd;
  T.st_boxes.assign(cat.begin() + n_all, cat.begin() + n_all + ns);
  T.n = n;
  T.cloud = h->cloud_cur;
  T.tf_bc = h->tf_bc;
  T.x_bc = h->x_bc;
  T.pending = true;
  T.dets_live = keep_dets;
  return GV_OK;
  GV_CATCH
}

int gv_tick_wait(gv_handle h, gv_tick_result *r)
{
  if (!h || !r) return GV_ERR_BAD_ARG;
  GV_TRY
  gv_context::Tick &T = h->tick;
  if (!T.pending) return GV_ERR_STATE;
  int rc = set_device_only(h);
  if (rc) return rc;
  GV_HIP(hipEventSynchronize(T.done));   // the tick's one host wait
  T.pending = false;
  uint8_t *blk = h->pose.res.payload();
  r->n_static = T.n_static;
  r->n_dynamic = T.n_dynamic;
  r->n_poses = 0;
  r->pca_empty = 0;
  if (T.n_static) {
    const float *dep = reinterpret_cast<const float *>(blk + T.off_depth);
    if (r->static_bboxes) std::memcpy(r->static_bboxes, T.st_boxes.data(), (size_t)T.n_static * sizeof(gv_bbox));
    if (r->depths) std::memcpy(r->depths, dep, (size_t)T.n_static * sizeof(float));
    if (r->base_points_xyz) convert_pixels_host(h->Kinv, T.x_bc, T.st_boxes.data(), dep, T.n_static, r->base_points_xyz);   // :180
  }
  if (T.vision_ran) {
    // transformLShapeObjects (:204)
    r->n_poses = collect_vision_poses(reinterpret_cast<const VisionOut *>(blk + T.off_vout), T.n_dynamic, &T.tf_bc, r->poses);
  } else if (T.pca_ran) {
    const PoseBlock pb(blk + T.off_pose, T.n_all);
    const gv_lshape_pose *ps = pb.poses();
    const uint8_t *valid = pb.valid();
    RansacState st;
    std::memcpy(&st, pb.state(), sizeof(st));
    if (segmented_cloud_empty(st, T.n)) r->pca_empty = 1;   // T.n: the cloud the tick read, not the handle's now
    else
      for (int32_t b = 0; b < T.n_all; ++b) {
        if (!valid[b]) continue;   // :174-175
        gv_lshape_pose p = ps[b];
        host::transform_pose(T.tf_bc, p);   // transformLShapeObjects (:227)
        if (r->poses) r->poses[r->n_poses] = p;
        r->n_poses++;
      }
  } else if (!(T.flags & GV_TICK_VISION_ORIENT) && T.n_dynamic > 0)
    r->pca_empty = 1;   // fewer than three points: no plane, no poses
  return GV_OK;
  GV_CATCH
}

// test hooks (gv_test_hooks.h): the list of the last GV_TICK_KEEP_DETS tick, read back; and its host twin
int gv_test_tick_dets(gv_handle h, gv_lshape_pose *out, int32_t *n, int32_t *n_total)
{
  if (!h || !out || !n || !n_total) return GV_ERR_BAD_ARG;
  GV_TRY
  if (!h->tick.dets_live) return state_error(h, "gv_test_tick_dets", "the last tick enqueued did not carry GV_TICK_KEEP_DETS");
  int rc = set_device_only(h);
  if (rc) return rc;
  std::vector<TickDetList> l(1);
  GV_HIP(hipMemcpyAsync(l.data(), h->tick.dets.get(), sizeof(TickDetList), hipMemcpyDeviceToHost, h->stream));
  GV_HIP(hipStreamSynchronize(h->stream));
  std::memcpy(out, l[0].p, sizeof(l[0].p));
  *n = l[0].n;
  *n_total = l[0].n_total;
  return GV_OK;
  GV_CATCH
}

int gv_test_tick_dets_host(const gv_lshape_pose *cam, const uint8_t *valid, int32_t n_cand, int32_t empty, const gv_transform *tf_bc,
                           gv_lshape_pose *out, int32_t *n, int32_t *n_total)
{
  if (n_cand < 0 || n_cand > kTickDetCandidates || (n_cand && (!cam || !valid)) || !tf_bc || !out || !n || !n_total) return GV_ERR_BAD_ARG;
  tick_dets_host(cam, valid, n_cand, empty != 0, *tf_bc, out, *n, *n_total);
  return GV_OK;
}

int gv_tick(gv_handle h, const gv_tick_desc *d, gv_tick_result *r)
{
  int rc = gv_tick_enqueue(h, d);
  if (rc) return rc;
  return gv_tick_wait(h, r);
}

}  // extern "C"
