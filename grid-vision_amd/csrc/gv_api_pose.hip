// gv_api_pose.hip -- the result block, kNN depth, RANSAC ground plane, per-box PCA poses, the vision
// post-processing and the node's tick (gv_tick_*).
#include <atomic>
#include <algorithm>
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
  if ((rc = upload_det(h, d, bboxes, nb, nullptr, 0, orient, conf, dims, h->stream, false))) return rc;
  GV_HIP(hipEventRecord(d.ready, h->stream));
  launch_vision(d.orient, d.conf, d.dims, d.bboxes, nb, h->cam, h->sb[0].vout, d.poses, nullptr, h->stream);
  GV_HIP(hipGetLastError());
  std::vector<VisionOut> vo((size_t)nb);
  GV_HIP(hipMemcpyAsync(vo.data(), h->sb[0].vout, (size_t)nb * sizeof(VisionOut), hipMemcpyDeviceToHost, h->stream));
  GV_HIP(hipStreamSynchronize(h->stream));
  int32_t m = 0;
  for (int32_t i = 0; i < nb; ++i) {
    if (!vo[i].valid) continue;   // vision_orientation.cpp:496-499
    poses_out[m++] = pose_of_vision_out(vo[i]);
  }
  *n_out = m;
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
  if ((rc = upload_det(h, d, bboxes, nb, nullptr, 0, orient, conf, dims, h->stream, false))) return rc;
  GV_HIP(hipEventRecord(d.ready, h->stream));
  DevBuf<float> dsets;   // nb * 64 * (loc0, loc1, loc2, err), then nb winners
  if ((rc = dsets.reserve(h, (size_t)nb * 257))) return rc;
  launch_vision(d.orient, d.conf, d.dims, d.bboxes, nb, h->cam, h->sb[0].vout, d.poses, dsets, h->stream);
  GV_HIP(hipGetLastError());
  GV_HIP(hipMemcpyAsync(sets, dsets, (size_t)nb * 256 * sizeof(float), hipMemcpyDeviceToHost, h->stream));
  GV_HIP(hipMemcpyAsync(winner, dsets + (size_t)nb * 256, (size_t)nb * sizeof(int32_t), hipMemcpyDeviceToHost, h->stream));
  GV_HIP(hipStreamSynchronize(h->stream));
  return GV_OK;
  GV_CATCH
}

// ---- the result block (see gv_context::res_host) ----
constexpr size_t kResHeader = 64;

// a block with room for `bytes` of payload; the CallDone of the call about to be enqueued
static int begin_result(gv_context *h, size_t bytes, CallDone &done)
{
  // a tick between gv_tick_enqueue and gv_tick_wait owns the result block (and the standalone detection set): the
  // calls that would reuse them are refused until the tick has been waited for
  if (h->tick.pending) { h->err = "a tick is pending: call gv_tick_wait first"; return GV_ERR_STATE; }
  int rc;
  if (bytes + kResHeader > h->res_host.cap()) {
    GV_HIP(hipStreamSynchronize(h->stream));   // nothing in flight writes the old block
    const size_t want = std::max<size_t>(2 * (bytes + kResHeader), 16384);
    // coherent (fine-grained) explicitly: the host must see the payload and the flag while the kernel that stores them
    // is still running, whatever HIP_HOST_COHERENT says
    if ((rc = h->res_host.reserve(h, want, hipHostMallocCoherent | hipHostMallocMapped))) return rc;
    std::memset(h->res_host, 0, want);
  }
  if ((rc = h->d_res_ticket.reserve_zeroed(h, 16, h->stream))) return rc;   // 64 bytes
  if (++h->res_seq == 0u) h->res_seq = 1u;   // 0 = "nothing published yet"
  done.ticket = h->d_res_ticket;
  done.flag = reinterpret_cast<unsigned *>(h->res_host.get());
  done.seq = h->res_seq;
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
static int wait_result(gv_context *h)
{
  volatile unsigned *flag = reinterpret_cast<volatile unsigned *>(h->res_host.get());
  const unsigned seq = h->res_seq;
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
  if ((rc = h->knn_partial.reserve(h, knn_partial_entries(nb, k)))) return rc;
  // depths | sorted squared distances, stored by the merge kernel straight into the result block
  CallDone done;
  if ((rc = begin_result(h, (size_t)nb * (1 + (size_t)k) * sizeof(float), done))) return rc;
  float *r_depths = reinterpret_cast<float *>(h->res_host + kResHeader), *r_d2 = r_depths + nb;
  // buildKDTree projection (cloud_detections.cpp:8-33) then the exact k nearest (:43-87)
  launch_project_uvd(h->cx, h->cy, h->cz, (uint32_t)h->n, h->m_cam, h->camk, h->tx, h->ty, h->tz, h->stream);
  launch_knn(h->tx, h->ty, h->tz, (uint32_t)h->n, h->det[2].bboxes, nb, k, h->knn_partial, r_depths, knn_d2 ? r_d2 : nullptr, done,
             h->stream);
  GV_HIP(hipGetLastError());
  if ((rc = wait_result(h))) return rc;
  std::memcpy(depths, r_depths, (size_t)nb * sizeof(float));
  if (knn_d2) std::memcpy(knn_d2, r_d2, (size_t)nb * k * sizeof(float));
  return GV_OK;
  GV_CATCH
}

static int ensure_ransac_buffers(gv_context *h, size_t n, int32_t iterations)
{
  int rc;
  if ((size_t)iterations > h->planes_cap) {
    h->planes_cap = 0;
    if ((rc = h->d_planes.reserve(h, (size_t)iterations)) ||
        (rc = h->d_plane_counts.reserve_zeroed(h, (size_t)iterations * kRansacCountSlices, h->stream)))   // every pass leaves them zero
      return rc;
    h->planes_cap = (size_t)iterations;
  }
  if ((rc = h->d_rscratch.reserve(h, ransac_scratch_doubles(n)))) return rc;
  return h->d_rstate.reserve_zeroed(h, 1, h->stream);
}

static size_t pose_block_valid_off(int32_t nb) { return (size_t)nb * sizeof(gv_lshape_pose) + sizeof(RansacState); }
static size_t pose_block_bytes(int32_t nb) { return pose_block_valid_off(nb) + (size_t)nb; }

// extractCloudPerBBox -> RadiusOutlierRemoval -> centroid + PCA rectangle, all on the device and all enqueued
// without a host wait in between; only the nb poses come back.  with_ground: the points of the refined RANSAC
// plane in *d_rstate are dropped first (computeBBoxPose, cloud_detections.cpp:300-321), and the "empty segmented
// cloud" outcomes (:307-309) are decided on the device.
// poses_dev (optional): the camera-frame poses also go to device memory (a NaN length marks "no pose": its
// corners fail getIndex, so k_rects_from_poses gives it no cells), for a map update enqueued right behind this without a trip to the host.
static int enqueue_bbox_pose(gv_context *h, int32_t nb, bool with_ground, float thr_f, uint8_t *out, const CallDone &done,
                             gv_lshape_pose *poses_dev = nullptr)
{
  const size_t n = h->n;
  int rc;
  if (n > h->pc_cap) {
    h->pc_cap = 0;
    const size_t want = n + n / 8 + 1024;
    if ((rc = h->d_nodes.reserve(h, want)) || (rc = h->d_keep.reserve(h, want)) || (rc = h->d_ticket_of.reserve(h, want))) return rc;
    h->pc_cap = want;
  }
  if ((size_t)nb > h->pca_cap) {
    h->pca_cap = 0;
    const size_t want = (size_t)nb + (size_t)nb / 4 + 64;
    if ((rc = h->d_pca_acc.reserve_zeroed(h, pca_acc_words((int)want), h->stream)) ||   // every call leaves them zero
        (rc = h->d_pca_ext.reserve_zeroed(h, pca_ext_words((int)want), h->stream)))
      return rc;
    h->pca_cap = want;
  }
  if ((rc = h->d_pca_ticket.reserve_zeroed(h, 16, h->stream))) return rc;   // 64 bytes
  // cell buckets: a power of two, about one per two points (the three arrays stay L2 resident at config-3 size;
  // cells that share a bucket only add candidates that fail the id or distance test)
  size_t n_buckets = 4096;
  while (n_buckets < n / 2 && n_buckets < ((size_t)1 << 25)) n_buckets <<= 1;
  if (n_buckets > h->head_cap) {
    h->head_cap = 0;
    if ((rc = h->d_cellcnt.reserve_zeroed(h, n_buckets, h->stream)) ||   // every call counts them back to zero
        (rc = h->d_cellpre.reserve(h, n_buckets + 4)) ||
        (rc = h->d_celloff.reserve_zeroed(h, n_buckets / 4096 + 4, h->stream)))   // [n_buckets / 4096 + 2] = the scan's ticket
      return rc;
    h->head_cap = n_buckets;
  }
  n_buckets = h->head_cap;   // the table only grows
  if ((rc = h->d_rstate.reserve_zeroed(h, 1, h->stream))) return rc;
  hipStream_t s = h->stream;
  // extractCloudPerBBox + RadiusOutlierRemoval(0.4, 10)  (cloud_detections.cpp:250-298, 150-154)
  const double radius = 0.4;
  launch_radius_filter(h->cx, h->cy, h->cz, (uint32_t)n, h->m_cam, h->camk, bbox_test_of(h, h->det[2]), nb, with_ground, thr_f,
                       h->d_rstate, h->sb[h->last.points].bbox_id, h->d_cellcnt, h->d_cellpre, h->d_celloff,
                       h->d_celloff + n_buckets / 4096 + 2, h->d_nodes, h->d_keep, h->d_ticket_of, h->d_pca_acc, (uint32_t)n_buckets,
                       host::floor_to_float(radius * radius), 10, s);
  h->last.bbox_id = true;
  // centroid + PCA rectangle per bbox from order-independent integer sums over the kept points (:156-247)
  launch_pca_rect(h->d_nodes, h->d_celloff + n_buckets / 4096, (uint32_t)n, h->d_keep, h->d_pca_acc, h->d_pca_ext, h->d_pca_ticket, nb,
                  h->d_rstate, with_ground, reinterpret_cast<gv_lshape_pose *>(out), out + pose_block_valid_off(nb),
                  reinterpret_cast<RansacState *>(out + (size_t)nb * sizeof(gv_lshape_pose)), done, s, poses_dev);
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
  if (with_ground) {   // segmentGroundPlane(0.04, 50 hypotheses) on the camera-frame cloud (grid_vision_node.cpp:215-216)
    if ((rc = ensure_ransac_buffers(h, n, 50))) return rc;
    launch_ransac_plane(h->cx, h->cy, h->cz, (uint32_t)n, h->m_cam, thr_f, 50, 12345ull, h->d_planes, h->d_plane_counts,
                        h->d_rscratch, h->d_rstate, h->stream);
    GV_HIP(hipGetLastError());
    h->ground_n = 0;   // the mask itself is not materialised on this path
  }
  if (nb) {
    // poses | state | flags: stored by the PCA kernel straight into the result block, no copy, no runtime wait
    CallDone done;
    if ((rc = begin_result(h, pose_block_bytes(nb), done))) return rc;
    const uint8_t *blk = h->res_host + kResHeader;
    if ((rc = enqueue_bbox_pose(h, nb, with_ground, thr_f, h->res_host + kResHeader, done))) return rc;
    if ((rc = wait_result(h))) return rc;
    std::memcpy(poses_out, blk, (size_t)nb * sizeof(gv_lshape_pose));
    std::memcpy(valid, blk + pose_block_valid_off(nb), (size_t)nb);
    if (st_out) std::memcpy(st_out, blk + (size_t)nb * sizeof(gv_lshape_pose), sizeof(RansacState));
    return GV_OK;
  }
  if (with_ground) {   // no boxes: the ground count still decides the return value
    if ((rc = h->d_ground.reserve(h, n))) return rc;
    CallDone done;
    if ((rc = begin_result(h, sizeof(RansacState), done))) return rc;
    launch_ransac_mask(h->cx, h->cy, h->cz, (uint32_t)n, h->m_cam, thr_f, h->d_rstate, h->d_ground,
                       reinterpret_cast<RansacState *>(h->res_host + kResHeader), done, h->stream);
    GV_HIP(hipGetLastError());
    if ((rc = wait_result(h))) return rc;
    if (st_out) std::memcpy(st_out, h->res_host + kResHeader, sizeof(RansacState));
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
  st = RansacState{};
  h->ground_n = 0;
  if (n < 3) return GV_OK;
  int rc;
  if ((rc = ensure_ransac_buffers(h, n, iterations))) return rc;
  if ((rc = h->d_ground.reserve(h, n))) return rc;
  const float thr_f = host::ceil_to_float(threshold);
  // camera-frame cloud (the reference segments transformed_cloud, grid_vision_node.cpp:215-216): transformed on the fly
  launch_ransac_plane(h->cx, h->cy, h->cz, (uint32_t)n, h->m_cam, thr_f, iterations, seed, h->d_planes, h->d_plane_counts,
                      h->d_rscratch, h->d_rstate, h->stream);
  CallDone done;
  if ((rc = begin_result(h, sizeof(RansacState), done))) return rc;
  launch_ransac_mask(h->cx, h->cy, h->cz, (uint32_t)n, h->m_cam, thr_f, h->d_rstate, h->d_ground,
                     reinterpret_cast<RansacState *>(h->res_host + kResHeader), done, h->stream);
  GV_HIP(hipGetLastError());
  if ((rc = wait_result(h))) return rc;
  std::memcpy(&st, h->res_host + kResHeader, sizeof(RansacState));
  h->ground_n = n;
  return GV_OK;
}

int gv_segment_ground_plane(gv_handle h, double threshold, int32_t iterations, uint64_t seed, uint8_t *is_ground,
                            float coeff[4], int64_t *n_inliers)
{
  if (!h || !(threshold > 0.0) || iterations < 1 || iterations > 4096) return GV_ERR_BAD_ARG;
  if (!h->has_cl) return GV_ERR_TF;
  GV_TRY
  int rc = use_device(h);
  if (rc) return rc;
  if (coeff) coeff[0] = coeff[1] = coeff[2] = coeff[3] = 0.0f;
  if (n_inliers) *n_inliers = 0;
  if (is_ground && h->n) std::memset(is_ground, 0, h->n);
  RansacState st;
  if ((rc = segment_ground_device(h, threshold, iterations, seed, st))) return rc;
  if (!st.best_count) return GV_OK;   // "Could not estimate a planar model" (:122-126)
  if (is_ground) {   // the caller asked for the per-point mask: the only O(N) transfer of this call
    GV_HIP(hipMemcpyAsync(is_ground, h->d_ground, h->n, hipMemcpyDeviceToHost, h->stream));
    GV_HIP(hipStreamSynchronize(h->stream));
  }
  if (coeff) { coeff[0] = st.refined.x; coeff[1] = st.refined.y; coeff[2] = st.refined.z; coeff[3] = st.refined.w; }
  if (n_inliers) *n_inliers = (int64_t)st.n_inliers;
  return GV_OK;
  GV_CATCH
}

int gv_compute_bbox_pose_ground_removed(gv_handle h, const gv_bbox *bboxes, int32_t nb, gv_lshape_pose *poses_out,
                                        uint8_t *valid, int32_t *n_poses_or_fail)
{
  if (!h || nb < 0 || (nb && (!bboxes || !poses_out || !valid))) return GV_ERR_BAD_ARG;
  if (!h->has_cl) return GV_ERR_TF;
  // computeBBoxPose (cloud_detections.cpp:300-321): segmentGroundPlane -> extractCloudPerBBox -> PCA, enqueued as
  // one batch: the device decides the "empty segmented cloud" cases, the host reads 56 bytes of state + the poses
  if (n_poses_or_fail) *n_poses_or_fail = 0;
  RansacState st;
  int rc = compute_bbox_pose_impl(h, bboxes, nb, poses_out, valid, true, &st);
  if (rc) return rc;
  const uint64_t m = st.best_count ? st.n_inliers : 0;
  if (m == 0 || (size_t)m == h->n) {   // empty segmented cloud -> the reference returns {} (:307-309)
    for (int32_t b = 0; b < nb; ++b) valid[b] = 0;
    if (n_poses_or_fail) *n_poses_or_fail = -1;
    return GV_OK;
  }
  if (n_poses_or_fail)
    for (int32_t b = 0; b < nb; ++b) *n_poses_or_fail += valid[b];
  return GV_OK;
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
  // the number of selected points sits behind the block offsets of the bucket table (enqueue_bbox_pose)
  uint32_t m = 0;
  GV_HIP(hipMemcpyAsync(&m, h->d_celloff + h->head_cap / 4096, sizeof(m), hipMemcpyDeviceToHost, h->stream));
  GV_HIP(hipStreamSynchronize(h->stream));
  if ((size_t)m > h->n) { h->err = "more selected points than points"; return GV_ERR_STATE; }
  if (m) {
    GV_HIP(hipMemcpyAsync(nodes, h->d_nodes, (size_t)m * sizeof(CellNode), hipMemcpyDeviceToHost, h->stream));
    GV_HIP(hipMemcpyAsync(keep, h->d_keep, (size_t)m, hipMemcpyDeviceToHost, h->stream));
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
    if ((rc = upload_det(h, D, cat.data(), 2 * n_all, nullptr, 0, net ? d->orient : nullptr, net ? d->conf : nullptr,
                         net ? d->dims : nullptr, s, pca, net ? nd : 0, n_all, true)))
      return rc;
    GV_HIP(hipEventRecord(D.ready, s));
  }
  // result block: depths | poses, state, valid (the PCA call's layout) | VisionOut
  T.off_depth = 0;
  T.off_pose = ((size_t)ns * sizeof(float) + 15) & ~(size_t)15;
  T.off_vout = (T.off_pose + pose_block_bytes(n_all) + 15) & ~(size_t)15;
  CallDone none;   // nothing published: the tick ends with an event on the public stream
  if ((rc = begin_result(h, T.off_vout + (size_t)nd * sizeof(VisionOut) + 16, none))) return rc;
  none = CallDone{};
  uint8_t *blk = h->res_host + kResHeader;
  // --- static boxes: buildKDTree + computeDepthForBoundingBoxes (:168-184).  Independent of the pose branch: it
  // runs on a lane beside it and joins the public stream before the tick's last event.
  T.knn_ran = ns > 0;
  bool knn_forked = false;
  if (ns > 0) {
    if ((rc = ensure_tbuf(h, std::max<size_t>(n, 1)))) return rc;
    if ((rc = h->knn_partial.reserve(h, knn_partial_entries(ns, k)))) return rc;
    hipStream_t sk = s;
    if (h->tune.tick_knn_lane && nd > 0) {
      sk = h->streams[1];
      GV_HIP(hipEventRecord(T.fork, s));
      GV_HIP(hipStreamWaitEvent(sk, T.fork, 0));
      h->sb[1].lane_clean = false;
      knn_forked = true;
    }
    launch_project_uvd(h->cx, h->cy, h->cz, (uint32_t)n, h->m_cam, h->camk, h->tx, h->ty, h->tz, sk);
    launch_knn(h->tx, h->ty, h->tz, (uint32_t)n, D.bboxes + n_all, ns, k, h->knn_partial,
               reinterpret_cast<float *>(blk + T.off_depth), nullptr, none, sk);
    GV_HIP(hipGetLastError());
    if (knn_forked) GV_HIP(hipEventRecord(T.join, sk));
  }
  // --- dynamic boxes -> camera-frame poses on the device -> rectangles
  int32_t n_rects = 0;
  Rect *rects = h->fs[0].rects;
  T.pca_ran = T.vision_ran = false;
  if (net) {   // VisionOrientation::postProcessOutputs (:190-209)
    launch_vision(D.orient, D.conf, D.dims, D.bboxes + n_all + ns, nd, h->cam, reinterpret_cast<VisionOut *>(blk + T.off_vout),
                  D.poses, nullptr, s);
    launch_rects_from_poses(D.poses, nd, h->g, true, h->x_bc, rects, s);
    n_rects = nd;
    T.vision_ran = true;
  } else if (pca) {   // cloud_detections::computeBBoxPose (:210-231)
    const float thr_f = host::ceil_to_float(0.04);
    if ((rc = ensure_ransac_buffers(h, n, 50))) return rc;
    launch_ransac_plane(h->cx, h->cy, h->cz, (uint32_t)n, h->m_cam, thr_f, 50, 12345ull, h->d_planes, h->d_plane_counts,
                        h->d_rscratch, h->d_rstate, s);
    h->ground_n = 0;
    if ((rc = enqueue_bbox_pose(h, n_all, true, thr_f, blk + T.off_pose, none, D.poses))) return rc;
    launch_rects_from_poses(D.poses, n_all, h->g, true, h->x_bc, rects, s);
    n_rects = n_all;
    T.pca_ran = true;
  }
  GV_HIP(hipGetLastError());
  // --- map update (:145, :206, :230, :235) + int8 pack (:265-278)
  if (lidar && n > 0) {   // [EXTENSION] the fused frame's kernels, serial on the public stream
    if ((rc = ensure_point_buffers(h, n))) return rc;
    if ((rc = enqueue_binning(h, D, 0, 0, 0, n, false, lidar_ray, false, true, nullptr))) return rc;
    if (lidar_ray && (rc = enqueue_sectors(h, 0, 0, 1, s))) return rc;
    if ((rc = enqueue_grid_pass(h, 0, rects, n_rects, true, 0, h->g.ny, s))) return rc;
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
  const uint8_t *blk = h->res_host + kResHeader;
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
    const VisionOut *vo = reinterpret_cast<const VisionOut *>(blk + T.off_vout);
    for (int32_t i = 0; i < T.n_dynamic; ++i) {
      if (!vo[i].valid) continue;   // vision_orientation.cpp:496-499
      gv_lshape_pose p = pose_of_vision_out(vo[i]);
      host::transform_pose(T.tf_bc, p);   // transformLShapeObjects (:204)
      if (r->poses) r->poses[r->n_poses] = p;
      r->n_poses++;
    }
  } else if (T.pca_ran) {
    const gv_lshape_pose *ps = reinterpret_cast<const gv_lshape_pose *>(blk + T.off_pose);
    RansacState st;
    std::memcpy(&st, blk + T.off_pose + (size_t)T.n_all * sizeof(gv_lshape_pose), sizeof(st));
    const uint8_t *valid = blk + T.off_pose + pose_block_valid_off(T.n_all);
    const uint64_t m = st.best_count ? st.n_inliers : 0;
    if (m == 0 || (size_t)m == T.n) r->pca_empty = 1;   // empty segmented cloud: computeBBoxPose returns {} (:307-309)
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

int gv_tick(gv_handle h, const gv_tick_desc *d, gv_tick_result *r)
{
  int rc = gv_tick_enqueue(h, d);
  if (rc) return rc;
  return gv_tick_wait(h, r);
}

}  // extern "C"
