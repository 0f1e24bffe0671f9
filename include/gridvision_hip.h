/*
 * gridvision_hip.h -- C ABI of the MI355X (gfx950) implementation of
 * grid-vision's per-frame hot path.  libgridvision_hip.so exports exactly the
 * functions declared here; plain pointers and sizes, no C++/torch types, no
 * exception ever crosses this boundary.
 *
 * The reference (rohankhaire-work/grid-vision) has no FFI boundary of its own:
 * the hot path is called in-process from GridVision::timerCallback
 * (src/grid_vision_node.cpp:108-244).  Each entry point below cites the
 * reference interface it replaces (file:line relative to the reference root).
 * INTEGRATION.md shows the node-side binding.
 *
 * Conventions
 *   - every function returns a gv_status (0 = ok); out-of-map rectangles and
 *     points are NOT errors (the reference skips them silently,
 *     src/occupancy_grid.cpp:152-156,171-172);
 *   - one handle = one GPU + one resident grid + the HIP streams of its frame
 *     pipeline (gv_stream returns the public one: every frame finishes there, in
 *     order, and callers may order their own work on it); a handle is used by
 *     one thread at a time; handles are independent;
 *   - host pointers are caller owned and may be pageable; every call returns
 *     after its results are complete in the caller's buffers (synchronous),
 *     except the streaming calls gv_frame_enqueue, gv_cloud_upload_*_async,
 *     gv_frame_set_detections_async and gv_grid_move (see there);
 *   - grid layers use the reference's storage order: grid_map's column-major
 *     Eigen::MatrixXf(size0,size1) with row = x index, i.e. linear = iy*nx+ix;
 *   - [EXTENSION] marks what north_star asks for and the reference lacks.
 *
 * [EXTENSION] X16, scan-to-costmap matching, has a header of its own beside this one, gridvision_hip_match.h, which
 * includes this one; the library exports its functions as well.
 */
#ifndef GRIDVISION_HIP_H_
#define GRIDVISION_HIP_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct gv_context *gv_handle;

typedef enum {
  GV_OK = 0,
  GV_ERR_BAD_ARG = 1,     /* null pointer, size out of range, bad flag        */
  GV_ERR_HIP = 2,         /* a HIP runtime call failed (gv_last_error)        */
  GV_ERR_RCCL = 3,        /* an RCCL call failed                               */
  GV_ERR_NO_DEVICE = 4,   /* no gfx950 device / device id out of range        */
  GV_ERR_STATE = 5,       /* call order violated (e.g. no cloud uploaded)     */
  GV_ERR_TF = 6           /* a required transform was never set (the          */
                          /* reference returns nullptr: grid_vision_node.cpp:292-297) */
} gv_status;

/* BoundingBox  include/grid_vision/object_detection.hpp:27-32 (40 bytes) */
typedef struct {
  double x_min, y_min, x_max, y_max;
  float confidence;
  int32_t label;          /* ObjectClass, object_detection.hpp:12-25 */
} gv_bbox;

/* LShapePose  include/grid_vision/cloud_detections.hpp:19-25 (80 bytes):
 * geometry_msgs/Pose (position xyz, orientation xyzw) + length, width, height */
typedef struct {
  double px, py, pz;
  double qx, qy, qz, qw;
  double length, width, height;
} gv_lshape_pose;

/* geometry_msgs/Transform as tf2_ros::Buffer::lookupTransform returns it
 * (src/grid_vision_node.cpp:290,348,371) */
typedef struct {
  double qx, qy, qz, qw;
  double tx, ty, tz;
} gv_transform;

/* CAMParams  include/grid_vision/vision_orientation.hpp:18-25 */
typedef struct {
  int32_t network_h, network_w, orig_h, orig_w;
  float fx, fy, cx, cy;
} gv_cam_params;

/* nav_msgs/OccupancyGrid.info as GridMapRosConverter::toOccupancyGrid fills it */
typedef struct {
  uint32_t width, height;     /* size(0), size(1) */
  double resolution;
  double origin_x, origin_y;  /* position - length/2 */
} gv_grid_info;

/* ------------------------------------------------------------ lifecycle -- */
/* Replaces OccupancyGridMap::OccupancyGridMap(base_link, uint8_t grid_x,
 * uint8_t grid_y, double resolution)  include/grid_vision/occupancy_grid.hpp:16,
 * src/occupancy_grid.cpp:4-14, plus object_detection::setIntrinsicMatrix /
 * computeKInverse (src/object_detection.cpp:241-249) from cam.  device_id < 0
 * picks the current device.  The call also makes sure the handle's upload stream has a hardware queue of its own
 * (a process gets four; profiles/r03/h2d_notes.md 6): three 150 us idle kernels + a timed 4-byte memset, only the
 * handle's own streams are waited for; 0.3-1 ms per handle, GV_QUEUE_PROBE=0 in the environment skips it. */
int gv_create(gv_handle *out, uint8_t grid_x, uint8_t grid_y, double resolution,
              const gv_cam_params *cam, int device_id);
int gv_destroy(gv_handle h);
/* text of the last HIP/RCCL failure on this handle ("" if none) */
const char *gv_last_error(gv_handle h);
/* ABI version of the library (this header: 4) */
int gv_abi_version(void);
/* geometry read-back: nx, ny, pos_x, pos_y (grid_map size / position) */
int gv_grid_geometry(gv_handle h, int32_t *nx, int32_t *ny, double *pos_x, double *pos_y);
/* Reset both layers to the constructor state (log_odds 0.0, occupancy 0.5). */
int gv_reset(gv_handle h);

/* Replaces the three tf lookups of the node: camera<-lidar
 * (grid_vision_node.cpp:290), base<-camera (:348,:371) and, [EXTENSION] for X1/X2,
 * base<-lidar.  A NULL pointer leaves that transform unset; calls that need it
 * then return GV_ERR_TF. */
int gv_set_transforms(gv_handle h, const gv_transform *camera_from_lidar,
                      const gv_transform *base_from_camera, const gv_transform *base_from_lidar);

/* ---------------------------------------------------------------- cloud -- */
/* Replaces GridVision::cloudCallback's pcl::fromROSMsg (grid_vision_node.cpp:103-106)
 * for a caller that already holds SoA x/y/z (fp32, lidar frame).  The cloud
 * stays resident in HBM until the next upload. */
int gv_cloud_upload_xyz(gv_handle h, const float *x, const float *y, const float *z, size_t n);
/* Same, from sensor_msgs/PointCloud2 bytes: n points of point_step bytes with
 * fp32 fields at off_x/off_y/off_z; de-interleaved on the device. */
int gv_cloud_upload_pointcloud2(gv_handle h, const uint8_t *data, size_t n, uint32_t point_step,
                                uint32_t off_x, uint32_t off_y, uint32_t off_z);
/* Streaming ingest: the node receives a new cloud (cloudCallback, grid_vision_node.cpp:103-106)
 * while the previous frame is still being processed (timerCallback, :108-244).  The handle
 * keeps THREE resident clouds in rotation: the *_async calls enqueue the host-to-device copy of the next one
 * on a copy stream, ordered after the last frame that reads the buffer being replaced, and return
 * at once; frames enqueued afterwards use the new cloud (stream-ordered, no host wait).  The copy
 * is truly asynchronous when the host buffers are pinned (gv_host_alloc); pageable buffers work
 * too (the HIP runtime then stages them before returning).  The host buffers must stay unchanged
 * until gv_cloud_upload_wait (or gv_synchronize) returns.  The synchronous gv_cloud_upload_*
 * calls above are the same upload followed by that wait; neither kind drains the frame pipeline. */
int gv_cloud_upload_xyz_async(gv_handle h, const float *x, const float *y, const float *z, size_t n);
int gv_cloud_upload_pointcloud2_async(gv_handle h, const uint8_t *data, size_t n, uint32_t point_step,
                                      uint32_t off_x, uint32_t off_y, uint32_t off_z);
/* wait until every upload enqueued so far has left the host buffers (the clouds' own completion events: frames
 * that run on the upload stream -- the third lane -- are not waited for) */
int gv_cloud_upload_wait(gv_handle h);
/* page-locked host memory for the *_async uploads (hipHostMalloc / hipHostFree) */
int gv_host_alloc(void **ptr, size_t bytes);
int gv_host_free(void *ptr);
/* Replaces GridVision::transformLidarToCamera (grid_vision_node.cpp:280-307,
 * include/grid_vision/grid_vision_node.hpp:95-97): camera-frame copy of the
 * resident cloud written to caller SoA buffers (each n floats). */
int gv_transform_lidar_to_camera(gv_handle h, float *x_cam, float *y_cam, float *z_cam);

/* ------------------------------------------------------ cloud_detections -- */
/* Replaces cloud_detections::extractCloudPerBBox (cloud_detections.hpp:46-48,
 * src/cloud_detections.cpp:250-298) on the resident cloud: bbox_id[i] is the
 * index of the first bbox containing the projection of point i, or -1.
 * counts (optional, nb ints) receives the per-bbox point counts. */
int gv_extract_cloud_per_bbox(gv_handle h, const gv_bbox *bboxes, int32_t nb,
                              int32_t *bbox_id, int32_t *counts);
/* Replaces cloud_detections::buildKDTree + computeDepthForBoundingBoxes
 * (cloud_detections.hpp:29-35, src/cloud_detections.cpp:8-87): exact k nearest
 * projected points of each bbox centre in (u,v,depth), upper median depth;
 * depths[i] = -1 when no point qualifies.  knn_d2 (optional, nb*k) receives the
 * sorted squared distances.  1 <= k <= 32. */
int gv_compute_depth_for_bboxes(gv_handle h, const gv_bbox *bboxes, int32_t nb, int32_t k,
                                float *depths, float *knn_d2);
/* Replaces GridVision::convertPixelsTo3D -> cloud_detections::pixelTo3D ->
 * transformPointToBaseFrame (grid_vision_node.cpp:309-359,
 * src/cloud_detections.cpp:89-103): base-frame points, 3 doubles per bbox. */
int gv_convert_pixels_to_3d(gv_handle h, const gv_bbox *bboxes, const float *depths, int32_t nb,
                            double *base_points_xyz);
/* Replaces cloud_detections::computeBBoxPose without the RANSAC ground removal
 * (cloud_detections.hpp:50-52, src/cloud_detections.cpp:140-247,300-321; see
 * DESIGN.md): extractCloudPerBBox + RadiusOutlierRemoval(0.4, 10) + centroid +
 * PCA rectangle per bbox.  poses_out holds nb entries; valid[i] = 0 where the
 * reference would have skipped the bbox (empty cloud, :174-175). */
int gv_compute_bbox_pose(gv_handle h, const gv_bbox *bboxes, int32_t nb,
                         gv_lshape_pose *poses_out, uint8_t *valid);

/* Replaces cloud_detections::segmentGroundPlane (cloud_detections.hpp:40-41,
 * src/cloud_detections.cpp:105-138: pcl SACSegmentation, plane, RANSAC, threshold 0.04,
 * optimised coefficients) on the camera-frame view of the resident cloud.  PCL's sample
 * sequence cannot be reproduced, so this is specified BY OUTCOME:
 * `iterations` hypotheses from a counter-based RNG (seed), inliers |n.p+d| < threshold
 * counted on the device, least-squares refinement, inliers re-selected.  is_ground
 * (optional, n bytes) marks the plane's points; *n_inliers == 0 means "could not
 * estimate a planar model" (the reference then returns an empty cloud, :122-126). */
int gv_segment_ground_plane(gv_handle h, double threshold, int32_t iterations, uint64_t seed,
                            uint8_t *is_ground, float coeff[4], int64_t *n_inliers);
/* Replaces cloud_detections::computeBBoxPose in full (src/cloud_detections.cpp:300-321):
 * segmentGroundPlane(0.04, 50 iterations) -> extractCloudPerBBox -> bboxPoseEstimation.
 * *n_poses = number of valid poses, or -1 where the reference returns {} (empty segmented cloud). */
int gv_compute_bbox_pose_ground_removed(gv_handle h, const gv_bbox *bboxes, int32_t nb,
                                        gv_lshape_pose *poses_out, uint8_t *valid, int32_t *n_poses);

/* ---------------------------------------------------- vision_orientation -- */
/* Replaces VisionOrientation::postProcessOutputs (+ computeAlpha,
 * computeThetaRay, calcLocation; vision_orientation.hpp:90-98,
 * src/vision_orientation.cpp:241-519) on precomputed network outputs
 * orient[nb*4], conf[nb*2], dims[nb*3].  Writes *n_out <= nb camera-frame poses
 * (unknown classes are skipped, :496-499). */
int gv_vision_post_process(gv_handle h, const float *orient, const float *conf, const float *dims,
                           const gv_bbox *bboxes, int32_t nb, gv_lshape_pose *poses_out,
                           int32_t *n_out);
/* Replaces GridVision::transformLShapeObjects (grid_vision_node.cpp:525-531,
 * :361-382): pose camera -> base, in place. */
int gv_transform_lshape_objects(gv_handle h, gv_lshape_pose *poses, int32_t n);

/* ------------------------------------------------------ object_detection -- */
/* Host-side post-processing on precomputed detector outputs; no GPU work.
 * Replaces object_detection::extract_bboxes (object_detection.hpp:48-49,
 * src/object_detection.cpp:94-146) incl. fast_non_max_suppression (:166-211),
 * denormalizeAndScaleBoundingBox (:226-239), getObjectClass (:252-269).
 * boxes[n*4], scores[n*c]; out must hold n entries; returns count in *n_out. */
int gv_extract_bboxes(const float *boxes, const float *scores, int32_t n, int32_t c,
                      double conf_threshold, double iou_threshold, int32_t orig_w, int32_t orig_h,
                      int32_t resize, gv_bbox *out, int32_t *n_out);
/* Replaces GridVision::filterBBoxes (grid_vision_node.cpp:384-403). */
int gv_filter_bboxes(const gv_bbox *in, int32_t n, gv_bbox *static_out, int32_t *n_static,
                     gv_bbox *dynamic_out, int32_t *n_dynamic);
/* Replaces setIntrinsicMatrix / computeKInverse (src/object_detection.cpp:241-249):
 * row-major 3x3 K and K^-1 of the handle. */
int gv_get_intrinsics(gv_handle h, double K[9], double K_inv[9]);

/* -------------------------------------------------------- occupancy grid -- */
/* Replaces OccupancyGridMap::updateMap(GridMap&)  occupancy_grid.hpp:20,
 * src/occupancy_grid.cpp:16-31 */
int gv_update_map(gv_handle h);
/* Replaces OccupancyGridMap::updateMap(GridMap&, vector<LShapePose>)
 * occupancy_grid.hpp:19, src/occupancy_grid.cpp:65-105,140-183 (poses in the
 * base frame) */
int gv_update_map_poses(gv_handle h, const gv_lshape_pose *poses, int32_t n);
/* Replaces OccupancyGridMap::updateMap(GridMap&, vector<Point>, vector<BoundingBox>)
 * occupancy_grid.hpp:17-18, src/occupancy_grid.cpp:33-63,107-138,185-196
 * (never called by the node; kept for the class surface) */
int gv_update_map_points(gv_handle h, const double *base_points_xyz, const gv_bbox *bboxes,
                         int32_t n);
/* Replaces GridVision::publishOccupancyGrid's
 * GridMapRosConverter::toOccupancyGrid(map,"occupancy",0,1,msg)
 * (grid_vision_node.cpp:265-278): data[G] int8 in OccupancyGrid order. */
int gv_to_occupancy_grid(gv_handle h, int8_t *data, gv_grid_info *info);
/* The same without stalling the frame pipeline: an asynchronous device-to-host copy of data[G] on
 * gv_stream(h), behind the grid pass of the last enqueued frame and ahead of the next one's.  data
 * should be pinned (gv_host_alloc); it is complete once an event recorded on gv_stream(h) after this
 * call has passed, or after gv_synchronize. */
int gv_to_occupancy_grid_async(gv_handle h, int8_t *data);
/* The same for a node that publishes the grid EVERY tick while clouds stream in (the reference does:
 * grid_vision_node.cpp:240, :265-278).  data must be pinned (gv_host_alloc): the grid is then written there by a small
 * kernel on gv_stream(h) instead of a copy command, so the copy engines stay with the cloud uploads and PCIe carries
 * both directions at once -- 262 us per frame, steady, against 292-349 us and erratic for the copy command beside an
 * upload (profiles/r04/publish_variants.txt).  Pageable memory, or a destination that is not 16-byte aligned, falls back to the
 * copy command.  Same completion rule as
 * gv_to_occupancy_grid_async. */
int gv_publish_grid_async(gv_handle h, int8_t *data);
/* Layer read-back (grid_map_["log_odds"], ["occupancy"]; occupancy_grid.hpp:22) */
int gv_get_log_odds(gv_handle h, float *out);
int gv_get_occupancy(gv_handle h, float *out);
/* Layer write (tests / checkpoint restore): G floats */
int gv_set_log_odds(gv_handle h, const float *in);

/* ------------------------------------------------ [EXTENSION] ego motion -- */
/* The reference keeps its grid fixed in base_link (src/occupancy_grid.cpp:4-14): nothing moves it when the vehicle
 * moves.  gv_grid_move is grid_map's GridMap::move() for that grid: it resamples the three layers (log_odds,
 * occupancy, the packed int8) so that they stay registered to the current base frame.
 *
 * motion = pose of the current base frame in the previous one (base_prev <- base_now), i.e. what
 * tf2 lookupTransform(base, t_prev, base, t_now, odom) returns.  Planar: only the yaw of the normalised quaternion,
 * atan2(2(qw qz + qx qy), 1 - 2(qy^2 + qz^2)), and tx, ty are used; z, roll and pitch are ignored.
 * The handle keeps an fp64 SE(2) residue E (the current base frame in the frame the layers are registered in; the
 * identity after gv_create, gv_reset and gv_set_log_odds).  Each call composes E <- E o motion and picks the resample
 * S: its rotation is E's where that moves a map corner by at least half a cell (|yaw| * r_max >= res/2, r_max the
 * largest distance from the base origin to a corner), 0 otherwise; its translation is E's rounded to whole cells.
 * E <- S^-1 o E keeps what is left, so sub-cell motion adds up over calls instead of being rounded away.
 * New cell (ix, iy) takes, bit for bit, all three layers of the old cell that contains S applied to its centre;
 * cells whose source lies off the map get the constructor state (0.0, 0.5, 50).  No new float value is created.
 * Asynchronous: the resample is enqueued on gv_stream(h) (nothing when S is the identity) and the call returns
 * without a host wait; it executes between the grid passes of the frames enqueued before and after it.  Allowed
 * between gv_tick_enqueue and gv_tick_wait (the tick's grid_out still receives the grid before the move).
 * gv_device_layers keeps returning the same pointers.  GV_ERR_BAD_ARG for a null handle or motion or a non-finite
 * field; GV_ERR_STATE with a communicator of more than one rank (ranks own row bands, a rotation crosses them). */
typedef struct {
  int32_t applied;              /* 1 = the layers were resampled, 0 = motion kept as residue only */
  double cos_yaw, sin_yaw;      /* rotation of the applied resample S (1, 0 when none)            */
  double tx, ty;                /* translation of S in metres: whole multiples of resolution       */
  double res_yaw, res_x, res_y; /* residue carried to the next call                                */
} gv_grid_move_info;
/* info may be NULL */
int gv_grid_move(gv_handle h, const gv_transform *motion, gv_grid_move_info *info);

/* ------------------------------------------------ [EXTENSION] height band -- */
/* The lidar map update (X1/X2: gv_frame_*, gv_tick with GV_TICK_LIDAR_BIN) counts every finite point as an obstacle.
 * The band classifies each point by its fp32 base-frame z (base<-lidar, the same transform and operation order as its
 * cell index), compared in fp32 exactly as written below, so z == z_ground and z == z_max are obstacles:
 *   z_ground <= z <= z_max   obstacle: a hit in map, a clipped ray end out of map (as without the band);
 *   z <  z_ground            ground return: with ground_clears, the end of a free-space ray that includes its own cell
 *                            (in map) or the clipped end on the border (out of map), never a hit; without, ignored;
 *   z >  z_max               ignored (overhangs, tree tops).
 * cell_idx stays the geometric cell of every point; bbox_id and the camera-side calls ignore the band.  gv_get_hits
 * counts the obstacles; gv_get_miss and gv_get_ray_stats describe the ends that were marched.
 * Handle configuration like the transforms: kept through gv_reset, gv_set_log_odds and gv_grid_move, applied to the
 * frames and ticks enqueued after the call (those in flight keep theirs); allowed between gv_tick_enqueue and
 * gv_tick_wait.  {-inf, +inf, any} gives the same bytes as the band off.  GV_ERR_BAD_ARG (band unchanged) for a null
 * handle, a NaN threshold, z_ground > z_max or ground_clears not in {0, 1}; +-inf are allowed. */
typedef struct {
  float z_ground;          /* base-frame z: a point with z <  z_ground is a ground return          */
  float z_max;             /* base-frame z: a point with z >  z_max    is above the band (ignored)  */
  int32_t ground_clears;   /* 1: a ground return ends a free-space ray that includes its own cell  */
                           /* 0: a ground return is ignored like a point above the band            */
} gv_height_band;
/* NULL turns the band off (the state after gv_create). */
int gv_set_height_band(gv_handle h, const gv_height_band *band);

/* --------------------------------------- [EXTENSION] inflated costmap layer -- */
/* X6.  What a planner reads is not the grid but the costmap made from it: every cell's distance to the nearest
 * obstacle and the inflation cost derived from that distance (nav2's InflationLayer).  gv_inflate computes both on
 * the device from the packed int8 layer.  The reference has no such step; this text is its definition.
 *
 * Lethal cells.  A cell is lethal iff its packed int8 value v (what gv_to_occupancy_grid returns) satisfies
 *   v >= lethal_threshold, compared signed: the -1 of a NaN occupancy is never lethal.  There is no "unknown"
 *   class; the never-observed prior, 50, is lethal or not by the threshold alone.
 * Distance.  d2(c) is the smallest dx^2 + dy^2, in whole cells and as an exact integer, from cell c to a lethal cell
 *   of the same map: the exact Euclidean distance transform, not nav2's wavefront approximation.  Cells off the map
 *   are not obstacles, nothing wraps from the end of one row into the next, and the search is bounded by d2max
 *   (below): a cell with no lethal cell within d2max has no distance and reads 65535 in the uint16 layer.
 * Cost table.  cost[q] for q = 0 .. d2max is built once on the host in fp64 with
 *   dist = sqrt((double)q) * resolution (one correctly rounded sqrt, one multiply):
 *     q == 0                     254 (lethal)
 *     dist <= inscribed_radius   253
 *     dist >  inflation_radius   0
 *     otherwise                  (uint8_t)(252.0 * exp(-cost_scaling_factor * (dist - inscribed_radius))), truncated
 *   (nav2_costmap_2d::InflationLayer::computeCost).  d2max is the largest q with
 *   sqrt((double)q) * resolution <= inflation_radius, and Rc = isqrt(d2max) <= 63 is required (d2 then fits 16 bits
 *   and a row's search window three 64-bit words).  A cell without a distance costs 0.
 *   With GV_INFLATE_OCCUPANCY_SCALE every table entry c goes through the translation Costmap2DPublisher applies
 *   before it publishes a costmap as an OccupancyGrid: 0 -> 0, 253 -> 99, 254 -> 100, otherwise
 *   1 + (97 * (c - 1)) / 251 in integer arithmetic.  The same kernel runs with that table.
 * Output layers.  cost[G] uint8 and, with GV_INFLATE_KEEP_DIST2, dist2[G] uint16, both in OccupancyGrid.data order
 *   (the order of gv_to_occupancy_grid), so the costmap publishes beside the grid with the same gv_grid_info.
 *
 * gv_set_inflation is handle configuration like the height band: no device work, kept through gv_reset,
 * gv_set_log_odds and gv_grid_move, applied to the gv_inflate calls after it (one already enqueued keeps the table it
 * was enqueued with); NULL turns it off (the state after gv_create).  GV_ERR_BAD_ARG, configuration unchanged, for a
 * null handle, a NaN or infinite field, a negative radius or factor, inflation_radius < inscribed_radius, a threshold
 * outside 1..100, unknown flag bits, or Rc > 63.
 * gv_inflate enqueues the pass on gv_stream(h) without a host wait (the allocations of the first call aside): it reads
 * the packed layer as the grid pass of the last enqueued frame or tick left it and is ordered ahead of the next one,
 * like gv_publish_grid_async and gv_grid_move; allowed between gv_tick_enqueue and gv_tick_wait, where it inflates the
 * tick's grid.  GV_ERR_STATE when no inflation is set and with a communicator of more than one rank (ranks own row
 * bands, the stencil crosses them).  The costmap is a snapshot of the grid at the call: a later frame, move or
 * gv_set_log_odds does not change it, gv_reset invalidates it.
 * gv_get_costmap (G bytes) and gv_get_obstacle_dist2 (G values) are synchronous read-backs like gv_get_log_odds;
 * GV_ERR_STATE before the first gv_inflate since gv_create or gv_reset, gv_get_obstacle_dist2 also when the last
 * gv_inflate ran without GV_INFLATE_KEEP_DIST2.  gv_publish_costmap_async follows gv_publish_grid_async's rules.
 * gv_inflation_cost_table is host only and takes no handle: the table a configuration gives at a resolution
 * (positive, finite), *n = d2max + 1 entries; GV_ERR_BAD_ARG for an invalid configuration, a null table or cap < *n
 * (*n is set whenever the configuration is valid). */
enum {
  GV_INFLATE_KEEP_DIST2      = 1 << 0,   /* keep the uint16 squared-distance layer         */
  GV_INFLATE_OCCUPANCY_SCALE = 1 << 1    /* costs translated to the 0..100 OccupancyGrid scale */
};
typedef struct {
  double inscribed_radius;      /* m, finite, >= 0                                   */
  double inflation_radius;      /* m, finite, >= inscribed_radius, Rc <= 63          */
  double cost_scaling_factor;   /* 1/m, finite, >= 0                                 */
  int32_t lethal_threshold;     /* 1..100                                            */
  int32_t flags;                /* GV_INFLATE_KEEP_DIST2 | GV_INFLATE_OCCUPANCY_SCALE */
} gv_inflation;
int gv_inflation_cost_table(const gv_inflation *cfg, double resolution, uint8_t *table, int32_t cap, int32_t *n);
int gv_set_inflation(gv_handle h, const gv_inflation *cfg);
int gv_inflate(gv_handle h);
int gv_get_costmap(gv_handle h, uint8_t *out);
int gv_get_obstacle_dist2(gv_handle h, uint16_t *out);
int gv_publish_costmap_async(gv_handle h, uint8_t *data);

/* ------------------------------------ [EXTENSION] trajectory scoring (planner) -- */
/* X7.  A sampling controller (MPPI, DWB) tests thousands of candidate trajectories of some tens of poses per control
 * cycle against the costmap.  gv_score_trajectories does that on the device against the resident costmap of the last
 * gv_inflate: K trajectories of P poses go in, K records of 16 bytes come out, the costmap never leaves the device.
 * The reference has no such step; this text is its definition, modelled on nav2's
 * FootprintCollisionChecker::footprintCost / lineCost.
 *
 * Footprint.  n_vertices == 0 is the circular robot: a pose costs what its centre cell costs (nav2 with
 *   consider_footprint: false), and its yaw is never read.  Otherwise 3..16 vertices (vx[i], vy[i]) in metres in the
 *   robot frame, x forward, all finite; the polygon is closed from the last vertex to the first.
 * Pose.  Three float32 (x, y, yaw) in the grid's frame (base_link at the last map update); poses[K][P][3],
 *   trajectory-major.
 * Vertices in the world.  c = cos((double)yaw), s = sin((double)yaw) in fp64 and, every operation one fp64 operation in
 *   this order, never contracted:
 *     wx = (double)x + (c * vx[i] - s * vy[i])
 *     wy = (double)y + (s * vx[i] + c * vy[i])
 * Cells.  getIndex -- the grid's own (position - 0.5 * length convention, exact division at cell borders, the one every
 *   map update uses) -- is applied to the centre ((double)x, (double)y) and to every vertex and gives grid_map cells
 *   (ix, iy).  The cost of cell (ix, iy) is cost[G - 1 - (iy * nx + ix)]: the costmap is in OccupancyGrid.data order.
 * Outline.  Edge i runs from the cell of vertex i to the cell of vertex (i + 1) % n.  Its cells are those of
 *   grid_map::LineIterator(cell_i, cell_i+1), both ends included: with ddx = |dx|, ddy = |dy| the major axis is x when
 *   ddx >= ddy and steps every cell, major + 1 cells in all; num = major / 2 at the start, num += minor after every
 *   cell, and the minor axis steps (num -= major) when num >= major.  Because of the truncated major / 2 and the tie
 *   at ddx == ddy THE DIRECTION OF AN EDGE MATTERS: the cells from a to b are not always those from b to a, so the
 *   order of the vertices is part of the footprint.  Only the outline is tested, as nav2 does; a lethal cell strictly
 *   inside the polygon does not count.
 * Pose cost.  If the centre or any vertex is off the map (getIndex's own test; a NaN or infinite coordinate fails it,
 *   and so does every vertex of a pose with a NaN or infinite yaw) the pose cost is off_map_cost.  Otherwise it is the
 *   maximum of the centre cell's cost and the cost of every outline cell.
 * Per trajectory (gv_traj_score):
 *   max_cost         the maximum pose cost;
 *   first_collision  the smallest pose index whose cost is >= collision_cost, -1 when none is;
 *   cost_sum         the sum over the poses of the centre cell's cost, off_map_cost for an off-map pose (what DWB's
 *                    BaseObstacle and MPPI's cost critic add up);
 *   n_off_map        the number of off-map poses.
 *   All four are maxima, minima and integer sums: the result does not depend on how the work is scheduled.
 * With GV_TRAJ_KEEP_POSE_COST, pose_cost[K * P] (uint8) also receives every pose cost.
 *
 * gv_set_footprint is handle configuration like gv_set_inflation: no device work, kept through gv_reset,
 * gv_set_log_odds and gv_grid_move; NULL turns it off (the state after gv_create).  Every scoring call carries the
 * footprint in force when it is enqueued; a later gv_set_footprint does not reach it.  GV_ERR_BAD_ARG, configuration
 * unchanged, for a null handle, n_vertices of 1, 2 or more than 16 (or negative), a non-finite vertex among the first
 * n_vertices, collision_cost outside 1..255, off_map_cost outside 0..255, or flags other than 0.
 * gv_score_trajectories_async enqueues the scoring on gv_stream(h) without a host wait (the allocations of a first or
 * larger call aside); it reads the costmap as the last enqueued gv_inflate left it and is ordered like gv_inflate
 * itself: behind everything enqueued before it, ahead of what follows; allowed between gv_tick_enqueue and
 * gv_tick_wait.  poses is host memory, copied on the public stream (it must stay unchanged until completion; pinned
 * memory, gv_host_alloc, makes the copy truly asynchronous); with GV_TRAJ_DEVICE_POSES it is device memory that the
 * kernel reads in place, and the caller orders its producer before gv_stream(h).  scores -- and pose_cost, required
 * with GV_TRAJ_KEEP_POSE_COST and ignored without -- follow gv_publish_grid_async's rules: pinned memory (scores
 * 16-byte aligned) is written by the kernel without a copy command, anything else through a copy command; either is
 * complete once an event recorded on gv_stream(h) after the call has passed, or after gv_synchronize.
 * K == 0 is a successful no-op (once the arguments and the state below have passed).  GV_ERR_BAD_ARG for a null
 * handle, null poses or scores, P outside 1..4096, K < 0 or K > 2^20, unknown flags, or GV_TRAJ_KEEP_POSE_COST with a
 * null pose_cost.  GV_ERR_STATE when no footprint is set,
 * when no gv_inflate has run since gv_create / gv_reset, and with a communicator of more than one rank.
 * gv_score_trajectories is the same call followed by the wait for it.
 * gv_footprint_cells is host only and takes no handle: the cells one pose tests on the grid gv_create(grid_x, grid_y,
 * resolution) makes, with the library's own geometry code -- cells[0] the centre, then the outline edge by edge (an
 * edge's cells in line order, shared vertex cells repeated), each as iy * nx + ix; *n receives their number, also
 * when that exceeds cap (then GV_ERR_BAD_ARG, nothing written), and -1 for an off-map pose (GV_OK).  GV_ERR_BAD_ARG
 * for an invalid footprint or geometry or a null n. */
enum {
  GV_TRAJ_KEEP_POSE_COST = 1 << 0,   /* write pose_cost[K * P]                    */
  GV_TRAJ_DEVICE_POSES   = 1 << 1    /* poses is device memory, read in place     */
};
typedef struct {
  int32_t n_vertices;         /* 0 (centre cell only) or 3..16                              */
  double vx[16], vy[16];      /* m, robot frame, x forward; the first n_vertices are read    */
  int32_t collision_cost;     /* 1..255: a pose collides when its cost is >= this            */
  int32_t off_map_cost;       /* 0..255: the cost of a pose that leaves the map              */
  uint32_t flags;             /* 0                                                           */
} gv_footprint;
typedef struct {
  int32_t max_cost;
  int32_t first_collision;
  uint32_t cost_sum;
  int32_t n_off_map;
} gv_traj_score;
int gv_set_footprint(gv_handle h, const gv_footprint *fp);
int gv_score_trajectories_async(gv_handle h, const float *poses, int32_t K, int32_t P, uint32_t flags,
                                gv_traj_score *scores, uint8_t *pose_cost);
int gv_score_trajectories(gv_handle h, const float *poses, int32_t K, int32_t P, uint32_t flags,
                          gv_traj_score *scores, uint8_t *pose_cost);
int gv_footprint_cells(uint8_t grid_x, uint8_t grid_y, double resolution, const gv_footprint *fp, float x, float y,
                       float yaw, int32_t *cells, int32_t cap, int32_t *n);

/* --------------------------------- [EXTENSION] goal / path distance field (planner) -- */
/* X9.  A controller ranks its candidates by the obstacle cost (X7) plus a goal-directed term: DWB's GoalDist and
 * PathDist critics, the obstacle heuristic of Smac and MPPI.  That term is a shortest-path distance field over the
 * costmap.  gv_nav_field computes it on the device from goal or path seeds over the resident costmap of the last
 * gv_inflate, and gv_score_nav samples it along the poses[K][P][3] that gv_score_trajectories scores; the costmap never
 * leaves the device.  The reference has no such step; this text is its definition, modelled on nav2's
 * dwb_critics::MapGridCritic (propogateManhattanDistances, GoalDistCritic, PathDistCritic).  One addition, the cost
 * weight, makes the same field a clearance-aware heuristic.
 *
 * Configuration (gv_nav_config).  step[v], for a cost byte v = 0..255, is 0 (blocked) for v >= obstacle_cost and
 *   1 + cost_weight * v otherwise; cost_weight = 0 gives MapGridCritic's hop count.  gv_set_nav_config is handle
 *   configuration like gv_set_footprint: no device work, kept through gv_reset, gv_set_log_odds and gv_grid_move; NULL
 *   turns it off (the state after gv_create).  GV_ERR_BAD_ARG, configuration unchanged, for a null handle,
 *   obstacle_cost outside 1..255, cost_weight outside 0..255, flags other than 0, or
 *     (1 + cost_weight * (obstacle_cost - 1)) * (G - 1) > 0xFFFFFFFD
 *   (G = nx * ny cells): every distance then fits 32 bits below the two sentinels.  On a 2000 x 2000 grid with
 *   obstacle_cost = 253 that allows the weights 0..4.
 *   gv_nav_step_table is host only and takes no handle, like gv_inflation_cost_table: table[v] = step[v];
 *   GV_ERR_BAD_ARG for a null pointer, a field out of range or flags other than 0.
 * Field.  field[G] is uint32 in OccupancyGrid.data order, like the costmap: cell (ix, iy) is field[G - 1 - (iy * nx + ix)],
 *   and the neighbours of entry y * nx + x are x - 1 and x + 1 of the same row y and the same x of the rows y - 1 and
 *   y + 1 (4-connectivity is its own mirror image under the 180 degree turn between the two orders).
 *     a blocked cell (step[cost] == 0)         GV_NAV_BLOCKED
 *     a seed cell                              0
 *     any other traversable cell               the minimum, over 4-connected paths of traversable cells from any seed
 *                                              cell, of the sum of step[cost[c]] over the cells ENTERED: every cell of
 *                                              the path except its seed
 *     a traversable cell no such path reaches  GV_NAV_UNREACHABLE
 *   There are no diagonal moves, nothing wraps from the end of one row into the next, cells off the map do not exist.
 *   The value is an exact integer and unique: the result does not depend on how the work is scheduled.
 * Seeds.  seeds_xy[S][2], float32 in the grid's frame, S in 1..65536, host memory, copied before the call returns.
 *   Each goes through the grid's own getIndex on ((double)x, (double)y), exactly as gv_score_trajectories treats a pose
 *   centre.  A seed off the map, non-finite or on a blocked cell is skipped (PathDistCritic skips such path poses
 *   too).  No usable seed is not an error: the field is then GV_NAV_BLOCKED or GV_NAV_UNREACHABLE everywhere.
 *
 * gv_nav_field reads the costmap as the last enqueued gv_inflate left it, with the configuration in force, and is
 * ordered on gv_stream(h) behind everything enqueued before it.  UNLIKE ITS NEIGHBOURS IT WAITS ON THE HOST: it returns
 * when the field is complete on the device.  The solver relaxes the field in rounds until a round changes nothing, and
 * how many rounds that takes depends on the map (convergence is data dependent), so the host has to see the rounds'
 * counters before it knows whether to enqueue more.  The field is a snapshot: a later gv_inflate, frame, move or
 * configuration change does not change it, gv_reset invalidates it.  Allowed between gv_tick_enqueue and
 * gv_tick_wait, where it waits for the tick's device work first.  info, when not NULL, receives n_seeds_used and the
 * number of relaxation rounds run (a diagnostic that depends on scheduling).  GV_ERR_BAD_ARG for a null handle or
 * seeds_xy or S outside 1..65536; GV_ERR_STATE when no configuration is set, when no gv_inflate has run since
 * gv_create / gv_reset, and with a communicator of more than one rank (ranks own row bands of the grid).
 * gv_get_nav_field (G values) is a synchronous read-back like gv_get_costmap; gv_device_nav_field gives the device
 * pointer of the same G values for device-side consumers, read-only, valid until gv_destroy.  Both return
 * GV_ERR_STATE before the first field since gv_create / gv_reset, GV_ERR_BAD_ARG for a null pointer.
 *
 * Sampling along trajectories (MapGridCritic::scoreTrajectory, all three of its aggregations at once).  A pose is
 *   GOOD when its centre ((double)x, (double)y) passes getIndex and the field at that cell is neither GV_NAV_BLOCKED
 *   nor GV_NAV_UNREACHABLE.  The yaw is never read.  Per trajectory (gv_nav_score, 24 bytes):
 *     sum        the sum of the field at the centre cell over the good poses;
 *     last       the field value of pose P - 1, GV_NAV_BLOCKED / GV_NAV_UNREACHABLE kept, GV_NAV_BLOCKED off the map;
 *     best       the smallest value over the good poses, GV_NAV_UNREACHABLE when there is none;
 *     best_pose  the smallest pose index that attains best, -1 when there is none;
 *     n_bad      the number of poses that are not good.
 *   Integer sums, minima and counts only: no order shows in the record.
 * gv_score_nav_async follows gv_score_trajectories_async in everything but the record: the pose layout and limits
 * (P in 1..4096, K in 0..2^20), GV_TRAJ_DEVICE_POSES, the ordering on gv_stream(h), and the destination rules -- pinned
 * scores aligned to 8 bytes are written by the kernel, anything else goes through a copy command.  It reads the field
 * of the last gv_nav_field.  K == 0 is a successful no-op.  GV_ERR_BAD_ARG for a null handle, poses or scores, P or K
 * out of range, or any flag other than GV_TRAJ_DEVICE_POSES (GV_TRAJ_KEEP_POSE_COST included); GV_ERR_STATE before the
 * first field and with a communicator of more than one rank.  gv_score_nav is the same call followed by the wait. */
#define GV_NAV_BLOCKED     0xFFFFFFFFu
#define GV_NAV_UNREACHABLE 0xFFFFFFFEu
typedef struct {
  int32_t obstacle_cost;   /* 1..255: a cell whose cost is >= this is blocked */
  int32_t cost_weight;     /* 0..255: entering a traversable cell of cost v costs 1 + cost_weight * v */
  uint32_t flags;          /* 0 */
} gv_nav_config;
typedef struct {
  int32_t n_seeds_used;   /* seeds that named a traversable map cell (duplicates counted) */
  int32_t rounds;         /* relaxation rounds run (diagnostic: depends on scheduling, never compared) */
} gv_nav_info;
typedef struct {
  uint64_t sum;        /* sum of the field at the centre cell over the good poses */
  uint32_t last;       /* field value of pose P-1; GV_NAV_BLOCKED / _UNREACHABLE kept; GV_NAV_BLOCKED if off map */
  uint32_t best;       /* smallest value over the good poses; GV_NAV_UNREACHABLE when there is none */
  int32_t best_pose;   /* smallest pose index that attains best; -1 when there is none */
  int32_t n_bad;       /* poses off the map (getIndex's own test), on a blocked or on an unreachable cell */
} gv_nav_score;        /* 24 bytes */
int gv_nav_step_table(const gv_nav_config *cfg, uint32_t table[256]);
int gv_set_nav_config(gv_handle h, const gv_nav_config *cfg);
int gv_nav_field(gv_handle h, const float *seeds_xy, int32_t S, gv_nav_info *info /* may be NULL */);
int gv_get_nav_field(gv_handle h, uint32_t *out);            /* synchronous read-back, G values */
int gv_device_nav_field(gv_handle h, uint32_t **field);     /* for device-side consumers, read-only */
int gv_score_nav_async(gv_handle h, const float *poses, int32_t K, int32_t P, uint32_t flags, gv_nav_score *scores);
int gv_score_nav(gv_handle h, const float *poses, int32_t K, int32_t P, uint32_t flags, gv_nav_score *scores);

/* ----------------------------------- [EXTENSION] rollout and control step (planner) -- */
/* X10.  A sampling controller (DWB, MPPI) closes its loop in three steps: roll K control sequences out into K
 * trajectories of P poses, score them (X7, X9), pick the best.  gv_rollout does the first on the device and keeps the
 * poses there, where gv_score_trajectories* and gv_score_nav* read them with GV_TRAJ_DEVICE_POSES; gv_control_step does
 * the other two over the resident rollout and returns 16 bytes.  The reference has no such step; this text is its
 * definition, modelled on nav2's dwb_plugins::StandardTrajectoryGenerator and MPPI's integrateStateVelocities.
 *
 * Motion model (gv_motion_model).  GV_MOTION_DIFF takes the controls (v, w), C = 2 floats per step; GV_MOTION_OMNI takes
 *   (vx, vy, w), C = 3 floats per step; dt is the step in seconds.  gv_set_motion_model is handle configuration like
 *   gv_set_footprint: no device work, kept through gv_reset, gv_set_log_odds and gv_grid_move; NULL turns it off (the
 *   state after gv_create).  Every rollout carries the model in force when it is enqueued; a later gv_set_motion_model
 *   does not reach it.  GV_ERR_BAD_ARG, configuration unchanged, for a null handle, a model other than the two, dt not
 *   finite or not > 0, or flags other than 0.
 * Rollout.  The state (X, Y, T) is fp64 and starts at start[3] (doubles, all finite, else GV_ERR_BAD_ARG).  For step
 *   p = 0 .. P-1, with the control values widened from float32 to double, every operation one fp64 operation in exactly
 *   this order, never contracted:
 *     c = cos(T);  s = sin(T)                       -- the yaw BEFORE the step, as MPPI does
 *     DIFF:  d = v * dt;                 X = X + d * c;              Y = Y + d * s
 *     OMNI:  a = vx * dt;  b = vy * dt;  X = X + (a * c - b * s);    Y = Y + (a * s + b * c)
 *     T = T + w * dt
 *     pose[p] = ((float)X, (float)Y, (float)T)      -- round to nearest even; pose p is the state AFTER step p
 *   The yaw is not wrapped.  Non-finite controls are not errors: they propagate by IEEE rules, and the scorers treat
 *   such poses as off the map.  On the device cos and sin are the device library's fp64 sincos, on the host (
 *   gv_rollout_poses) the C library's; the two may differ in the last bit, which reaches a float32 pose only when the
 *   fp64 value lies within about 2^-44 (relative) of a rounding midpoint.  Everything else is the same on both sides.
 * Controls.  controls[K][P][C] float32, trajectory-major; with GV_ROLLOUT_CONSTANT controls[K][C], one control held for
 *   all P steps (DWB's generator).  Host memory, copied on the public stream under gv_score_trajectories_async's rules
 *   for host poses (unchanged until completion; pinned memory makes the copy truly asynchronous); with
 *   GV_ROLLOUT_DEVICE_CONTROLS device memory that the kernel reads in place, the caller ordering its producer before
 *   gv_stream(h): the door for a caller that samples its noise on the device.
 * Limits.  P in 1..4096 and K in 0..2^20 as for X7, and K * P <= 2^24 because the handle owns the pose buffer.  K == 0
 *   is a successful no-op that leaves the previous rollout in place (once the arguments and the state have passed).
 *   GV_ERR_BAD_ARG for a null handle, start or controls, a non-finite start, P, K or K * P out of range or unknown flags;
 *   GV_ERR_STATE without a motion model.
 * The rollout buffer.  poses[K][P][3] float32, the layout X7 and X9 read, in a buffer of the handle's own (not the
 *   staging copy of host poses, which every scoring call overwrites).  gv_rollout_async enqueues on gv_stream(h) without
 *   a host wait (the allocations of a first or larger call aside), ordered like every planner call: behind everything
 *   enqueued before it, ahead of what follows; allowed between gv_tick_enqueue and gv_tick_wait.  It does not depend on
 *   the map: gv_reset keeps it.  gv_rollout is the same call followed by the wait for it.
 *   gv_device_rollout gives the device pointer and the K and P of the last rollout (K, P may be NULL), read-only, for
 *   GV_TRAJ_DEVICE_POSES; the pointer stays valid until gv_destroy or a larger rollout -- IT MAY CHANGE WHEN THE BUFFER
 *   GROWS, so ask again after a rollout with a larger K * P.  gv_get_rollout is a synchronous read-back of K * P * 3
 *   floats.  Both return GV_ERR_STATE before the first rollout, GV_ERR_BAD_ARG for a null handle or pointer.
 *   gv_rollout_poses is host only and takes no handle: the same arithmetic text compiled for the host, with the C
 *   library's sin and cos.  Same limits; GV_ERR_BAD_ARG also for a null or invalid model, a null poses_out, or
 *   GV_ROLLOUT_DEVICE_CONTROLS.
 *
 * Control step.  Scores the resident rollout with X7 (the footprint in force) against the costmap of the last
 *   gv_inflate and, when a nav weight is set, with X9 against the field of the last gv_nav_field, then combines the two
 *   records of every trajectory and selects.  The records are integers: everything below is exact and does not depend
 *   on how the work is scheduled.
 *     nav_used = any of w_nav_last, w_nav_sum, w_nav_best is non-zero.
 *     Trajectory k is REJECTED iff traj[k].first_collision >= 0, or nav_used and nav[k].n_bad > 0.
 *     For an admitted trajectory, in uint64 arithmetic (max_cost taken as uint32),
 *       total = w_cost_sum * cost_sum + w_max_cost * max_cost
 *               (+ w_nav_last * last + w_nav_sum * sum + w_nav_best * best   when nav_used).
 *     With n_bad == 0, last and best are field values, so no sentinel is ever multiplied, and with every weight at most
 *     65535 and P <= 4096 the total stays below 2^61:
 *       65535 * (4096 * 255 + 255 + (4096 + 2) * 0xFFFFFFFD) = 1.1535e18 < 2^61.
 *     best = the smallest k that attains the smallest total among the admitted, n_valid = their number, best_total that
 *     total; best = -1 and best_total = UINT64_MAX when none is admitted.
 *     With GV_CONTROL_KEEP_TOTALS, totals[K] receives every total, UINT64_MAX for a rejected trajectory.
 *   gv_control_step_async enqueues three kernels on gv_stream(h) -- the two samplers, then the selection -- without a
 *   host wait, ordered and allowed like gv_score_trajectories_async.  The samplers' records stay on the device.
 *   result and totals follow gv_publish_grid_async's rules: pinned result aligned to 16 bytes and pinned totals aligned
 *   to 8 bytes are written by the kernel, anything else goes through a landing buffer and a copy command; either is
 *   complete once an event recorded on gv_stream(h) after the call has passed, or after gv_synchronize.
 *   gv_control_step is the same call followed by the wait.  GV_ERR_BAD_ARG for a null handle, weights or result, a
 *   weight above 65535, weight flags other than 0, flags other than GV_CONTROL_KEEP_TOTALS, or that flag with null
 *   totals (ignored without it).  GV_ERR_STATE without a footprint, without a rollout, without a costmap since
 *   gv_create / gv_reset, without a field when nav_used, and with a communicator of more than one rank.
 *   gv_control_select is host only and takes no handle: the same combine / select text over K caller records (K in
 *   0..2^20; nav may be NULL when no nav weight is set, GV_ERR_BAD_ARG when one is; totals may be NULL). */
enum {
  GV_MOTION_DIFF = 0,   /* controls (v, w):      C = 2 floats per step */
  GV_MOTION_OMNI = 1    /* controls (vx, vy, w): C = 3 floats per step */
};
typedef struct {
  int32_t model;    /* GV_MOTION_DIFF or GV_MOTION_OMNI */
  double dt;        /* s, finite, > 0                    */
  uint32_t flags;   /* 0                                 */
} gv_motion_model;
enum {
  GV_ROLLOUT_DEVICE_CONTROLS = 1 << 0,   /* controls is device memory, read in place       */
  GV_ROLLOUT_CONSTANT        = 1 << 1    /* controls[K][C]: one control for all P steps    */
};
typedef struct {
  uint32_t w_cost_sum, w_max_cost, w_nav_last, w_nav_sum, w_nav_best;   /* each 0..65535 */
  uint32_t flags;                                                       /* 0 */
} gv_critic_weights;
typedef struct {
  int32_t best;          /* the selected trajectory, -1 when none is admitted */
  int32_t n_valid;       /* admitted trajectories                             */
  uint64_t best_total;   /* its total, UINT64_MAX when none is admitted       */
} gv_control_result;     /* 16 bytes */
enum {
  GV_CONTROL_KEEP_TOTALS = 1 << 0   /* write totals[K] */
};
int gv_set_motion_model(gv_handle h, const gv_motion_model *m);
int gv_rollout_async(gv_handle h, const double start[3], const float *controls, int32_t K, int32_t P, uint32_t flags);
int gv_rollout(gv_handle h, const double start[3], const float *controls, int32_t K, int32_t P, uint32_t flags);
int gv_device_rollout(gv_handle h, float **poses, int32_t *K, int32_t *P);   /* read-only, for GV_TRAJ_DEVICE_POSES */
int gv_get_rollout(gv_handle h, float *poses_out);                           /* synchronous read-back, K*P*3 floats */
int gv_rollout_poses(const gv_motion_model *m, const double start[3], const float *controls, int32_t K, int32_t P,
                     uint32_t flags, float *poses_out);
int gv_control_step_async(gv_handle h, const gv_critic_weights *w, uint32_t flags, gv_control_result *result,
                          uint64_t *totals);
int gv_control_step(gv_handle h, const gv_critic_weights *w, uint32_t flags, gv_control_result *result, uint64_t *totals);
int gv_control_select(const gv_critic_weights *w, const gv_traj_score *traj, const gv_nav_score *nav, int32_t K,
                      gv_control_result *result, uint64_t *totals /* may be NULL */);

/* ------------------------------------- [EXTENSION] MPPI sampling and softmax update (planner) -- */
/* X11.  The two ends of an MPPI iteration that X10 left with the caller: sampling the K x P x C controls around a
 * nominal sequence, and the softmax average of them over the totals that becomes the next nominal sequence.  Both run on
 * the device over buffers of the handle's own, so one iteration takes a seed and 16 bytes in and gives P x C floats
 * back.  The reference has no such step; this text is its definition, modelled on nav2's mppi::Optimizer (coloured noise
 * is not part of it; X12 below adds the limits on the samples and the control-cost term).
 *
 * Configuration (gv_mppi_config).  sigma[c] the standard deviation of channel c, [u_min[c], u_max[c]] its clamp, lambda
 *   the temperature in units of a total.  gv_set_mppi is handle configuration like gv_set_footprint: no device work,
 *   kept through gv_reset, gv_set_log_odds and gv_grid_move; NULL turns it off (the state after gv_create); every call
 *   carries the configuration in force when it is enqueued.  GV_ERR_BAD_ARG, configuration unchanged, for a null handle,
 *   a sigma that is not finite or < 0, a NaN clamp or u_min > u_max (+-inf allowed), lambda not finite or not > 0, or
 *   flags other than 0.  gv_set_mppi checks all three channels, the host twins below the first C.
 * Nominal.  nominal[P][C] float32, C from the motion model in force (X10), in a buffer of the handle's own that remembers
 *   its P and C.  gv_mppi_set_nominal copies host values (all finite, P in 1..4096, else GV_ERR_BAD_ARG) and returns when
 *   the caller's array is free; GV_ERR_STATE without a motion model.  gv_get_mppi_nominal is a synchronous read-back of
 *   P * C floats (out may be NULL to ask for P alone; GV_ERR_STATE before the first gv_mppi_set_nominal).  A later
 *   sampling or cycle call under a model with another C returns GV_ERR_STATE.  The nominal does not depend on the map:
 *   gv_reset keeps it.
 * Sampling.  Per (k, p), every operation one fp64 operation in exactly this order, never contracted:
 *     r[0..3] = Philox4x32-10(counter = (k, p, iteration_lo, iteration_hi), key = (seed_lo, seed_hi))
 *                 -- the Random123 function: multipliers 0xD2511F53 and 0xCD9E8D57, key increments 0x9E3779B9 and
 *                    0xBB67AE85, ten rounds; one call serves one pose, no state is carried
 *     u_i = ((double)r[i] + 0.5) * 2^-32                       -- never 0 or 1
 *     R = sqrt(-2.0 * log(u_0));  A = 6.283185307179586 * u_1;  z_0 = R * cos(A);  z_1 = R * sin(A)
 *     z_2 = the cosine branch of the same text on (u_2, u_3)   -- OMNI only
 *     pn = p, with GV_MPPI_SHIFT pn = min(p + 1, P - 1)         -- sample around the nominal advanced by one step
 *     v = (double)nominal[pn][c]                     for k == 0: trajectory 0 is the nominal itself
 *     v = (double)nominal[pn][c] + sigma[c] * z_c    for k >= 1; DIFF reads z_0, z_1 for (v, w), OMNI z_0, z_1, z_2
 *     f = (float)v;  f = f < u_min[c] ? u_min[c] : f;  f = f > u_max[c] ? u_max[c] : f;  controls[k][p][c] = f
 *   On the device log, sin and cos are the device library's, in gv_mppi_sample_controls the C library's; the two may
 *   differ in the last bit, which reaches a float32 control only near a rounding midpoint, as for X10's sincos.
 *   gv_mppi_sample_async enqueues one kernel on gv_stream(h) that reads the resident nominal when it runs (behind an
 *   update enqueued before it) and writes controls[K][P][C], the layout gv_rollout reads with
 *   GV_ROLLOUT_DEVICE_CONTROLS, into a buffer of the handle's own.  Limits as for the rollout: K in 0..2^20,
 *   K * P <= 2^24, K == 0 a successful no-op.  GV_ERR_BAD_ARG for a null handle, K out of range or flags other than
 *   GV_MPPI_SHIFT; GV_ERR_STATE without a configuration, a motion model or a nominal, or when the model's C is not the
 *   nominal's.  gv_device_controls gives the device pointer and K, P, C of the last sampling (any of the three may be
 *   NULL); the pointer stays valid until gv_destroy or a larger sampling -- IT MAY CHANGE WHEN THE BUFFER GROWS, like
 *   gv_device_rollout's.  gv_get_controls is a synchronous read-back of K * P * C floats.  Both return GV_ERR_STATE
 *   before the first sampling.
 * Update.  gv_mppi_update_async scores the resident rollout exactly as gv_control_step_async does -- the same samplers,
 *   record buffers, combine and selection; result and totals are byte for byte what gv_control_step returns on that
 *   rollout -- and then, over the admitted trajectories k (none admitted: the nominal is unchanged),
 *     x_k = (double)(total_k - best_total)        -- an exact uint64 difference
 *     e_k = exp(-(x_k / lambda));   S = sum e_k;   N[p][c] = sum e_k * (double)controls[k][p][c]
 *     nominal[p][c] = (float)(N[p][c] / S)        -- S >= 1: the best trajectory contributes e = 1
 *   The sums are fp64, in an order fixed by (K, P, C) alone: no floating-point atomics, the same call on the same bytes
 *   gives the same bytes.  gv_mppi_average adds in index order, so the device may differ from it by the reordering of a
 *   K-term fp64 sum.  nominal_out (P * C floats, may be NULL) follows the rules of result and totals: pinned memory
 *   (nominal_out and totals aligned to 8 bytes, result to 16) is written by a kernel, anything else by a copy command
 *   behind it.  GV_ERR_BAD_ARG as for gv_control_step_async.  GV_ERR_STATE without a configuration, a footprint, a
 *   costmap, a field when a nav weight is set, a rollout, sampled controls of the rollout's K and P, a nominal of that P
 *   and the controls' C, and with a communicator of more than one rank.
 *   gv_mppi_cycle_async is gv_mppi_sample_async + gv_rollout_async on the sampled controls + gv_mppi_update_async, all on
 *   gv_stream(h) without a host wait; every argument and state rule is checked before the first of them is enqueued, and
 *   the results equal the three calls' by bytes.  The synchronous forms add the wait.  All of these are ordered and
 *   allowed like gv_control_step_async, also between gv_tick_enqueue and gv_tick_wait.
 *   gv_mppi_words, gv_mppi_sample_controls and gv_mppi_average are host only and take no handle: the same arithmetic
 *   text compiled for the host (C is 2 or 3; the rollout's limits; in gv_mppi_average a total of UINT64_MAX marks a
 *   rejected trajectory, and nominal_in is copied to nominal_out when every trajectory is). */
typedef struct {
  double sigma[3];             /* per control channel, finite, >= 0; the first C are read */
  float u_min[3], u_max[3];    /* clamp, u_min <= u_max, +-inf allowed, no NaN            */
  double lambda;               /* temperature in units of a total, finite, > 0            */
  uint32_t flags;              /* 0                                                       */
} gv_mppi_config;
enum {
  GV_MPPI_SHIFT = 1 << 0   /* sample around the nominal advanced by one step */
};
int gv_set_mppi(gv_handle h, const gv_mppi_config *cfg);
int gv_mppi_set_nominal(gv_handle h, const float *nominal, int32_t P);
int gv_get_mppi_nominal(gv_handle h, float *out /* may be NULL */, int32_t *P /* may be NULL */);
int gv_mppi_sample_async(gv_handle h, int32_t K, uint64_t seed, uint64_t iteration, uint32_t flags);
int gv_mppi_sample(gv_handle h, int32_t K, uint64_t seed, uint64_t iteration, uint32_t flags);
int gv_device_controls(gv_handle h, float **controls, int32_t *K, int32_t *P, int32_t *C);
int gv_get_controls(gv_handle h, float *out);
int gv_mppi_update_async(gv_handle h, const gv_critic_weights *w, uint32_t flags, gv_control_result *result,
                         uint64_t *totals, float *nominal_out /* may be NULL */);
int gv_mppi_update(gv_handle h, const gv_critic_weights *w, uint32_t flags, gv_control_result *result, uint64_t *totals,
                   float *nominal_out /* may be NULL */);
int gv_mppi_cycle_async(gv_handle h, const double start[3], int32_t K, uint64_t seed, uint64_t iteration,
                        uint32_t sample_flags, const gv_critic_weights *w, uint32_t flags, gv_control_result *result,
                        uint64_t *totals, float *nominal_out /* may be NULL */);
int gv_mppi_cycle(gv_handle h, const double start[3], int32_t K, uint64_t seed, uint64_t iteration, uint32_t sample_flags,
                  const gv_critic_weights *w, uint32_t flags, gv_control_result *result, uint64_t *totals,
                  float *nominal_out /* may be NULL */);
int gv_mppi_words(uint64_t seed, uint64_t iteration, uint32_t k, uint32_t p, uint32_t words[4]);
int gv_mppi_sample_controls(const gv_mppi_config *cfg, int32_t C, const float *nominal, int32_t K, int32_t P, uint64_t seed,
                            uint64_t iteration, uint32_t flags, float *controls_out);
int gv_mppi_average(const gv_mppi_config *cfg, int32_t C, const float *controls, const uint64_t *totals, int32_t K,
                    int32_t P, const float *nominal_in, float *nominal_out);

/* ------------------------- [EXTENSION] MPPI rate and turning-radius limits, control cost (planner) -- */
/* X12.  What X11 left out of nav2's mppi::Optimizer, except coloured noise: limits on how fast a sampled control may
 * change from one step to the next, a minimum turning radius for a car-like base, and the control-cost term in the
 * exponent of the weights.  All three run on the device between the nominal and the next nominal; with no limits set
 * (the state after gv_create) every X11 call gives the bytes it gave before.
 *
 * Configuration (gv_mppi_limits).  rate_up[c] / rate_down[c] the largest increase / decrease of control channel c per
 *   SECOND; u_prev[c] the control in force before step 0 (the measured velocity; NaN: step 0 of that channel is free);
 *   min_turn_radius in metres (0: off); gamma the control-cost weight in units of a total (0: off).
 *   gv_set_mppi_limits is handle configuration like gv_set_mppi: no device work, kept through gv_reset,
 *   gv_set_log_odds and gv_grid_move; NULL turns it off; every sampling, update and cycle carries the limits in force
 *   when it is enqueued, by value; it is meant to be called every control cycle with the measured velocity.
 *   GV_ERR_BAD_ARG, limits unchanged, for a null handle, a rate that is NaN or < 0 (+inf: none), a radius or gamma
 *   that is negative or not finite, or flags other than 0; all three channels are checked.  A radius > 0 needs
 *   GV_MOTION_DIFF: the sampling or cycle call that would use it under GV_MOTION_OMNI returns GV_ERR_STATE and
 *   enqueues nothing (the setter cannot know the model a later call runs under).
 * Constrained sampling.  Let f[p][c] be the X11 value of controls[k][p][c], the complete text above, clamp included
 *   (trajectory 0: z = 0).  Once per call, with the model's dt:
 *     up[c] = (float)(rate_up[c] * dt);  dn[c] = (float)(rate_down[c] * dt)
 *     inv_r = min_turn_radius > 0 ? (float)(1.0 / min_turn_radius) : 0
 *   Then per trajectory k, every operation one float32 operation in exactly this order, never contracted:
 *     s[c] = u_prev[c]
 *     for p = 0 .. P-1:
 *       for c:  q[c] = f[p][c]
 *               if s[c] is not NaN:  lo = s[c] - dn[c];  hi = s[c] + up[c]
 *                                    q[c] = q[c] < lo ? lo : q[c];   q[c] = q[c] > hi ? hi : q[c]
 *       if inv_r > 0:  b = fabsf(q[0]) * inv_r;  q[1] = q[1] < -b ? -b : q[1];  q[1] = q[1] > b ? b : q[1]
 *       s = q;  controls[k][p][c] = q[c]
 *   The limits are signed rates on the control value: rate_up bounds an increase of the value, rate_down a decrease,
 *   whatever its sign.  nav2 tells accelerating from braking by the sign of v; THIS DEFINITION DOES NOT.  The radius is
 *   applied behind the rate window and wins: where it binds, q[1] may lie outside [lo, hi].  Trajectory 0
 *   is the constrained nominal; the rollout, the scorers and the average read the constrained controls.  Limits with
 *   every rate +inf, every u_prev NaN and radius 0 change no byte.  The chain holds no library call, so the device
 *   equals gv_mppi_constrain byte for byte given the same f.  The new nominal an update writes is a weighted mean of
 *   constrained sequences; IT IS NOT PASSED THROUGH THE CHAIN AGAIN.  A caller who wants the executed command
 *   constrained applies gv_mppi_constrain with K = 1; the next cycle's trajectory 0 is constrained anyway.
 *   gv_mppi_constrain is host only: controls[K][P][C] in place, C from m->model, the rollout's limits on K and P;
 *   GV_ERR_BAD_ARG for a null pointer, limits or a model that the setters refuse, or a radius > 0 under OMNI.
 * Control cost.  Active when gamma > 0 (gamma == 0: the update is X11's text and bytes).  Over the resident controls
 *   and the nominal the sampling read -- pn = p, or min(p + 1, P - 1) when the sampling that made the controls had
 *   GV_MPPI_SHIFT (the handle remembers it) -- with J = P * C and j = p * C + c, in fp64, never contracted:
 *     q_c    = sigma[c] > 0 ? gamma / (sigma[c] * sigma[c]) : 0.0
 *     term_j = q_c * ((double)nominal[pn][c] * ((double)controls[k][p][c] - (double)nominal[pn][c]))
 *     a_l    = 0.0;  a_l = a_l + term_j   for j = l, l + 64, l + 128, ..   (l = 0 .. 63, ascending j)
 *     for w = 32, 16, 8, 4, 2, 1:  a_l = a_l + a_(l+w)   for l < w
 *     g_k    = a_0
 *   for every k, rejected or not.  Then, over the admitted trajectories,
 *     x_k = (double)(total_k - best_total) + g_k;   m = min x_k;   e_k = exp(-((x_k - m) / lambda))
 *   and S, N and the new nominal exactly as in X11, in the same order of sums.  The trajectory that attains m
 *   contributes e = 1, so S >= 1.  result, best, best_total and totals remain the critics' alone, byte for byte what
 *   gv_control_step returns.  With no trajectory admitted the nominal stays as it is (g is still written).
 *   gv_get_mppi_control_costs is a synchronous read-back of the K values g_k of the last update; GV_ERR_STATE when
 *   the last update ran without gamma > 0 (or none has run).  gv_mppi_control_costs (host only) is the same text:
 *   the first C sigmas of cfg, lim->gamma, sample_flags 0 or GV_MPPI_SHIFT.  gv_mppi_average_cc (host only) is
 *   gv_mppi_average with x_k and m as above, sums in index order; control_costs == NULL: gv_mppi_average itself. */
typedef struct {
  double rate_up[3], rate_down[3];  /* largest increase / decrease of control channel c per SECOND; >= 0, +inf = none, no NaN */
  float  u_prev[3];                 /* the control in force before step 0 (the measured velocity); NaN = step 0 of that channel is free */
  double min_turn_radius;           /* m; 0 = off; finite, >= 0; > 0 needs GV_MOTION_DIFF when a call uses it */
  double gamma;                     /* control-cost weight, in units of a total; finite, >= 0; 0 = off */
  uint32_t flags;                   /* 0 */
} gv_mppi_limits;
int gv_set_mppi_limits(gv_handle h, const gv_mppi_limits *lim);   /* NULL = off, the state after gv_create */
int gv_mppi_constrain(const gv_mppi_limits *lim, const gv_motion_model *m, float *controls /* [K][P][C], in place */,
                      int32_t K, int32_t P);
int gv_get_mppi_control_costs(gv_handle h, double *out);
int gv_mppi_control_costs(const gv_mppi_config *cfg, const gv_mppi_limits *lim, int32_t C, const float *controls,
                          const float *nominal, int32_t K, int32_t P, uint32_t sample_flags, double *g_out);
int gv_mppi_average_cc(const gv_mppi_config *cfg, int32_t C, const float *controls, const uint64_t *totals,
                       const double *control_costs /* may be NULL: gv_mppi_average */, int32_t K, int32_t P,
                       const float *nominal_in, float *nominal_out);

/* ------------------------------ [EXTENSION] scoring against predicted moving objects (planner) -- */
/* X13.  The costmap X7 scores against is a snapshot: a car that crosses the path is lethal where it was at the last map
 * update and free where it will be when the robot gets there.  gv_score_dynamic tests every pose of K trajectories
 * against a set of moving oriented rectangles -- what gv_tick returns as gv_lshape_pose, plus a velocity -- propagated
 * at constant velocity to the pose's own time, and gives one integer record per trajectory, which the control step and
 * the MPPI update use like the X7 and X9 records.  The reference has no such step; this text is its definition.  With
 * no configuration set (the state after gv_create) every X10 .. X12 call gives the bytes it gave before.
 *
 * Robot.  n_circles circles of one radius with their centres at (off_x[i], 0) in the robot frame, x forward.
 * Cost table.  table[q] for q = 0 .. d2max is what gv_inflation_cost_table returns for {inscribed_radius = radius,
 *   inflation_radius = influence_radius, cost_scaling_factor, lethal_threshold = 100, flags = 0} at resolution =
 *   quantum -- the same host code: 254 at q == 0, 253 while sqrt(q) * quantum <= radius, then nav2's exponential, 0
 *   beyond the influence radius.  T = d2max + 1 entries, Rc = isqrt(d2max) <= 63 as for X6.  A moving object costs
 *   what an inflated lethal rectangle would cost at that distance, on the 0..254 scale of the X7 costs it is added to.
 * Object table.  Built once per gv_set_moving_objects, on the host, in fp64, every operation one operation in this
 *   order:
 *     c  = 1.0 - 2.0 * (qy*qy + qz*qz);    s  = 2.0 * (qw*qz + qx*qy)
 *     hl = 0.5 * length;                   hw = 0.5 * width
 *   the terms of gv_grid_move's yaw: no atan2 and no normalisation, THE QUATERNION IS USED AS GIVEN.  Length lies along
 *   the heading, width across it; an identity quaternion gives the axis-aligned rectangle updateMap(poses) stamps.
 * Per pose p (x, y, yaw: three float32 as for X7), circle i and object j, in fp64, every operation one operation in
 *   exactly this order, never contracted:
 *     t  = t0 + (double)p * dt
 *     ax = (double)x,  ay = (double)y                                   when off_x[i] == 0.0 (the yaw is not read)
 *     ax = (double)x + cy * off_x[i],  ay = (double)y + sy * off_x[i]   otherwise; cy, sy = cos, sin of (double)yaw,
 *                                                       computed once per pose and only if some off_x != 0
 *     ox = x_j + vx_j * t;   oy = y_j + vy_j * t
 *     dx = ax - ox;          dy = ay - oy
 *     lx = c_j * dx + s_j * dy;      ly = c_j * dy - s_j * dx
 *     ex = fabs(lx) - hl_j;  ex = ex > 0.0 ? ex : 0.0      -- a NaN lands on 0.0: a NaN pose lies "inside" every object
 *     ey = fabs(ly) - hw_j;  ey = ey > 0.0 ? ey : 0.0
 *     d2 = ex * ex + ey * ey                               -- squared distance, circle centre to rectangle
 * Pose cost.  m2 = the minimum of d2 over all circles and objects, +inf with no objects; u = m2 * inv_q2 with
 *   inv_q2 = 1.0 / (quantum * quantum) computed once on the host; the cost is u < (double)T ? table[(uint32_t)u] : 0.
 *   A minimum over finite-or-inf fp64 values does not depend on order, so no order shows in any field.
 * Per trajectory (gv_dyn_score, 24 bytes): max_cost, first_collision and cost_sum as for X7 over these pose costs;
 *   min_dist2 the smallest d2 over poses, circles and objects (+inf with no objects); nearest_object the smallest j
 *   whose own minimum over poses and circles equals min_dist2 (-1 with no objects).
 *   On the device cos and sin are the device library's, in gv_dyn_score_poses the C library's; they may differ in the
 *   last bit.  When every off_x is 0 neither is called and the two agree byte for byte.
 *
 * gv_dyn_cost_table is host only and takes no handle, in the manner of gv_inflation_cost_table: *n = T whenever the
 *   configuration is valid; GV_ERR_BAD_ARG for a null or invalid configuration, a null table or cap < T.
 * gv_set_dyn_config is handle configuration like gv_set_footprint: no device work, kept through gv_reset,
 *   gv_set_log_odds and gv_grid_move; NULL turns it off (the state after gv_create).  Every enqueued call keeps the
 *   configuration and the table it was enqueued with (the table reaches the device through X6's alternating slots).
 *   GV_ERR_BAD_ARG, configuration unchanged, for a null handle or any field outside the ranges written beside it.
 * gv_set_moving_objects replaces the set: n in 0..128, objs may be NULL when n == 0; every field that is read must be
 *   finite, length and width >= 0, else GV_ERR_BAD_ARG and the set is unchanged.  The caller's array is free on return.
 *   The set is stream-ordered on gv_stream(h): calls enqueued before it keep the old set, calls after it see the new
 *   one.  It is kept through gv_reset; the state after gv_create is n = 0.
 * gv_score_dynamic_async takes the arguments, flags (GV_TRAJ_KEEP_POSE_COST, GV_TRAJ_DEVICE_POSES), limits and
 *   destination rules of gv_score_trajectories_async; pinned scores aligned to 8 bytes are written by the kernel.  It
 *   needs neither a grid nor a costmap: GV_ERR_STATE only without a configuration.  K == 0 is a successful no-op.
 *   Allowed between gv_tick_enqueue and gv_tick_wait.  gv_score_dynamic is the same call followed by the wait.
 * gv_dyn_score_poses is host only and takes no handle: the same arithmetic text compiled for the host (pose_cost may
 *   be NULL; the rules of the three calls above on cfg, objs, n, K and P).
 *
 * Control step.  dyn_used holds iff a configuration is set.  Then gv_control_step*, gv_mppi_update* and gv_mppi_cycle*
 *   launch this sampler over the resident rollout between the nav sampler and the selection, trajectory k is also
 *   REJECTED when dyn[k].first_collision >= 0, and an admitted total gains
 *     w_sum * cost_sum + w_max * max_cost      (max_cost taken as uint32),
 *   at most 65535 * (4096 * 255 + 255) more: the total stays below 2^61.  With zero objects every dyn record is
 *   {0, -1, 0, -1, +inf} and the totals are those without a configuration.
 *   gv_control_select_dyn is the host twin: gv_control_select with the third record; cfg gives w_sum and w_max.  With
 *   cfg == NULL it is gv_control_select (dyn is not read); with one, GV_ERR_BAD_ARG for a null dyn or weights above
 *   65535. */
typedef struct {
  gv_lshape_pose pose;   /* frame of the trajectory poses (base_link at the last map update): px, py, the quaternion,
                            length, width are read; pz and height are ignored */
  double vx, vy;         /* m/s in that frame */
} gv_moving_object;      /* 96 bytes */
typedef struct {
  int32_t n_circles;            /* 1..8: the robot is n circles of one radius on its x axis */
  double off_x[8];              /* m, robot frame, x forward; the first n_circles are read, all finite */
  double radius;                /* m, finite, >= 0: circle radius, any safety margin included */
  double influence_radius;      /* m, finite, >= radius: a centre farther than this from every object costs 0 */
  double cost_scaling_factor;   /* 1/m, finite, >= 0 */
  double quantum;               /* m, finite, > 0: distance step of the cost table; Rc <= 63 as for X6 */
  double t0, dt;                /* s, finite, dt >= 0: pose p is at time t0 + p * dt */
  int32_t collision_cost;       /* 1..255: a pose collides when its cost is >= this */
  uint32_t w_sum, w_max;        /* 0..65535: weights in the control step */
  uint32_t flags;               /* 0 */
} gv_dyn_config;
typedef struct {
  int32_t max_cost;          /* maximum pose cost */
  int32_t first_collision;   /* smallest pose index with cost >= collision_cost, -1 when none */
  uint32_t cost_sum;         /* sum of the pose costs */
  int32_t nearest_object;    /* smallest object index that attains min_dist2, -1 with no objects */
  double min_dist2;          /* smallest d2 over poses, circles and objects; +inf with no objects */
} gv_dyn_score;              /* 24 bytes */
int gv_dyn_cost_table(const gv_dyn_config *cfg, uint8_t *table, int32_t cap, int32_t *n);
int gv_set_dyn_config(gv_handle h, const gv_dyn_config *cfg);   /* NULL = off, the state after gv_create */
int gv_set_moving_objects(gv_handle h, const gv_moving_object *objs, int32_t n);
int gv_score_dynamic_async(gv_handle h, const float *poses, int32_t K, int32_t P, uint32_t flags, gv_dyn_score *scores,
                           uint8_t *pose_cost);
int gv_score_dynamic(gv_handle h, const float *poses, int32_t K, int32_t P, uint32_t flags, gv_dyn_score *scores,
                     uint8_t *pose_cost);
int gv_dyn_score_poses(const gv_dyn_config *cfg, const gv_moving_object *objs, int32_t n, const float *poses, int32_t K,
                       int32_t P, gv_dyn_score *scores, uint8_t *pose_cost /* may be NULL */);
int gv_control_select_dyn(const gv_critic_weights *w, const gv_traj_score *traj, const gv_nav_score *nav,
                          const gv_dyn_score *dyn, const gv_dyn_config *cfg, int32_t K, gv_control_result *result,
                          uint64_t *totals /* may be NULL */);

/* ------------------------------ [EXTENSION] tracking the detected boxes (perception -> planner) -- */
/* X14.  X13 takes a velocity for each rectangle, and gv_tick returns gv_lshape_pose boxes one frame at a time, with no
 * identity and no motion.  gv_track_update is the link: a multi-object tracker over the tick's boxes, nearest-neighbour
 * association inside a gate and a constant-velocity Kalman filter per axis, with at most 128 tracks.  Its state lives
 * on the device next to its consumer, it is enqueued on gv_stream(h) like every planner call, and it can hand its
 * confirmed tracks to X13 without the set crossing the host.  The reference has no such step; this text is its
 * definition, and the device kernel, the host twin gv_track_step and tests/track_ref.py follow it byte for byte.  With
 * no configuration set (the state after gv_create) every existing call gives the bytes it gave before.
 *
 * State.  128 slots; a live slot holds a gv_track (128 bytes).  Beside the slots a uint32_t next_id, 1 after gv_create.
 *   The frame is X13's: the base frame at the last map update, velocities over ground expressed in its axes.
 *   WITHOUT motion THE VELOCITIES ARE RELATIVE TO THE VEHICLE: a parked car seen from a vehicle that drives at 5 m/s
 *   gets -5 m/s.  Pass every update the motion that gv_grid_move was given for the same interval.
 * Configuration (gv_track_config).  Computed once on the host:
 *     q = sigma_accel*sigma_accel;  r = sigma_meas*sigma_meas;  v0 = sigma_v0*sigma_v0;
 *     gate2 = gate*gate;            min2 = min_speed*min_speed
 * One update.  The inputs are dets[n], dt and an optional motion.  All arithmetic is fp64; every operation is one
 *   operation in exactly the order given here, never contracted.
 *   Step 1, ego motion, only when motion != NULL.  motion is gv_grid_move's argument, base_prev <- base_now, and as in
 *   X13 THE QUATERNION IS USED AS GIVEN:
 *     ce = 1.0 - 2.0*(qy*qy + qz*qz);    se = 2.0*(qw*qz + qx*qy)
 *   and for every live track
 *     dx = x - tx;  dy = y - ty
 *     x = ce*dx + se*dy;       y = ce*dy - se*dx
 *     vx' = ce*vx + se*vy;     vy' = ce*vy - se*vx
 *     q <- conj(q_motion) (x) q, a Hamilton product: with a = (-mx, -my, -mz, mw) and b = q, each line left to right,
 *       w = aw*bw - ax*bx - ay*by - az*bz
 *       x = aw*bx + ax*bw + ay*bz - az*by
 *       y = aw*by - ax*bz + ay*bw + az*bx
 *       z = aw*bz + ax*by - ay*bx + az*bw
 *   Step 2, predict, for every live track, with dt2 = dt*dt and the old p's on the right-hand sides:
 *     x = x + vx*dt;  y = y + vy*dt
 *     p00' = ((p00 + (2.0*dt)*p01) + dt2*p11) + q*(0.25*(dt2*dt2))
 *     p01' = (p01 + dt*p11) + q*(0.5*(dt2*dt))
 *     p11' = p11 + q*dt2
 *     age increases by 1 and saturates at 2^31 - 1;  det = -1.
 *   Step 3, validity.  Detection d is valid iff px, py, qx, qy, qz, qw, length, width are all finite and length,
 *     width >= 0.  Invalid detections take no part in the update and are counted in n_invalid.  pz and height are not
 *     read.
 *   Step 4, association.  For live slot s and valid detection d:
 *     ex = px - x;  ey = py - y;  d2 = ex*ex + ey*ey
 *     the pair is a candidate iff d2 <= gate2 (a NaN fails).  The matching is the greedy one over the total order
 *     (d2, s, d): take the smallest remaining candidate, match it, drop every other candidate of that slot and of that
 *     detection, repeat until no candidate remains.  No order of evaluation shows in the result.
 *   Step 5, matched pair, old values on the right-hand sides:
 *     S = p00 + r;  k0 = p00/S;  k1 = p01/S
 *     x = x + k0*ex;  vx = vx + k1*ex
 *     y = y + k0*ey;  vy = vy + k1*ey
 *     p11' = p11 - k1*p01;  p01' = p01 - k1*p00;  p00' = p00 - k0*p00
 *     q, length and width are taken from the detection; hits increases by 1 and saturates; misses = 0; det = d.
 *   Step 6, unmatched live track.  misses increases by 1 (and saturates); the slot is freed when misses > max_misses and
 *     counted in n_deleted.
 *   Step 7, births.  Unmatched valid detections in ascending d, each into the lowest free slot; slots freed in step 6
 *     count as free.  id = next_id++ (wraps mod 2^32); slot = the slot; hits = 1, misses = 0, age = 0, det = d; x, y from
 *     the detection; vx = vy = 0.0; q, length, width from the detection; p00 = r, p01 = 0.0, p11 = v0.  With no free
 *     slot the detection is dropped and counted in n_dropped.
 *   Step 8, export.  Live slots in ascending order; a track is exported iff hits >= confirm_hits and x, y, vx, vy are
 *     all finite.  sp2 = vx*vx + vy*vy; the exported velocity is (0.0, 0.0) when sp2 < min2, otherwise (vx, vy).  The
 *     export is a gv_moving_object {pose = {x, y, 0, q, length, width, 0}, vx, vy}, and its X13 table row is what
 *     gv_set_moving_objects builds of it, the same text.
 * Update record (gv_track_info, 40 bytes).  n_tracks: live slots after the update; n_confirmed: those with hits >=
 *   confirm_hits; n_exported, n_matched, n_born, n_deleted, n_dropped, n_invalid as above; next_id after the update;
 *   reserved = 0.
 *
 * gv_set_track_config is handle configuration like gv_set_dyn_config: no device work, kept through gv_reset,
 *   gv_set_log_odds and gv_grid_move (which keep the tracks too: they read no map).  NULL turns it off and empties the
 *   tracks: the state after gv_create, next_id = 1.  GV_ERR_BAD_ARG, configuration unchanged, for a null handle or
 *   any field outside the ranges written beside it.
 * gv_set_tracks replaces the state, stream-ordered on gv_stream(h): n in 0..128 (n == 0 empties the state; tracks may
 *   then be NULL), the slot fields distinct, ascending and in 0..127; every other value is taken as given, non-finite
 *   included.  GV_ERR_BAD_ARG and the state unchanged otherwise.  The caller's array is free on return.
 * gv_get_tracks is a synchronous read-back (it waits for gv_stream(h)) of the live records in ascending slot order:
 *   *n receives their number and *next_id the counter (either may be NULL); GV_ERR_BAD_ARG when cap is below the
 *   number, after writing *n, and then nothing is written to out.
 * gv_track_update_async enqueues one update on gv_stream(h) without a host wait (the allocations of a first call
 *   aside), behind everything enqueued before it; allowed between gv_tick_enqueue and gv_tick_wait.  dets is host
 *   memory, copied through a pinned staging slot (the caller's array is free on return), or with GV_TRACK_DEVICE_DETS
 *   device memory read in place; NULL is allowed when n == 0.  info (one record) and tracks (room for 128 records) may each be
 *   NULL and follow the destination rules of gv_score_trajectories_async: pinned memory aligned to 8 bytes is written
 *   by the kernel, other host memory by a copy behind it.  tracks receives the live records in ascending slot order
 *   and zero bytes in the records after them, all 128 written.
 *   With GV_TRACK_FEED_DYNAMIC the exported rows become X13's object set: they are written on the device, in slot
 *   order, into the next object slot, with their count beside them.  This is stream-ordered exactly like
 *   gv_set_moving_objects: calls enqueued before it keep the old set, calls after it see the new one, and a later
 *   gv_set_moving_objects replaces it again.  The host does not learn the count: a fed set is "up to 128" to it.
 *   GV_ERR_BAD_ARG for a null handle, n outside 0..128, null dets with n > 0, dt not finite or < 0, a non-finite field
 *   of motion, or unknown flags; GV_ERR_STATE without a configuration.  gv_track_update is the same call followed by
 *   the wait.
 *   [EXTENSION] X15: with GV_TRACK_TICK_DETS the detections are the list of the most recently enqueued tick
 *   (GV_TICK_KEEP_DETS: the poses of grid_vision_node.cpp:204 / :227), read in place on the device behind the tick,
 *   pending or already waited for; the kernel reads their number there and the host never learns it.  dets must be
 *   NULL and n 0, and GV_TRACK_DEVICE_DETS must not be set with it: GV_ERR_BAD_ARG otherwise.  GV_ERR_STATE when no
 *   tick was enqueued or the last one enqueued did not carry GV_TICK_KEEP_DETS.  Everything else is as above; two
 *   updates from one list see the same list twice, and a later gv_tick_enqueue is ordered behind them.
 * gv_track_step is host only and takes no handle: the same arithmetic text compiled for the host.  tracks (room for
 *   128), *n_tracks and *next_id are in/out, under gv_set_tracks' rules on the way in and gv_get_tracks' order on the
 *   way out; info may be NULL; objs (room for 128) and n_objs may be NULL together.  Its objs, given to
 *   gv_set_moving_objects, produce the rows the device feed writes.  GV_ERR_BAD_ARG for a null or invalid cfg and for
 *   what the two calls above reject. */
typedef struct {
  uint32_t id;             /* unique while 2^32 births have not passed */
  int32_t slot;            /* 0..127, where the track lives */
  int32_t hits, misses;    /* matched updates in all; updates without a match since the last one */
  int32_t age;             /* updates since birth */
  int32_t det;             /* the detection matched in the last update, -1 when none */
  double x, y, vx, vy;     /* m, m/s: centre and velocity in the frame above */
  double qx, qy, qz, qw;   /* of the last matched detection, moved with the vehicle since */
  double length, width;    /* of the last matched detection */
  double p00, p01, p11;    /* position / position-velocity / velocity covariance, the same for both axes */
} gv_track;                /* 128 bytes */
typedef struct {
  double gate;          /* m, finite, > 0: a detection farther than this from a track is no candidate */
  double sigma_accel;   /* m/s^2, finite, >= 0: process noise */
  double sigma_meas;    /* m, finite, > 0: measurement noise of a box centre */
  double sigma_v0;      /* m/s, finite, >= 0: velocity uncertainty at birth */
  double min_speed;     /* m/s, finite, >= 0: a slower track is exported with velocity (0, 0) */
  int32_t confirm_hits; /* 1..255: a track is exported from this many hits on */
  int32_t max_misses;   /* 0..255: a track is deleted after more consecutive misses than this */
  uint32_t flags;       /* 0 */
} gv_track_config;
typedef struct {
  int32_t n_tracks, n_confirmed, n_exported, n_matched, n_born, n_deleted, n_dropped, n_invalid;
  uint32_t next_id, reserved;
} gv_track_info;        /* 40 bytes */
enum {
  GV_TRACK_DEVICE_DETS  = 1 << 0,   /* dets is device memory, read in place                  */
  GV_TRACK_FEED_DYNAMIC = 1 << 1,   /* the exported tracks become X13's moving-object set    */
  GV_TRACK_TICK_DETS    = 1 << 2    /* [EXTENSION] X15: the detections are the last tick's list */
};
int gv_set_track_config(gv_handle h, const gv_track_config *cfg);   /* NULL = off, the state after gv_create */
int gv_set_tracks(gv_handle h, const gv_track *tracks, int32_t n, uint32_t next_id);
int gv_get_tracks(gv_handle h, gv_track *out, int32_t cap, int32_t *n, uint32_t *next_id);
int gv_track_update_async(gv_handle h, const gv_lshape_pose *dets, int32_t n, double dt,
                          const gv_transform *motion /* may be NULL */, uint32_t flags, gv_track_info *info /* may be NULL */,
                          gv_track *tracks /* may be NULL, room for 128 */);
int gv_track_update(gv_handle h, const gv_lshape_pose *dets, int32_t n, double dt,
                    const gv_transform *motion /* may be NULL */, uint32_t flags, gv_track_info *info /* may be NULL */,
                    gv_track *tracks /* may be NULL, room for 128 */);
int gv_track_step(const gv_track_config *cfg, gv_track *tracks, int32_t *n_tracks, uint32_t *next_id,
                  const gv_lshape_pose *dets, int32_t n, double dt, const gv_transform *motion /* may be NULL */,
                  gv_track_info *info /* may be NULL */, gv_moving_object *objs /* may be NULL, room for 128 */,
                  int32_t *n_objs);

/* ------------------------------------------------------ [EXTENSION] frame -- */
/* One fused per-frame pass over the resident cloud (SURVEY rows X1, X2, A5, A8,
 * A7, A18):  bin points into hit counts, ray-march free space from the sensor
 * origin, first-match bbox id per point, then one grid pass: decay, rectangle
 * adds, hit/miss rule, clamp, sigmoid, int8 pack. */
enum {
  GV_FRAME_BIN       = 1 << 0,   /* X1: hits, optional cell_idx                 */
  GV_FRAME_RAYMARCH  = 1 << 1,   /* X2: miss (needs GV_FRAME_BIN)               */
  GV_FRAME_BBOX_TEST = 1 << 2,   /* A5: bbox_id per point                       */
  GV_FRAME_KEEP_CELL_IDX = 1 << 3,  /* write cell_idx[N] (debug/parity output)  */
  GV_FRAME_KEEP_COUNTS   = 1 << 4,  /* keep hits/miss of this frame for getters */
  GV_FRAME_VISION_ORIENT = 1 << 5   /* poses come from net outputs (A13/A14/A15)
                                       instead of base-frame poses             */
};
typedef struct {
  uint32_t flags;
  const gv_bbox *bboxes;          /* nb bboxes (GV_FRAME_BBOX_TEST / VISION_ORIENT) */
  int32_t n_bboxes;
  const gv_lshape_pose *poses;    /* base-frame poses for the rectangle adds     */
  int32_t n_poses;
  const float *orient, *conf, *dims;  /* GV_FRAME_VISION_ORIENT: nb*4, nb*2, nb*3 */
} gv_frame_desc;
/* Upload the small per-frame detection inputs (bboxes, poses / net outputs).  Two sets alternate: the
 * arrays are copied into pinned staging (the caller's arrays are free on return), go to the device in
 * one copy on the stream of the frame that reads them first -- in order ahead of it -- and are turned
 * into the bbox-test tables there.
 * Neither form waits for the copy or drains the frame pipeline (the _async name is kept for symmetry
 * with the cloud uploads).  The standalone entry points above (gv_extract_cloud_per_bbox,
 * gv_update_map_poses, ...) keep their inputs in a set of their own and never change what
 * gv_frame_enqueue uses. */
int gv_frame_set_detections(gv_handle h, const gv_frame_desc *desc);
int gv_frame_set_detections_async(gv_handle h, const gv_frame_desc *desc);
/* Enqueue one frame using the resident cloud and the last detections set (asynchronous).
 * GV_ERR_STATE before the first gv_frame_set_detections.  Two or three frames run side by side (the third lane is
 * the upload stream while no cloud has been uploaded for a while; GV_LANES=2: never): binning and ray stage of
 * frame f on an internal stream, its grid pass on gv_stream(h) behind them, so
 * the grid passes -- and anything the caller puts on gv_stream(h) between two frames -- execute in
 * enqueue order and see every result of the frames before them.  At most SIX frames are in flight (four
 * with two lanes): the call waits on the host for the frame six back when the caller runs further ahead. */
int gv_frame_enqueue(gv_handle h);
/* Make gv_stream(h) wait (on the device, not the host) for every upload enqueued so far as well
 * (frames are ordered on gv_stream(h) by construction): afterwards an event recorded or a kernel
 * launched there sees the results of everything enqueued on the handle. */
int gv_frame_fence(gv_handle h);
/* Wait (host) for everything enqueued on the handle. */
int gv_synchronize(gv_handle h);
/* gv_frame_set_detections + gv_frame_enqueue + gv_synchronize */
int gv_process_frame(gv_handle h, const gv_frame_desc *desc);
/* Per-frame outputs of the last frame (need GV_FRAME_KEEP_* where noted). */
int gv_get_hits(gv_handle h, int32_t *out);          /* G ints; any BIN frame (generic grids: KEEP_COUNTS) */
int gv_get_miss(gv_handle h, int32_t *out);          /* G ints in {0,1}, KEEP_COUNTS */
int gv_get_cell_idx(gv_handle h, int32_t *out);      /* N ints, KEEP_CELL_IDX */
int gv_get_bbox_id(gv_handle h, int32_t *out);       /* N ints, BBOX_TEST     */
/* number of grid cells visited by the last ray-march (sum over marched rays) */
int gv_get_ray_stats(gv_handle h, uint64_t *n_rays, uint64_t *n_visits);

/* ------------------------------------------------------------ the node's tick -- */
/* Replaces GridVision::timerCallback from filterBBoxes to publishOccupancyGrid (src/grid_vision_node.cpp:153-244) as
 * ONE batch of device work with ONE host wait:
 *   filterBBoxes (:384-403, host)                                   -> static / dynamic boxes
 *   static boxes: buildKDTree + computeDepthForBoundingBoxes (:168-184, cloud_detections.cpp:8-87) + convertPixelsTo3D
 *   dynamic boxes, GV_TICK_VISION_ORIENT: VisionOrientation::postProcessOutputs on the network outputs (:190-209)
 *                  otherwise:             cloud_detections::computeBBoxPose on ALL boxes (:210-231, cloud_detections.cpp:300-321)
 *   transformLShapeObjects (:204, :227), updateMap(grid, poses) / updateMap(grid) (:145, :206, :230, :235),
 *   GridMapRosConverter::toOccupancyGrid (:265-278).
 * The poses go from the kernel that computes them through the camera->base transform and the rectangle kernel into the
 * grid pass without leaving the device; the depths, the poses (for the markers, :243) and optionally the packed grid
 * come back through pinned memory and are complete when gv_tick_wait returns.  The static boxes' kNN runs on a second
 * stream beside the pose branch.  The caller runs extract_bboxes and, for GV_TICK_VISION_ORIENT, the orientation
 * network on the dynamic boxes (gv_filter_bboxes gives their order) first; a tick with no boxes is the :141-147 path.
 * GV_ERR_TF when a transform the tick needs was never set (the node publishes the stale grid, :160-164).
 * One tick may be pending per handle; frames in flight (gv_frame_enqueue) are drained first. */
enum {
  GV_TICK_VISION_ORIENT  = 1 << 0,  /* use_vision_orientation (config/grid_vision_cfg.yaml:24) */
  GV_TICK_LIDAR_BIN      = 1 << 1,  /* [EXTENSION] the map update also bins the resident cloud (X1) ...  */
  GV_TICK_LIDAR_RAYMARCH = 1 << 2,  /* [EXTENSION] ... and marks free space (X2); tile-path grids only   */
  GV_TICK_KEEP_DETS      = 1 << 3   /* [EXTENSION] X15: the tick leaves its detection list on the device (below) */
};
/* [EXTENSION] X15 the tick's detection list.  With GV_TICK_KEEP_DETS the tick's batch ends, inside what gv_tick_wait
 * waits for, with one more kernel that leaves in device memory of the handle's own exactly what gv_tick_wait returns in
 * poses[0 .. min(n_poses, 128)): the dynamic objects' base-frame poses after transformLShapeObjects
 * (grid_vision_node.cpp:204 for the orientation network, :227 for computeBBoxPose), 128 records with zero bytes behind
 * the last one, their number and n_poses itself.  The list is empty where gv_tick_wait returns no poses (no dynamic
 * boxes, n_net == 0, fewer than three points, pca_empty: the kernel decides that from the ground plane's state on the
 * device).  The selection and the camera->base arithmetic are the host's text compiled for the device and give its bytes;
 * only the orientation network's quaternion starts from the device's fp64 sincos of -orient/2 instead of the host's and
 * may differ from gv_tick_wait's by a few units of 2^-53.  Without the flag a tick enqueues what it always
 * did.  gv_track_update* with GV_TRACK_TICK_DETS reads the list in place: tick -> tracker -> X13 -> gv_mppi_cycle_async
 * is then one batch on gv_stream(h) with one wait, and the host never sees the detections. */
typedef struct {
  uint32_t flags;
  const gv_bbox *bboxes;             /* what extract_bboxes returned (:138-139): static and dynamic mixed */
  int32_t n_bboxes;
  const float *orient, *conf, *dims; /* GV_TICK_VISION_ORIENT: n_net * 4 / 2 / 3 network outputs, dynamic-box order */
  int32_t n_net;                     /* 0 (no poses this tick, the reference's empty vector) or the number of dynamic boxes */
  int32_t k_near;                    /* k_near (grid_vision_cfg.yaml:20), 1..32 */
  int8_t *grid_out;                  /* optional: G bytes (gv_host_alloc for a true DMA) receive OccupancyGrid.data */
} gv_tick_desc;
typedef struct {
  int32_t n_static, n_dynamic;       /* out */
  gv_bbox *static_bboxes;            /* optional, room for n_bboxes: the static boxes (marker labels, :413-480)      */
  float *depths;                     /* optional, room for n_bboxes: depth of every static box (:176-177)            */
  double *base_points_xyz;           /* optional, room for 3 * n_bboxes: their base-frame points (:180)              */
  gv_lshape_pose *poses;             /* optional, room for n_bboxes: the dynamic objects' base-frame poses           */
  int32_t n_poses;                   /* out */
  int32_t pca_empty;                 /* out: 1 = computeBBoxPose returned {} (no plane / empty segmented cloud)      */
} gv_tick_result;
/* One tick at a time (the reference's timer is single threaded): a second gv_tick_enqueue before gv_tick_wait returns
 * GV_ERR_STATE, and so do, between the two, the synchronous calls that would reuse the tick's result block or its
 * detection set (gv_compute_depth_for_bboxes, gv_compute_bbox_pose*, gv_segment_ground_plane, gv_extract_cloud_per_bbox,
 * ...).  Cloud uploads (synchronous or not), gv_frame_*, the grid getters, gv_publish_grid_async, gv_update_map*,
 * gv_grid_move, gv_set_transforms, gv_set_height_band, gv_set_inflation, gv_inflate, the costmap getters,
 * gv_set_footprint, gv_score_trajectories*, gv_set_motion_model, gv_rollout*, the rollout getters and
 * gv_control_step*, gv_set_dyn_config, gv_set_moving_objects and gv_score_dynamic* may be called, and so may
 * gv_set_track_config, gv_set_tracks, gv_get_tracks and gv_track_update*; their device work is ordered behind the tick on gv_stream(h), and an upload never
 * overwrites the cloud the tick reads.  What gv_tick_wait returns reflects the handle's state at gv_tick_enqueue: the
 * cloud (its size decides pca_empty) and the camera->base transform of the poses and base points; a transform or height
 * band set in between applies from the next tick on.  (tests/test_gpu_tick.py) */
int gv_tick_enqueue(gv_handle h, const gv_tick_desc *d);
int gv_tick_wait(gv_handle h, gv_tick_result *r);
int gv_tick(gv_handle h, const gv_tick_desc *d, gv_tick_result *r);   /* = enqueue + wait */

/* ------------------------------------------------ raw stream / timing hooks -- */
/* The public HIP stream of the handle (hipStream_t as void*), for callers that record their own
 * events around gv_frame_enqueue or consume the grid layers on the device: every frame's grid pass
 * runs on it, behind the frame's other kernels. */
void *gv_stream(gv_handle h);
/* Device pointers of the resident grid for consumers on the device (stream-ordered behind a frame on gv_stream):
 * the packed OccupancyGrid.data bytes (G int8, `OccupancyGrid.data` order) and the two float layers (G floats,
 * grid_map order).  Any of the three may be null.  Read-only for the caller: the grid pass leaves cells alone whose
 * log-odds it does not change, so writing through these pointers puts the three layers out of step with each other
 * until gv_reset or gv_set_log_odds. */
int gv_device_layers(gv_handle h, int8_t **occ_i8, float **log_odds, float **occupancy);
/* Time `frames` back-to-back gv_frame_enqueue calls with HIP events on the
 * handle's stream; *ms_total is the elapsed device time. */
int gv_time_frames(gv_handle h, int32_t frames, float *ms_total);
/* Per-stage device time of one frame, averaged over `frames` serial frames.  On the tile path
 * the four kernels carry their own start / end events (dispatch-packet timestamps); other stages are
 * intervals between HIP events recorded on the handle's stream.
 * stage_ms has GV_NUM_STAGES entries. */
enum {
  GV_STAGE_DETECTIONS = 0,   /* vision-orientation geometry + rectangles       */
  GV_STAGE_POINTS = 1,       /* transform + cell index + ray ends + bbox test, keys partitioned by tile */
  GV_STAGE_RAY_COMPACT = 2,  /* per-tile hit histogram -> hits[] + ray-end bitmaps */
  GV_STAGE_RAY_MARCH = 3,    /* Bresenham free-space march                     */
  GV_STAGE_FINALIZE = 4,     /* decay/rect/hit-miss/clamp/sigmoid/int8 pass    */
  GV_NUM_STAGES = 5
};
int gv_time_frame_stages(gv_handle h, int32_t frames, float *stage_ms);

/* ---------------------------------------- [EXTENSION] multi-GPU (RCCL/xGMI) -- */
/* One large frame sharded by POINTS over `world` ranks: every rank bins its
 * slice into private ray-end bitmaps; the bitmaps are OR-ed across ranks (all-to-all of slices +
 * local OR + all-gather); every rank runs every world-th workgroup of the ray stage; the free-cell
 * bitmaps are OR-ed by row band (rank r receives band r), each rank finalises its band and the
 * packed int8 bands are broadcast.  After the frame log_odds/occupancy are valid for the rank's own
 * band only (gv_comm_band), the int8 grid everywhere.  With GV_FRAME_KEEP_COUNTS the hit counts are
 * reduce-scattered by band: gv_get_hits then holds the SUMMED counts at the rank's band
 * and this rank's partial counts elsewhere; gv_get_miss returns GV_ERR_STATE.
 * gv_comm_unique_id fills a 128-byte RCCL id on rank 0 (broadcast it by any
 * means); gv_comm_init joins the communicator (and creates the handle's exchange stream). */
int gv_comm_unique_id(uint8_t id_out[128]);
int gv_comm_init(gv_handle h, const uint8_t id[128], int32_t rank, int32_t world);
int gv_comm_destroy(gv_handle h);
/* What RCCL itself says about the communicator (ncclCommCount / ncclCommUserRank / ncclCommCuDevice): the number of
 * ranks that joined, this rank, and the device it runs on -- bench.py prints them, so that a scaling line proves that
 * N ranks on N devices took part.  GV_ERR_STATE before gv_comm_init. */
int gv_comm_info(gv_handle h, int32_t *n_ranks, int32_t *rank, int32_t *device);
/* Sharded frame, asynchronous: the counterpart of gv_frame_enqueue (same detection sets, same back-pressure of
 * four frames in flight on two lanes, results on the public stream behind it) for a resident cloud that is this rank's
 * slice.  Binning, sector share and band packing run on the frame's lane, the RCCL exchanges on the handle's
 * exchange stream, the band's grid pass on the public stream: frame f's exchanges overlap frame f+1's binning.
 * Collective: every rank of the communicator must enqueue the same sequence of frames. */
int gv_frame_enqueue_sharded(gv_handle h);
/* = gv_frame_set_detections + gv_frame_enqueue_sharded + gv_synchronize */
int gv_process_frame_sharded(gv_handle h, const gv_frame_desc *desc);
/* Device time of the six steps of the sharded frame -- binning, ends exchange, sector share + packing, free-band
 * exchange, band grid pass, band broadcast (+ count reduce) -- averaged over `frames` frames run one at a time.
 * Collective. */
int gv_time_frame_sharded_stages(gv_handle h, int32_t frames, float stage_ms[6]);
/* Pure host helpers (no handle, no GPU): rows [*y0, *y1) rank `rank` of `world` finalises in a grid of `ny` rows
 * (whole 64-row blocks of the grid padded to 128 rows, clipped to ny), and the words of one of the `world`
 * equal slices a bitmap of `words` words is exchanged in.  The multi-rank CPU tests use the same functions. */
int gv_shard_band_rows(int32_t rank, int32_t world, int32_t ny, int32_t *y0, int32_t *y1);
int64_t gv_shard_slice_words(int64_t words, int32_t world);
/* Band of cells [begin,end) this rank finalises (linear cell indices): whole 64-row blocks. */
int gv_comm_band(gv_handle h, int64_t *begin, int64_t *end);
#ifdef __cplusplus
}
#endif
#include "gridvision_hip_path.h"
#endif /* GRIDVISION_HIP_H_ */
