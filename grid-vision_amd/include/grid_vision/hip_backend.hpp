// grid_vision/hip_backend.hpp -- C++ host-side mirror of the reference's per-frame
// interface, implemented over the C ABI of libgridvision_hip.so (include/gridvision_hip.h).
//
// Same names, argument meaning and error behaviour as the reference classes/namespaces:
//   OccupancyGridMap            include/grid_vision/occupancy_grid.hpp:13-40
//   namespace cloud_detections  include/grid_vision/cloud_detections.hpp:27-56
//   namespace object_detection  include/grid_vision/object_detection.hpp:34-67 (post-processing)
//   VisionOrientation           include/grid_vision/vision_orientation.hpp:41-99 (geometry half)
// ROS message types are replaced by layout-compatible PODs; on a ROS2 machine the node shim
// converts.  Errors: the reference logs and carries on; here
// every call returns/raises gv::Error only for programming errors and HIP/RCCL failures,
// out-of-map rectangles/points are silently skipped exactly like the reference.
#pragma once

#include <cstdint>
#include <stdexcept>
#include <string>
#include <tuple>
#include <cstring>
#include <vector>

#include "../../../include/gridvision_hip.h"
#include "../../../include/gridvision_hip_match.h"

namespace gv {

struct Error : std::runtime_error {
  int code;
  Error(int c, const std::string &what) : std::runtime_error(what), code(c) {}
};

inline void check(int rc, gv_handle h, const char *where)
{
  if (rc != GV_OK) throw Error(rc, std::string(where) + ": status " + std::to_string(rc) + " " + (h ? gv_last_error(h) : ""));
}

}  // namespace gv

// ObjectClass / BoundingBox  object_detection.hpp:12-32
enum class ObjectClass : int32_t {
  BIKE = 0, MOTORBIKE = 1, PERSON = 2, TRAFFIC_LIGHT_GREEN = 3, TRAFFIC_LIGHT_ORANGE = 4, TRAFFIC_LIGHT_RED = 5,
  TRAFFIC_SIGN_30 = 6, TRAFFIC_SIGN_60 = 7, TRAFFIC_SIGN_90 = 8, VEHICLE = 9, UNKNOWN = 10
};
using BoundingBox = gv_bbox;          // {x_min,y_min,x_max,y_max:f64, confidence:f32, label:i32}
using LShapePose = gv_lshape_pose;    // geometry_msgs/Pose + length, width, height
using CAMParams = gv_cam_params;      // vision_orientation.hpp:18-25

namespace geometry {
struct Point { double x, y, z; };
}

// One context = one GPU + one stream + one resident grid (the node owns exactly one).
class GridVisionContext {
public:
  GridVisionContext(uint8_t grid_x, uint8_t grid_y, double resolution, const CAMParams &cam, int device = -1)
  {
    gv::check(gv_create(&h_, grid_x, grid_y, resolution, &cam, device), nullptr, "gv_create");
  }
  ~GridVisionContext()
  {
    if (h_) gv_destroy(h_);
    for (auto &st : stage_)
      if (st.p) gv_host_free(st.p);
  }
  GridVisionContext(const GridVisionContext &) = delete;
  GridVisionContext &operator=(const GridVisionContext &) = delete;
  gv_handle handle() const { return h_; }

  // tf lookups of the node (grid_vision_node.cpp:290,348,371) handed over as transforms
  void setTransforms(const gv_transform *camera_from_lidar, const gv_transform *base_from_camera,
                     const gv_transform *base_from_lidar)
  {
    gv::check(gv_set_transforms(h_, camera_from_lidar, base_from_camera, base_from_lidar), h_, "gv_set_transforms");
  }
  // GridVision::cloudCallback (grid_vision_node.cpp:103-106)
  void setCloud(const float *x, const float *y, const float *z, size_t n)
  {
    gv::check(gv_cloud_upload_xyz(h_, x, y, z, n), h_, "gv_cloud_upload_xyz");
    n_ = n;
  }
  void setCloudPointCloud2(const uint8_t *data, size_t n, uint32_t point_step, uint32_t ox, uint32_t oy, uint32_t oz)
  {
    gv::check(gv_cloud_upload_pointcloud2(h_, data, n, point_step, ox, oy, oz), h_, "gv_cloud_upload_pointcloud2");
    n_ = n;
  }
  // Streaming form: the copy of the next cloud is enqueued on the handle's copy stream and overlaps the frames in
  // flight (three resident clouds rotate).  The ROS message is released when the callback returns, so the
  // bytes are staged in the context's own pinned buffers first (two, alternating); the host never waits for the
  // device here.
  void setCloudPointCloud2Async(const uint8_t *data, size_t n, uint32_t point_step, uint32_t ox, uint32_t oy, uint32_t oz)
  {
    const size_t bytes = n * (size_t)point_step;
    Staging &st = stage_[flip_ ^= 1];
    if (bytes > st.cap) {
      gv::check(gv_cloud_upload_wait(h_), h_, "gv_cloud_upload_wait");   // the old buffer may still be in flight
      if (st.p) gv_host_free(st.p);
      st.p = nullptr;
      gv::check(gv_host_alloc(&st.p, bytes + bytes / 8 + 4096), nullptr, "gv_host_alloc");
      st.cap = bytes + bytes / 8 + 4096;
    }
    // The copy that last read this buffer was enqueued two clouds ago.  At the node's 20 Hz it has long
    // finished and the wait returns at once; behind a held-back copy stream (back-pressure, a burst of clouds)
    // it keeps the bytes under an in-flight DMA unchanged, as the header demands.
    if (st.submitted) gv::check(gv_cloud_upload_wait(h_), h_, "gv_cloud_upload_wait");
    std::memcpy(st.p, data, bytes);
    st.submitted = true;
    gv::check(gv_cloud_upload_pointcloud2_async(h_, static_cast<const uint8_t *>(st.p), n, point_step, ox, oy, oz), h_,
              "gv_cloud_upload_pointcloud2_async");
    n_ = n;
  }
  // the fused frame without a host wait (gv_frame_set_detections + gv_frame_enqueue); results through
  // occupancyGridAsync / gv_synchronize
  void enqueueFrame(const gv_frame_desc &d)
  {
    gv::check(gv_frame_set_detections_async(h_, &d), h_, "gv_frame_set_detections_async");
    gv::check(gv_frame_enqueue(h_), h_, "gv_frame_enqueue");
  }
  void synchronize() { gv::check(gv_synchronize(h_), h_, "gv_synchronize"); }
  size_t cloudSize() const { return n_; }

  // The device half of one timerCallback as a single batch (gv_tick_enqueue / gv_tick_wait): kNN depth of the static
  // boxes, poses of the dynamic ones (orientation-network geometry or cloud PCA), rectangles, map update, int8 pack.
  // tickWait is the tick's only host wait.
  struct TickOutput {
    std::vector<BoundingBox> static_bboxes;
    std::vector<float> depths;                   // :176-177
    std::vector<geometry::Point> base_points;    // :180
    std::vector<LShapePose> poses;               // base frame (:204, :227)
    bool pca_empty = false;                      // computeBBoxPose returned {} (:307-309)
  };
  void tickEnqueue(const std::vector<BoundingBox> &bboxes, uint32_t flags, uint16_t k_near, const float *orient = nullptr,
                   const float *conf = nullptr, const float *dims = nullptr, int32_t n_net = 0, int8_t *grid_out = nullptr)
  {
    gv_tick_desc d{};
    d.flags = flags;
    d.bboxes = bboxes.data();
    d.n_bboxes = (int32_t)bboxes.size();
    d.orient = orient; d.conf = conf; d.dims = dims;
    d.n_net = n_net;
    d.k_near = k_near;
    d.grid_out = grid_out;
    tick_n_ = bboxes.size();
    gv::check(gv_tick_enqueue(h_, &d), h_, "gv_tick_enqueue");
  }
  TickOutput tickWait()
  {
    TickOutput o;
    const size_t cap = tick_n_ ? tick_n_ : 1;
    o.static_bboxes.resize(cap); o.depths.resize(cap); o.base_points.resize(cap); o.poses.resize(cap);
    gv_tick_result r{};
    r.static_bboxes = o.static_bboxes.data();
    r.depths = o.depths.data();
    r.base_points_xyz = reinterpret_cast<double *>(o.base_points.data());
    r.poses = o.poses.data();
    gv::check(gv_tick_wait(h_, &r), h_, "gv_tick_wait");
    o.static_bboxes.resize((size_t)r.n_static); o.depths.resize((size_t)r.n_static); o.base_points.resize((size_t)r.n_static);
    o.poses.resize((size_t)r.n_poses);
    o.pca_empty = r.pca_empty != 0;
    return o;
  }

private:
  struct Staging {
    void *p = nullptr;
    size_t cap = 0;
    bool submitted = false;   // a copy out of this buffer has been enqueued
  };
  Staging stage_[2];
  int flip_ = 0;
  gv_handle h_ = nullptr;
  size_t n_ = 0;
  size_t tick_n_ = 0;
};

// OccupancyGridMap  occupancy_grid.hpp:13-40.  grid_map_ is the device-resident grid.
class OccupancyGridMap {
public:
  explicit OccupancyGridMap(GridVisionContext &ctx) : ctx_(ctx)
  {
    int32_t nx, ny;
    gv::check(gv_grid_geometry(ctx_.handle(), &nx, &ny, nullptr, nullptr), ctx_.handle(), "gv_grid_geometry");
    cells_ = (size_t)nx * ny;
  }
  // updateMap(GridMap&)  occupancy_grid.cpp:16-31
  void updateMap() { gv::check(gv_update_map(ctx_.handle()), ctx_.handle(), "gv_update_map"); }
  // updateMap(GridMap&, vector<LShapePose>)  :65-105
  void updateMap(const std::vector<LShapePose> &bboxes_pose)
  {
    gv::check(gv_update_map_poses(ctx_.handle(), bboxes_pose.data(), (int32_t)bboxes_pose.size()), ctx_.handle(),
              "gv_update_map_poses");
  }
  // updateMap(GridMap&, vector<Point>, vector<BoundingBox>)  :33-63
  void updateMap(const std::vector<geometry::Point> &base_points, const std::vector<BoundingBox> &bboxes)
  {
    gv::check(gv_update_map_points(ctx_.handle(), reinterpret_cast<const double *>(base_points.data()), bboxes.data(),
                                   (int32_t)bboxes.size()), ctx_.handle(), "gv_update_map_points");
  }
  // [EXTENSION] X3 grid_map's GridMap::move() for the base-frame grid: motion = base_prev <- base_now (tf2's
  // time-travel lookup through odom).  Asynchronous on the context's stream, like the frame calls.
  gv_grid_move_info moveMap(const gv_transform &motion)
  {
    gv_grid_move_info info{};
    gv::check(gv_grid_move(ctx_.handle(), &motion, &info), ctx_.handle(), "gv_grid_move");
    return info;
  }
  // [EXTENSION] X4 obstacle height band of the lidar map update (base-frame z, metres; rounded to float): below
  // ground_z a return is ground -- it clears free space when ground_clears --, above max_obstacle_z it is ignored.
  // Applies to the frames and ticks enqueued afterwards.
  void setHeightBand(double ground_z, double max_obstacle_z, bool ground_clears = true)
  {
    const gv_height_band b{(float)ground_z, (float)max_obstacle_z, ground_clears ? 1 : 0};
    gv::check(gv_set_height_band(ctx_.handle(), &b), ctx_.handle(), "gv_set_height_band");
  }
  void clearHeightBand() { gv::check(gv_set_height_band(ctx_.handle(), nullptr), ctx_.handle(), "gv_set_height_band"); }
  // [EXTENSION] X6 inflated costmap layer (nav2's InflationLayer with an exact distance transform): configure once,
  // inflate() after a map update (asynchronous on the context's stream), getCostmap() in OccupancyGrid.data order.
  void setInflation(const gv_inflation &cfg) { gv::check(gv_set_inflation(ctx_.handle(), &cfg), ctx_.handle(), "gv_set_inflation"); }
  void clearInflation() { gv::check(gv_set_inflation(ctx_.handle(), nullptr), ctx_.handle(), "gv_set_inflation"); }
  void inflate() { gv::check(gv_inflate(ctx_.handle()), ctx_.handle(), "gv_inflate"); }
  std::vector<uint8_t> getCostmap() const
  {
    std::vector<uint8_t> data(cells_);
    gv::check(gv_get_costmap(ctx_.handle(), data.data()), ctx_.handle(), "gv_get_costmap");
    return data;
  }
  // [EXTENSION] X7 trajectory scoring against the costmap of the last inflate(): configure the footprint once, then
  // score K trajectories of P poses (poses[K * P * 3]: x, y, yaw in the grid's frame).  One record per trajectory;
  // pose_cost, when given, receives the K * P pose costs.  Synchronous; a controller that must not wait calls
  // gv_score_trajectories_async with pinned buffers on the context's stream.
  void setFootprint(const gv_footprint &fp) { gv::check(gv_set_footprint(ctx_.handle(), &fp), ctx_.handle(), "gv_set_footprint"); }
  void clearFootprint() { gv::check(gv_set_footprint(ctx_.handle(), nullptr), ctx_.handle(), "gv_set_footprint"); }
  std::vector<gv_traj_score> scoreTrajectories(const std::vector<float> &poses, int32_t K, int32_t P,
                                               std::vector<uint8_t> *pose_cost = nullptr)
  {
    if (K < 0 || P < 1 || poses.size() < (size_t)K * (size_t)P * 3) throw gv::Error(GV_ERR_BAD_ARG, "scoreTrajectories: poses is K * P * 3");
    std::vector<gv_traj_score> scores((size_t)K);
    if (pose_cost) pose_cost->resize((size_t)K * (size_t)P);
    if (K == 0) return scores;
    gv::check(gv_score_trajectories(ctx_.handle(), poses.data(), K, P, pose_cost ? GV_TRAJ_KEEP_POSE_COST : 0u, scores.data(),
                                    pose_cost ? pose_cost->data() : nullptr), ctx_.handle(), "gv_score_trajectories");
    return scores;
  }
  // [EXTENSION] X9 goal / path distance field over the costmap of the last inflate(): configure once, solve from goal
  // or path seeds (seeds_xy[S * 2] in the grid's frame; waits until the field is complete on the device), then sample
  // it along the same poses scoreTrajectories takes.  navField() reads the G values back.
  void setNavConfig(const gv_nav_config &cfg) { gv::check(gv_set_nav_config(ctx_.handle(), &cfg), ctx_.handle(), "gv_set_nav_config"); }
  void clearNavConfig() { gv::check(gv_set_nav_config(ctx_.handle(), nullptr), ctx_.handle(), "gv_set_nav_config"); }
  gv_nav_info solveNavField(const std::vector<float> &seeds_xy)
  {
    gv_nav_info info{};
    gv::check(gv_nav_field(ctx_.handle(), seeds_xy.data(), (int32_t)(seeds_xy.size() / 2), &info), ctx_.handle(), "gv_nav_field");
    return info;
  }
  std::vector<uint32_t> navField()
  {
    int32_t nx = 0, ny = 0;
    gv::check(gv_grid_geometry(ctx_.handle(), &nx, &ny, nullptr, nullptr), ctx_.handle(), "gv_grid_geometry");
    std::vector<uint32_t> out((size_t)nx * (size_t)ny);
    gv::check(gv_get_nav_field(ctx_.handle(), out.data()), ctx_.handle(), "gv_get_nav_field");
    return out;
  }
  std::vector<gv_nav_score> scoreNav(const std::vector<float> &poses, int32_t K, int32_t P)
  {
    if (K < 0 || P < 1 || poses.size() < (size_t)K * (size_t)P * 3) throw gv::Error(GV_ERR_BAD_ARG, "scoreNav: poses is K * P * 3");
    std::vector<gv_nav_score> scores((size_t)K);
    if (K == 0) return scores;
    gv::check(gv_score_nav(ctx_.handle(), poses.data(), K, P, 0u, scores.data()), ctx_.handle(), "gv_score_nav");
    return scores;
  }
  // [EXTENSION] X10 the controller's loop on the device: configure the motion model once, roll K control sequences out
  // into the context's resident pose buffer (controls[K * P * C], or [K * C] held for P steps when constant; C = 2 for
  // GV_MOTION_DIFF, 3 for GV_MOTION_OMNI), then controlStep(): both samplers over the resident rollout, the records
  // combined with integer weights, the best admissible trajectory selected -- 16 bytes back.  totals, when given,
  // receives the K totals.  Synchronous; a controller that must not wait calls the _async forms with pinned buffers.
  void setMotionModel(const gv_motion_model &m) { gv::check(gv_set_motion_model(ctx_.handle(), &m), ctx_.handle(), "gv_set_motion_model"); }
  void rollout(const double start[3], const std::vector<float> &controls, int32_t K, int32_t P, bool constant = false)
  {
    gv::check(gv_rollout(ctx_.handle(), start, controls.data(), K, P, constant ? (uint32_t)GV_ROLLOUT_CONSTANT : 0u), ctx_.handle(),
              "gv_rollout");
  }
  std::vector<float> getRollout()
  {
    float *dev = nullptr;
    int32_t K = 0, P = 0;
    gv::check(gv_device_rollout(ctx_.handle(), &dev, &K, &P), ctx_.handle(), "gv_device_rollout");
    std::vector<float> poses((size_t)K * (size_t)P * 3);
    gv::check(gv_get_rollout(ctx_.handle(), poses.data()), ctx_.handle(), "gv_get_rollout");
    return poses;
  }
  gv_control_result controlStep(const gv_critic_weights &w, std::vector<uint64_t> *totals = nullptr)
  {
    gv_control_result r{};
    if (totals) {
      float *dev = nullptr;
      int32_t K = 0;
      gv::check(gv_device_rollout(ctx_.handle(), &dev, &K, nullptr), ctx_.handle(), "gv_device_rollout");
      totals->resize((size_t)K);
    }
    gv::check(gv_control_step(ctx_.handle(), &w, totals ? (uint32_t)GV_CONTROL_KEEP_TOTALS : 0u, &r, totals ? totals->data() : nullptr),
              ctx_.handle(), "gv_control_step");
    return r;
  }
  // [EXTENSION] X11 MPPI with its two ends on the device: configure once, give the first nominal sequence
  // (nominal[P * C], C of the motion model in force), then one mppiCycle() per iteration: K control sequences sampled
  // around the resident nominal, rolled out, scored and selected as controlStep() does, and the nominal replaced by
  // their softmax average, which the call returns.  Synchronous, like controlStep().
  void setMppi(const gv_mppi_config &c) { gv::check(gv_set_mppi(ctx_.handle(), &c), ctx_.handle(), "gv_set_mppi"); }
  void setMppiNominal(const std::vector<float> &nominal, int32_t P)
  {
    gv::check(gv_mppi_set_nominal(ctx_.handle(), nominal.data(), P), ctx_.handle(), "gv_mppi_set_nominal");
    nominal_floats_ = nominal.size();
  }
  std::vector<float> mppiCycle(const double start[3], int32_t K, uint64_t seed, uint64_t iteration, const gv_critic_weights &w,
                               gv_control_result *result = nullptr, bool shift = false)
  {
    gv_control_result r{};
    std::vector<float> nominal(nominal_floats_);
    gv::check(gv_mppi_cycle(ctx_.handle(), start, K, seed, iteration, shift ? (uint32_t)GV_MPPI_SHIFT : 0u, &w, 0u, &r, nullptr,
                            nominal.data()),
              ctx_.handle(), "gv_mppi_cycle");
    if (result) *result = r;
    return nominal;
  }
  // [EXTENSION] X12 rate and turning-radius limits on the sampled controls and the control-cost weight gamma of the
  // mppiCycle() calls that follow: call it every control cycle with the measured velocity in u_prev.  A car-like base
  // sets min_turn_radius under GV_MOTION_DIFF.  clearMppiLimits() turns them off.
  void setMppiLimits(const gv_mppi_limits &l) { gv::check(gv_set_mppi_limits(ctx_.handle(), &l), ctx_.handle(), "gv_set_mppi_limits"); }
  void clearMppiLimits() { gv::check(gv_set_mppi_limits(ctx_.handle(), nullptr), ctx_.handle(), "gv_set_mppi_limits"); }
  // the control costs g_k of the last mppiCycle() that ran with gamma > 0 (K values)
  std::vector<double> mppiControlCosts(int32_t K) const
  {
    std::vector<double> g((size_t)K);
    gv::check(gv_get_mppi_control_costs(ctx_.handle(), g.data()), ctx_.handle(), "gv_get_mppi_control_costs");
    return g;
  }
  // [EXTENSION] X13 predicted moving objects: the dynamic boxes of a tick (LShapePose) with a velocity each.  With a
  // configuration set, controlStep() and mppiCycle() also score the resident rollout against them, each pose at its own
  // time; scoreDynamic() is the sampler alone.  clearDynConfig() turns it off.
  void setDynConfig(const gv_dyn_config &c) { gv::check(gv_set_dyn_config(ctx_.handle(), &c), ctx_.handle(), "gv_set_dyn_config"); }
  void clearDynConfig() { gv::check(gv_set_dyn_config(ctx_.handle(), nullptr), ctx_.handle(), "gv_set_dyn_config"); }
  void setMovingObjects(const std::vector<gv_moving_object> &objs)
  {
    gv::check(gv_set_moving_objects(ctx_.handle(), objs.data(), (int32_t)objs.size()), ctx_.handle(), "gv_set_moving_objects");
  }
  std::vector<gv_dyn_score> scoreDynamic(const std::vector<float> &poses, int32_t K, int32_t P)
  {
    std::vector<gv_dyn_score> scores((size_t)K);
    gv::check(gv_score_dynamic(ctx_.handle(), poses.data(), K, P, 0u, scores.data(), nullptr), ctx_.handle(), "gv_score_dynamic");
    return scores;
  }
  // [EXTENSION] X14 the tracker that gives those objects their identity and velocity: trackUpdate() associates the
  // boxes of a tick with the resident tracks, filters position and velocity and, with feed, makes the confirmed tracks
  // the moving objects of the scoring calls that follow, without the set crossing the host.  motion is moveMap()'s
  // argument for the same interval; without it the velocities are relative to the vehicle.
  void setTrackConfig(const gv_track_config &c) { gv::check(gv_set_track_config(ctx_.handle(), &c), ctx_.handle(), "gv_set_track_config"); }
  void clearTrackConfig() { gv::check(gv_set_track_config(ctx_.handle(), nullptr), ctx_.handle(), "gv_set_track_config"); }
  void setTracks(const std::vector<gv_track> &tracks, uint32_t next_id)
  {
    gv::check(gv_set_tracks(ctx_.handle(), tracks.data(), (int32_t)tracks.size(), next_id), ctx_.handle(), "gv_set_tracks");
  }
  std::vector<gv_track> getTracks(uint32_t *next_id = nullptr)
  {
    std::vector<gv_track> t(128);
    int32_t n = 0;
    gv::check(gv_get_tracks(ctx_.handle(), t.data(), 128, &n, next_id), ctx_.handle(), "gv_get_tracks");
    t.resize((size_t)n);
    return t;
  }
  // enqueued on the context's stream, no host wait; dets is free on return
  void trackUpdateAsync(const std::vector<LShapePose> &dets, double dt, const gv_transform *motion, bool feed)
  {
    gv::check(gv_track_update_async(ctx_.handle(), dets.data(), (int32_t)dets.size(), dt, motion, feed ? GV_TRACK_FEED_DYNAMIC : 0u,
                                    nullptr, nullptr),
              ctx_.handle(), "gv_track_update_async");
  }
  // [EXTENSION] X15: the detections are the list the last tickEnqueue with GV_TICK_KEEP_DETS leaves on the device
  // (GV_TRACK_TICK_DETS), read in place behind the tick; the tick may still be pending
  void trackUpdateFromTickAsync(double dt, const gv_transform *motion, bool feed)
  {
    gv::check(gv_track_update_async(ctx_.handle(), nullptr, 0, dt, motion, GV_TRACK_TICK_DETS | (feed ? GV_TRACK_FEED_DYNAMIC : 0u),
                                    nullptr, nullptr),
              ctx_.handle(), "gv_track_update_async");
  }
  gv_track_info trackUpdate(const std::vector<LShapePose> &dets, double dt, const gv_transform *motion, bool feed,
                            std::vector<gv_track> *tracks = nullptr)
  {
    gv_track_info info{};
    std::vector<gv_track> t(128);
    gv::check(gv_track_update(ctx_.handle(), dets.data(), (int32_t)dets.size(), dt, motion, feed ? GV_TRACK_FEED_DYNAMIC : 0u, &info,
                              t.data()),
              ctx_.handle(), "gv_track_update");
    t.resize((size_t)info.n_tracks);
    if (tracks) *tracks = std::move(t);
    return info;
  }
  // the host twin (no handle): tracks (the live records in ascending slot order) and next_id in and out; objs, when
  // given, receives the exported objects
  static gv_track_info trackStep(const gv_track_config &c, std::vector<gv_track> &tracks, uint32_t &next_id, const std::vector<LShapePose> &dets,
                                 double dt, const gv_transform *motion, std::vector<gv_moving_object> *objs = nullptr)
  {
    gv_track_info info{};
    int32_t n = (int32_t)tracks.size(), n_objs = 0;
    tracks.resize(128);
    std::vector<gv_moving_object> o(128);
    gv::check(gv_track_step(&c, tracks.data(), &n, &next_id, dets.data(), (int32_t)dets.size(), dt, motion, &info, o.data(), &n_objs), nullptr,
              "gv_track_step");
    tracks.resize((size_t)n);
    o.resize((size_t)n_objs);
    if (objs) *objs = std::move(o);
    return info;
  }
  // [EXTENSION] X16 scan-to-costmap matching (gridvision_hip_match.h): configure once, then matchScan() correlates the
  // resident cloud with the costmap of the last inflate() around a guess and returns the best pose; matchMotion() is
  // that pose as the motion of gridMove() and trackUpdate().  scores, when given, receives the NT * NY * NX volume.
  void setMatchConfig(const gv_match_config &c)
  {
    gv::check(gv_set_match_config(ctx_.handle(), &c), ctx_.handle(), "gv_set_match_config");
    match_scores_ = (size_t)(2 * c.wt + 1) * (size_t)(2 * c.wy + 1) * (size_t)(2 * c.wx + 1);
  }
  void clearMatchConfig()
  {
    gv::check(gv_set_match_config(ctx_.handle(), nullptr), ctx_.handle(), "gv_set_match_config");
    match_scores_ = 0;
  }
  gv_match_result matchScan(const gv_match_guess &guess, std::vector<uint32_t> *scores = nullptr)
  {
    gv_match_result r{};
    if (scores) scores->assign(match_scores_ ? match_scores_ : 1, 0u);
    gv::check(gv_match_scan(ctx_.handle(), &guess, scores ? (uint32_t)GV_MATCH_KEEP_SCORES : 0u, &r, scores ? scores->data() : nullptr),
              ctx_.handle(), "gv_match_scan");
    return r;
  }
  // result (and scores, NT * NY * NX values, or null) stay the caller's until the context's stream has been waited for
  void matchScanAsync(const gv_match_guess &guess, gv_match_result *result, uint32_t *scores = nullptr)
  {
    gv::check(gv_match_scan_async(ctx_.handle(), &guess, scores ? (uint32_t)GV_MATCH_KEEP_SCORES : 0u, result, scores), ctx_.handle(),
              "gv_match_scan_async");
  }
  static gv_transform matchMotion(const gv_match_result &r)
  {
    gv_transform m{};
    gv::check(gv_match_motion(&r, &m), nullptr, "gv_match_motion");
    return m;
  }
  // the host twin (no handle)
  static gv_match_result matchScanHost(uint8_t grid_x, uint8_t grid_y, double resolution, const std::vector<uint8_t> &cost,
                                       const std::vector<float> &x, const std::vector<float> &y, const std::vector<float> &z,
                                       const gv_transform &base_from_lidar, const gv_height_band *band, const gv_match_config &c,
                                       const gv_match_guess &guess, std::vector<uint32_t> *scores = nullptr)
  {
    gv_match_result r{};
    if (scores) scores->assign((size_t)(2 * c.wt + 1) * (size_t)(2 * c.wy + 1) * (size_t)(2 * c.wx + 1), 0u);
    gv::check(gv_match_scan_host(grid_x, grid_y, resolution, cost.data(), x.data(), y.data(), z.data(), x.size(), &base_from_lidar, band,
                                 &c, &guess, scores ? (uint32_t)GV_MATCH_KEEP_SCORES : 0u, &r, scores ? scores->data() : nullptr),
              nullptr, "gv_match_scan_host");
    return r;
  }
  // the host twins (no handle): the chain over controls[K][P][C] in place, e.g. K = 1 for the command to execute; the
  // control costs; the sequential average with them
  static void mppiConstrain(const gv_mppi_limits &l, const gv_motion_model &m, std::vector<float> &controls, int32_t K, int32_t P)
  {
    gv::check(gv_mppi_constrain(&l, &m, controls.data(), K, P), nullptr, "gv_mppi_constrain");
  }
  static std::vector<double> mppiControlCostsHost(const gv_mppi_config &c, const gv_mppi_limits &l, int32_t C, const std::vector<float> &controls,
                                                  const std::vector<float> &nominal, int32_t K, int32_t P, bool shift = false)
  {
    std::vector<double> g((size_t)K);
    gv::check(gv_mppi_control_costs(&c, &l, C, controls.data(), nominal.data(), K, P, shift ? (uint32_t)GV_MPPI_SHIFT : 0u, g.data()), nullptr,
              "gv_mppi_control_costs");
    return g;
  }
  static std::vector<float> mppiAverageCc(const gv_mppi_config &c, int32_t C, const std::vector<float> &controls, const std::vector<uint64_t> &totals,
                                          const std::vector<double> *costs, int32_t K, int32_t P, const std::vector<float> &nominal)
  {
    std::vector<float> out(nominal.size());
    gv::check(gv_mppi_average_cc(&c, C, controls.data(), totals.data(), costs ? costs->data() : nullptr, K, P, nominal.data(), out.data()), nullptr,
              "gv_mppi_average_cc");
    return out;
  }
  // GridMapRosConverter::toOccupancyGrid(map, "occupancy", 0, 1, msg)  grid_vision_node.cpp:270-271
  std::vector<int8_t> toOccupancyGrid(gv_grid_info *info = nullptr) const
  {
    std::vector<int8_t> data(cells_);
    gv::check(gv_to_occupancy_grid(ctx_.handle(), data.data(), info), ctx_.handle(), "gv_to_occupancy_grid");
    return data;
  }
  std::vector<float> layer(const char *name) const   // "log_odds" | "occupancy"
  {
    std::vector<float> v(cells_);
    const bool lo = std::string(name) == "log_odds";
    gv::check(lo ? gv_get_log_odds(ctx_.handle(), v.data()) : gv_get_occupancy(ctx_.handle(), v.data()), ctx_.handle(), name);
    return v;
  }
  size_t cells() const { return cells_; }

private:
  GridVisionContext &ctx_;
  size_t cells_ = 0;
  size_t nominal_floats_ = 0;   // P * C of the nominal given to setMppiNominal
  size_t match_scores_ = 0;     // NT * NY * NX of the configuration given to setMatchConfig
};

namespace cloud_detections {

// transformLidarToCamera  grid_vision_node.hpp:95-97; empty result where the reference returns nullptr
inline bool transformLidarToCamera(GridVisionContext &ctx, std::vector<float> &x, std::vector<float> &y,
                                   std::vector<float> &z)
{
  x.resize(ctx.cloudSize()); y.resize(ctx.cloudSize()); z.resize(ctx.cloudSize());
  const int rc = gv_transform_lidar_to_camera(ctx.handle(), x.data(), y.data(), z.data());
  if (rc == GV_ERR_TF) return false;   // tf lookup failed: the node publishes the stale grid (:160-164)
  gv::check(rc, ctx.handle(), "gv_transform_lidar_to_camera");
  return true;
}

// buildKDTree + computeDepthForBoundingBoxes  cloud_detections.hpp:29-35
inline std::vector<float> computeDepthForBoundingBoxes(GridVisionContext &ctx, const std::vector<BoundingBox> &bboxes,
                                                       uint16_t k = 10)
{
  std::vector<float> depths(bboxes.size(), -1.0f);
  if (!bboxes.empty())
    gv::check(gv_compute_depth_for_bboxes(ctx.handle(), bboxes.data(), (int32_t)bboxes.size(), k, depths.data(), nullptr),
              ctx.handle(), "gv_compute_depth_for_bboxes");
  return depths;
}

// convertPixelsTo3D -> pixelTo3D -> transformPointToBaseFrame  grid_vision_node.cpp:309-359
inline std::vector<geometry::Point> convertPixelsTo3D(GridVisionContext &ctx, const std::vector<BoundingBox> &bboxes,
                                                      const std::vector<float> &depths)
{
  std::vector<geometry::Point> out(bboxes.size());
  if (!bboxes.empty())
    gv::check(gv_convert_pixels_to_3d(ctx.handle(), bboxes.data(), depths.data(), (int32_t)bboxes.size(),
                                      reinterpret_cast<double *>(out.data())), ctx.handle(), "gv_convert_pixels_to_3d");
  return out;
}

// extractCloudPerBBox  cloud_detections.hpp:46-48: bbox id of every point instead of copies
inline std::vector<int32_t> extractCloudPerBBox(GridVisionContext &ctx, const std::vector<BoundingBox> &bboxes,
                                                std::vector<int32_t> *counts = nullptr)
{
  std::vector<int32_t> ids(ctx.cloudSize());
  std::vector<int32_t> cnt(bboxes.size());
  gv::check(gv_extract_cloud_per_bbox(ctx.handle(), bboxes.data(), (int32_t)bboxes.size(), ids.data(), cnt.data()),
            ctx.handle(), "gv_extract_cloud_per_bbox");
  if (counts) *counts = cnt;
  return ids;
}

// segmentGroundPlane  cloud_detections.hpp:40-41: mask of the ground points of the camera-frame cloud
// (empty vector where the reference returns an empty cloud: no plane found)
inline std::vector<uint8_t> segmentGroundPlane(GridVisionContext &ctx, float coeff[4] = nullptr)
{
  std::vector<uint8_t> mask(ctx.cloudSize());
  int64_t m = 0;
  gv::check(gv_segment_ground_plane(ctx.handle(), 0.04, 50, 12345ull, mask.data(), coeff, &m), ctx.handle(),
            "gv_segment_ground_plane");
  if (m == 0) mask.clear();
  return mask;
}

// computeBBoxPose  cloud_detections.hpp:50-52.  remove_ground = true is the reference's flow
// (segmentGroundPlane first, :306-314); false skips the RANSAC step.
inline std::vector<LShapePose> computeBBoxPose(GridVisionContext &ctx, const std::vector<BoundingBox> &bboxes,
                                               bool remove_ground = true)
{
  std::vector<LShapePose> all(bboxes.size()), out;
  std::vector<uint8_t> valid(bboxes.size());
  if (!bboxes.empty()) {
    if (remove_ground) {
      int32_t np = 0;
      gv::check(gv_compute_bbox_pose_ground_removed(ctx.handle(), bboxes.data(), (int32_t)bboxes.size(), all.data(),
                                                    valid.data(), &np), ctx.handle(), "gv_compute_bbox_pose_ground_removed");
      if (np < 0) return out;   // empty segmented cloud: the reference returns {} (:307-309)
    } else
      gv::check(gv_compute_bbox_pose(ctx.handle(), bboxes.data(), (int32_t)bboxes.size(), all.data(), valid.data()),
                ctx.handle(), "gv_compute_bbox_pose");
  }
  for (size_t i = 0; i < all.size(); ++i)
    if (valid[i]) out.push_back(all[i]);   // the reference appends only non-empty clouds (:174-181)
  return out;
}

}  // namespace cloud_detections

namespace object_detection {

// extract_bboxes  object_detection.hpp:48-49 on precomputed detector outputs
inline std::vector<BoundingBox> extract_bboxes(const float *boxes, const float *scores, int num_detections, int num_classes,
                                               double conf_threshold, double iou_threshold, int orig_w, int orig_h,
                                               int resize)
{
  std::vector<BoundingBox> out((size_t)num_detections);
  int32_t n = 0;
  gv::check(gv_extract_bboxes(boxes, scores, num_detections, num_classes, conf_threshold, iou_threshold, orig_w, orig_h,
                              resize, out.data(), &n), nullptr, "gv_extract_bboxes");
  out.resize((size_t)n);
  return out;
}

// GridVision::filterBBoxes  grid_vision_node.cpp:384-403 -> (static, dynamic)
inline std::tuple<std::vector<BoundingBox>, std::vector<BoundingBox>> filterBBoxes(const std::vector<BoundingBox> &bboxes)
{
  std::vector<BoundingBox> st(bboxes.size()), dy(bboxes.size());
  int32_t ns = 0, nd = 0;
  gv::check(gv_filter_bboxes(bboxes.data(), (int32_t)bboxes.size(), st.data(), &ns, dy.data(), &nd), nullptr,
            "gv_filter_bboxes");
  st.resize((size_t)ns);
  dy.resize((size_t)nd);
  return {st, dy};
}

}  // namespace object_detection

// VisionOrientation, geometry half (postProcessOutputs and below, vision_orientation.hpp:90-98)
class VisionOrientation {
public:
  explicit VisionOrientation(GridVisionContext &ctx) : ctx_(ctx) {}
  // orient[nb*4], conf[nb*2], dims[nb*3] are the network outputs runInference copies back (:220-225)
  std::vector<LShapePose> postProcessOutputs(const float *orient, const float *conf, const float *dims,
                                             const std::vector<BoundingBox> &bboxes)
  {
    std::vector<LShapePose> out(bboxes.size());
    int32_t n = 0;
    if (!bboxes.empty())
      gv::check(gv_vision_post_process(ctx_.handle(), orient, conf, dims, bboxes.data(), (int32_t)bboxes.size(), out.data(),
                                       &n), ctx_.handle(), "gv_vision_post_process");
    out.resize((size_t)n);
    return out;
  }
  // GridVision::transformLShapeObjects  grid_vision_node.cpp:525-531
  void transformLShapeObjects(std::vector<LShapePose> &poses)
  {
    gv::check(gv_transform_lshape_objects(ctx_.handle(), poses.data(), (int32_t)poses.size()), ctx_.handle(),
              "gv_transform_lshape_objects");
  }

private:
  GridVisionContext &ctx_;
};
