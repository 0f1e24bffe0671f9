// tick_track_demo.cpp -- [EXTENSION] X15: the tick's dynamic objects reach the tracker without leaving the device.  Two
// objects cross in front of the camera for 8 ticks of 0.1 s (the PCA branch: ground removal, per-box clouds, PCA
// rectangle).  Handle A runs the device path: gv_tick_enqueue with GV_TICK_KEEP_DETS, gv_track_update_async with
// GV_TRACK_TICK_DETS enqueued BEFORE gv_tick_wait.  Handle B runs the host path: gv_tick, then gv_track_update with the
// poses gv_tick_wait returned.  The resident tracks must agree byte for byte after every tick.
// Then, on A: tick -> tracker update (fed to X13) -> gv_mppi_cycle_async as one batch on the handle's stream, with one
// wait for all of it.
// Plain g++ host code over the C ABI and its C++ mirror headers:
//   g++ -std=c++17 -O2 tick_track_demo.cpp -o tick_track_demo -L.. -lgridvision_hip -Wl,-rpath,$PWD/..
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../include/grid_vision/frame_flow.hpp"

static uint64_t sm64(uint64_t &s)
{
  uint64_t z = (s += 0x9E3779B97F4A7C15ull);
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}
static float u01(uint64_t &s) { return (float)(sm64(s) >> 40) * (1.0f / 16777216.0f); }

struct Scene {
  std::vector<float> x, y, z;
  std::vector<BoundingBox> boxes;
};

// tick t of 8: an exact ground plane (lidar z = -1.3) and two clusters of 14 points, 8 and 10 m ahead, behind the centres
// of two 14-pixel boxes that move 34 pixels per tick in opposite directions.  camera <- lidar is x_c = -y_l,
// y_c = 0.4 - z_l, z_c = x_l - 0.3 (the transform below).
static Scene scene(int t)
{
  Scene s;
  uint64_t seed = 100 + (uint64_t)t;
  const double u[2] = {200.0 + 240.0 * t / 7.0, 440.0 - 240.0 * t / 7.0}, v[2] = {120.0, 60.0}, depth[2] = {8.0, 10.0};
  for (int i = 0; i < 2; ++i) {
    const double uc = std::round(u[i]);
    s.boxes.push_back(BoundingBox{uc - 7, v[i] - 7, uc + 7, v[i] + 7, 0.9f, i == 0 ? 9 : 2});
    for (int k = 0; k < 14; ++k) {
      const double zc = depth[i] + 0.3 * (u01(seed) - 0.5);
      const double xc = (uc - 320.0) / 320.0 * zc + 0.12 * (u01(seed) - 0.5), yc = (v[i] - 240.0) / 320.0 * zc + 0.12 * (u01(seed) - 0.5);
      s.x.push_back((float)(zc + 0.3)); s.y.push_back((float)(-xc)); s.z.push_back((float)(0.4 - yc));
    }
  }
  uint64_t gs = 5;
  for (int k = 0; k < 3000; ++k) {
    s.x.push_back(2.f + 28.f * u01(gs)); s.y.push_back(-10.f + 20.f * u01(gs)); s.z.push_back(-1.3f);
  }
  for (int k = 0; k < 30; ++k) {   // clutter behind the camera, off the plane
    s.x.push_back(-6.f + 3.f * u01(gs)); s.y.push_back(-2.f + 4.f * u01(gs)); s.z.push_back(u01(gs));
  }
  return s;
}

int main()
{
  try {
    const CAMParams cam{224, 224, 480, 640, 320.f, 320.f, 320.f, 240.f};
    GridVisionContext ctx_a(50, 20, 0.1, cam), ctx_b(50, 20, 0.1, cam);
    OccupancyGridMap grid_a(ctx_a), grid_b(ctx_b);
    const gv_transform cam_lidar{0.5, -0.5, 0.5, 0.5, 0.0, 0.4, -0.3};
    const gv_transform base_cam{0.5, -0.5, 0.5, -0.5, 0.3, 0.0, 2.2};
    const gv_transform base_lidar{0, 0, 0, 1, 0, 0, 1.8};
    const gv_track_config cfg{2.0, 2.0, 0.3, 5.0, 0.3, 2, 3, 0};
    gv_dyn_config dyn{};
    dyn.n_circles = 1; dyn.radius = 0.4; dyn.influence_radius = 2.0; dyn.cost_scaling_factor = 2.0; dyn.quantum = 0.05;
    dyn.t0 = 0.2; dyn.dt = 0.2; dyn.collision_cost = 253; dyn.w_sum = 1;
    for (GridVisionContext *c : {&ctx_a, &ctx_b}) c->setTransforms(&cam_lidar, &base_cam, &base_lidar);
    for (OccupancyGridMap *g : {&grid_a, &grid_b}) {
      g->setTrackConfig(cfg);
      g->setDynConfig(dyn);
    }

    const double dt = 0.1;
    bool agree = true;
    size_t n_tracks = 0;
    for (int t = 0; t < 8; ++t) {
      const Scene s = scene(t);
      ctx_a.setCloud(s.x.data(), s.y.data(), s.z.data(), s.x.size());
      ctx_b.setCloud(s.x.data(), s.y.data(), s.z.data(), s.x.size());
      // device path: the update is enqueued from the tick's list before the tick's wait
      ctx_a.tickEnqueue(s.boxes, GV_TICK_KEEP_DETS, 4);
      grid_a.trackUpdateFromTickAsync(dt, nullptr, true);
      const GridVisionContext::TickOutput out_a = ctx_a.tickWait();
      // host path: the poses come up, and go down again as host detections
      ctx_b.tickEnqueue(s.boxes, 0u, 4);
      const GridVisionContext::TickOutput out_b = ctx_b.tickWait();
      grid_b.trackUpdate(out_b.poses, dt, nullptr, true);
      uint32_t id_a = 0, id_b = 0;
      const std::vector<gv_track> ta = grid_a.getTracks(&id_a), tb = grid_b.getTracks(&id_b);
      const bool same = ta.size() == tb.size() && id_a == id_b && out_a.poses.size() == out_b.poses.size() &&
                        (ta.empty() || std::memcmp(ta.data(), tb.data(), ta.size() * sizeof(gv_track)) == 0);
      agree = agree && same;
      n_tracks = ta.size();
      std::printf("tick %d: %zu poses, %zu tracks, device path %s the host path\n", t, out_b.poses.size(), ta.size(),
                  same ? "equals" : "DIFFERS FROM");
      if (t == 7)
        for (const gv_track &k : ta)
          std::printf("track id %u hits %d at (%.2f, %.2f) velocity (%.2f, %.2f)\n", k.id, k.hits, k.x, k.y, k.vx, k.vy);
    }
    std::printf("%s\n", agree ? "tracks agree on every tick" : "TRACKS DISAGREE");

    // tick -> update(feed) -> MPPI cycle: one batch on the stream, one wait
    grid_a.setInflation(gv_inflation{0.35, 0.55, 10.0, 65, 0});
    grid_a.inflate();
    gv_footprint fp{};
    fp.collision_cost = 253;
    fp.off_map_cost = 255;
    grid_a.setFootprint(fp);
    const int32_t K = 256, P = 30, C = 2;
    grid_a.setMotionModel(gv_motion_model{GV_MOTION_DIFF, 0.2, 0});
    gv_mppi_config mc{};
    mc.sigma[0] = 0.4; mc.sigma[1] = 0.15;
    mc.u_min[0] = 0.0f; mc.u_max[0] = 3.0f;
    mc.u_min[1] = -0.6f; mc.u_max[1] = 0.6f;
    mc.lambda = 2000.0;
    grid_a.setMppi(mc);
    std::vector<float> nominal((size_t)P * C, 0.0f);
    for (int32_t p = 0; p < P; ++p) nominal[(size_t)p * C] = 1.0f;
    grid_a.setMppiNominal(nominal, P);
    const Scene s = scene(7);
    const double start[3] = {0.0, 0.0, 0.0};
    const gv_critic_weights weights{1, 1, 0, 0, 0, 0};
    gv_control_result res{};
    const gv_handle h = ctx_a.handle();
    ctx_a.tickEnqueue(s.boxes, GV_TICK_KEEP_DETS, 4);
    grid_a.trackUpdateFromTickAsync(dt, nullptr, true);
    gv::check(gv_mppi_cycle_async(h, start, K, 42, 0, 0u, &weights, 0u, &res, nullptr, nominal.data()), h, "gv_mppi_cycle_async");
    ctx_a.synchronize();                                            // the one wait
    const GridVisionContext::TickOutput last = ctx_a.tickWait();    // returns at once: the tick's event has passed
    std::printf("tick -> update -> mppi cycle with one wait: %zu poses, %d of %d sequences admitted, best %d, nominal v %.3f\n",
                last.poses.size(), res.n_valid, K, res.best, nominal[0]);
    // the same choice inside the frame flow: FlowParams::track_on_device on one context, off on the other, with ego motion
    // and a skipped tick whose dt and motion the next update is owed
    bool flow_agree = true;
    {
      GridVisionContext ctx_c(50, 20, 0.1, cam), ctx_d(50, 20, 0.1, cam);
      OccupancyGridMap grid_c(ctx_c), grid_d(ctx_d);
      grid_vision::FlowParams fp_c;
      fp_c.use_vision_orientation = false;
      fp_c.ego_motion = true;
      fp_c.track_objects = true;
      grid_vision::FlowParams fp_d = fp_c;
      fp_c.track_on_device = true;
      grid_vision::FrameFlow flow_c(ctx_c, grid_c, fp_c), flow_d(ctx_d, grid_d, fp_d);
      size_t flow_tracks = 0;
      for (int t = 0; t < 6; ++t) {
        const Scene sc = scene(t);
        gv_transform m{};
        m.qz = std::sin(0.005 * t); m.qw = std::cos(0.005 * t);
        m.tx = 0.05 * t; m.ty = -0.01;
        grid_vision::TickInput in;
        in.have_image = in.have_cloud = t != 2;   // tick 2 is skipped: missing inputs
        in.bboxes = &sc.boxes;
        in.motion = t % 2 ? &m : nullptr;
        in.dt = 0.1;
        std::vector<gv_track> got[2];
        uint32_t ids[2] = {0, 0};
        int k = 0;
        for (auto *f : {&flow_c, &flow_d}) {
          GridVisionContext &c = k == 0 ? ctx_c : ctx_d;
          c.setTransforms(&cam_lidar, &base_cam, &base_lidar);
          c.setCloud(sc.x.data(), sc.y.data(), sc.z.data(), sc.x.size());
          f->setTransformsAvailable(true);
          const grid_vision::TickResult r = f->tick(in);
          flow_agree = flow_agree && (t == 2 ? r.branch == grid_vision::TickBranch::MissingInputs : r.branch == grid_vision::TickBranch::CloudPCA);
          got[k] = (k == 0 ? grid_c : grid_d).getTracks(&ids[k]);
          ++k;
        }
        flow_agree = flow_agree && got[0].size() == got[1].size() && ids[0] == ids[1] &&
                     (got[0].empty() || std::memcmp(got[0].data(), got[1].data(), got[0].size() * sizeof(gv_track)) == 0);
        flow_tracks = got[0].size();
      }
      flow_agree = flow_agree && flow_tracks >= 2;
      std::printf("frame flow, track_on_device against the host path over 6 ticks (one skipped): %s\n", flow_agree ? "flow tracks agree" : "FLOW TRACKS DISAGREE");
    }
    const bool ok = agree && flow_agree && n_tracks == 2 && last.poses.size() == 2 && res.n_valid > 0 && res.best >= 0;
    std::printf("tick track check %s\n", ok ? "ok" : "FAILED");
    return ok ? 0 : 1;
  } catch (const gv::Error &e) {
    std::fprintf(stderr, "gv error %d: %s\n", e.code, e.what());
    return 2;
  }
}
