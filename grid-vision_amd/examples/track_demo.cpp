// track_demo.cpp -- [EXTENSION] X14: the link between the boxes a tick detects and the controller.  Three boxes are seen
// for 20 ticks of 0.1 s: a car that crosses the robot's path from the right, an oncoming car in the other lane and a
// parked car.  gv_track_update gives each an identity and a velocity and feeds the confirmed tracks to X13 on the device
// (GV_TRACK_FEED_DYNAMIC), so the control step that follows rejects the trajectory that would meet the crossing car
// where it WILL be -- nobody handed the library a velocity.
// Plain g++ host code over the C ABI and its C++ mirror headers:
//   g++ -std=c++17 -O2 track_demo.cpp -o track_demo -L.. -lgridvision_hip -Wl,-rpath,$PWD/..
// The last lines replay the 20 updates on the host with gv_track_step (trackStep): its tracks must equal the device's
// byte for byte, and gv_dyn_score_poses over its exported objects must equal the records the device scored against the
// fed set.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../include/grid_vision/frame_flow.hpp"

static LShapePose box(double x, double y, double yaw, double length, double width)
{
  LShapePose p{};
  p.px = x; p.py = y;
  p.qz = std::sin(0.5 * yaw); p.qw = std::cos(0.5 * yaw);
  p.length = length; p.width = width; p.height = 1.5;
  return p;
}

int main()
{
  try {
    const CAMParams cam{224, 224, 480, 640, 320.f, 320.f, 320.f, 240.f};
    GridVisionContext ctx(50, 20, 0.1, cam);
    OccupancyGridMap grid(ctx);

    // an empty map and the seven straight runs of dynamic_demo.cpp: 5 s in 20 steps, the fastest first
    grid.setInflation(gv_inflation{0.35, 0.55, 10.0, 65, 0});
    grid.inflate();
    gv_footprint fp{};
    fp.collision_cost = 253;
    fp.off_map_cost = 255;
    grid.setFootprint(fp);
    const int32_t K = 7, P = 20;
    const gv_motion_model model{GV_MOTION_DIFF, 0.25, 0};
    grid.setMotionModel(model);
    std::vector<float> controls;
    for (int32_t k = 0; k < K; ++k) {
      controls.push_back(3.0f - 0.4f * (float)k);
      controls.push_back(0.0f);
    }
    const double start[3] = {0.0, 0.0, 0.0};
    grid.rollout(start, controls, K, P, true);
    const std::vector<float> poses = grid.getRollout();
    gv_dyn_config dyn{};
    dyn.n_circles = 1;
    dyn.radius = 0.4;
    dyn.influence_radius = 2.0;
    dyn.cost_scaling_factor = 2.0;
    dyn.quantum = 0.05;
    dyn.t0 = model.dt; dyn.dt = model.dt;
    dyn.collision_cost = 253;
    dyn.w_sum = 1; dyn.w_max = 0;
    grid.setDynConfig(dyn);

    // the tracker: a 2 m gate, confirmed at the second hit, a track slower than 0.3 m/s stands
    const gv_track_config cfg{2.0, 2.0, 0.3, 5.0, 0.3, 2, 3, 0};
    grid.setTrackConfig(cfg);
    const double dt = 0.1;
    const int ticks = 20;
    std::vector<gv_track> tracks, host_tracks;
    uint32_t host_next = 1;
    std::vector<gv_moving_object> host_objs;
    gv_track_info info{}, host_info{};
    for (int i = 0; i < ticks; ++i) {
      const double t = dt * (double)i;
      const std::vector<LShapePose> dets = {box(9.0, -12.0 + 3.0 * t + 0.3, 0.5 * M_PI, 4.5, 2.0),   // crossing, +y at 3 m/s
                                            box(30.0 - 5.0 * t, 3.0, M_PI, 4.5, 2.0),                 // oncoming, -x at 5 m/s
                                            box(15.0, -4.0, 0.0, 4.5, 2.0)};                          // parked
      info = grid.trackUpdate(dets, dt, nullptr, true, &tracks);
      host_info = OccupancyGridMap::trackStep(cfg, host_tracks, host_next, dets, dt, nullptr, &host_objs);
      if (i == 0 || i == 1 || i == ticks - 1)
        std::printf("tick %2d: %d tracks, %d confirmed, %d exported, %d matched, %d born\n", i, info.n_tracks, info.n_confirmed,
                    info.n_exported, info.n_matched, info.n_born);
    }
    for (const gv_track &k : tracks)
      std::printf("track id %u slot %d hits %d at (%.2f, %.2f) velocity (%.2f, %.2f)\n", k.id, k.slot, k.hits, k.x, k.y, k.vx, k.vy);
    const int track_diff = host_tracks.size() != tracks.size() || std::memcmp(tracks.data(), host_tracks.data(), tracks.size() * sizeof(gv_track)) != 0 ||
                           std::memcmp(&info, &host_info, sizeof(info)) != 0;
    std::printf("parked car exported with velocity (%.2f, %.2f)\n", host_objs[2].vx, host_objs[2].vy);

    // the control step against the fed set
    const gv_critic_weights weights{1, 1, 0, 0, 0, 0};
    std::vector<uint64_t> totals;
    const gv_control_result res = grid.controlStep(weights, &totals);
    const std::vector<gv_dyn_score> rec = grid.scoreDynamic(poses, K, P);
    for (int32_t k = 0; k < K; ++k)
      std::printf("trajectory %d (%.1f m/s): max cost %d first collision %d nearest %d at %.2f m %s\n", k, controls[(size_t)k * 2],
                  rec[(size_t)k].max_cost, rec[(size_t)k].first_collision, rec[(size_t)k].nearest_object, std::sqrt(rec[(size_t)k].min_dist2),
                  totals[(size_t)k] == UINT64_MAX ? "REJECTED" : "admitted");
    std::printf("with the tracked cars: best %d (%.1f m/s) admitted %d\n", res.best, res.best < 0 ? 0.0f : controls[(size_t)res.best * 2], res.n_valid);

    // the host's replay of the scoring
    std::vector<gv_dyn_score> host_rec((size_t)K);
    gv::check(gv_dyn_score_poses(&dyn, host_objs.data(), (int32_t)host_objs.size(), poses.data(), K, P, host_rec.data(), nullptr), nullptr,
              "gv_dyn_score_poses");
    const int rec_diff = std::memcmp(rec.data(), host_rec.data(), rec.size() * sizeof(gv_dyn_score)) != 0;
    std::printf("tracks %s the host's, records against the fed set %s the host's\n", track_diff ? "DIFFER from" : "equal",
                rec_diff ? "DIFFER from" : "equal");
    const bool ok = tracks.size() == 3 && info.n_exported == 3 && std::fabs(tracks[0].vy - 3.0) < 0.2 && std::fabs(tracks[0].vx) < 0.2 &&
                    std::fabs(tracks[1].vx + 5.0) < 0.2 && host_objs.size() == 3 && host_objs[2].vx == 0.0 && host_objs[2].vy == 0.0 && rec[0].first_collision >= 0 &&
                    rec[0].nearest_object == 0 && totals[0] == UINT64_MAX && res.best > 0 && !track_diff && !rec_diff;
    std::printf("track check %s\n", ok ? "ok" : "FAILED");
    return ok ? 0 : 1;
  } catch (const gv::Error &e) {
    std::fprintf(stderr, "gv error %d: %s\n", e.code, e.what());
    return 2;
  }
}
