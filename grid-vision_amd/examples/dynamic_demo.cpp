// dynamic_demo.cpp -- [EXTENSION] X13: a car crosses the robot's path.  The map is empty, so the costmap critic (X7) alone
// takes the fastest of seven straight trajectories; with the car given to gv_set_moving_objects as a rectangle with a
// velocity, the control step rejects the trajectories that would meet it where it WILL be and takes a slower one.
// Plain g++ host code over the C ABI and its C++ mirror headers:
//   g++ -std=c++17 -O2 dynamic_demo.cpp -o dynamic_demo -L.. -lgridvision_hip -Wl,-rpath,$PWD/..
// The last lines replay the step on the host: gv_dyn_score_poses over the read-back rollout must equal the device's
// records byte for byte (one circle at the centre: no sin or cos is involved), and gv_control_select_dyn over the three
// records must give the device's result and totals.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../include/grid_vision/frame_flow.hpp"

int main()
{
  try {
    const CAMParams cam{224, 224, 480, 640, 320.f, 320.f, 320.f, 240.f};
    GridVisionContext ctx(50, 20, 0.1, cam);
    OccupancyGridMap grid(ctx);

    // an empty map: nothing is lethal, every X7 cost is 0
    grid.setInflation(gv_inflation{0.35, 0.55, 10.0, 65, 0});
    grid.inflate();
    gv_footprint fp{};
    fp.collision_cost = 253;
    fp.off_map_cost = 255;
    grid.setFootprint(fp);

    // seven straight runs from the origin along +x, the fastest first: 5 s in 20 steps
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

    const gv_critic_weights weights{1, 1, 0, 0, 0, 0};
    std::vector<uint64_t> totals;
    const gv_control_result before = grid.controlStep(weights, &totals);
    std::printf("without objects: best %d (%.1f m/s) admitted %d\n", before.best, controls[(size_t)before.best * 2], before.n_valid);

    // the car: 4.5 m x 2.0 m, heading +y (yaw 90 degrees), at (9, -9) with 3 m/s: it covers the robot's line from 2.25 s to 3.75 s
    gv_moving_object car{};
    car.pose.px = 9.0; car.pose.py = -9.0;
    car.pose.qz = std::sin(0.25 * M_PI); car.pose.qw = std::cos(0.25 * M_PI);
    car.pose.length = 4.5; car.pose.width = 2.0; car.pose.height = 1.5;
    car.vx = 0.0; car.vy = 3.0;
    gv_dyn_config dyn{};
    dyn.n_circles = 1;                 // a round robot of 0.4 m
    dyn.radius = 0.4;
    dyn.influence_radius = 2.0;
    dyn.cost_scaling_factor = 2.0;
    dyn.quantum = 0.05;
    dyn.t0 = model.dt; dyn.dt = model.dt;   // pose p is the state after step p
    dyn.collision_cost = 253;
    dyn.w_sum = 1; dyn.w_max = 0;
    grid.setDynConfig(dyn);
    grid.setMovingObjects({car});

    const gv_control_result after = grid.controlStep(weights, &totals);
    const std::vector<gv_dyn_score> rec = grid.scoreDynamic(poses, K, P);
    for (int32_t k = 0; k < K; ++k)
      std::printf("trajectory %d (%.1f m/s): max cost %d first collision %d cost sum %u nearest %d at %.2f m %s\n", k, controls[(size_t)k * 2],
                  rec[(size_t)k].max_cost, rec[(size_t)k].first_collision, rec[(size_t)k].cost_sum, rec[(size_t)k].nearest_object,
                  std::sqrt(rec[(size_t)k].min_dist2), totals[(size_t)k] == UINT64_MAX ? "REJECTED" : "admitted");
    std::printf("with the car: best %d (%.1f m/s) admitted %d total %llu\n", after.best, after.best < 0 ? 0.0f : controls[(size_t)after.best * 2],
                after.n_valid, (unsigned long long)after.best_total);

    // the host's replay
    std::vector<gv_dyn_score> host_rec((size_t)K);
    gv::check(gv_dyn_score_poses(&dyn, &car, 1, poses.data(), K, P, host_rec.data(), nullptr), nullptr, "gv_dyn_score_poses");
    const int rec_diff = std::memcmp(rec.data(), host_rec.data(), rec.size() * sizeof(gv_dyn_score)) != 0;
    const std::vector<gv_traj_score> traj = grid.scoreTrajectories(poses, K, P);
    gv_control_result host_res{};
    std::vector<uint64_t> host_totals((size_t)K);
    gv::check(gv_control_select_dyn(&weights, traj.data(), nullptr, host_rec.data(), &dyn, K, &host_res, host_totals.data()), nullptr,
              "gv_control_select_dyn");
    const int sel_diff = std::memcmp(&host_res, &after, sizeof(after)) != 0 ||
                         std::memcmp(host_totals.data(), totals.data(), totals.size() * sizeof(uint64_t)) != 0;
    std::printf("dyn records %s the host's, selection %s the host's\n", rec_diff ? "DIFFER from" : "equal", sel_diff ? "DIFFERS from" : "equals");
    const bool ok = before.best == 0 && before.n_valid == K && totals[0] == UINT64_MAX && rec[0].first_collision >= 0 && after.best > 0 &&
                    after.n_valid < K && !rec_diff && !sel_diff;
    std::printf("dynamic check %s\n", ok ? "ok" : "FAILED");
    return ok ? 0 : 1;
  } catch (const gv::Error &e) {
    std::fprintf(stderr, "gv error %d: %s\n", e.code, e.what());
    return 2;
  }
}
