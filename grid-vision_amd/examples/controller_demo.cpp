// controller_demo.cpp -- [EXTENSION] X10: one control cycle of a sampling controller with the host out of the loop:
// tick -> inflate -> distance field from the goal -> a fan of constant controls rolled out on the device -> control step
// (both samplers over the resident rollout, the records combined, the best admissible trajectory selected: 16 bytes back).
// Plain g++ host code over the C ABI and its C++ mirror headers:
//   g++ -std=c++17 -O2 controller_demo.cpp -o controller_demo -L.. -lgridvision_hip -Wl,-rpath,$PWD/..
// The map is planner_demo's: a wall across the lane 12 m ahead and a post, from three lidar ticks of the flow.  Neither the
// poses nor the records leave the device.  The last lines replay the choice the way a host controller would have made it --
// gv_rollout_poses on one core, the two synchronous scorers on those host poses, gv_control_select -- and compare the
// result and every total: tests/test_gpu_rollout.py::test_controller_demo reads them.  The device's sincos may differ from
// the C library's in the last bit, so a pose float may differ by one unit in the last place; the demo counts those and
// fails only if the choice or a total differs.
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

int main()
{
  try {
    const uint8_t grid_x = 50, grid_y = 20;
    const double resolution = 0.1;
    const CAMParams cam{224, 224, 480, 640, 320.f, 320.f, 320.f, 240.f};
    GridVisionContext ctx(grid_x, grid_y, resolution, cam);
    OccupancyGridMap grid(ctx);
    const gv_transform cam_lidar{0.5, -0.5, 0.5, 0.5, 0.0, 0.4, -0.3};
    const gv_transform base_cam{0.5, -0.5, 0.5, -0.5, 0.3, 0.0, 2.2};
    const gv_transform base_lidar{0, 0, 0, 1, 0, 0, 1.8};
    ctx.setTransforms(&cam_lidar, &base_cam, &base_lidar);

    // a wall across the lane 12 m ahead, from y = -3 to y = 1, and a post to the left of it
    uint64_t seed = 11;
    const size_t n = 20000;
    std::vector<float> x(n), y(n), z(n);
    for (size_t i = 0; i < n; ++i) {
      const bool wall = i % 8 != 0;
      x[i] = wall ? 12.f + 0.8f * u01(seed) : 9.f + 0.3f * u01(seed);
      y[i] = wall ? -3.f + 4.f * u01(seed) : 5.f + 0.3f * u01(seed);
      z[i] = -1.5f + 1.2f * u01(seed);
    }
    ctx.setCloud(x.data(), y.data(), z.data(), n);

    grid_vision::FlowParams params;
    params.lidar_binning = true;        // the map update counts the lidar returns
    params.inflate_costmap = true;      // ... and the costmap follows every update
    grid_vision::FrameFlow flow(ctx, grid, params);
    flow.setTransformsAvailable(true);
    grid_vision::TickInput in;
    in.have_cloud = true;
    for (int t = 0; t < 3; ++t) flow.tick(in);   // no detections: the lidar map update alone

    // the robot: 4.5 m x 2.0 m, origin over the rear axle
    gv_footprint fp{};
    fp.n_vertices = 4;
    const double vx[4] = {3.4, -1.1, -1.1, 3.4}, vy[4] = {1.0, 1.0, -1.0, -1.0};
    for (int i = 0; i < 4; ++i) { fp.vx[i] = vx[i]; fp.vy[i] = vy[i]; }
    fp.collision_cost = 253;
    fp.off_map_cost = 255;
    grid.setFootprint(fp);

    // the goal behind the wall: distance over the costmap, one step a cell plus the cell's cost
    const gv_nav_config nav{253, 1, 0};
    grid.setNavConfig(nav);
    const std::vector<float> goal{22.0f, -1.0f};
    const gv_nav_info info = grid.solveNavField(goal);

    // the controller's samples: a fan of constant (v, w) held for P steps, as DWB's generator makes them
    const int32_t K = 41, P = 40;
    const gv_motion_model model{GV_MOTION_DIFF, 0.2, 0};
    const double start[3] = {0.0, 0.0, 0.0};
    std::vector<float> controls((size_t)K * 2);
    for (int32_t k = 0; k < K; ++k) {
      controls[2 * k] = 2.0f;                                  // 0.4 m a step
      controls[2 * k + 1] = (float)(2.0 * 0.0125 * (k - K / 2));   // curvature 0.0125 (k - K / 2) per metre
    }
    grid.setMotionModel(model);
    grid.rollout(start, controls, K, P, true);

    // DWB's BaseObstacle + GoalDist: the summed centre cost plus four times the goal distance of the last pose
    const gv_critic_weights weights{1, 0, 4, 0, 0, 0};
    std::vector<uint64_t> totals;
    const gv_control_result got = grid.controlStep(weights, &totals);
    std::printf("trajectories %d poses %d admitted %d\n", K, P, got.n_valid);
    std::printf("field rounds %d seeds %d\n", info.rounds, info.n_seeds_used);
    if (got.best >= 0)
      std::printf("best %d w %.4f total %llu\n", got.best, controls[2 * got.best + 1], (unsigned long long)got.best_total);
    else
      std::printf("best none\n");
    std::printf("straight total %llu\n", (unsigned long long)totals[K / 2]);

    // the host loop this replaces: roll out on one core, upload the poses twice, download two record arrays, select
    std::vector<float> poses((size_t)K * P * 3);
    gv::check(gv_rollout_poses(&model, start, controls.data(), K, P, GV_ROLLOUT_CONSTANT, poses.data()), nullptr, "gv_rollout_poses");
    const std::vector<float> resident = grid.getRollout();
    int ulp = 0;
    for (size_t i = 0; i < poses.size(); ++i) ulp += std::memcmp(&poses[i], &resident[i], sizeof(float)) != 0;
    std::printf("pose floats that differ from the host rollout %d of %zu\n", ulp, poses.size());
    const std::vector<gv_traj_score> obstacle = grid.scoreTrajectories(poses, K, P);
    const std::vector<gv_nav_score> to_goal = grid.scoreNav(poses, K, P);
    gv_control_result want{};
    std::vector<uint64_t> want_totals((size_t)K);
    gv::check(gv_control_select(&weights, obstacle.data(), to_goal.data(), K, &want, want_totals.data()), nullptr, "gv_control_select");
    int mismatches = std::memcmp(&want, &got, sizeof(want)) != 0;
    for (int32_t k = 0; k < K; ++k) mismatches += want_totals[k] != totals[k];
    std::printf("host check %s (%d mismatches)\n", mismatches ? "FAILED" : "ok", mismatches);
    return mismatches ? 1 : 0;
  } catch (const gv::Error &e) {
    std::fprintf(stderr, "gv error %d: %s\n", e.code, e.what());
    return 2;
  }
}
