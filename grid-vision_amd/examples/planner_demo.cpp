// planner_demo.cpp -- [EXTENSION] X7: tick -> inflate -> score a fan of arcs -> pick the best one, written against the
// C++ mirror headers: plain g++ host code over the C ABI.
//   g++ -std=c++17 -O2 planner_demo.cpp -o planner_demo -L.. -lgridvision_hip -Wl,-rpath,$PWD/..
// The map comes from three lidar ticks of the flow (FlowParams::inflate_costmap refreshes the costmap behind every map
// update); the controller's candidates never see the costmap: K * P poses go to the device, K records come back.
// The last lines repeat the scoring on the host -- the downloaded costmap and gv_footprint_cells, the library's own
// geometry -- and compare: tests/test_gpu_traj.py::test_planner_demo reads them.
#include <algorithm>
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

    // a fan of constant-curvature arcs from the origin
    const int32_t K = 41, P = 40;
    const double step = 0.4;
    std::vector<float> poses((size_t)K * P * 3);
    std::vector<double> curvature(K);
    for (int32_t k = 0; k < K; ++k) {
      const double c = 0.0125 * (k - K / 2);
      curvature[k] = c;
      for (int32_t p = 0; p < P; ++p) {
        const double s = step * p;
        float *q = &poses[((size_t)k * P + p) * 3];
        q[0] = (float)(c == 0.0 ? s : std::sin(c * s) / c);
        q[1] = (float)(c == 0.0 ? 0.0 : (1.0 - std::cos(c * s)) / c);
        q[2] = (float)(c * s);
      }
    }
    std::vector<uint8_t> pose_cost;
    const std::vector<gv_traj_score> scores = grid.scoreTrajectories(poses, K, P, &pose_cost);

    // the controller's choice: among the arcs that do not collide, the cheapest; ties go to the straighter one
    int best = -1, collisions = 0;
    for (int32_t k = 0; k < K; ++k) {
      if (scores[k].first_collision >= 0) { ++collisions; continue; }
      if (best < 0 || scores[k].cost_sum < scores[best].cost_sum ||
          (scores[k].cost_sum == scores[best].cost_sum && std::fabs(curvature[k]) < std::fabs(curvature[best])))
        best = k;
    }
    std::printf("trajectories %d poses %d collisions %d\n", K, P, collisions);
    if (best >= 0)
      std::printf("best %d curvature %.4f cost_sum %u max_cost %d\n", best, curvature[best], scores[best].cost_sum, scores[best].max_cost);
    else
      std::printf("best none\n");
    std::printf("straight first_collision %d max_cost %d\n", scores[K / 2].first_collision, scores[K / 2].max_cost);

    // the host alternative this replaces: download the costmap, walk every pose's cells on one core
    const std::vector<uint8_t> cost = grid.getCostmap();
    const size_t G = cost.size();
    std::vector<int32_t> cells(4096);
    int mismatches = 0;
    for (int32_t k = 0; k < K; ++k) {
      gv_traj_score want{0, -1, 0, 0};
      for (int32_t p = 0; p < P; ++p) {
        const float *q = &poses[((size_t)k * P + p) * 3];
        int32_t m = 0;
        gv::check(gv_footprint_cells(grid_x, grid_y, resolution, &fp, q[0], q[1], q[2], cells.data(), (int32_t)cells.size(), &m),
                  nullptr, "gv_footprint_cells");
        int pc = fp.off_map_cost, centre = fp.off_map_cost;
        if (m < 0) ++want.n_off_map;
        else {
          centre = cost[G - 1 - (size_t)cells[0]];
          pc = 0;
          for (int32_t i = 0; i < m; ++i) pc = std::max(pc, (int)cost[G - 1 - (size_t)cells[i]]);
        }
        want.cost_sum += (uint32_t)centre;
        want.max_cost = std::max(want.max_cost, pc);
        if (want.first_collision < 0 && pc >= fp.collision_cost) want.first_collision = p;
        mismatches += pc != (int)pose_cost[(size_t)k * P + p];
      }
      mismatches += std::memcmp(&want, &scores[k], sizeof(want)) != 0;
    }
    std::printf("host check %s (%d mismatches)\n", mismatches ? "FAILED" : "ok", mismatches);
    return mismatches ? 1 : 0;
  } catch (const gv::Error &e) {
    std::fprintf(stderr, "gv error %d: %s\n", e.code, e.what());
    return 2;
  }
}
