// mppi_demo.cpp -- [EXTENSION] X11: a few MPPI iterations with the host out of the loop.  The map and the goal are
// controller_demo's (a wall across the lane 12 m ahead, the goal behind it); every iteration is ONE call, gv_mppi_cycle:
// sample K control sequences around the resident nominal on the device, roll them out, score them with both samplers,
// select, and replace the nominal by the softmax average -- a seed and 16 bytes in, P x C floats back.
// Plain g++ host code over the C ABI and its C++ mirror headers:
//   g++ -std=c++17 -O2 mppi_demo.cpp -o mppi_demo -L.. -lgridvision_hip -Wl,-rpath,$PWD/..
// The robot does not move here: the iterations refine one plan from the same start, the way MPPI's inner loop does.
// The last lines replay the final iteration's average on the host (gv_mppi_average over the read-backs) and compare:
// the device adds in chunks, so a float may differ in its last place; the demo counts those and fails only on more.
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
    const gv_handle h = ctx.handle();
    const gv_transform cam_lidar{0.5, -0.5, 0.5, 0.5, 0.0, 0.4, -0.3};
    const gv_transform base_cam{0.5, -0.5, 0.5, -0.5, 0.3, 0.0, 2.2};
    const gv_transform base_lidar{0, 0, 0, 1, 0, 0, 1.8};
    ctx.setTransforms(&cam_lidar, &base_cam, &base_lidar);

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
    params.lidar_binning = true;
    params.inflate_costmap = true;
    grid_vision::FrameFlow flow(ctx, grid, params);
    flow.setTransformsAvailable(true);
    grid_vision::TickInput in;
    in.have_cloud = true;
    for (int t = 0; t < 3; ++t) flow.tick(in);

    gv_footprint fp{};
    fp.n_vertices = 4;
    const double vx[4] = {3.4, -1.1, -1.1, 3.4}, vy[4] = {1.0, 1.0, -1.0, -1.0};
    for (int i = 0; i < 4; ++i) { fp.vx[i] = vx[i]; fp.vy[i] = vy[i]; }
    fp.collision_cost = 253;
    fp.off_map_cost = 255;
    grid.setFootprint(fp);
    const gv_nav_config nav{253, 1, 0};
    grid.setNavConfig(nav);
    const std::vector<float> goal{22.0f, -1.0f};
    grid.solveNavField(goal);

    // MPPI: 512 sequences of 40 steps of (v, w) around a nominal that starts as "creep ahead"
    const int32_t K = 512, P = 40, C = 2;
    const gv_motion_model model{GV_MOTION_DIFF, 0.2, 0};
    grid.setMotionModel(model);
    gv_mppi_config cfg{};
    cfg.sigma[0] = 0.4; cfg.sigma[1] = 0.15;
    cfg.u_min[0] = 0.0f; cfg.u_max[0] = 3.0f;
    cfg.u_min[1] = -0.6f; cfg.u_max[1] = 0.6f;
    cfg.lambda = 2000.0;
    gv::check(gv_set_mppi(h, &cfg), h, "gv_set_mppi");
    std::vector<float> nominal((size_t)P * C, 0.0f);
    for (int32_t p = 0; p < P; ++p) nominal[(size_t)p * C] = 0.5f;
    gv::check(gv_mppi_set_nominal(h, nominal.data(), P), h, "gv_mppi_set_nominal");

    const double start[3] = {0.0, 0.0, 0.0};
    const gv_critic_weights weights{1, 0, 4, 0, 0, 0};   // controller_demo's: centre cost plus four times the goal distance
    std::vector<uint64_t> totals((size_t)K);
    std::vector<float> before, after((size_t)P * C);
    gv_control_result res{};
    const int iterations = 6;
    for (int it = 0; it < iterations; ++it) {
      before = it == 0 ? nominal : after;
      gv::check(gv_mppi_cycle(h, start, K, 42, (uint64_t)it, 0, &weights, GV_CONTROL_KEEP_TOTALS, &res, totals.data(), after.data()), h,
                "gv_mppi_cycle");
      std::printf("iteration %d admitted %d best %d total %llu\n", it, res.n_valid, res.best, (unsigned long long)res.best_total);
    }
    std::printf("nominal v %.3f .. %.3f w %.3f .. %.3f\n", after[0], after[(size_t)(P - 1) * C], after[1], after[(size_t)(P - 1) * C + 1]);

    // the host's replay of the last average over the device's own controls and totals
    std::vector<float> controls((size_t)K * P * C), want((size_t)P * C);
    gv::check(gv_get_controls(h, controls.data()), h, "gv_get_controls");
    gv::check(gv_mppi_average(&cfg, C, controls.data(), totals.data(), K, P, before.data(), want.data()), nullptr, "gv_mppi_average");
    int ulp = 0, wrong = 0;
    for (size_t i = 0; i < want.size(); ++i) {
      ulp += std::memcmp(&want[i], &after[i], sizeof(float)) != 0;
      wrong += !(std::fabs(want[i] - after[i]) <= 1e-6f * (1.0f + std::fabs(want[i])));
    }
    std::printf("nominal floats that differ from the host average %d of %zu\n", ulp, want.size());
    std::printf("host check %s (%d mismatches)\n", wrong ? "FAILED" : "ok", wrong);
    return wrong ? 1 : 0;
  } catch (const gv::Error &e) {
    std::fprintf(stderr, "gv error %d: %s\n", e.code, e.what());
    return 2;
  }
}
