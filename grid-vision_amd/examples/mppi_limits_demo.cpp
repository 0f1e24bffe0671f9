// mppi_limits_demo.cpp -- [EXTENSION] X12: mppi_demo's loop for a car-like base.  The map, the goal and the critics are
// mppi_demo's; what is new is gv_set_mppi_limits before every iteration: acceleration limits on (v, w) from the measured
// velocity, a minimum turning radius of 4 m, and the control-cost weight gamma.  Every iteration is still ONE call,
// gv_mppi_cycle; the sampled sequences are constrained on the device before the rollout reads them.
// Plain g++ host code over the C ABI and its C++ mirror headers:
//   g++ -std=c++17 -O2 mppi_limits_demo.cpp -o mppi_limits_demo -L.. -lgridvision_hip -Wl,-rpath,$PWD/..
// After each iteration the demo reads trajectory 0 (the constrained nominal) back and checks every control of it against
// the limits with the definition's own float32 arithmetic; the last lines replay the final average on the host
// (gv_mppi_control_costs and gv_mppi_average_cc over the read-backs) and compare as mppi_demo does.
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

    // a car-like base: 1.5 m/s^2 up, 3 m/s^2 down, 0.8 rad/s^2 either way, 4 m turning radius, measured (0.4 m/s, 0)
    gv_mppi_limits lim{};
    lim.rate_up[0] = 1.5; lim.rate_down[0] = 3.0;
    lim.rate_up[1] = 0.8; lim.rate_down[1] = 0.8;
    lim.rate_up[2] = lim.rate_down[2] = INFINITY;
    lim.u_prev[0] = 0.4f; lim.u_prev[1] = 0.0f; lim.u_prev[2] = NAN;
    lim.min_turn_radius = 4.0;
    lim.gamma = 30.0;
    const float up[2] = {(float)(lim.rate_up[0] * model.dt), (float)(lim.rate_up[1] * model.dt)};
    const float dn[2] = {(float)(lim.rate_down[0] * model.dt), (float)(lim.rate_down[1] * model.dt)};
    const float inv_r = (float)(1.0 / lim.min_turn_radius);

    const double start[3] = {0.0, 0.0, 0.0};
    const gv_critic_weights weights{1, 0, 4, 0, 0, 0};
    std::vector<uint64_t> totals((size_t)K);
    std::vector<float> before, after((size_t)P * C), controls((size_t)K * P * C);
    gv_control_result res{};
    const int iterations = 10;
    int violations = 0;
    for (int it = 0; it < iterations; ++it) {
      before = it == 0 ? nominal : after;
      gv::check(gv_set_mppi_limits(h, &lim), h, "gv_set_mppi_limits");   // every cycle, with the measured velocity
      gv::check(gv_mppi_cycle(h, start, K, 42, (uint64_t)it, 0, &weights, GV_CONTROL_KEEP_TOTALS, &res, totals.data(), after.data()), h,
                "gv_mppi_cycle");
      gv::check(gv_get_controls(h, controls.data()), h, "gv_get_controls");
      // trajectory 0, step by step: inside [s - dn, s + up] of the step before it, and |w| <= |v| / r
      float s[2] = {lim.u_prev[0], lim.u_prev[1]};
      int bad = 0;
      float worst_dv = 0.f, worst_curv = 0.f;
      for (int32_t p = 0; p < P; ++p) {
        const float v = controls[(size_t)p * C], w = controls[(size_t)p * C + 1];
        const float b = std::fabs(v) * inv_r;
        bad += !(v >= s[0] - dn[0] && v <= s[0] + up[0]);
        bad += !(std::fabs(w) <= b);
        // the radius is applied behind the rate window and wins: where it binds, w may have left the window
        if (std::fabs(w) != b) bad += !(w >= s[1] - dn[1] && w <= s[1] + up[1]);
        worst_dv = std::fmax(worst_dv, std::fabs(v - s[0]));
        if (v != 0.f) worst_curv = std::fmax(worst_curv, std::fabs(w / v));
        s[0] = v; s[1] = w;
      }
      violations += bad;
      std::printf("iteration %d admitted %d best %d total %llu trajectory 0: largest |dv| %.3f (limit %.3f) largest |w/v| %.4f (limit %.4f) violations %d\n",
                  it, res.n_valid, res.best, (unsigned long long)res.best_total, worst_dv, std::fmax(up[0], dn[0]), worst_curv, inv_r, bad);
    }
    std::printf("nominal v %.3f .. %.3f w %.3f .. %.3f\n", after[0], after[(size_t)(P - 1) * C], after[1], after[(size_t)(P - 1) * C + 1]);

    // the host's replay of the last average over the device's own controls, totals and control costs
    std::vector<double> g((size_t)K), g_host((size_t)K);
    std::vector<float> want((size_t)P * C);
    gv::check(gv_get_mppi_control_costs(h, g.data()), h, "gv_get_mppi_control_costs");
    gv::check(gv_mppi_control_costs(&cfg, &lim, C, controls.data(), before.data(), K, P, 0, g_host.data()), nullptr, "gv_mppi_control_costs");
    const int cost_diff = std::memcmp(g.data(), g_host.data(), g.size() * sizeof(double)) != 0;
    gv::check(gv_mppi_average_cc(&cfg, C, controls.data(), totals.data(), g.data(), K, P, before.data(), want.data()), nullptr,
              "gv_mppi_average_cc");
    int ulp = 0, wrong = 0;
    for (size_t i = 0; i < want.size(); ++i) {
      ulp += std::memcmp(&want[i], &after[i], sizeof(float)) != 0;
      wrong += !(std::fabs(want[i] - after[i]) <= 1e-6f * (1.0f + std::fabs(want[i])));
    }
    std::printf("control costs %s the host's\n", cost_diff ? "DIFFER from" : "equal");
    std::printf("nominal floats that differ from the host average %d of %zu\n", ulp, want.size());
    const bool ok = !wrong && !violations && !cost_diff;
    std::printf("limits check %s (%d violations, %d mismatches)\n", ok ? "ok" : "FAILED", violations, wrong);
    return ok ? 0 : 1;
  } catch (const gv::Error &e) {
    std::fprintf(stderr, "gv error %d: %s\n", e.code, e.what());
    return 2;
  }
}
