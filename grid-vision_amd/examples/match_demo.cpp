// match_demo.cpp -- [EXTENSION] X16: map a wall scene, see it again from a displaced pose, match the scan to the costmap,
// feed the recovered motion to the map, written against the C++ mirror headers: plain g++ host code over the C ABI.
//   g++ -std=c++17 -O2 match_demo.cpp -o match_demo -L.. -lgridvision_hip -Wl,-rpath,$PWD/..
// The map comes from three lidar ticks of the flow at the first pose and is inflated into a likelihood field (a narrow
// inscribed radius: the field should peak on the wall).  The vehicle then moves by a pose the demo knows and odometry
// does not; the same world points, seen from there, are the new cloud.  gv_match_scan from a zero guess returns that
// pose, gv_match_motion makes it the motion gv_grid_move takes, and the map follows the vehicle.  The last lines repeat
// the match on the host (gv_match_scan_host over the downloaded costmap) and compare the 64 bytes:
// tests/test_gpu_match.py::test_match_demo reads them.
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

    // an L-shaped wall: along x = 12 m from y = -3 to 3, and along y = 3 m from x = 8 to 12 (base frame of the first pose)
    uint64_t seed = 16;
    const size_t n = 20000;
    std::vector<float> x(n), y(n), z(n);
    for (size_t i = 0; i < n; ++i) {
      const bool across = i % 5 < 3;
      x[i] = across ? 12.f + 0.05f * u01(seed) : 8.f + 4.f * u01(seed);
      y[i] = across ? -3.f + 6.f * u01(seed) : 3.f + 0.05f * u01(seed);
      z[i] = -1.5f + 1.2f * u01(seed);
    }
    ctx.setCloud(x.data(), y.data(), z.data(), n);

    grid_vision::FlowParams params;
    params.lidar_binning = true;        // the map update counts the lidar returns
    grid_vision::FrameFlow flow(ctx, grid, params);
    flow.setTransformsAvailable(true);
    grid_vision::TickInput in;
    in.have_cloud = true;
    for (int t = 0; t < 3; ++t) flow.tick(in);   // no detections: the lidar map update alone
    gv_inflation infl{};
    infl.inscribed_radius = 0.05;
    infl.inflation_radius = 0.6;
    infl.cost_scaling_factor = 6.0;
    infl.lethal_threshold = 65;
    grid.setInflation(infl);
    grid.inflate();

    // the vehicle moves; the same points seen from the new base frame (the lidar sits 1.8 m above it, unrotated)
    const double tx = 0.3, ty = -0.2, tyaw = 0.04;
    std::vector<float> x2(n), y2(n);
    for (size_t i = 0; i < n; ++i) {
      const double dx = (double)x[i] - tx, dy = (double)y[i] - ty;
      x2[i] = (float)(std::cos(tyaw) * dx + std::sin(tyaw) * dy);
      y2[i] = (float)(-std::sin(tyaw) * dx + std::cos(tyaw) * dy);
    }
    ctx.setCloud(x2.data(), y2.data(), z.data(), n);

    gv_match_config cfg{};
    cfg.wx = 6; cfg.wy = 6; cfg.wt = 6;
    cfg.yaw_step = 0.01;
    cfg.stride = 4;
    cfg.min_points = 100;
    grid.setMatchConfig(cfg);
    const gv_match_guess guess{0.0, 0.0, 0.0};   // odometry saw nothing
    std::vector<uint32_t> scores;
    const gv_match_result r = grid.matchScan(guess, &scores);
    std::printf("candidates %zu used points %u guess score %u best score %u valid %d\n", scores.size(), r.n_used, r.guess_score,
                r.best_score, r.valid);
    std::printf("best shift t %d j %d i %d\n", r.best_t, r.best_j, r.best_i);
    std::printf("recovered pose x %.4f y %.4f yaw %.4f (true %.4f %.4f %.4f)\n", r.x, r.y, r.yaw, tx, ty, tyaw);

    // the host alternative this replaces: download the costmap, correlate on one core
    const std::vector<uint8_t> cost = grid.getCostmap();
    std::vector<uint32_t> host_scores;
    const gv_match_result want = OccupancyGridMap::matchScanHost(grid_x, grid_y, resolution, cost, x2, y2, z, base_lidar, nullptr, cfg,
                                                                 guess, &host_scores);
    const bool same = std::memcmp(&want, &r, sizeof(r)) == 0 && host_scores == scores;
    std::printf("host twin %s\n", same ? "ok" : "FAILED");

    // close the loop: the map follows the vehicle, and a second match from a zero guess finds nothing left to correct
    // beyond the move's sub-cell residue
    const gv_transform motion = OccupancyGridMap::matchMotion(r);
    const gv_grid_move_info moved = grid.moveMap(motion);
    grid.inflate();
    const gv_match_result again = grid.matchScan(guess);
    std::printf("grid moved applied %d; second match shift t %d j %d i %d score %u\n", moved.applied, again.best_t, again.best_j,
                again.best_i, again.best_score);
    return same && r.valid ? 0 : 1;
  } catch (const gv::Error &e) {
    std::fprintf(stderr, "gv error %d: %s\n", e.code, e.what());
    return 2;
  }
}
