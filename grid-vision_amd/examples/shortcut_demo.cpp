// shortcut_demo.cpp -- [EXTENSION] X21: from the staircase a grid planner gives to the waypoints a controller follows,
// without the path or the costmap crossing the host.  A wall with a doorway between the vehicle and the goal:
// map -> inflate -> field from the goal -> gv_nav_path_async from the vehicle -> gvx3_shortcut_async (no wait in
// between) pulls the staircase tight by line of sight over the costmap and thins it to a waypoint every 0.5 m ->
// gvx3_nav_field_from_shortcut seeds X9's field with the waypoints: the one host wait of the chain is the one X9's
// solver itself makes.
// Plain g++ host code over the C headers:
//   g++ -std=c++17 -O2 shortcut_demo.cpp -o shortcut_demo -L.. -lgridvision_hip -Wl,-rpath,$PWD/..
// The last lines replay the shortcut with the host twin on the downloaded costmap and path and compare:
// tests/test_gpu_shortcut.py::test_shortcut_demo reads them.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../include/gridvision_hip_shortcut.h"

#define CHECK(call)                                                                              \
  do {                                                                                           \
    const int rc_ = (call);                                                                      \
    if (rc_ != GV_OK) {                                                                          \
      std::fprintf(stderr, "%s -> %d: %s\n", #call, rc_, h ? gv_last_error(h) : "");             \
      return 2;                                                                                  \
    }                                                                                            \
  } while (0)

int main()
{
  const uint8_t grid_x = 50, grid_y = 20;
  const double resolution = 0.1;
  const gv_cam_params cam{224, 224, 480, 640, 320.f, 320.f, 320.f, 240.f};
  gv_handle h = nullptr;
  CHECK(gv_create(&h, grid_x, grid_y, resolution, &cam, -1));
  int32_t nx = 0, ny = 0;
  double pos_x = 0.0, pos_y = 0.0;
  CHECK(gv_grid_geometry(h, &nx, &ny, &pos_x, &pos_y));
  const size_t G = (size_t)nx * (size_t)ny;

  // free ground; a wall across the map at x = 5 .. 5.3 m with a doorway 1.2 m wide about y = 4 m
  const double x_hi = pos_x + 0.5 * nx * resolution, y_hi = pos_y + 0.5 * ny * resolution;
  std::vector<float> log_odds(G, -10.0f);
  for (int32_t iy = 0; iy < ny; ++iy)
    for (int32_t ix = 0; ix < nx; ++ix) {
      const double cx = x_hi - (ix + 0.5) * resolution, cy = y_hi - (iy + 0.5) * resolution;
      if (cx >= 5.0 && cx < 5.3 && std::fabs(cy - 4.0) >= 0.6) log_odds[(size_t)iy * nx + ix] = 10.0f;
    }
  CHECK(gv_set_log_odds(h, log_odds.data()));
  CHECK(gv_update_map(h));
  const gv_inflation infl{0.3, 0.8, 4.0, 65, 0};
  CHECK(gv_set_inflation(h, &infl));
  CHECK(gv_inflate(h));
  const gv_nav_config nav{253, 2, 0};
  CHECK(gv_set_nav_config(h, &nav));
  const float goal[2] = {20.0f, -6.0f}, vehicle[2] = {0.0f, 0.0f};
  CHECK(gv_nav_field(h, goal, 1, nullptr));

  // the staircase and its waypoints, back to back on the stream: shortcuts of up to 256 path cells over cells of cost
  // 128 at the most, none that cuts a corner, a waypoint every 5 cells
  gvx3_shortcut_config cfg{};
  cfg.max_cost = 128;
  cfg.window = 256;
  cfg.spacing = 5;
  CHECK(gvx3_set_shortcut_config(h, &cfg));
  const int32_t cap = 4096, wcap = 1024;
  gv_nav_path_info path{};
  gvx3_shortcut_info cut{};
  CHECK(gv_nav_path_async(h, vehicle, 1, cap, GV_PATH_DIAGONAL, &path, nullptr));
  CHECK(gvx3_shortcut_async(h, wcap, GVX3_SHORTCUT_NO_CORNER, &cut, nullptr));
  gv_nav_info seeded{};
  CHECK(gvx3_nav_field_from_shortcut(h, 0, &seeded));   // waits as gv_nav_field does: path and waypoints are complete behind it
  std::printf("path cells %d diagonal %d status %d\n", path.n_cells, path.n_diagonal, path.status);
  std::printf("waypoints %d anchors %d status %d steps %d diagonal %d max_cost_seen %d\n", cut.n_waypoints, cut.n_anchors, cut.status,
              cut.n_steps, cut.n_diag_steps, cut.max_cost_seen);
  std::printf("waypoint field seeds %d rounds %d\n", seeded.n_seeds_used, seeded.rounds);

  std::vector<int32_t> ways((size_t)wcap), index((size_t)wcap);
  std::vector<float> xy(2 * (size_t)wcap);
  CHECK(gvx3_get_shortcut(h, 0, ways.data(), index.data(), xy.data(), wcap, nullptr));
  for (int32_t k = 0; k < cut.n_waypoints; ++k)
    if (index[(size_t)k] >= 0) std::printf("  anchor at path cell %5d: (%7.2f, %7.2f)\n", index[(size_t)k], xy[2 * (size_t)k], xy[2 * (size_t)k + 1]);
  double length = 0.0;
  for (int32_t k = 1; k < cut.n_waypoints; ++k)
    length += std::hypot((double)xy[2 * (size_t)k] - xy[2 * (size_t)k - 2], (double)xy[2 * (size_t)k + 1] - xy[2 * (size_t)k - 1]);
  std::printf("straightened length %.2f m, staircase %.2f m\n", length,
              resolution * ((path.n_cells - 1 - path.n_diagonal) + std::sqrt(2.0) * path.n_diagonal));

  // the host alternative this replaces: download the costmap and the path, shortcut on one core (the twin: the same
  // arithmetic text)
  std::vector<uint8_t> cost(G);
  std::vector<int32_t> cells((size_t)cap);
  CHECK(gv_get_costmap(h, cost.data()));
  CHECK(gv_get_nav_path(h, 0, cells.data(), nullptr, cap, nullptr));
  gvx3_shortcut_info want{};
  std::vector<int32_t> want_ways((size_t)wcap), want_index((size_t)wcap);
  std::vector<float> want_xy(2 * (size_t)wcap);
  CHECK(gvx3_shortcut_host(grid_x, grid_y, resolution, cost.data(), &cfg, cells.data(), &path.n_cells, 1, cap, wcap, GVX3_SHORTCUT_NO_CORNER,
                           &want, want_ways.data(), want_index.data(), want_xy.data()));
  int mismatches = std::memcmp(&want, &cut, sizeof(want)) != 0;
  const size_t k = (size_t)(want.n_waypoints > 0 ? want.n_waypoints : 0);
  mismatches += std::memcmp(want_ways.data(), ways.data(), k * sizeof(int32_t)) != 0;
  mismatches += std::memcmp(want_index.data(), index.data(), k * sizeof(int32_t)) != 0;
  mismatches += std::memcmp(want_xy.data(), xy.data(), 2 * k * sizeof(float)) != 0;
  std::printf("host check %s (%d mismatches)\n", mismatches ? "FAILED" : "ok", mismatches);
  gv_destroy(h);
  return mismatches ? 1 : 0;
}
