// search_demo.cpp -- [EXTENSION] X18: a vehicle that lost its pose.  A corner of two walls is on the map; the scan sees
// it from a pose 8 m and 0.1 rad away from where odometry believes the vehicle is.  One gv_match_search over a window of
// +-8.8 m x +-8.8 m x +-0.12 rad recovers the pose; gv_match_scan's window ends at +-3.2 m.  Plain g++ host code over
// the C headers:
//   g++ -std=c++17 -O2 search_demo.cpp -o search_demo -I../../include -L.. -lgridvision_hip -Wl,-rpath,$PWD/..
// The last lines repeat the search on the host (gv_match_search_host over the downloaded costmap) and compare the
// record's 64 bytes and the stats' 32: tests/test_gpu_search.py::test_search_demo reads them.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../include/gridvision_hip_search.h"

#define CK(call)                                                                       \
  do {                                                                                 \
    const int rc_ = (call);                                                            \
    if (rc_) {                                                                         \
      std::fprintf(stderr, "%s: error %d (%s)\n", #call, rc_, h ? gv_last_error(h) : ""); \
      return 2;                                                                        \
    }                                                                                  \
  } while (0)

int main()
{
  const uint8_t grid_x = 20, grid_y = 20;
  const double res = 0.1;
  const gv_cam_params cam{224, 224, 480, 640, 320.f, 320.f, 320.f, 240.f};
  gv_handle h = nullptr;
  CK(gv_create(&h, grid_x, grid_y, res, &cam, 0));
  int32_t nx = 0, ny = 0;
  double pos_x = 0, pos_y = 0;
  CK(gv_grid_geometry(h, &nx, &ny, &pos_x, &pos_y));
  const gv_transform base_lidar{0, 0, 0, 1, 0, 0, 0};
  CK(gv_set_transforms(h, nullptr, nullptr, &base_lidar));

  // the map: a wall along cells (60..150, 120) and one along (60, 60..120); lethal where the log-odds are high
  std::vector<int> wall_x, wall_y;
  for (int ix = 60; ix <= 150; ++ix) { wall_x.push_back(ix); wall_y.push_back(120); }
  for (int iy = 60; iy < 120; ++iy) { wall_x.push_back(60); wall_y.push_back(iy); }
  const size_t G = (size_t)nx * (size_t)ny;
  std::vector<float> lo(G, -10.0f);
  for (size_t k = 0; k < wall_x.size(); ++k) lo[(size_t)wall_y[k] * (size_t)nx + (size_t)wall_x[k]] = 10.0f;   // cell order
  CK(gv_set_log_odds(h, lo.data()));
  CK(gv_update_map(h));
  gv_inflation infl{};
  infl.inscribed_radius = 0.05;
  infl.inflation_radius = 0.6;
  infl.cost_scaling_factor = 6.0;
  infl.lethal_threshold = 65;
  CK(gv_set_inflation(h, &infl));
  CK(gv_inflate(h));

  // the scan: the lethal cells' centres (read back from the costmap: entry e is cell G - 1 - e) as the vehicle sees them
  // from its true pose; odometry says (0, 0, 0)
  std::vector<uint8_t> cost(G);
  CK(gv_get_costmap(h, cost.data()));
  wall_x.clear();
  wall_y.clear();
  for (size_t e = 0; e < G; ++e)
    if (cost[e] == 254) {
      wall_x.push_back((int)((G - 1 - e) % (size_t)nx));
      wall_y.push_back((int)((G - 1 - e) / (size_t)nx));
    }
  const double tx = -6.5, ty = 4.8, tyaw = 0.1;
  const size_t n = wall_x.size();
  std::vector<float> x(n), y(n), z(n, 0.3f);
  for (size_t k = 0; k < n; ++k) {
    const double gx = pos_x + 0.5 * nx * res - (wall_x[k] + 0.5) * res, gy = pos_y + 0.5 * ny * res - (wall_y[k] + 0.5) * res;
    const double dx = gx - tx, dy = gy - ty;
    x[k] = (float)(std::cos(tyaw) * dx + std::sin(tyaw) * dy);
    y[k] = (float)(-std::sin(tyaw) * dx + std::cos(tyaw) * dy);
  }
  CK(gv_cloud_upload_xyz(h, x.data(), y.data(), z.data(), n));

  gv_search_config cfg{};
  cfg.wx = 88; cfg.wy = 88; cfg.wt = 12;
  cfg.stride = 1;
  cfg.yaw_step = 0.01;
  cfg.min_points = 50;
  cfg.block_log2 = 3;
  CK(gv_set_search_config(h, &cfg));
  const gv_match_guess guess{0.0, 0.0, 0.0};
  gv_match_result r{};
  gv_search_stats st{};
  CK(gv_match_search(h, &guess, 0, &r, &st));
  std::printf("window %d x %d x %d candidates, %u blocks, %u survive, %u candidates scored exactly\n", 2 * cfg.wt + 1, 2 * cfg.wy + 1,
              2 * cfg.wx + 1, st.n_blocks, st.n_survivors, st.n_scored);
  std::printf("used points %u guess score %u best score %u valid %d, bound max %u, seed's best %u\n", r.n_used, r.guess_score, r.best_score,
              r.valid, st.bound_max, st.lower_score);
  std::printf("best shift t %d j %d i %d\n", r.best_t, r.best_j, r.best_i);
  std::printf("recovered pose x %.4f y %.4f yaw %.4f (true %.4f %.4f %.4f)\n", r.x, r.y, r.yaw, tx, ty, tyaw);

  // the host alternative: download the costmap, search on one core
  gv_match_result want{};
  gv_search_stats want_st{};
  CK(gv_match_search_host(grid_x, grid_y, res, cost.data(), x.data(), y.data(), z.data(), n, &base_lidar, nullptr, &cfg, &guess, 0, &want,
                          &want_st));
  const bool same = std::memcmp(&want, &r, sizeof(r)) == 0 && std::memcmp(&want_st, &st, sizeof(st)) == 0;
  std::printf("host twin %s\n", same ? "ok" : "FAILED");
  gv_destroy(h);
  return same && r.valid ? 0 : 1;
}
