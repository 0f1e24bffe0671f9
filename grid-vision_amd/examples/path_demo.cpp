// path_demo.cpp -- [EXTENSION] X17: plan, then follow the plan, without the plan crossing the host.  A wall with one gap,
// the goal behind it: inflate -> distance field from the goal (X9) -> gv_nav_path walks it downhill from the vehicle ->
// gv_nav_field_from_path turns that path into the field nav2's PathDist critic reads -> a fan of arcs scored against it
// with gv_score_nav; the arc that follows the path wins.
// Plain g++ host code over the two C headers:
//   g++ -std=c++17 -O2 path_demo.cpp -o path_demo -L.. -lgridvision_hip -Wl,-rpath,$PWD/..
// The host sees 32 bytes of record, and here, for the printout, the path's cell centres; neither field leaves the device
// except for the last lines, which replay the walk with the host twin on the downloaded goal field and compare:
// tests/test_gpu_path.py::test_path_demo reads them.
#include <cmath>
#include <cstdio>
#include <vector>

#include "../../include/gridvision_hip_path.h"

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

  // the map of nav_demo.cpp: a wall across the whole map 12 m ahead, 0.3 m thick, with one gap from y = 4 to y = 9
  const double x_hi = pos_x + 0.5 * nx * resolution, y_hi = pos_y + 0.5 * ny * resolution;
  const double wall_x0 = 12.0, wall_x1 = 12.3, gap_y0 = 4.0, gap_y1 = 9.0;
  std::vector<float> log_odds(G, -10.0f);
  for (int32_t iy = 0; iy < ny; ++iy)
    for (int32_t ix = 0; ix < nx; ++ix) {
      const double cx = x_hi - (ix + 0.5) * resolution, cy = y_hi - (iy + 0.5) * resolution;
      if (cx > wall_x0 && cx < wall_x1 && !(cy > gap_y0 && cy < gap_y1)) log_odds[(size_t)iy * nx + ix] = 10.0f;
    }
  CHECK(gv_set_log_odds(h, log_odds.data()));
  CHECK(gv_update_map(h));
  const gv_inflation infl{0.5, 1.0, 3.0, 65, 0};
  CHECK(gv_set_inflation(h, &infl));
  CHECK(gv_inflate(h));
  gv_footprint fp{};
  fp.n_vertices = 0;   // a disc: a pose costs what its centre cell costs
  fp.collision_cost = 253;
  fp.off_map_cost = 255;
  CHECK(gv_set_footprint(h, &fp));

  // plan: the field of the goal, then the path from the vehicle down that field
  const gv_nav_config nav{253, 1, 0};
  CHECK(gv_set_nav_config(h, &nav));
  const float goal[2] = {22.0f, 0.0f}, vehicle[2] = {0.0f, 0.0f};
  CHECK(gv_nav_field(h, goal, 1, nullptr));
  const int32_t cap = 4096;
  gv_nav_path_info rec{};
  CHECK(gv_nav_path(h, vehicle, 1, cap, GV_PATH_DIAGONAL, &rec, nullptr));   // the path stays on the device
  std::vector<int32_t> entries((size_t)cap);
  std::vector<float> xy((size_t)cap * 2);
  CHECK(gv_get_nav_path(h, 0, entries.data(), xy.data(), cap, nullptr));      // for the printout and the check only
  int in_gap = 0, in_wall = 0;
  double length = 0.0;
  for (int32_t i = 0; i < rec.n_cells; ++i) {
    const double cx = xy[2 * i], cy = xy[2 * i + 1];
    if (cx > wall_x0 && cx < wall_x1) (cy > gap_y0 && cy < gap_y1 ? in_gap : in_wall) += 1;
    if (i > 0) length += std::hypot(cx - xy[2 * i - 2], cy - xy[2 * i - 1]);
  }
  const bool through_gap = rec.status == GV_PATH_REACHED && in_gap > 0 && in_wall == 0;
  std::printf("path cells %d diagonal %d status %d length %.1f m through_gap %s\n", rec.n_cells, rec.n_diagonal, rec.status, length,
              through_gap ? "yes" : "no");

  // the host alternative this replaces: download the field, walk it on one core (the twin: the same arithmetic text)
  std::vector<uint32_t> field(G);
  CHECK(gv_get_nav_field(h, field.data()));
  gv_nav_path_info want{};
  std::vector<int32_t> want_entries((size_t)cap);
  CHECK(gv_nav_path_host(grid_x, grid_y, resolution, field.data(), vehicle, 1, cap, GV_PATH_DIAGONAL, &want, want_entries.data(), nullptr));
  int mismatches = want.status != rec.status || want.n_cells != rec.n_cells || want.start_value != rec.start_value ||
                   want.end_entry != rec.end_entry || want.n_diagonal != rec.n_diagonal;
  for (int32_t i = 0; i < rec.n_cells && i < want.n_cells; ++i) mismatches += entries[(size_t)i] != want_entries[(size_t)i];

  // follow the plan: the field seeded by every cell of the path, on the device, and a fan of arcs scored against it
  gv_nav_info seeded{};
  CHECK(gv_nav_field_from_path(h, 0, &seeded));
  std::printf("path field seeds %d rounds %d\n", seeded.n_seeds_used, seeded.rounds);
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
  std::vector<gv_traj_score> obstacle((size_t)K);
  std::vector<gv_nav_score> to_path((size_t)K);
  CHECK(gv_score_trajectories(h, poses.data(), K, P, 0, obstacle.data(), nullptr));
  CHECK(gv_score_nav(h, poses.data(), K, P, 0, to_path.data()));
  // PathDist: among the arcs that neither collide nor leave the reachable map, the smallest summed distance to the path;
  // ties go to the straighter one
  int best = -1;
  for (int32_t k = 0; k < K; ++k) {
    if (obstacle[k].first_collision >= 0 || to_path[k].n_bad > 0) continue;
    if (best < 0 || to_path[k].sum < to_path[best].sum ||
        (to_path[k].sum == to_path[best].sum && std::fabs(curvature[k]) < std::fabs(curvature[best])))
      best = k;
  }
  bool follows = false;
  if (best >= 0) {
    const int mirrored = K - 1 - best;   // the same arc to the other side: away from the gap
    follows = curvature[best] > 0.0 && to_path[best].sum < to_path[mirrored].sum;   // the gap, and the path, are to the left
    std::printf("best %d curvature %.4f path_dist_sum %llu mirrored %llu straight %llu follows_path %s\n", best, curvature[best],
                (unsigned long long)to_path[best].sum, (unsigned long long)to_path[mirrored].sum,
                (unsigned long long)to_path[K / 2].sum, follows ? "yes" : "no");
  } else {
    std::printf("best none\n");
  }
  std::printf("host check %s (%d mismatches)\n", mismatches ? "FAILED" : "ok", mismatches);
  CHECK(gv_destroy(h));
  return through_gap && follows && seeded.n_seeds_used == rec.n_cells && mismatches == 0 ? 0 : 1;
}
