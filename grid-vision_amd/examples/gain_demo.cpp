// gain_demo.cpp -- [EXTENSION] X20: which frontier is worth the trip, without the map crossing the host.  A room the
// vehicle has seen: behind its right side lies a strip nobody observed, one cell wide, and then a wall; in its left wall
// is a doorway into a hall nobody has seen.  By size the long frontier on the right wins; it would reveal next to nothing.
// map -> inflate -> field from the vehicle -> gvx_frontier -> gvx2_frontier_gain (no wait in between) ranks the clusters'
// goal cells by the unknown cells in sight against the way there -> gvx2_nav_field_from_gain seeds X9's field with the
// chosen goal -> gv_nav_path from the vehicle ends on it.
// Plain g++ host code over the C headers:
//   g++ -std=c++17 -O2 gain_demo.cpp -o gain_demo -L.. -lgridvision_hip -Wl,-rpath,$PWD/..
// The last lines replay the ranking with the host twin on the downloaded layer and field and compare:
// tests/test_gpu_gain.py::test_gain_demo reads them.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../include/gridvision_hip_gain.h"

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

  // seen so far: the room |x| < 8, |y| < 6 about the vehicle at the origin (free); walls above and below it; a wall on the
  // left with a doorway 0.8 m wide; on the right nothing for 0.1 m, then a wall.  Everything else keeps the prior.  The
  // decay of one plain update (-0.2) is planted on top, so unknown stays 0.0 -> 50.
  const double x_hi = pos_x + 0.5 * nx * resolution, y_hi = pos_y + 0.5 * ny * resolution;
  std::vector<float> log_odds(G, 0.2f);
  for (int32_t iy = 0; iy < ny; ++iy)
    for (int32_t ix = 0; ix < nx; ++ix) {
      const double cx = x_hi - (ix + 0.5) * resolution, cy = y_hi - (iy + 0.5) * resolution;
      float &v = log_odds[(size_t)iy * nx + ix];
      if (std::fabs(cx) < 8.0 && std::fabs(cy) < 6.0) v = -10.0f;
      if (std::fabs(cy) >= 6.0 && std::fabs(cy) < 6.3 && cx > -8.3 && cx < 8.4) v = 10.0f;
      if (cx <= -8.0 && cx > -8.3 && std::fabs(cy) < 6.0) v = std::fabs(cy) < 0.4 ? -10.0f : 10.0f;
      if (cx >= 8.1 && cx < 8.4 && std::fabs(cy) < 6.0) v = 10.0f;
    }
  CHECK(gv_set_log_odds(h, log_odds.data()));
  CHECK(gv_update_map(h));
  const gv_inflation infl{0.1, 0.5, 3.0, 65, 0};
  CHECK(gv_set_inflation(h, &infl));
  CHECK(gv_inflate(h));
  const gv_nav_config nav{253, 1, 0};
  CHECK(gv_set_nav_config(h, &nav));
  const float vehicle[2] = {0.0f, 0.0f};
  CHECK(gv_nav_field(h, vehicle, 1, nullptr));

  // the clusters by X19's own ranking (the largest), then by gain: 4 m of sight, 10 per unknown cell against 1 per step
  gvx_frontier_config fcfg{};
  fcfg.free_max = 25;
  fcfg.unknown_min = 40;
  fcfg.unknown_max = 60;
  fcfg.max_cost = 256;
  fcfg.min_cells = 4;
  CHECK(gvx_set_frontier_config(h, &fcfg));
  gvx2_gain_config cfg{};
  cfg.free_max = 25;
  cfg.unknown_min = 40;
  cfg.unknown_max = 60;
  cfg.radius = 40;
  cfg.min_gain = 1;
  cfg.w_gain = 10;
  cfg.w_dist = 1;
  CHECK(gvx2_set_gain_config(h, &cfg));
  const int32_t cap = 16;
  gvx_frontier_info by_size{}, finfo{};
  std::vector<gvx_frontier_record> frecs((size_t)cap);
  CHECK(gvx_frontier(h, cap, 0, &by_size, frecs.data()));
  gvx2_gain_info info{};
  std::vector<gvx2_gain_record> recs((size_t)cap);
  CHECK(gvx_frontier_async(h, cap, GVX_FRONTIER_USE_FIELD, &finfo, frecs.data()));
  CHECK(gvx2_frontier_gain_async(h, GVX2_GAIN_USE_FIELD, &info, recs.data()));   // behind it on the stream: no wait in between
  CHECK(gv_synchronize(h));
  std::printf("clusters %d written %d largest %d best by size %d\n", finfo.n_clusters, finfo.n_written, finfo.largest, by_size.best);
  for (int32_t i = 0; i < info.n_candidates; ++i)
    std::printf("  cluster %d: %d cells, goal (%.2f, %.2f): unknown in sight %d, free %d, opaque %d, dist %u, score %lld, status %u\n", i,
                frecs[(size_t)i].n_cells, frecs[(size_t)i].goal_x, frecs[(size_t)i].goal_y, recs[(size_t)i].n_unknown, recs[(size_t)i].n_free,
                recs[(size_t)i].n_opaque, recs[(size_t)i].dist, (long long)recs[(size_t)i].score, recs[(size_t)i].status);
  std::printf("candidates %d ranked %d best by gain %d entry %d score %lld\n", info.n_candidates, info.n_ranked, info.best, info.best_entry,
              (long long)info.best_score);

  // the field of the chosen goal, on the device, and the path from the vehicle down it
  gv_nav_info seeded{};
  CHECK(gvx2_nav_field_from_gain(h, -1, &seeded));
  gv_nav_path_info path{};
  CHECK(gv_nav_path(h, vehicle, 1, 4096, GV_PATH_DIAGONAL, &path, nullptr));
  std::printf("goal field seeds %d rounds %d\npath cells %d status %d ends_on_goal %s\n", seeded.n_seeds_used, seeded.rounds, path.n_cells,
              path.status, path.status == GV_PATH_REACHED && path.end_entry == info.best_entry ? "yes" : "no");

  // the host alternative this replaces: download the layer and the field, cast the rays on one core (the twin: the same
  // arithmetic text) -- with the field the records were made with, the vehicle's
  CHECK(gv_nav_field(h, vehicle, 1, nullptr));
  std::vector<int8_t> i8(G);
  std::vector<uint32_t> field(G);
  gv_grid_info gi{};
  CHECK(gv_to_occupancy_grid(h, i8.data(), &gi));
  CHECK(gv_get_nav_field(h, field.data()));
  int mismatches = 0;
  if (info.n_candidates > 0) {
    std::vector<int32_t> entries;
    for (int32_t i = 0; i < info.n_candidates; ++i) entries.push_back(frecs[(size_t)i].goal_entry);
    gvx2_gain_info want{};
    std::vector<gvx2_gain_record> want_recs(entries.size());
    CHECK(gvx2_gain_host(grid_x, grid_y, resolution, i8.data(), field.data(), &cfg, (int32_t)entries.size(), entries.data(),
                         GVX2_GAIN_USE_FIELD, &want, want_recs.data()));
    mismatches += std::memcmp(&want, &info, sizeof(want)) != 0;
    mismatches += std::memcmp(want_recs.data(), recs.data(), entries.size() * sizeof(gvx2_gain_record)) != 0;
  }
  for (int32_t i = info.n_candidates; i < cap; ++i) {
    const gvx2_gain_record zero{};
    mismatches += std::memcmp(&zero, &recs[(size_t)i], sizeof(zero)) != 0;
  }
  std::printf("host check %s (%d mismatches)\n", mismatches ? "FAILED" : "ok", mismatches);
  gv_destroy(h);
  return mismatches ? 1 : 0;
}
