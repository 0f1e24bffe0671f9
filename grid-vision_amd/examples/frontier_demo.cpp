// frontier_demo.cpp -- [EXTENSION] X19: where to go when nobody supplies a goal, without the map crossing the host.  A
// room the vehicle has seen (free inside a disc, unknown outside it) with a wall in it: map -> inflate -> gvx_frontier
// finds the clusters of free cells that border unknown space -> gvx_nav_field_from_frontier seeds X9's distance field
// with every cell of every written cluster -> gv_nav_path from the vehicle ends on the nearest reachable frontier cell.
// Plain g++ host code over the C headers:
//   g++ -std=c++17 -O2 frontier_demo.cpp -o frontier_demo -L.. -lgridvision_hip -Wl,-rpath,$PWD/..
// The host sees 32 bytes of info, the records and 32 bytes of path record; the last lines replay the clustering with the
// host twin on the downloaded layer and compare: tests/test_gpu_frontier.py::test_frontier_demo reads them.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../include/gridvision_hip_frontier.h"

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

  // seen so far: a disc of 8 m about the vehicle at the origin (free), a wall 3 m ahead with its ends inside the disc;
  // everything else keeps the prior.  The decay of one plain update (-0.2) is planted on top, so unknown stays 0.0 -> 50.
  const double x_hi = pos_x + 0.5 * nx * resolution, y_hi = pos_y + 0.5 * ny * resolution;
  std::vector<float> log_odds(G, 0.2f);
  for (int32_t iy = 0; iy < ny; ++iy)
    for (int32_t ix = 0; ix < nx; ++ix) {
      const double cx = x_hi - (ix + 0.5) * resolution, cy = y_hi - (iy + 0.5) * resolution;
      if (std::hypot(cx, cy) < 8.0) log_odds[(size_t)iy * nx + ix] = -10.0f;
      if (cx > 3.0 && cx < 3.3 && std::fabs(cy) < 5.0) log_odds[(size_t)iy * nx + ix] = 10.0f;
    }
  CHECK(gv_set_log_odds(h, log_odds.data()));
  CHECK(gv_update_map(h));
  const gv_inflation infl{0.5, 1.0, 3.0, 65, 0};
  CHECK(gv_set_inflation(h, &infl));
  CHECK(gv_inflate(h));

  // the clusters: free 0..25, unknown 40..60, cells the inflation forbids left out, clusters of 5 cells at least
  gvx_frontier_config cfg{};
  cfg.free_max = 25;
  cfg.unknown_min = 40;
  cfg.unknown_max = 60;
  cfg.max_cost = 253;
  cfg.min_cells = 5;
  CHECK(gvx_set_frontier_config(h, &cfg));
  const int32_t cap = 64;
  gvx_frontier_info info{};
  std::vector<gvx_frontier_record> recs((size_t)cap);
  CHECK(gvx_frontier(h, cap, 0, &info, recs.data()));
  std::printf("frontier cells %d components %d clusters %d written %d largest %d best %d\n", info.n_frontier_cells, info.n_components,
              info.n_clusters, info.n_written, info.largest, info.best);
  for (int32_t i = 0; i < info.n_written && i < 4; ++i)
    std::printf("  cluster %d: %d cells, x %d..%d y %d..%d, goal (%.2f, %.2f)\n", i, recs[(size_t)i].n_cells, recs[(size_t)i].min_x,
                recs[(size_t)i].max_x, recs[(size_t)i].min_y, recs[(size_t)i].max_y, recs[(size_t)i].goal_x, recs[(size_t)i].goal_y);

  // the field of every written cluster's cells, on the device, and the path from the vehicle down it
  const gv_nav_config nav{253, 1, 0};
  CHECK(gv_set_nav_config(h, &nav));
  gv_nav_info seeded{};
  CHECK(gvx_nav_field_from_frontier(h, -1, &seeded));
  std::printf("frontier field seeds %d rounds %d\n", seeded.n_seeds_used, seeded.rounds);
  const float vehicle[2] = {0.0f, 0.0f};
  gv_nav_path_info rec{};
  CHECK(gv_nav_path(h, vehicle, 1, 4096, GV_PATH_DIAGONAL, &rec, nullptr));
  std::vector<uint32_t> labels(G);
  CHECK(gvx_get_frontier_labels(h, labels.data()));
  bool on_frontier = false;
  if (rec.status == GV_PATH_REACHED && rec.end_entry >= 0)
    for (int32_t i = 0; i < info.n_written; ++i) on_frontier = on_frontier || labels[(size_t)rec.end_entry] == (uint32_t)recs[(size_t)i].label;
  std::printf("path cells %d status %d ends_on_frontier %s\n", rec.n_cells, rec.status, on_frontier ? "yes" : "no");

  // with the field of the vehicle: every cluster ranked by its distance from it
  CHECK(gv_nav_field(h, vehicle, 1, nullptr));
  gvx_frontier_info ranked{};
  std::vector<gvx_frontier_record> by_field((size_t)cap);
  CHECK(gvx_frontier(h, cap, GVX_FRONTIER_USE_FIELD, &ranked, by_field.data()));
  if (ranked.best >= 0)
    std::printf("nearest cluster %d field_min %u goal (%.2f, %.2f)\n", ranked.best, by_field[(size_t)ranked.best].field_min,
                by_field[(size_t)ranked.best].goal_x, by_field[(size_t)ranked.best].goal_y);

  // the host alternative this replaces: download the layers, flood on one core (the twin: the same arithmetic text)
  std::vector<int8_t> i8(G);
  std::vector<uint8_t> cost(G);
  std::vector<uint32_t> field(G), want_labels(G);
  gv_grid_info gi{};
  CHECK(gv_to_occupancy_grid(h, i8.data(), &gi));
  CHECK(gv_get_costmap(h, cost.data()));
  CHECK(gv_get_nav_field(h, field.data()));
  gvx_frontier_info want{};
  std::vector<gvx_frontier_record> want_recs((size_t)cap);
  CHECK(gvx_frontier_host(grid_x, grid_y, resolution, i8.data(), cost.data(), field.data(), &cfg, cap, GVX_FRONTIER_USE_FIELD, &want,
                          want_recs.data(), want_labels.data()));
  CHECK(gvx_get_frontier_labels(h, labels.data()));
  int mismatches = std::memcmp(&want, &ranked, sizeof(want)) != 0;
  mismatches += std::memcmp(want_recs.data(), by_field.data(), (size_t)cap * sizeof(gvx_frontier_record)) != 0;
  mismatches += std::memcmp(want_labels.data(), labels.data(), G * sizeof(uint32_t)) != 0;
  std::printf("host check %s (%d mismatches)\n", mismatches ? "FAILED" : "ok", mismatches);
  gv_destroy(h);
  return mismatches ? 1 : 0;
}
