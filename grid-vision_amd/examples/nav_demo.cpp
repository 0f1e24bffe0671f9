// nav_demo.cpp -- [EXTENSION] X9: a goal behind a wall with one gap; inflate -> distance field from the goal -> a fan of
// arcs scored twice on the device, gv_score_trajectories for the obstacle cost and gv_score_nav for the distance to the
// goal -> the arc that heads for the gap wins over the straight one that points at the goal through the wall.
// Plain g++ host code over the C ABI and its C++ mirror headers:
//   g++ -std=c++17 -O2 nav_demo.cpp -o nav_demo -L.. -lgridvision_hip -Wl,-rpath,$PWD/..
// The controller's candidates never see the costmap or the field: K * P poses go to the device, two records per
// trajectory come back.  The last lines replay every gv_nav_score on the host from gv_get_nav_field and compare:
// tests/test_gpu_nav.py::test_nav_demo reads them.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../include/grid_vision/frame_flow.hpp"

int main()
{
  try {
    const uint8_t grid_x = 50, grid_y = 20;
    const double resolution = 0.1;
    const CAMParams cam{224, 224, 480, 640, 320.f, 320.f, 320.f, 240.f};
    GridVisionContext ctx(grid_x, grid_y, resolution, cam);
    OccupancyGridMap grid(ctx);
    int32_t nx = 0, ny = 0;
    double pos_x = 0.0, pos_y = 0.0;
    gv::check(gv_grid_geometry(ctx.handle(), &nx, &ny, &pos_x, &pos_y), ctx.handle(), "gv_grid_geometry");
    const size_t G = (size_t)nx * (size_t)ny;

    // the map: a wall across the whole map 12 m ahead, 0.3 m thick, with one gap from y = 4 to y = 9.  Cell (ix, iy)
    // covers x in (x_hi - (ix + 1) res, x_hi - ix res]; the log-odds layer is in grid_map order, iy * nx + ix.
    const double x_hi = pos_x + 0.5 * nx * resolution, y_hi = pos_y + 0.5 * ny * resolution;
    const double wall_x0 = 12.0, wall_x1 = 12.3, gap_y0 = 4.0, gap_y1 = 9.0;
    std::vector<float> log_odds(G, -10.0f);
    for (int32_t iy = 0; iy < ny; ++iy)
      for (int32_t ix = 0; ix < nx; ++ix) {
        const double cx = x_hi - (ix + 0.5) * resolution, cy = y_hi - (iy + 0.5) * resolution;
        if (cx > wall_x0 && cx < wall_x1 && !(cy > gap_y0 && cy < gap_y1)) log_odds[(size_t)iy * nx + ix] = 10.0f;
      }
    gv::check(gv_set_log_odds(ctx.handle(), log_odds.data()), ctx.handle(), "gv_set_log_odds");
    grid.updateMap();

    const gv_inflation infl{0.5, 1.0, 3.0, 65, 0};
    grid.setInflation(infl);
    grid.inflate();

    // the robot is a disc: a pose costs what its centre cell costs, and collides inside the inscribed radius
    gv_footprint fp{};
    fp.n_vertices = 0;
    fp.collision_cost = 253;
    fp.off_map_cost = 255;
    grid.setFootprint(fp);

    // the goal-directed half: distance to the goal over the costmap, one step a cell plus the cell's cost
    const gv_nav_config nav{253, 1, 0};
    grid.setNavConfig(nav);
    const std::vector<float> goal{22.0f, 0.0f};
    const gv_nav_info info = grid.solveNavField(goal);

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
    const std::vector<gv_traj_score> obstacle = grid.scoreTrajectories(poses, K, P);
    const std::vector<gv_nav_score> to_goal = grid.scoreNav(poses, K, P);

    // the controller's choice (DWB's GoalDist): among the arcs that do not collide, the one that ends nearest the goal
    // along the field; ties go to the straighter one
    int best = -1, collisions = 0;
    for (int32_t k = 0; k < K; ++k) {
      if (obstacle[k].first_collision >= 0) { ++collisions; continue; }
      if (to_goal[k].last >= GV_NAV_UNREACHABLE) continue;
      if (best < 0 || to_goal[k].last < to_goal[best].last ||
          (to_goal[k].last == to_goal[best].last && std::fabs(curvature[k]) < std::fabs(curvature[best])))
        best = k;
    }
    std::printf("trajectories %d poses %d collisions %d\n", K, P, collisions);
    std::printf("field rounds %d seeds %d\n", info.rounds, info.n_seeds_used);
    if (best >= 0) {
      const float *end = &poses[((size_t)best * P + (P - 1)) * 3];
      // an arc that ends behind the wall without a collision went through the gap
      std::printf("best %d curvature %.4f goal_dist %u through_gap %s\n", best, curvature[best], to_goal[best].last,
                  end[0] > wall_x1 ? "yes" : "no");
    } else {
      std::printf("best none\n");
    }
    std::printf("straight first_collision %d goal_dist %u\n", obstacle[K / 2].first_collision, to_goal[K / 2].last);

    // the host alternative this replaces: download the field, look every pose up on one core
    std::vector<uint32_t> field = grid.navField();
    int mismatches = 0;
    for (int32_t k = 0; k < K; ++k) {
      gv_nav_score want{0, GV_NAV_BLOCKED, GV_NAV_UNREACHABLE, -1, 0};
      for (int32_t p = 0; p < P; ++p) {
        const float *q = &poses[((size_t)k * P + p) * 3];
        int32_t cell = 0, m = 0;
        gv::check(gv_footprint_cells(grid_x, grid_y, resolution, &fp, q[0], q[1], q[2], &cell, 1, &m), nullptr, "gv_footprint_cells");
        const uint32_t v = m < 0 ? GV_NAV_BLOCKED : field[G - 1 - (size_t)cell];
        if (v >= GV_NAV_UNREACHABLE) ++want.n_bad;
        else {
          want.sum += v;
          if (v < want.best) { want.best = v; want.best_pose = p; }
        }
        if (p == P - 1) want.last = v;
      }
      mismatches += want.sum != to_goal[k].sum || want.last != to_goal[k].last || want.best != to_goal[k].best ||
                    want.best_pose != to_goal[k].best_pose || want.n_bad != to_goal[k].n_bad;
    }
    std::printf("host check %s (%d mismatches)\n", mismatches ? "FAILED" : "ok", mismatches);
    return mismatches ? 1 : 0;
  } catch (const gv::Error &e) {
    std::fprintf(stderr, "gv error %d: %s\n", e.code, e.what());
    return 2;
  }
}
