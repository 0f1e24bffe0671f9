// gv_api_planner_host.hip -- the host-only entry points of the planner side: the twins of the kernels' arithmetic (the
// shared headers' text in sequential loops: what the GPU tests hold the device calls to) and the host-built tables.
// None takes a handle or enqueues anything; plain C++17 without a HIP header, so a host compiler alone builds it too.
#include <algorithm>
#include <cstring>
#include <vector>

#include "gv_mppi.hpp"
#include "gv_navpath.hpp"
#include "gv_planner_rules.hpp"

using namespace gv;
using namespace gv_internal;

#define GV_HOST_TRY try {   // no exception crosses the C ABI; there is no handle to leave a text in
#define GV_HOST_CATCH } catch (...) { return GV_ERR_HIP; }

// a cost table into the caller's array when it fits; *n (if asked for) is its length either way
static int table_out(const host::InflationTable &t, uint8_t *table, int32_t cap, int32_t *n)
{
  if (n) *n = t.d2max + 1;
  if (!table || cap < t.d2max + 1) return GV_ERR_BAD_ARG;
  std::memcpy(table, t.cost.data(), t.cost.size());
  return GV_OK;
}

extern "C" {

// ---- X6, X7, X9: the tables and the footprint's cells
int gv_inflation_cost_table(const gv_inflation *cfg, double resolution, uint8_t *table, int32_t cap, int32_t *n)
{
  if (!cfg) return GV_ERR_BAD_ARG;
  GV_HOST_TRY
  host::InflationTable t;
  return host::inflation_table(*cfg, resolution, t) ? table_out(t, table, cap, n) : GV_ERR_BAD_ARG;
  GV_HOST_CATCH
}

// the twin of the kernel's geometry (host::footprint_cells), on the geometry gv_create gives
int gv_footprint_cells(uint8_t grid_x, uint8_t grid_y, double resolution, const gv_footprint *fp, float x, float y, float yaw,
                       int32_t *cells, int32_t cap, int32_t *n)
{
  if (!fp || !n) return GV_ERR_BAD_ARG;
  GV_HOST_TRY
  GridParams g{};
  if (!host::footprint_valid(*fp) || !host::grid_params(grid_x, grid_y, resolution, g)) return GV_ERR_BAD_ARG;
  std::vector<int32_t> out;
  if (!host::footprint_cells(g, *fp, x, y, yaw, out)) {
    *n = -1;
    return GV_OK;
  }
  *n = (int32_t)out.size();
  if (!cells || cap < *n) return GV_ERR_BAD_ARG;
  std::memcpy(cells, out.data(), out.size() * sizeof(int32_t));
  return GV_OK;
  GV_HOST_CATCH
}

int gv_nav_step_table(const gv_nav_config *cfg, uint32_t table[256])
{
  if (!cfg || !table || !host::nav_config_valid(*cfg)) return GV_ERR_BAD_ARG;
  host::nav_step_table(*cfg, table);
  return GV_OK;
}

// ---- X17: path_next (gv_navpath.hpp) over a plain array, one start after the other, one step after the other
int gv_nav_path_host(uint8_t grid_x, uint8_t grid_y, double resolution, const uint32_t *field, const float *starts_xy, int32_t S,
                     int32_t cap, uint32_t flags, gv_nav_path_info *info, int32_t *entries, float *paths_xy)
{
  if (!field || !starts_xy || !info || !path_call_ok(S, cap, flags)) return GV_ERR_BAD_ARG;
  GridParams g{};
  if (!host::grid_params(grid_x, grid_y, resolution, g)) return GV_ERR_BAD_ARG;
  const int32_t nx = g.nx;
  const int32_t ny = g.ny;
  const auto at = [field, nx, ny](int32_t x, int32_t y) {   // any array of G values; path_next also asks one cell off the map
    return x >= 0 && x < nx && y >= 0 && y < ny ? field[(size_t)y * (size_t)nx + (size_t)x] : GV_NAV_BLOCKED;
  };
  const bool diagonal = (flags & GV_PATH_DIAGONAL) != 0u;
  for (int32_t s = 0; s < S; ++s) {
    const int32_t e0 = host::nav_seed_entry(g, starts_xy[2 * s], starts_xy[2 * s + 1]);
    uint32_t v = e0 >= 0 ? field[e0] : GV_NAV_BLOCKED;
    gv_nav_path_info rec = path_record_begin(e0, v);
    if (rec.status == GV_PATH_REACHED) {   // a start that walks
      int32_t y = e0 / nx, x = e0 - y * nx;
      const size_t first = (size_t)s * (size_t)cap;
      int32_t n = 0, n_diag = 0;
      for (;;) {
        if (entries) entries[first + (size_t)n] = y * nx + x;
        if (paths_xy) {
          paths_xy[2 * (first + (size_t)n)] = path_centre(g.pos_x, g.off_x, g.res, g.nx, x);
          paths_xy[2 * (first + (size_t)n) + 1] = path_centre(g.pos_y, g.off_y, g.res, g.ny, y);
        }
        ++n;
        if (v == 0u) break;                                   // rec.status is GV_PATH_REACHED
        if (n == cap) { rec.status = GV_PATH_TRUNCATED; break; }
        bool diag = false;
        if (!path_next(at, nx, g.ny, diagonal, x, y, v, diag)) { rec.status = GV_PATH_STUCK; break; }
        n_diag += diag ? 1 : 0;
      }
      rec.n_cells = n;
      rec.end_value = v;
      rec.end_entry = y * nx + x;
      rec.n_diagonal = n_diag;
    }
    info[s] = rec;
  }
  return GV_OK;
}

// ---- X10: motion_step (gv_motion.hpp), one trajectory after the other, one step after the other
int gv_rollout_poses(const gv_motion_model *m, const double start[3], const float *controls, int32_t K, int32_t P,
                     uint32_t flags, float *poses_out)
{
  if (!m || !poses_out || !motion_model_valid(*m) || !rollout_ok(start, controls, K, P, flags, GV_ROLLOUT_CONSTANT))
    return GV_ERR_BAD_ARG;
  const MotionModel mm{m->model, m->dt};
  const size_t C = (size_t)motion_controls(m->model);
  const bool constant = (flags & GV_ROLLOUT_CONSTANT) != 0;
  for (size_t k = 0; k < (size_t)K; ++k) {
    double X = start[0], Y = start[1], T = start[2];
    for (size_t p = 0; p < (size_t)P; ++p) {
      const float *u = controls + (constant ? k : k * (size_t)P + p) * C;
      motion_step(mm, u, X, Y, T);
      float *q = poses_out + (k * (size_t)P + p) * 3;
      q[0] = (float)X; q[1] = (float)Y; q[2] = (float)T;
    }
  }
  return GV_OK;
}

int gv_control_select(const gv_critic_weights *w, const gv_traj_score *traj, const gv_nav_score *nav, int32_t K,
                      gv_control_result *result, uint64_t *totals)
{
  if (!w || !traj || !result || !critic_weights_valid(*w) || !shape_ok(K, 1, false)) return GV_ERR_BAD_ARG;
  if (critic_nav_used(*w) && !nav) return GV_ERR_BAD_ARG;
  control_select_host(*w, traj, nav, nullptr, 0u, 0u, K, result, totals);
  return GV_OK;
}

// gv_control_select with the third record (X13)
int gv_control_select_dyn(const gv_critic_weights *w, const gv_traj_score *traj, const gv_nav_score *nav,
                          const gv_dyn_score *dyn, const gv_dyn_config *cfg, int32_t K, gv_control_result *result,
                          uint64_t *totals)
{
  if (!cfg) return gv_control_select(w, traj, nav, K, result, totals);
  if (!w || !traj || !dyn || !result || !critic_weights_valid(*w) || !shape_ok(K, 1, false) || cfg->w_sum > 65535u ||
      cfg->w_max > 65535u || (critic_nav_used(*w) && !nav))
    return GV_ERR_BAD_ARG;
  control_select_host(*w, traj, nav, dyn, cfg->w_sum, cfg->w_max, K, result, totals);
  return GV_OK;
}

// ---- X11, X12: gv_mppi.hpp's text in loops
int gv_mppi_words(uint64_t seed, uint64_t iteration, uint32_t k, uint32_t p, uint32_t words[4])
{
  if (!words) return GV_ERR_BAD_ARG;
  mppi_words(seed, iteration, k, p, words);
  return GV_OK;
}

int gv_mppi_sample_controls(const gv_mppi_config *cfg, int32_t C, const float *nominal, int32_t K, int32_t P, uint64_t seed,
                            uint64_t iteration, uint32_t flags, float *controls_out)
{
  if (!cfg || (C != 2 && C != 3) || !nominal || !controls_out || !shape_ok(K, P, true) || !mppi_config_valid(*cfg, C) ||
      (flags & ~(uint32_t)GV_MPPI_SHIFT) != 0)
    return GV_ERR_BAD_ARG;
  for (size_t i = 0; i < (size_t)P * (size_t)C; ++i)
    if (!std::isfinite(nominal[i])) return GV_ERR_BAD_ARG;
  const bool shift = (flags & GV_MPPI_SHIFT) != 0;
  for (size_t k = 0; k < (size_t)K; ++k)
    for (size_t p = 0; p < (size_t)P; ++p)
      mppi_sample(*cfg, C, nominal, P, seed, iteration, shift, (uint32_t)k, (uint32_t)p, controls_out + (k * (size_t)P + p) * (size_t)C);
  return GV_OK;
}

// the chain, trajectory after trajectory
int gv_mppi_constrain(const gv_mppi_limits *lim, const gv_motion_model *m, float *controls, int32_t K, int32_t P)
{
  if (!lim || !m || !controls || !shape_ok(K, P, true) || !mppi_limits_valid(*lim) || !motion_model_valid(*m) ||
      (lim->min_turn_radius > 0.0 && m->model != GV_MOTION_DIFF))
    return GV_ERR_BAD_ARG;
  const int32_t C = motion_controls(m->model);
  const MppiChain L = mppi_chain(*lim, m->dt);
  for (size_t k = 0; k < (size_t)K; ++k) {
    float s[3] = {L.u_prev[0], L.u_prev[1], L.u_prev[2]};
    float *u = controls + k * (size_t)P * (size_t)C;
    for (size_t p = 0; p < (size_t)P; ++p) {
      float q[3] = {0.0f, 0.0f, 0.0f};
      for (int32_t c = 0; c < C; ++c) q[c] = u[p * (size_t)C + (size_t)c];
      mppi_constrain_step(L, C, s, q);
      for (int32_t c = 0; c < C; ++c) u[p * (size_t)C + (size_t)c] = q[c];
    }
  }
  return GV_OK;
}

// the 64 partial sums and the tree
int gv_mppi_control_costs(const gv_mppi_config *cfg, const gv_mppi_limits *lim, int32_t C, const float *controls,
                          const float *nominal, int32_t K, int32_t P, uint32_t sample_flags, double *g_out)
{
  if (!cfg || !lim || (C != 2 && C != 3) || !controls || !nominal || !g_out || !shape_ok(K, P, true) ||
      !mppi_config_valid(*cfg, C) || !mppi_limits_valid(*lim) || (sample_flags & ~(uint32_t)GV_MPPI_SHIFT) != 0)
    return GV_ERR_BAD_ARG;
  double qc[3] = {0.0, 0.0, 0.0};
  for (int32_t c = 0; c < C; ++c) qc[c] = mppi_cost_scale(lim->gamma, cfg->sigma[c]);
  const bool shift = (sample_flags & GV_MPPI_SHIFT) != 0;
  const size_t J = (size_t)P * (size_t)C;
  for (size_t k = 0; k < (size_t)K; ++k) {
    double a[kMppiCostLanes];
    for (int32_t l = 0; l < kMppiCostLanes; ++l) a[l] = mppi_cost_lane(qc, C, nominal, P, shift, controls + k * J, l);
    for (int32_t w = kMppiCostLanes / 2; w >= 1; w /= 2)
      for (int32_t l = 0; l < w; ++l) a[l] = a[l] + a[l + w];
    g_out[k] = a[0];
  }
  return GV_OK;
}

// The sequential definition: the admitted trajectories in index order, one column after the other, sums in index
// order.  control_costs null: x_k is the totals' difference alone, gv_mppi_average.
int gv_mppi_average_cc(const gv_mppi_config *cfg, int32_t C, const float *controls, const uint64_t *totals,
                       const double *control_costs, int32_t K, int32_t P, const float *nominal_in, float *nominal_out)
{
  if (!cfg || (C != 2 && C != 3) || !controls || !totals || !nominal_in || !nominal_out || !shape_ok(K, P, true) ||
      !mppi_config_valid(*cfg, C))
    return GV_ERR_BAD_ARG;
  GV_HOST_TRY
  const size_t J = (size_t)P * (size_t)C;
  uint64_t best = UINT64_MAX;
  for (int32_t k = 0; k < K; ++k) best = std::min(best, totals[k]);
  if (best == UINT64_MAX) {
    std::memmove(nominal_out, nominal_in, J * sizeof(float));
    return GV_OK;
  }
  std::vector<double> e((size_t)K, -1.0);
  double S = 0.0;
  if (control_costs) {
    bool first = true;
    double xm = 0.0;
    for (int32_t k = 0; k < K; ++k)
      if (totals[k] != UINT64_MAX) {
        const double x = mppi_cost_x(totals[k], best, control_costs[k]);
        if (first || x < xm) xm = x;
        first = false;
      }
    for (int32_t k = 0; k < K; ++k)
      if (totals[k] != UINT64_MAX) {
        e[(size_t)k] = mppi_weight_cc(mppi_cost_x(totals[k], best, control_costs[k]), xm, cfg->lambda);
        S = S + e[(size_t)k];
      }
  } else {
    for (int32_t k = 0; k < K; ++k)
      if (totals[k] != UINT64_MAX) {
        e[(size_t)k] = mppi_weight(totals[k], best, cfg->lambda);
        S = S + e[(size_t)k];
      }
  }
  for (size_t j = 0; j < J; ++j) {
    double N = 0.0;
    for (size_t k = 0; k < (size_t)K; ++k)
      if (e[k] >= 0.0) N = N + e[k] * (double)controls[k * J + j];
    nominal_out[j] = (float)(N / S);
  }
  return GV_OK;
  GV_HOST_CATCH
}

int gv_mppi_average(const gv_mppi_config *cfg, int32_t C, const float *controls, const uint64_t *totals, int32_t K,
                    int32_t P, const float *nominal_in, float *nominal_out)
{
  return gv_mppi_average_cc(cfg, C, controls, totals, nullptr, K, P, nominal_in, nominal_out);
}

// ---- X13: gv_dyn.hpp's text in loops, one trajectory after the other, one pose after the other
int gv_dyn_cost_table(const gv_dyn_config *cfg, uint8_t *table, int32_t cap, int32_t *n)
{
  if (!cfg) return GV_ERR_BAD_ARG;
  GV_HOST_TRY
  host::InflationTable t;
  return dyn_config_table(*cfg, t) ? table_out(t, table, cap, n) : GV_ERR_BAD_ARG;
  GV_HOST_CATCH
}

int gv_dyn_score_poses(const gv_dyn_config *cfg, const gv_moving_object *objs, int32_t n, const float *poses, int32_t K,
                       int32_t P, gv_dyn_score *scores, uint8_t *pose_cost)
{
  if (!cfg || !batch_ok(poses, scores, K, P, 0u, 0u) || !moving_objects_ok(objs, n)) return GV_ERR_BAD_ARG;
  GV_HOST_TRY
  host::InflationTable t;
  if (!dyn_config_table(*cfg, t)) return GV_ERR_BAD_ARG;
  const DynParams c = dyn_params(*cfg, t.d2max + 1);
  std::vector<DynObject> rows((size_t)n);
  for (int32_t j = 0; j < n; ++j) rows[(size_t)j] = dyn_object(objs[j]);
  for (size_t k = 0; k < (size_t)K; ++k) {
    DynAccum acc;
    for (int32_t p = 0; p < P; ++p) {
      double best = INFINITY;
      int32_t best_j = -1;
      dyn_pose_min(c, rows.data(), n, 0, 1, poses + (k * (size_t)P + (size_t)p) * 3, p, best, best_j);
      const int32_t cost = dyn_cost(c, t.cost.data(), best);
      dyn_accumulate(c, p, cost, best, best_j, acc);
      if (pose_cost) pose_cost[k * (size_t)P + (size_t)p] = (uint8_t)cost;
    }
    scores[k] = dyn_record(acc);
  }
  return GV_OK;
  GV_HOST_CATCH
}

// ---- X14: gv_track.hpp's text, the association as a literal sort
int gv_track_step(const gv_track_config *cfg, gv_track *tracks, int32_t *n_tracks, uint32_t *next_id, const gv_lshape_pose *dets,
                  int32_t n, double dt, const gv_transform *motion, gv_track_info *info, gv_moving_object *objs, int32_t *n_objs)
{
  if (!cfg || !track_config_valid(*cfg) || !tracks || !n_tracks || !next_id || !track_update_ok(dets, n, dt, motion) ||
      (objs != nullptr) != (n_objs != nullptr))
    return GV_ERR_BAD_ARG;
  GV_HOST_TRY
  std::vector<TrackState> st(1);
  if (!track_state_from(tracks, *n_tracks, *next_id, st[0])) return GV_ERR_BAD_ARG;
  track_step(track_params(*cfg), st[0], dets, n, dt, motion, info, objs, n_objs);
  *n_tracks = track_state_live(st[0], tracks, kTrackSlots);
  *next_id = st[0].next_id;
  return GV_OK;
  GV_HOST_CATCH
}

}  // extern "C"
