// gv_planner_rules.hpp -- what the planner's device calls (gv_api_planner.hip, gv_api_control.hip) and their host-only
// twins (gv_api_planner_host.hip) check alike, and the host-only selection.  Plain C++: no HIP header, no handle.
#pragma once

#include <cmath>
#include <cstring>

#include "gv_host_math.hpp"
#include "gv_motion.hpp"
#include "gv_track.hpp"   // and gv_dyn.hpp

namespace gv_internal __attribute__((visibility("hidden"))) {
using namespace gv;

// the shape of a batch: P in 1..4096, K in 0..2^20, and where the call makes K * P of something, K * P <= 2^24
inline bool shape_ok(int32_t K, int32_t P, bool cap_product)
{
  return P >= 1 && P <= 4096 && K >= 0 && K <= (1 << 20) && (!cap_product || (int64_t)K * (int64_t)P <= (int64_t)(1 << 24));
}

// a sampler's batch: (K, P, 3) poses and K records, flags within `allowed`
inline bool batch_ok(const float *poses, const void *scores, int32_t K, int32_t P, uint32_t flags, uint32_t allowed)
{
  return poses && scores && shape_ok(K, P, false) && (flags & ~allowed) == 0;
}

// a handle configuration: null turns it off, a rejected one (`valid` false) leaves the one in force alone
template <typename T>
int set_config(const T *cfg, bool valid, T &dst, bool &set)
{
  if (cfg && !valid) return GV_ERR_BAD_ARG;
  if (cfg) dst = *cfg;
  set = cfg != nullptr;
  return GV_OK;
}

// ---- X10
inline bool motion_model_valid(const gv_motion_model &m)
{
  return (m.model == GV_MOTION_DIFF || m.model == GV_MOTION_OMNI) && std::isfinite(m.dt) && m.dt > 0.0 && m.flags == 0u;
}

// a rollout's batch: a finite start, K * P * C controls (K * C with GV_ROLLOUT_CONSTANT), flags within `allowed`
inline bool rollout_ok(const double *start, const float *controls, int32_t K, int32_t P, uint32_t flags, uint32_t allowed)
{
  return start && controls && std::isfinite(start[0]) && std::isfinite(start[1]) && std::isfinite(start[2]) &&
         shape_ok(K, P, true) && (flags & ~allowed) == 0;
}

inline bool critic_weights_valid(const gv_critic_weights &w)
{
  return w.w_cost_sum <= 65535u && w.w_max_cost <= 65535u && w.w_nav_last <= 65535u && w.w_nav_sum <= 65535u &&
         w.w_nav_best <= 65535u && w.flags == 0u;
}

// what gv_control_step_async and gv_mppi_update_async refuse alike
inline bool control_args_ok(const gv_critic_weights *w, uint32_t flags, const gv_control_result *result, const uint64_t *totals)
{
  return w && result && critic_weights_valid(*w) && (flags & ~(uint32_t)GV_CONTROL_KEEP_TOTALS) == 0 &&
         (!(flags & GV_CONTROL_KEEP_TOTALS) || totals);
}

// control_total / control_take (gv_motion.hpp) in a loop; dyn null: the two records alone
inline void control_select_host(const gv_critic_weights &w, const gv_traj_score *traj, const gv_nav_score *nav, const gv_dyn_score *dyn,
                                uint32_t w_dyn_sum, uint32_t w_dyn_max, int32_t K, gv_control_result *result, uint64_t *totals)
{
  const bool nav_used = critic_nav_used(w);
  uint64_t best_total = UINT64_MAX;
  int32_t best_k = -1, n = 0;
  for (int32_t k = 0; k < K; ++k) {
    uint64_t total = UINT64_MAX;
    const bool ok = control_total(w, nav_used, traj[k], nav_used ? nav + k : nullptr, dyn ? dyn + k : nullptr, w_dyn_sum, w_dyn_max, total);
    if (!ok) total = UINT64_MAX;
    if (totals) totals[k] = total;
    if (ok) {
      ++n;
      control_take(total, k, best_total, best_k);
    }
  }
  result->best = best_k;
  result->n_valid = n;
  result->best_total = best_k < 0 ? UINT64_MAX : best_total;
}

// ---- X11, X12 (all three channels)
inline bool mppi_config_valid(const gv_mppi_config &c, int32_t channels)
{
  for (int32_t i = 0; i < channels; ++i)
    if (!std::isfinite(c.sigma[i]) || !(c.sigma[i] >= 0.0) || std::isnan(c.u_min[i]) || std::isnan(c.u_max[i]) || !(c.u_min[i] <= c.u_max[i]))
      return false;
  return std::isfinite(c.lambda) && c.lambda > 0.0 && c.flags == 0u;
}

inline bool mppi_limits_valid(const gv_mppi_limits &l)
{
  for (int i = 0; i < 3; ++i)
    if (!(l.rate_up[i] >= 0.0) || !(l.rate_down[i] >= 0.0)) return false;   // NaN lands here
  return std::isfinite(l.min_turn_radius) && l.min_turn_radius >= 0.0 && std::isfinite(l.gamma) && l.gamma >= 0.0 && l.flags == 0u;
}

// ---- X13
// the cost table of a configuration; false (t untouched) for anything gv_set_dyn_config rejects.  The radii, the
// factor, the quantum and Rc <= 63 are host::inflation_table's own checks.
inline bool dyn_config_table(const gv_dyn_config &c, host::InflationTable &t)
{
  if (c.n_circles < 1 || c.n_circles > kDynMaxCircles) return false;
  for (int32_t i = 0; i < c.n_circles; ++i)
    if (!std::isfinite(c.off_x[i])) return false;
  if (!std::isfinite(c.t0) || !std::isfinite(c.dt) || !(c.dt >= 0.0)) return false;
  if (c.collision_cost < 1 || c.collision_cost > 255 || c.w_sum > 65535u || c.w_max > 65535u || c.flags != 0u) return false;
  gv_inflation f{};
  f.inscribed_radius = c.radius;
  f.inflation_radius = c.influence_radius;
  f.cost_scaling_factor = c.cost_scaling_factor;
  f.lethal_threshold = 100;
  f.flags = 0;
  return host::inflation_table(f, c.quantum, t);
}

inline bool moving_objects_ok(const gv_moving_object *objs, int32_t n)
{
  if (n < 0 || n > kDynMaxObjects || (n > 0 && !objs)) return false;
  for (int32_t j = 0; j < n; ++j) {
    const gv_lshape_pose &q = objs[j].pose;
    const double read[] = {q.px, q.py, q.qx, q.qy, q.qz, q.qw, q.length, q.width, objs[j].vx, objs[j].vy};
    for (double v : read)
      if (!std::isfinite(v)) return false;
    if (q.length < 0.0 || q.width < 0.0) return false;
  }
  return true;
}

// ---- X14
inline bool transform_finite(const gv_transform &m)
{
  const double v[] = {m.qx, m.qy, m.qz, m.qw, m.tx, m.ty, m.tz};
  for (double x : v)
    if (!std::isfinite(x)) return false;
  return true;
}

inline bool track_update_ok(const gv_lshape_pose *dets, int32_t n, double dt, const gv_transform *motion)
{
  return n >= 0 && n <= kTrackSlots && (n == 0 || dets) && std::isfinite(dt) && dt >= 0.0 && (!motion || transform_finite(*motion));
}

// gv_track_update*'s flag word: known bits only; [EXTENSION] X15 GV_TRACK_TICK_DETS names its own detections, so it goes
// with no dets, n == 0 and not with GV_TRACK_DEVICE_DETS
inline bool track_update_flags_ok(uint32_t flags, const gv_lshape_pose *dets, int32_t n)
{
  if ((flags & ~(uint32_t)(GV_TRACK_DEVICE_DETS | GV_TRACK_FEED_DYNAMIC | GV_TRACK_TICK_DETS)) != 0) return false;
  return !(flags & GV_TRACK_TICK_DETS) || (!dets && n == 0 && !(flags & GV_TRACK_DEVICE_DETS));
}

// gv_set_tracks' rules into a state block; false (st untouched) when they do not hold
inline bool track_state_from(const gv_track *tracks, int32_t n, uint32_t next_id, TrackState &st)
{
  if (n < 0 || n > kTrackSlots || (n > 0 && !tracks)) return false;
  for (int32_t i = 0; i < n; ++i)
    if (tracks[i].slot < 0 || tracks[i].slot >= kTrackSlots || (i > 0 && tracks[i].slot <= tracks[i - 1].slot)) return false;
  std::memset(&st, 0, sizeof(st));
  for (int32_t i = 0; i < n; ++i) {
    st.t[tracks[i].slot] = tracks[i];
    st.live[tracks[i].slot] = 1;
  }
  st.next_id = next_id;
  return true;
}

// gv_get_tracks' order: the live records in ascending slot order into out when they fit; returns their number
inline int32_t track_state_live(const TrackState &st, gv_track *out, int32_t cap)
{
  int32_t n = 0;
  for (int32_t s = 0; s < kTrackSlots; ++s) n += st.live[s] ? 1 : 0;
  if (!out || cap < n) return n;
  int32_t k = 0;
  for (int32_t s = 0; s < kTrackSlots; ++s)
    if (st.live[s]) out[k++] = st.t[s];
  return n;
}

}  // namespace gv_internal
