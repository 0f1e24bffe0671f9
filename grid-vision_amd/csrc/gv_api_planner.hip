// gv_api_planner.hip -- the planner side of the C ABI, everything that makes or reads the costmap:
//   [EXTENSION] X6  the inflated costmap layer (gv_set_inflation, gv_inflate, its getters and publisher),
//   [EXTENSION] X7  footprint scoring of trajectories against it (gv_set_footprint, gv_score_trajectories*),
//   [EXTENSION] X9  the goal / path distance field over it (gv_set_nav_config, gv_nav_field and its getters) and its
//                   sampler along trajectories (gv_score_nav*),
//   [EXTENSION] X10 the rollout that makes such trajectories on the device and the control step that scores the resident
//                   rollout with X7 and X9 and selects (gv_set_motion_model, gv_rollout*, gv_control_step*),
//   [EXTENSION] X11 MPPI's two ends around them: sampling the controls and the softmax average (gv_set_mppi, gv_mppi_*).
//   [EXTENSION] X12 rate and turning-radius limits on those samples and the control cost in the average
//                   (gv_set_mppi_limits, gv_mppi_constrain, gv_*mppi_control_costs, gv_mppi_average_cc).
//   [EXTENSION] X13 scoring of trajectories against predicted moving objects, as a call of its own and as a third
//                   record of the control step (gv_set_dyn_config, gv_set_moving_objects, gv_score_dynamic*).
//   [EXTENSION] X14 the tracker over the tick's boxes that gives those objects their velocities, and can feed X13's set
//                   on the device (gv_set_track_config, gv_set_tracks, gv_get_tracks, gv_track_update*, gv_track_step).
// The kernels are gv_inflate.hip, gv_trajscore.hip, gv_navfield.hip (which also argues why the rounds end at the
// exact field), gv_rollout.hip, gv_mppi.hip, gv_dynscore.hip and gv_track.hip.  What the two samplers do alike, and what a control step and an MPPI
// update enqueue alike, is written once, in front of the entry points.
#include <algorithm>
#include <cstring>
#include <string>
#include <vector>

#include "gv_context.hpp"
#include "gv_motion.hpp"
#include "gv_mppi.hpp"

namespace gv_internal __attribute__((visibility("hidden"))) {

// What a call refuses with GV_ERR_STATE, checked in this order: `missing` (the call's own configuration is not set:
// the caller passes the text, or null), a rollout or a layer in `needs` that no call has made since gv_create (the
// rollout) or gv_create / gv_reset (the layers), and a communicator of more than one rank (`sharded`: why a row band
// of the grid will not do).  h->err says which.
int refuse_state(gv_context *h, const char *call, const char *missing, unsigned needs, const char *sharded)
{
  std::string why;
  if (missing) why = missing;
  else if ((needs & kNeedRollout) && !h->roll.have) why = "no rollout (gv_rollout)";
  else if ((needs & kNeedCostmap) && !h->infl.have_cost) why = "no costmap (gv_inflate)";
  else if ((needs & kNeedField) && !h->nav.have_field) why = "no distance field (gv_nav_field)";
  else if (h->sh.world > 1) why = std::string("ranks own row bands of the grid, ") + sharded;
  else return GV_OK;
  h->err = std::string(call) + ": " + why;
  return GV_ERR_STATE;
}

}  // namespace gv_internal

namespace {

// a sampler's batch: (K, P, 3) poses and K records, flags within `allowed`
bool batch_ok(const float *poses, const void *scores, int32_t K, int32_t P, uint32_t flags, uint32_t allowed)
{
  return poses && scores && P >= 1 && P <= 4096 && K >= 0 && K <= (1 << 20) && (flags & ~allowed) == 0;
}

// the poses where the kernel reads them: the caller's device pointer as given, else the handle's copy of host poses
int stage_poses(gv_context *h, const float *poses, size_t n_poses, uint32_t flags, const float **dev)
{
  *dev = poses;
  if (flags & GV_TRAJ_DEVICE_POSES) return GV_OK;
  if (int rc = h->d_poses.reserve(h, n_poses * 3)) return rc;
  GV_HIP(hipMemcpyAsync(h->d_poses, poses, n_poses * 3 * sizeof(float), hipMemcpyHostToDevice, h->stream));
  *dev = h->d_poses;
  return GV_OK;
}

// Where a kernel writes n results bound for `dst`: dst's own device view when it is pinned host memory aligned to
// `align` bytes, else `landing`, which copy_back empties into dst on the public stream behind the kernel.
template <typename T>
struct ResultDest {
  T *dev = nullptr;    // what the kernel is given
  T *host = nullptr;   // non-null: the results land in device memory and are copied here
  size_t n = 0;
  int open(gv_context *h, T *dst, size_t count, size_t align, DevBuf<T> &landing)
  {
    n = count;
    if ((dev = static_cast<T *>(pinned_device_view(dst, align)))) return GV_OK;
    if (int rc = landing.reserve(h, n)) return rc;
    dev = landing;
    host = dst;
    return GV_OK;
  }
  int copy_back(gv_context *h) const
  {
    if (host) GV_HIP(hipMemcpyAsync(host, dev, n * sizeof(T), hipMemcpyDeviceToHost, h->stream));
    return GV_OK;
  }
};

// the synchronous form of a sampler: rc is what its asynchronous form returned
int wait_scored(gv_context *h, int rc, int32_t K)
{
  if (rc || K == 0) return rc;
  GV_HIP(hipStreamSynchronize(h->stream));
  return GV_OK;
}

// ---- X10: what the device calls and their host twins check alike
bool motion_model_valid(const gv_motion_model &m)
{
  return (m.model == GV_MOTION_DIFF || m.model == GV_MOTION_OMNI) && std::isfinite(m.dt) && m.dt > 0.0 && m.flags == 0u;
}

// a rollout's batch: a finite start, K * P * C controls (K * C with GV_ROLLOUT_CONSTANT), flags within `allowed`
bool rollout_ok(const double *start, const float *controls, int32_t K, int32_t P, uint32_t flags, uint32_t allowed)
{
  return start && controls && std::isfinite(start[0]) && std::isfinite(start[1]) && std::isfinite(start[2]) && P >= 1 &&
         P <= 4096 && K >= 0 && K <= (1 << 20) && (int64_t)K * (int64_t)P <= (int64_t)(1 << 24) && (flags & ~allowed) == 0;
}

bool critic_weights_valid(const gv_critic_weights &w)
{
  return w.w_cost_sum <= 65535u && w.w_max_cost <= 65535u && w.w_nav_last <= 65535u && w.w_nav_sum <= 65535u &&
         w.w_nav_best <= 65535u && w.flags == 0u;
}

// what gv_control_step_async and gv_mppi_update_async refuse alike
bool control_args_ok(const gv_critic_weights *w, uint32_t flags, const gv_control_result *result, const uint64_t *totals)
{
  return w && result && critic_weights_valid(*w) && (flags & ~(uint32_t)GV_CONTROL_KEEP_TOTALS) == 0 &&
         (!(flags & GV_CONTROL_KEEP_TOTALS) || totals);
}

// ---- X13: what the device calls and their host twins check alike
// the cost table of a configuration; false (t untouched) for anything gv_set_dyn_config rejects.  The radii, the
// factor, the quantum and Rc <= 63 are host::inflation_table's own checks.
bool dyn_config_table(const gv_dyn_config &c, host::InflationTable &t)
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

bool moving_objects_ok(const gv_moving_object *objs, int32_t n)
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

// `bytes` (> 0) of host data into the slot of `u` that is not the current one, of `cap` bytes, by a copy command on the
// public stream; that slot is the current one afterwards.  Inflation's mechanism for its table, written once for X13.
int upload_slot(gv_context *h, gv_context::UploadSlots &u, const void *src, size_t bytes, size_t cap)
{
  const int k = u.slot ^ 1;
  int rc = GV_OK;
  if ((rc = u.dev[k].reserve(h, cap)) || (rc = u.stage[k].reserve(h, cap, hipHostMallocDefault))) return rc;
  if (!u.staged[k]) GV_HIP(u.staged[k].create(hipEventDisableTiming));
  if (u.staged_used[k]) GV_HIP(hipEventSynchronize(u.staged[k]));
  std::memcpy(u.stage[k].get(), src, bytes);
  GV_HIP(hipMemcpyAsync(u.dev[k], u.stage[k].get(), bytes, hipMemcpyHostToDevice, h->stream));
  GV_HIP(hipEventRecord(u.staged[k], h->stream));
  u.staged_used[k] = true;
  u.slot = k;
  return GV_OK;
}

// A slot of X13's object table: the rows, and behind them the count that a fed gv_track_update (X14) writes.
constexpr size_t kDynRowsBytes = (size_t)kDynMaxObjects * sizeof(DynObject);
constexpr size_t kDynSlotBytes = kDynRowsBytes + 16;

// ---- X14: what the device calls and the host twin check alike
bool transform_finite(const gv_transform &m)
{
  const double v[] = {m.qx, m.qy, m.qz, m.qw, m.tx, m.ty, m.tz};
  for (double x : v)
    if (!std::isfinite(x)) return false;
  return true;
}

bool track_update_ok(const gv_lshape_pose *dets, int32_t n, double dt, const gv_transform *motion)
{
  return n >= 0 && n <= kTrackSlots && (n == 0 || dets) && std::isfinite(dt) && dt >= 0.0 && (!motion || transform_finite(*motion));
}

// gv_set_tracks' rules into a state block; false (st untouched) when they do not hold
bool track_state_from(const gv_track *tracks, int32_t n, uint32_t next_id, TrackState &st)
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
int32_t track_state_live(const TrackState &st, gv_track *out, int32_t cap)
{
  int32_t n = 0;
  for (int32_t s = 0; s < kTrackSlots; ++s) n += st.live[s] ? 1 : 0;
  if (!out || cap < n) return n;
  int32_t k = 0;
  for (int32_t s = 0; s < kTrackSlots; ++s)
    if (st.live[s]) out[k++] = st.t[s];
  return n;
}

// What every launch of the dyn sampler carries, with the configuration and the set in force now; a changed cost table
// goes to the device first.
int dyn_kernel_args(gv_context *h, DynArgs &a)
{
  gv_context::DynScore &d = h->dyn;
  if (d.dirty) {
    constexpr size_t kTableBytes = (size_t)(host::kInflateMaxRc + 1) * (host::kInflateMaxRc + 1);
    if (int rc = upload_slot(h, d.table, d.tab.cost.data(), d.tab.cost.size(), kTableBytes)) return rc;
    d.dirty = false;
  }
  a.p = dyn_params(d.cfg, d.tab.d2max + 1);
  a.objs = reinterpret_cast<const DynObject *>(d.objs.dev[d.objs.slot].get());
  a.n_obj = d.n_obj;
  a.n_obj_dev = d.n_obj_dev;
  a.table = d.table.dev[d.table.slot];
  return GV_OK;
}

// host only: control_total / control_take (gv_motion.hpp) in a loop; dyn null: the two records alone
void control_select_host(const gv_critic_weights &w, const gv_traj_score *traj, const gv_nav_score *nav, const gv_dyn_score *dyn,
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

// The samplers over the resident rollout into their device record buffers (X7, X9 when a nav weight is set, X13 when a
// dyn configuration is), then the selection into `result` and `totals` (null: no totals), on the public stream: what a
// control step and an MPPI update enqueue alike.
int enqueue_control_scores(gv_context *h, const gv_critic_weights &w, gv_control_result *result, uint64_t *totals)
{
  const bool nav_used = critic_nav_used(w), dyn_used = h->dyn.set;
  gv_context::Rollout &r = h->roll;
  const int32_t K = r.K, P = r.P;
  int rc = GV_OK;
  if ((rc = h->traj.d_scores.reserve(h, (size_t)K)) || (nav_used && (rc = h->nav.d_scores.reserve(h, (size_t)K))) ||
      (dyn_used && (rc = h->dyn.d_scores.reserve(h, (size_t)K))))
    return rc;
  TrajArgs t{};
  t.g = h->g;
  t.fp = h->traj.fp;
  t.poses = r.poses;
  t.K = K; t.P = P;
  t.cost = h->infl.cost;
  t.scores = h->traj.d_scores;
  t.pose_cost = nullptr;
  launch_score_trajectories(t, h->stream);
  if (nav_used) {
    NavScoreArgs n{};
    n.g = h->g;
    n.poses = r.poses;
    n.K = K; n.P = P;
    n.field = h->nav.field;
    n.scores = h->nav.d_scores;
    launch_score_nav(n, h->stream);
  }
  if (dyn_used) {
    DynArgs d{};
    if ((rc = dyn_kernel_args(h, d))) return rc;
    d.poses = r.poses;
    d.K = K; d.P = P;
    d.scores = h->dyn.d_scores;
    d.pose_cost = nullptr;
    launch_score_dynamic(d, h->stream);
  }
  ControlSelectArgs s{};
  s.w = w;
  s.traj = h->traj.d_scores;
  s.nav = nav_used ? h->nav.d_scores.get() : nullptr;
  s.dyn = dyn_used ? h->dyn.d_scores.get() : nullptr;
  s.w_dyn_sum = h->dyn.cfg.w_sum;
  s.w_dyn_max = h->dyn.cfg.w_max;
  s.K = K;
  s.result = result;
  s.totals = totals;
  launch_control_select(s, h->stream);
  GV_HIP(hipGetLastError());
  return GV_OK;
}

// ---- X11: what the device calls and their host twins check alike
bool mppi_config_valid(const gv_mppi_config &c, int32_t channels)
{
  for (int32_t i = 0; i < channels; ++i)
    if (!std::isfinite(c.sigma[i]) || !(c.sigma[i] >= 0.0) || std::isnan(c.u_min[i]) || std::isnan(c.u_max[i]) || !(c.u_min[i] <= c.u_max[i]))
      return false;
  return std::isfinite(c.lambda) && c.lambda > 0.0 && c.flags == 0u;
}

bool mppi_shape_ok(int32_t K, int32_t P)
{
  return P >= 1 && P <= 4096 && K >= 0 && K <= (1 << 20) && (int64_t)K * (int64_t)P <= (int64_t)(1 << 24);
}

// X12: what gv_set_mppi_limits and the host twins check alike (all three channels)
bool mppi_limits_valid(const gv_mppi_limits &l)
{
  for (int i = 0; i < 3; ++i)
    if (!(l.rate_up[i] >= 0.0) || !(l.rate_down[i] >= 0.0)) return false;   // NaN lands here
  return std::isfinite(l.min_turn_radius) && l.min_turn_radius >= 0.0 && std::isfinite(l.gamma) && l.gamma >= 0.0 && l.flags == 0u;
}

// What a sampling refuses with GV_ERR_STATE: no configuration, no motion model, no nominal, a nominal of another C,
// a turning radius under a model that is not DIFF.
int mppi_sample_refused(gv_context *h, const char *call)
{
  const gv_context::Mppi &m = h->mppi;
  const char *why = !m.set ? "no MPPI configuration set (gv_set_mppi)"
                    : !h->roll.set ? "no motion model set (gv_set_motion_model)"
                    : !m.have_nominal ? "no nominal sequence (gv_mppi_set_nominal)"
                    : motion_controls(h->roll.model.model) != m.C ? "the nominal sequence was set under a motion model with other controls per step"
                    : m.lim_set && m.lim.min_turn_radius > 0.0 && h->roll.model.model != GV_MOTION_DIFF
                        ? "a minimum turning radius (gv_set_mppi_limits) needs GV_MOTION_DIFF"
                        : nullptr;
  if (!why) return GV_OK;
  h->err = std::string(call) + ": " + why;
  return GV_ERR_STATE;
}

// What an update refuses with GV_ERR_STATE.  `cycle`: the call makes the controls and the rollout itself before it
// updates, so neither needs to exist yet.
int mppi_update_refused(gv_context *h, const char *call, const gv_critic_weights &w, bool cycle)
{
  const gv_context::Mppi &m = h->mppi;
  const char *missing = !h->traj.set ? "no footprint set (gv_set_footprint)" : !m.set ? "no MPPI configuration set (gv_set_mppi)" : nullptr;
  int rc = refuse_state(h, call, missing, (cycle ? 0u : kNeedRollout) | kNeedCostmap | (critic_nav_used(w) ? kNeedField : 0u),
                        "there is no whole costmap");
  if (rc) return rc;
  const char *why = nullptr;
  if (!m.have_nominal) why = "no nominal sequence (gv_mppi_set_nominal)";
  else if (!cycle) {
    if (!m.have_controls) why = "no sampled controls (gv_mppi_sample)";
    else if (m.cK != h->roll.K || m.cP != h->roll.P) why = "the resident rollout is not of the sampled controls' K and P";
    else if (m.cP != m.P || m.cC != m.C) why = "the nominal sequence is not of the sampled controls' P and C";
  }
  if (!why) return GV_OK;
  h->err = std::string(call) + ": " + why;
  return GV_ERR_STATE;
}

int mppi_enqueue_sample(gv_context *h, int32_t K, uint64_t seed, uint64_t iteration, uint32_t flags)
{
  gv_context::Mppi &m = h->mppi;
  const size_t n = (size_t)K * (size_t)m.P * (size_t)m.C;
  if (n > m.controls.cap()) m.have_controls = false;   // the buffer is about to move
  if (int rc = m.controls.reserve(h, n)) return rc;
  MppiSampleArgs a{};
  a.cfg = m.cfg;
  a.C = m.C;
  a.K = K; a.P = m.P;
  a.seed = seed; a.iteration = iteration;
  a.shift = (flags & GV_MPPI_SHIFT) != 0;
  a.nominal = m.nominal;
  a.controls = m.controls;
  launch_mppi_sample(a, h->stream);
  if (m.lim_set) {   // X12: the chain over what was just sampled, when it can change a control at all
    MppiConstrainArgs c{};
    c.chain = mppi_chain(m.lim, h->roll.model.dt);
    c.C = m.C;
    c.K = K; c.P = m.P;
    c.controls = m.controls;
    if (mppi_chain_active(c.chain, m.C)) launch_mppi_constrain(c, h->stream);
  }
  GV_HIP(hipGetLastError());
  m.cK = K; m.cP = m.P; m.cC = m.C;
  m.c_shift = a.shift;
  m.have_controls = true;
  return GV_OK;
}

// the scoring of the resident rollout and the two launches of the average; results a kernel cannot write go by copy
int mppi_enqueue_update(gv_context *h, const gv_critic_weights &w, uint32_t flags, gv_control_result *result, uint64_t *totals,
                        float *nominal_out)
{
  gv_context::Mppi &m = h->mppi;
  gv_context::Rollout &r = h->roll;
  const bool keep = (flags & GV_CONTROL_KEEP_TOTALS) != 0;
  const int32_t K = r.K;
  const int64_t J = (int64_t)m.P * (int64_t)m.C;
  int rc = GV_OK;
  MppiAverageArgs a{};
  a.lambda = m.cfg.lambda;
  a.K = K; a.J = (int32_t)J;
  a.rows = mppi_chunk_rows(K, J);
  a.tile = mppi_tile_cols(J);
  const size_t chunks = (size_t)((K + a.rows - 1) / a.rows);
  if ((rc = r.d_result.reserve(h, 1)) || (rc = r.d_totals.reserve(h, (size_t)K)) || (rc = m.partial.reserve(h, chunks * ((size_t)J + 1))))
    return rc;
  const bool cc = m.lim_set && m.lim.gamma > 0.0;   // X12: the control cost joins the exponent
  if (cc && ((rc = m.cost.reserve(h, 2 * (size_t)K)) || (rc = m.x_min.reserve(h, 1)))) return rc;
  if ((rc = enqueue_control_scores(h, w, r.d_result, r.d_totals))) return rc;
  m.have_costs = false;
  if (cc) {
    MppiCostArgs c{};
    for (int i = 0; i < 3; ++i) c.qc[i] = mppi_cost_scale(m.lim.gamma, m.cfg.sigma[i]);
    c.C = m.C;
    c.K = K; c.P = m.P;
    c.shift = m.c_shift;
    c.nominal = m.nominal;
    c.controls = m.controls;
    c.totals = r.d_totals;
    c.result = r.d_result;
    c.g = m.cost;
    c.x = m.cost.get() + K;
    c.x_min_key = m.x_min;
    GV_HIP(hipMemsetAsync(m.x_min.get(), 0xFF, sizeof(uint64_t), h->stream));
    launch_mppi_control_cost(c, h->stream);
    a.x = c.x;
    a.x_min_key = c.x_min_key;
    m.costK = K;
    m.have_costs = true;
  }
  a.controls = m.controls;
  a.totals = r.d_totals;
  a.result = r.d_result;
  a.partial = m.partial;
  a.nominal = m.nominal;
  a.result_out = static_cast<gv_control_result *>(pinned_device_view(result, 16));
  a.totals_out = keep ? static_cast<uint64_t *>(pinned_device_view(totals, 8)) : nullptr;
  a.nominal_out = nominal_out ? static_cast<float *>(pinned_device_view(nominal_out, 8)) : nullptr;
  launch_mppi_average(a, h->stream);
  GV_HIP(hipGetLastError());
  if (!a.result_out) GV_HIP(hipMemcpyAsync(result, r.d_result, sizeof(gv_control_result), hipMemcpyDeviceToHost, h->stream));
  if (keep && !a.totals_out) GV_HIP(hipMemcpyAsync(totals, r.d_totals, (size_t)K * sizeof(uint64_t), hipMemcpyDeviceToHost, h->stream));
  if (nominal_out && !a.nominal_out)
    GV_HIP(hipMemcpyAsync(nominal_out, m.nominal, (size_t)J * sizeof(float), hipMemcpyDeviceToHost, h->stream));
  return GV_OK;
}

}  // namespace

extern "C" {

// [EXTENSION] X6: handle configuration, the table is built here on the host and reaches the device with the next
// gv_inflate (gv_context::Inflation).  A rejected configuration leaves the one in force alone.
int gv_inflation_cost_table(const gv_inflation *cfg, double resolution, uint8_t *table, int32_t cap, int32_t *n)
{
  gv_context *h = nullptr;
  if (!cfg) return GV_ERR_BAD_ARG;
  GV_TRY
  host::InflationTable t;
  if (!host::inflation_table(*cfg, resolution, t)) return GV_ERR_BAD_ARG;
  if (n) *n = t.d2max + 1;
  if (!table || cap < t.d2max + 1) return GV_ERR_BAD_ARG;
  std::memcpy(table, t.cost.data(), t.cost.size());
  return GV_OK;
  GV_CATCH
}

int gv_set_inflation(gv_handle h, const gv_inflation *cfg)
{
  if (!h) return GV_ERR_BAD_ARG;
  GV_TRY
  if (!cfg) {
    h->infl.set = false;
    return GV_OK;
  }
  host::InflationTable t;
  if (!host::inflation_table(*cfg, h->g.res, t)) return GV_ERR_BAD_ARG;
  h->infl.tab = std::move(t);
  h->infl.thr = cfg->lethal_threshold;
  h->infl.flags = cfg->flags;
  h->infl.dirty = true;
  h->infl.set = true;
  return GV_OK;
  GV_CATCH
}

// Two kernels on the public stream, between the grid passes of the frames around them (set_device_only: the streams
// are not drained).  No host wait once the buffers exist.
int gv_inflate(gv_handle h)
{
  if (!h) return GV_ERR_BAD_ARG;
  GV_TRY
  gv_context::Inflation &f = h->infl;
  int rc = refuse_state(h, "gv_inflate", f.set ? nullptr : "no inflation set (gv_set_inflation)", 0, "the stencil crosses them");
  if (rc || (rc = set_device_only(h))) return rc;
  const size_t G = (size_t)h->g.G;
  const bool keep = (f.flags & GV_INFLATE_KEEP_DIST2) != 0;
  const int32_t row_words = inflate_row_words(h->g.nx);
  if ((rc = f.bits.reserve_zeroed(h, (size_t)h->g.ny * (size_t)row_words, h->stream))) return rc;
  if ((rc = f.cost.reserve(h, G + 16))) return rc;
  if (keep && (rc = f.dist2.reserve(h, G))) return rc;
  constexpr size_t kTableBytes = (size_t)(host::kInflateMaxRc + 1) * (host::kInflateMaxRc + 1);
  if (f.dirty) {
    const int k = f.slot ^ 1;
    if ((rc = f.d_table[k].reserve(h, kTableBytes))) return rc;
    if ((rc = f.stage[k].reserve(h, kTableBytes, hipHostMallocDefault))) return rc;
    if (!f.staged[k]) GV_HIP(f.staged[k].create(hipEventDisableTiming));
    if (f.staged_used[k]) GV_HIP(hipEventSynchronize(f.staged[k]));
    std::memcpy(f.stage[k].get(), f.tab.cost.data(), f.tab.cost.size());
    GV_HIP(hipMemcpyAsync(f.d_table[k], f.stage[k].get(), f.tab.cost.size(), hipMemcpyHostToDevice, h->stream));
    GV_HIP(hipEventRecord(f.staged[k], h->stream));
    f.staged_used[k] = true;
    f.slot = k;
    f.dirty = false;
  }
  InflateArgs a{};
  a.nx = h->g.nx; a.ny = h->g.ny;
  a.row_words = row_words;
  a.thr = f.thr;
  a.rc = f.tab.rc; a.d2max = f.tab.d2max;
  a.i8 = h->occ_i8;
  a.bits = f.bits;
  a.table = f.d_table[f.slot];
  a.cost = f.cost;
  a.dist2 = keep ? f.dist2.get() : nullptr;
  launch_lethal_bits(a, h->stream);
  launch_inflate_tiles(a, h->stream);
  GV_HIP(hipGetLastError());
  f.have_cost = true;
  f.have_dist2 = keep;
  return GV_OK;
  GV_CATCH
}

int gv_get_costmap(gv_handle h, uint8_t *out)
{
  if (!h || !out) return GV_ERR_BAD_ARG;
  if (!h->infl.have_cost) return GV_ERR_STATE;
  return copy_out(h, out, h->infl.cost, (size_t)h->g.G);
}

int gv_get_obstacle_dist2(gv_handle h, uint16_t *out)
{
  if (!h || !out) return GV_ERR_BAD_ARG;
  if (!h->infl.have_cost || !h->infl.have_dist2) return GV_ERR_STATE;
  return copy_out(h, out, h->infl.dist2, (size_t)h->g.G * sizeof(uint16_t));
}

int gv_publish_costmap_async(gv_handle h, uint8_t *data)
{
  if (!h || !data) return GV_ERR_BAD_ARG;
  if (!h->infl.have_cost) return GV_ERR_STATE;
  GV_TRY
  return publish_layer_async(h, reinterpret_cast<const int8_t *>(h->infl.cost.get()), reinterpret_cast<int8_t *>(data));
  GV_CATCH
}

// [EXTENSION] X7: handle configuration only; every scoring call copies h->traj.fp into its kernel arguments.
int gv_set_footprint(gv_handle h, const gv_footprint *fp)
{
  if (!h) return GV_ERR_BAD_ARG;
  if (!fp) {
    h->traj.set = false;
    return GV_OK;
  }
  if (!host::footprint_valid(*fp)) return GV_ERR_BAD_ARG;
  h->traj.fp = *fp;
  for (int32_t i = fp->n_vertices; i < host::kFootprintMaxVertices; ++i) h->traj.fp.vx[i] = h->traj.fp.vy[i] = 0.0;
  h->traj.set = true;
  return GV_OK;
}

// A copy of the poses (host poses only), one kernel, and a copy per result the kernel cannot write in place, all on
// the public stream: between the grid passes of the frames around them, behind the last gv_inflate.
int gv_score_trajectories_async(gv_handle h, const float *poses, int32_t K, int32_t P, uint32_t flags,
                                gv_traj_score *scores, uint8_t *pose_cost)
{
  if (!h) return GV_ERR_BAD_ARG;
  GV_TRY
  const bool keep = (flags & GV_TRAJ_KEEP_POSE_COST) != 0;
  if (!batch_ok(poses, scores, K, P, flags, host::kTrajFlags) || (keep && !pose_cost)) return GV_ERR_BAD_ARG;
  gv_context::TrajScore &t = h->traj;
  int rc = refuse_state(h, "gv_score_trajectories", t.set ? nullptr : "no footprint set (gv_set_footprint)", kNeedCostmap,
                        "there is no whole costmap");
  if (rc || K == 0 || (rc = set_device_only(h))) return rc;
  const size_t n_poses = (size_t)K * (size_t)P;
  TrajArgs a{};
  a.g = h->g;
  a.fp = t.fp;
  a.K = K; a.P = P;
  a.cost = h->infl.cost;
  ResultDest<gv_traj_score> to_scores;
  ResultDest<uint8_t> to_pose_cost;   // stays closed (null, no copy) without GV_TRAJ_KEEP_POSE_COST
  if ((rc = stage_poses(h, poses, n_poses, flags, &a.poses)) || (rc = to_scores.open(h, scores, (size_t)K, 16, t.d_scores)) ||
      (keep && (rc = to_pose_cost.open(h, pose_cost, n_poses, 1, t.d_pose_cost))))
    return rc;
  a.scores = to_scores.dev;
  a.pose_cost = to_pose_cost.dev;
  launch_score_trajectories(a, h->stream);
  GV_HIP(hipGetLastError());
  if ((rc = to_scores.copy_back(h)) || (rc = to_pose_cost.copy_back(h))) return rc;
  return GV_OK;
  GV_CATCH
}

int gv_score_trajectories(gv_handle h, const float *poses, int32_t K, int32_t P, uint32_t flags, gv_traj_score *scores,
                          uint8_t *pose_cost)
{
  return wait_scored(h, gv_score_trajectories_async(h, poses, K, P, flags, scores, pose_cost), K);
}

// host only: the twin of the kernel's geometry (host::footprint_cells), on the geometry gv_create gives
int gv_footprint_cells(uint8_t grid_x, uint8_t grid_y, double resolution, const gv_footprint *fp, float x, float y, float yaw,
                       int32_t *cells, int32_t cap, int32_t *n)
{
  gv_context *h = nullptr;
  if (!fp || !n) return GV_ERR_BAD_ARG;
  GV_TRY
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
  GV_CATCH
}

// ---- [EXTENSION] X9: the distance field and its sampler ----
int gv_nav_step_table(const gv_nav_config *cfg, uint32_t table[256])
{
  if (!cfg || !table || !host::nav_config_valid(*cfg)) return GV_ERR_BAD_ARG;
  host::nav_step_table(*cfg, table);
  return GV_OK;
}

// handle configuration only; gv_nav_field copies it into its kernel arguments
int gv_set_nav_config(gv_handle h, const gv_nav_config *cfg)
{
  if (!h) return GV_ERR_BAD_ARG;
  if (!cfg) {
    h->nav.set = false;
    return GV_OK;
  }
  if (!host::nav_config_valid(*cfg) || !host::nav_config_fits(*cfg, h->g.G)) return GV_ERR_BAD_ARG;
  h->nav.cfg = *cfg;
  h->nav.set = true;
  return GV_OK;
}

// Everything goes on the public stream, behind what was enqueued before (a pending tick's grid pass and inflate
// included).  Seeds become field entries here on the host (the exact getIndex); whether a seed's cell is blocked only
// the device knows, so k_nav_seeds drops those and counts the rest.  Then rounds in batches of 4, 8, .. kBatchMax
// launches; a batch ends with its counters copied into the pinned block and one event wait, and the loop stops after
// the first round whose counter is 0 (the rounds behind it in the batch found no active tile and did nothing).
int gv_nav_field(gv_handle h, const float *seeds_xy, int32_t S, gv_nav_info *info)
{
  if (!h) return GV_ERR_BAD_ARG;
  GV_TRY
  if (!seeds_xy || S < 1 || S > 65536) return GV_ERR_BAD_ARG;
  gv_context::NavField &f = h->nav;
  int rc = refuse_state(h, "gv_nav_field", f.set ? nullptr : "no configuration set (gv_set_nav_config)", kNeedCostmap,
                        "there is no whole costmap");
  if (rc || (rc = set_device_only(h))) return rc;
  constexpr int kBatchMax = gv_context::NavField::kBatchMax;
  constexpr size_t kSeedOff = 512;   // bytes of the pinned block in front of the seeds: the counters land there
  static_assert((1 + kBatchMax) * sizeof(uint32_t) <= kSeedOff, "the counters fit in front of the seeds");
  const int32_t G = h->g.G;
  const int32_t tiles_x = (h->g.nx + kNavTile - 1) / kNavTile, tiles_y = (h->g.ny + kNavTile - 1) / kNavTile;
  const size_t n_tiles = (size_t)tiles_x * (size_t)tiles_y;
  if ((rc = f.field.reserve(h, ((size_t)G + 3) / 4 * 4))) return rc;
  if ((rc = f.flags.reserve(h, 2 * n_tiles))) return rc;
  if ((rc = f.counters.reserve(h, 1 + kBatchMax))) return rc;
  if ((rc = f.d_seeds.reserve(h, (size_t)S))) return rc;
  if ((rc = f.stage.reserve(h, kSeedOff + (size_t)S * sizeof(int32_t), hipHostMallocDefault))) return rc;
  if (!f.done) GV_HIP(f.done.create(hipEventDisableTiming));
  f.have_field = false;   // until this call has converged

  int32_t *cells = reinterpret_cast<int32_t *>(f.stage.get() + kSeedOff);
  int32_t n = 0;
  for (int32_t i = 0; i < S; ++i) {
    const int32_t e = host::nav_seed_entry(h->g, seeds_xy[2 * i], seeds_xy[2 * i + 1]);
    if (e >= 0) cells[n++] = e;
  }
  const volatile uint32_t *landed = reinterpret_cast<const volatile uint32_t *>(f.stage.get());

  NavArgs a{};
  a.nx = h->g.nx; a.ny = h->g.ny; a.G = G;
  a.tiles_x = tiles_x; a.tiles_y = tiles_y;
  a.step = NavStep{f.cfg.obstacle_cost, f.cfg.cost_weight};
  a.pass_cap = h->tune.nav_pass_cap;
  a.cost = h->infl.cost;
  a.field = f.field;
  a.seeds = f.d_seeds;
  a.n_seeds = n;
  a.flags_out = f.flags;          // round 0 reads the first half
  a.counter = f.counters;         // [0]: seeds used
  GV_HIP(hipMemsetAsync(f.flags, 0, 2 * n_tiles * sizeof(uint32_t), h->stream));
  GV_HIP(hipMemsetAsync(f.counters, 0, sizeof(uint32_t), h->stream));
  if (n > 0) GV_HIP(hipMemcpyAsync(f.d_seeds, cells, (size_t)n * sizeof(int32_t), hipMemcpyHostToDevice, h->stream));
  launch_nav_init(a, h->stream);
  launch_nav_seeds(a, h->stream);
  GV_HIP(hipGetLastError());

  const int64_t max_rounds = (int64_t)G + 2;
  int64_t rounds = 0;
  int batch = 4;
  for (bool converged = false; !converged;) {
    if (rounds >= max_rounds) {
      h->err = "gv_nav_field: no convergence within G + 2 rounds";
      return GV_ERR_STATE;
    }
    const int nb = (int)std::min<int64_t>(batch, max_rounds - rounds);
    GV_HIP(hipMemsetAsync(f.counters.get() + 1, 0, (size_t)nb * sizeof(uint32_t), h->stream));
    for (int i = 0; i < nb; ++i) {
      const int64_t r = rounds + i;
      a.flags_in = f.flags.get() + (size_t)(r & 1) * n_tiles;
      a.flags_out = f.flags.get() + (size_t)((r + 1) & 1) * n_tiles;
      a.counter = f.counters.get() + 1 + i;
      launch_nav_relax(a, h->stream);
    }
    GV_HIP(hipGetLastError());
    GV_HIP(hipMemcpyAsync(f.stage.get(), f.counters, (size_t)(1 + nb) * sizeof(uint32_t), hipMemcpyDeviceToHost, h->stream));
    GV_HIP(hipEventRecord(f.done, h->stream));
    GV_HIP(hipEventSynchronize(f.done));
    int used = nb;
    for (int i = 0; i < nb; ++i)
      if (landed[1 + i] == 0u) {
        used = i + 1;
        converged = true;
        break;
      }
    rounds += used;
    batch = std::min(batch * 2, kBatchMax);
  }
  f.have_field = true;
  if (info) {
    info->n_seeds_used = (int32_t)landed[0];
    info->rounds = (int32_t)std::min<int64_t>(rounds, INT32_MAX);
  }
  return GV_OK;
  GV_CATCH
}

int gv_get_nav_field(gv_handle h, uint32_t *out)
{
  if (!h || !out) return GV_ERR_BAD_ARG;
  if (!h->nav.have_field) return GV_ERR_STATE;
  return copy_out(h, out, h->nav.field, (size_t)h->g.G * sizeof(uint32_t));
}

int gv_device_nav_field(gv_handle h, uint32_t **field)
{
  if (!h || !field) return GV_ERR_BAD_ARG;
  if (!h->nav.have_field) return GV_ERR_STATE;
  *field = h->nav.field.get();
  return GV_OK;
}

// gv_score_trajectories_async with another kernel and another record
int gv_score_nav_async(gv_handle h, const float *poses, int32_t K, int32_t P, uint32_t flags, gv_nav_score *scores)
{
  if (!h) return GV_ERR_BAD_ARG;
  GV_TRY
  if (!batch_ok(poses, scores, K, P, flags, GV_TRAJ_DEVICE_POSES)) return GV_ERR_BAD_ARG;
  gv_context::NavField &f = h->nav;
  int rc = refuse_state(h, "gv_score_nav", nullptr, kNeedField, "there is no whole field");
  if (rc || K == 0 || (rc = set_device_only(h))) return rc;
  NavScoreArgs a{};
  a.g = h->g;
  a.K = K; a.P = P;
  a.field = f.field;
  ResultDest<gv_nav_score> to_scores;
  if ((rc = stage_poses(h, poses, (size_t)K * (size_t)P, flags, &a.poses)) || (rc = to_scores.open(h, scores, (size_t)K, 8, f.d_scores)))
    return rc;
  a.scores = to_scores.dev;
  launch_score_nav(a, h->stream);
  GV_HIP(hipGetLastError());
  return to_scores.copy_back(h);
  GV_CATCH
}

int gv_score_nav(gv_handle h, const float *poses, int32_t K, int32_t P, uint32_t flags, gv_nav_score *scores)
{
  return wait_scored(h, gv_score_nav_async(h, poses, K, P, flags, scores), K);
}

// ---- [EXTENSION] X10: rollout and control step ----
// handle configuration only; every rollout copies h->roll.model into its kernel arguments
int gv_set_motion_model(gv_handle h, const gv_motion_model *m)
{
  if (!h) return GV_ERR_BAD_ARG;
  if (!m) {
    h->roll.set = false;
    return GV_OK;
  }
  if (!motion_model_valid(*m)) return GV_ERR_BAD_ARG;
  h->roll.model = *m;
  h->roll.set = true;
  return GV_OK;
}

// A copy of the controls (host controls only) and one kernel on the public stream.  The pose buffer grows by
// DevBuf::reserve (hipFree waits for the device: no kernel in flight loses the block it reads); the rollout it held is
// gone then, and this call writes the next one.
int gv_rollout_async(gv_handle h, const double start[3], const float *controls, int32_t K, int32_t P, uint32_t flags)
{
  if (!h) return GV_ERR_BAD_ARG;
  GV_TRY
  if (!rollout_ok(start, controls, K, P, flags, GV_ROLLOUT_DEVICE_CONTROLS | GV_ROLLOUT_CONSTANT)) return GV_ERR_BAD_ARG;
  gv_context::Rollout &r = h->roll;
  if (!r.set) {
    h->err = "gv_rollout: no motion model set (gv_set_motion_model)";
    return GV_ERR_STATE;
  }
  int rc = GV_OK;
  if (K == 0 || (rc = set_device_only(h))) return rc;
  RolloutArgs a{};
  a.model = r.model.model;
  a.dt = r.model.dt;
  for (int i = 0; i < 3; ++i) a.start[i] = start[i];
  a.K = K; a.P = P;
  a.constant = (flags & GV_ROLLOUT_CONSTANT) != 0;
  const size_t n_poses = (size_t)K * (size_t)P;
  const size_t n_controls = (a.constant ? (size_t)K : n_poses) * (size_t)motion_controls(a.model);
  if (n_poses * 3 > r.poses.cap()) r.have = false;   // the buffer is about to move
  if ((rc = r.poses.reserve(h, n_poses * 3))) return rc;
  a.controls = controls;
  if (!(flags & GV_ROLLOUT_DEVICE_CONTROLS)) {
    if ((rc = r.d_controls.reserve(h, n_controls))) return rc;
    GV_HIP(hipMemcpyAsync(r.d_controls, controls, n_controls * sizeof(float), hipMemcpyHostToDevice, h->stream));
    a.controls = r.d_controls;
  }
  a.poses = r.poses;
  launch_rollout(a, h->stream);
  GV_HIP(hipGetLastError());
  r.K = K; r.P = P;
  r.have = true;
  return GV_OK;
  GV_CATCH
}

int gv_rollout(gv_handle h, const double start[3], const float *controls, int32_t K, int32_t P, uint32_t flags)
{
  return wait_scored(h, gv_rollout_async(h, start, controls, K, P, flags), K);
}

int gv_device_rollout(gv_handle h, float **poses, int32_t *K, int32_t *P)
{
  if (!h || !poses) return GV_ERR_BAD_ARG;
  if (!h->roll.have) return GV_ERR_STATE;
  *poses = h->roll.poses.get();
  if (K) *K = h->roll.K;
  if (P) *P = h->roll.P;
  return GV_OK;
}

int gv_get_rollout(gv_handle h, float *poses_out)
{
  if (!h || !poses_out) return GV_ERR_BAD_ARG;
  if (!h->roll.have) return GV_ERR_STATE;
  return copy_out(h, poses_out, h->roll.poses, (size_t)h->roll.K * (size_t)h->roll.P * 3 * sizeof(float));
}

// host only: motion_step (gv_motion.hpp), one trajectory after the other, one step after the other
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

// The two samplers over the resident rollout into their device record buffers, then the selection, all on the public
// stream; the existing launchers and argument blocks, as gv_score_trajectories_async / gv_score_nav_async fill them.
int gv_control_step_async(gv_handle h, const gv_critic_weights *w, uint32_t flags, gv_control_result *result,
                          uint64_t *totals)
{
  if (!h) return GV_ERR_BAD_ARG;
  GV_TRY
  const bool keep = (flags & GV_CONTROL_KEEP_TOTALS) != 0;
  if (!control_args_ok(w, flags, result, totals)) return GV_ERR_BAD_ARG;
  const bool nav_used = critic_nav_used(*w);
  gv_context::Rollout &r = h->roll;
  int rc = refuse_state(h, "gv_control_step", h->traj.set ? nullptr : "no footprint set (gv_set_footprint)",
                        kNeedRollout | kNeedCostmap | (nav_used ? kNeedField : 0u), "there is no whole costmap");
  if (rc || (rc = set_device_only(h))) return rc;
  ResultDest<gv_control_result> to_result;
  ResultDest<uint64_t> to_totals;   // stays closed (null, no copy) without GV_CONTROL_KEEP_TOTALS
  if ((rc = to_result.open(h, result, 1, 16, r.d_result)) || (keep && (rc = to_totals.open(h, totals, (size_t)r.K, 8, r.d_totals))))
    return rc;
  if ((rc = enqueue_control_scores(h, *w, to_result.dev, to_totals.dev))) return rc;
  if ((rc = to_result.copy_back(h)) || (rc = to_totals.copy_back(h))) return rc;
  return GV_OK;
  GV_CATCH
}

int gv_control_step(gv_handle h, const gv_critic_weights *w, uint32_t flags, gv_control_result *result, uint64_t *totals)
{
  return wait_scored(h, gv_control_step_async(h, w, flags, result, totals), 1);
}

// host only: control_total / control_take (gv_motion.hpp) in a loop
int gv_control_select(const gv_critic_weights *w, const gv_traj_score *traj, const gv_nav_score *nav, int32_t K,
                      gv_control_result *result, uint64_t *totals)
{
  if (!w || !traj || !result || !critic_weights_valid(*w) || K < 0 || K > (1 << 20)) return GV_ERR_BAD_ARG;
  if (critic_nav_used(*w) && !nav) return GV_ERR_BAD_ARG;
  control_select_host(*w, traj, nav, nullptr, 0u, 0u, K, result, totals);
  return GV_OK;
}

// ---- [EXTENSION] X11: MPPI sampling and softmax update ----
// handle configuration only; every sampling and update copies h->mppi.cfg into its kernel arguments
int gv_set_mppi(gv_handle h, const gv_mppi_config *cfg)
{
  if (!h) return GV_ERR_BAD_ARG;
  if (!cfg) {
    h->mppi.set = false;
    return GV_OK;
  }
  if (!mppi_config_valid(*cfg, 3)) return GV_ERR_BAD_ARG;
  h->mppi.cfg = *cfg;
  h->mppi.set = true;
  return GV_OK;
}

// One copy on the public stream and the wait for it: the caller's array is free on return.
int gv_mppi_set_nominal(gv_handle h, const float *nominal, int32_t P)
{
  if (!h) return GV_ERR_BAD_ARG;
  GV_TRY
  if (!nominal || P < 1 || P > 4096) return GV_ERR_BAD_ARG;
  if (!h->roll.set) {
    h->err = "gv_mppi_set_nominal: no motion model set (gv_set_motion_model)";
    return GV_ERR_STATE;
  }
  gv_context::Mppi &m = h->mppi;
  const int32_t C = motion_controls(h->roll.model.model);
  const size_t n = (size_t)P * (size_t)C;
  for (size_t i = 0; i < n; ++i)
    if (!std::isfinite(nominal[i])) return GV_ERR_BAD_ARG;
  int rc = set_device_only(h);
  if (rc) return rc;
  if (n > m.nominal.cap()) m.have_nominal = false;
  if ((rc = m.nominal.reserve(h, n))) return rc;
  GV_HIP(hipMemcpyAsync(m.nominal, nominal, n * sizeof(float), hipMemcpyHostToDevice, h->stream));
  GV_HIP(hipStreamSynchronize(h->stream));
  m.P = P; m.C = C;
  m.have_nominal = true;
  return GV_OK;
  GV_CATCH
}

int gv_get_mppi_nominal(gv_handle h, float *out, int32_t *P)
{
  if (!h || (!out && !P)) return GV_ERR_BAD_ARG;
  if (!h->mppi.have_nominal) return GV_ERR_STATE;
  if (P) *P = h->mppi.P;
  return out ? copy_out(h, out, h->mppi.nominal, (size_t)h->mppi.P * (size_t)h->mppi.C * sizeof(float)) : GV_OK;
}

// One kernel on the public stream.  The controls buffer grows by DevBuf::reserve, like the rollout's.
int gv_mppi_sample_async(gv_handle h, int32_t K, uint64_t seed, uint64_t iteration, uint32_t flags)
{
  if (!h) return GV_ERR_BAD_ARG;
  GV_TRY
  if (K < 0 || K > (1 << 20) || (flags & ~(uint32_t)GV_MPPI_SHIFT) != 0) return GV_ERR_BAD_ARG;
  int rc = mppi_sample_refused(h, "gv_mppi_sample");
  if (rc) return rc;
  if (!mppi_shape_ok(K, h->mppi.P)) return GV_ERR_BAD_ARG;
  if (K == 0 || (rc = set_device_only(h))) return rc;
  return mppi_enqueue_sample(h, K, seed, iteration, flags);
  GV_CATCH
}

int gv_mppi_sample(gv_handle h, int32_t K, uint64_t seed, uint64_t iteration, uint32_t flags)
{
  return wait_scored(h, gv_mppi_sample_async(h, K, seed, iteration, flags), K);
}

int gv_device_controls(gv_handle h, float **controls, int32_t *K, int32_t *P, int32_t *C)
{
  if (!h || !controls) return GV_ERR_BAD_ARG;
  if (!h->mppi.have_controls) return GV_ERR_STATE;
  *controls = h->mppi.controls.get();
  if (K) *K = h->mppi.cK;
  if (P) *P = h->mppi.cP;
  if (C) *C = h->mppi.cC;
  return GV_OK;
}

int gv_get_controls(gv_handle h, float *out)
{
  if (!h || !out) return GV_ERR_BAD_ARG;
  const gv_context::Mppi &m = h->mppi;
  if (!m.have_controls) return GV_ERR_STATE;
  return copy_out(h, out, m.controls, (size_t)m.cK * (size_t)m.cP * (size_t)m.cC * sizeof(float));
}

int gv_mppi_update_async(gv_handle h, const gv_critic_weights *w, uint32_t flags, gv_control_result *result,
                         uint64_t *totals, float *nominal_out)
{
  if (!h) return GV_ERR_BAD_ARG;
  GV_TRY
  if (!control_args_ok(w, flags, result, totals)) return GV_ERR_BAD_ARG;
  int rc = mppi_update_refused(h, "gv_mppi_update", *w, false);
  if (rc || (rc = set_device_only(h))) return rc;
  return mppi_enqueue_update(h, *w, flags, result, totals, nominal_out);
  GV_CATCH
}

int gv_mppi_update(gv_handle h, const gv_critic_weights *w, uint32_t flags, gv_control_result *result, uint64_t *totals,
                   float *nominal_out)
{
  return wait_scored(h, gv_mppi_update_async(h, w, flags, result, totals, nominal_out), 1);
}

// Every rule of the three calls first, then their enqueues: sample, rollout of the sampled controls, update.
int gv_mppi_cycle_async(gv_handle h, const double start[3], int32_t K, uint64_t seed, uint64_t iteration,
                        uint32_t sample_flags, const gv_critic_weights *w, uint32_t flags, gv_control_result *result,
                        uint64_t *totals, float *nominal_out)
{
  if (!h) return GV_ERR_BAD_ARG;
  GV_TRY
  if (!start || !std::isfinite(start[0]) || !std::isfinite(start[1]) || !std::isfinite(start[2]) || K < 0 || K > (1 << 20) ||
      (sample_flags & ~(uint32_t)GV_MPPI_SHIFT) != 0 || !control_args_ok(w, flags, result, totals))
    return GV_ERR_BAD_ARG;
  int rc = mppi_sample_refused(h, "gv_mppi_cycle");
  if (rc || (rc = mppi_update_refused(h, "gv_mppi_cycle", *w, true))) return rc;
  if (!mppi_shape_ok(K, h->mppi.P)) return GV_ERR_BAD_ARG;
  if (K == 0 || (rc = set_device_only(h))) return rc;
  if ((rc = mppi_enqueue_sample(h, K, seed, iteration, sample_flags))) return rc;
  if ((rc = gv_rollout_async(h, start, h->mppi.controls, K, h->mppi.P, GV_ROLLOUT_DEVICE_CONTROLS))) return rc;
  return mppi_enqueue_update(h, *w, flags, result, totals, nominal_out);
  GV_CATCH
}

int gv_mppi_cycle(gv_handle h, const double start[3], int32_t K, uint64_t seed, uint64_t iteration, uint32_t sample_flags,
                  const gv_critic_weights *w, uint32_t flags, gv_control_result *result, uint64_t *totals, float *nominal_out)
{
  return wait_scored(h, gv_mppi_cycle_async(h, start, K, seed, iteration, sample_flags, w, flags, result, totals, nominal_out), K);
}

// host only: gv_mppi.hpp's text in loops
int gv_mppi_words(uint64_t seed, uint64_t iteration, uint32_t k, uint32_t p, uint32_t words[4])
{
  if (!words) return GV_ERR_BAD_ARG;
  mppi_words(seed, iteration, k, p, words);
  return GV_OK;
}

int gv_mppi_sample_controls(const gv_mppi_config *cfg, int32_t C, const float *nominal, int32_t K, int32_t P, uint64_t seed,
                            uint64_t iteration, uint32_t flags, float *controls_out)
{
  if (!cfg || (C != 2 && C != 3) || !nominal || !controls_out || !mppi_shape_ok(K, P) || !mppi_config_valid(*cfg, C) ||
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

// the sequential definition: the admitted trajectories in index order, one column after the other
int gv_mppi_average(const gv_mppi_config *cfg, int32_t C, const float *controls, const uint64_t *totals, int32_t K,
                    int32_t P, const float *nominal_in, float *nominal_out)
{
  return gv_mppi_average_cc(cfg, C, controls, totals, nullptr, K, P, nominal_in, nominal_out);
}

// ---- [EXTENSION] X12: limits on the samples, control cost ----
// handle configuration only, like gv_set_mppi
int gv_set_mppi_limits(gv_handle h, const gv_mppi_limits *lim)
{
  if (!h) return GV_ERR_BAD_ARG;
  if (!lim) {
    h->mppi.lim_set = false;
    return GV_OK;
  }
  if (!mppi_limits_valid(*lim)) return GV_ERR_BAD_ARG;
  h->mppi.lim = *lim;
  h->mppi.lim_set = true;
  return GV_OK;
}

int gv_get_mppi_control_costs(gv_handle h, double *out)
{
  if (!h || !out) return GV_ERR_BAD_ARG;
  const gv_context::Mppi &m = h->mppi;
  if (!m.have_costs) return GV_ERR_STATE;
  return copy_out(h, out, m.cost, (size_t)m.costK * sizeof(double));
}

// host only: the chain of gv_mppi.hpp, trajectory after trajectory
int gv_mppi_constrain(const gv_mppi_limits *lim, const gv_motion_model *m, float *controls, int32_t K, int32_t P)
{
  if (!lim || !m || !controls || !mppi_shape_ok(K, P) || !mppi_limits_valid(*lim) || !motion_model_valid(*m) ||
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

// host only: the 64 partial sums and the tree of gv_mppi.hpp
int gv_mppi_control_costs(const gv_mppi_config *cfg, const gv_mppi_limits *lim, int32_t C, const float *controls,
                          const float *nominal, int32_t K, int32_t P, uint32_t sample_flags, double *g_out)
{
  if (!cfg || !lim || (C != 2 && C != 3) || !controls || !nominal || !g_out || !mppi_shape_ok(K, P) ||
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

// host only, sums in index order.  control_costs null: x_k is the totals' difference alone, gv_mppi_average.
int gv_mppi_average_cc(const gv_mppi_config *cfg, int32_t C, const float *controls, const uint64_t *totals,
                       const double *control_costs, int32_t K, int32_t P, const float *nominal_in, float *nominal_out)
{
  gv_context *h = nullptr;
  if (!cfg || (C != 2 && C != 3) || !controls || !totals || !nominal_in || !nominal_out || !mppi_shape_ok(K, P) ||
      !mppi_config_valid(*cfg, C))
    return GV_ERR_BAD_ARG;
  GV_TRY
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
  GV_CATCH
}

// ---- [EXTENSION] X13: scoring against predicted moving objects ----
int gv_dyn_cost_table(const gv_dyn_config *cfg, uint8_t *table, int32_t cap, int32_t *n)
{
  gv_context *h = nullptr;
  if (!cfg) return GV_ERR_BAD_ARG;
  GV_TRY
  host::InflationTable t;
  if (!dyn_config_table(*cfg, t)) return GV_ERR_BAD_ARG;
  if (n) *n = t.d2max + 1;
  if (!table || cap < t.d2max + 1) return GV_ERR_BAD_ARG;
  std::memcpy(table, t.cost.data(), t.cost.size());
  return GV_OK;
  GV_CATCH
}

// handle configuration: the table is built here on the host and reaches the device with the next call that scores
// (dyn_kernel_args).  A rejected configuration leaves the one in force alone.
int gv_set_dyn_config(gv_handle h, const gv_dyn_config *cfg)
{
  if (!h) return GV_ERR_BAD_ARG;
  GV_TRY
  gv_context::DynScore &d = h->dyn;
  if (!cfg) {
    d.set = false;
    return GV_OK;
  }
  host::InflationTable t;
  if (!dyn_config_table(*cfg, t)) return GV_ERR_BAD_ARG;
  d.tab = std::move(t);
  d.cfg = *cfg;
  for (int32_t i = cfg->n_circles; i < kDynMaxCircles; ++i) d.cfg.off_x[i] = 0.0;
  d.dirty = true;
  d.set = true;
  return GV_OK;
  GV_CATCH
}

// The object table is built on the host into a pinned slot and goes to the device by one copy command on the public
// stream: the calls enqueued before it read the slot they were given, the calls after it the new one.
int gv_set_moving_objects(gv_handle h, const gv_moving_object *objs, int32_t n)
{
  if (!h) return GV_ERR_BAD_ARG;
  GV_TRY
  if (!moving_objects_ok(objs, n)) return GV_ERR_BAD_ARG;
  gv_context::DynScore &d = h->dyn;
  if (n > 0) {
    int rc = set_device_only(h);
    if (rc) return rc;
    DynObject rows[kDynMaxObjects];
    for (int32_t j = 0; j < n; ++j) rows[j] = dyn_object(objs[j]);
    if ((rc = upload_slot(h, d.objs, rows, (size_t)n * sizeof(DynObject), kDynSlotBytes))) return rc;
  }
  d.n_obj = n;
  d.n_obj_dev = nullptr;   // a set a gv_track_update fed (X14) ends here
  return GV_OK;
  GV_CATCH
}

// gv_score_trajectories_async with another kernel and another record; no grid and no costmap is read
int gv_score_dynamic_async(gv_handle h, const float *poses, int32_t K, int32_t P, uint32_t flags, gv_dyn_score *scores,
                           uint8_t *pose_cost)
{
  if (!h) return GV_ERR_BAD_ARG;
  GV_TRY
  const bool keep = (flags & GV_TRAJ_KEEP_POSE_COST) != 0;
  if (!batch_ok(poses, scores, K, P, flags, host::kTrajFlags) || (keep && !pose_cost)) return GV_ERR_BAD_ARG;
  gv_context::DynScore &d = h->dyn;
  if (!d.set) {
    h->err = "gv_score_dynamic: no configuration set (gv_set_dyn_config)";
    return GV_ERR_STATE;
  }
  int rc = GV_OK;
  if (K == 0 || (rc = set_device_only(h))) return rc;
  const size_t n_poses = (size_t)K * (size_t)P;
  DynArgs a{};
  a.K = K; a.P = P;
  ResultDest<gv_dyn_score> to_scores;
  ResultDest<uint8_t> to_pose_cost;   // stays closed (null, no copy) without GV_TRAJ_KEEP_POSE_COST
  if ((rc = dyn_kernel_args(h, a)) || (rc = stage_poses(h, poses, n_poses, flags, &a.poses)) ||
      (rc = to_scores.open(h, scores, (size_t)K, 8, d.d_scores)) || (keep && (rc = to_pose_cost.open(h, pose_cost, n_poses, 1, d.d_pose_cost))))
    return rc;
  a.scores = to_scores.dev;
  a.pose_cost = to_pose_cost.dev;
  launch_score_dynamic(a, h->stream);
  GV_HIP(hipGetLastError());
  if ((rc = to_scores.copy_back(h)) || (rc = to_pose_cost.copy_back(h))) return rc;
  return GV_OK;
  GV_CATCH
}

int gv_score_dynamic(gv_handle h, const float *poses, int32_t K, int32_t P, uint32_t flags, gv_dyn_score *scores,
                     uint8_t *pose_cost)
{
  return wait_scored(h, gv_score_dynamic_async(h, poses, K, P, flags, scores, pose_cost), K);
}

// host only: gv_dyn.hpp's text in loops, one trajectory after the other, one pose after the other
int gv_dyn_score_poses(const gv_dyn_config *cfg, const gv_moving_object *objs, int32_t n, const float *poses, int32_t K,
                       int32_t P, gv_dyn_score *scores, uint8_t *pose_cost)
{
  gv_context *h = nullptr;
  if (!cfg || !batch_ok(poses, scores, K, P, 0u, 0u) || !moving_objects_ok(objs, n)) return GV_ERR_BAD_ARG;
  GV_TRY
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
  GV_CATCH
}

// host only: gv_control_select with the third record
int gv_control_select_dyn(const gv_critic_weights *w, const gv_traj_score *traj, const gv_nav_score *nav,
                          const gv_dyn_score *dyn, const gv_dyn_config *cfg, int32_t K, gv_control_result *result,
                          uint64_t *totals)
{
  if (!cfg) return gv_control_select(w, traj, nav, K, result, totals);
  if (!w || !traj || !dyn || !result || !critic_weights_valid(*w) || K < 0 || K > (1 << 20) || cfg->w_sum > 65535u ||
      cfg->w_max > 65535u || (critic_nav_used(*w) && !nav))
    return GV_ERR_BAD_ARG;
  control_select_host(*w, traj, nav, dyn, cfg->w_sum, cfg->w_max, K, result, totals);
  return GV_OK;
}

// ---- [EXTENSION] X14: the tracker over the tick's boxes ----
// handle configuration: it travels in the kernel arguments of the updates enqueued from now on.  Turning it off makes
// the state the one after gv_create without touching the device: the next update is told to ignore the block.
int gv_set_track_config(gv_handle h, const gv_track_config *cfg)
{
  if (!h) return GV_ERR_BAD_ARG;
  gv_context::Track &t = h->trk;
  if (!cfg) {
    t.set = false;
    t.fresh = true;
    return GV_OK;
  }
  if (!track_config_valid(*cfg)) return GV_ERR_BAD_ARG;
  t.cfg = *cfg;
  t.set = true;
  return GV_OK;
}

// The block is built on the host into a pinned staging slot and replaces the resident one by one copy command on the
// public stream, behind the updates enqueued before it.
int gv_set_tracks(gv_handle h, const gv_track *tracks, int32_t n, uint32_t next_id)
{
  if (!h) return GV_ERR_BAD_ARG;
  GV_TRY
  TrackState st;
  if (!track_state_from(tracks, n, next_id, st)) return GV_ERR_BAD_ARG;
  gv_context::Track &t = h->trk;
  int rc = GV_OK;
  if ((rc = set_device_only(h)) || (rc = t.state.reserve(h, 1))) return rc;
  const int k = t.up.slot ^ 1;
  if ((rc = t.up.stage[k].reserve(h, sizeof(TrackState), hipHostMallocDefault))) return rc;
  if (!t.up.staged[k]) GV_HIP(t.up.staged[k].create(hipEventDisableTiming));
  if (t.up.staged_used[k]) GV_HIP(hipEventSynchronize(t.up.staged[k]));
  std::memcpy(t.up.stage[k].get(), &st, sizeof(st));
  GV_HIP(hipMemcpyAsync(t.state.get(), t.up.stage[k].get(), sizeof(st), hipMemcpyHostToDevice, h->stream));
  GV_HIP(hipEventRecord(t.up.staged[k], h->stream));
  t.up.staged_used[k] = true;
  t.up.slot = k;
  t.fresh = false;
  return GV_OK;
  GV_CATCH
}

int gv_get_tracks(gv_handle h, gv_track *out, int32_t cap, int32_t *n, uint32_t *next_id)
{
  if (!h || cap < 0 || (cap > 0 && !out)) return GV_ERR_BAD_ARG;
  GV_TRY
  gv_context::Track &t = h->trk;
  std::vector<TrackState> st(1);
  if (t.fresh) {
    std::memset(st.data(), 0, sizeof(TrackState));
    st[0].next_id = 1u;
  } else {
    if (int rc = set_device_only(h)) return rc;
    GV_HIP(hipMemcpyAsync(st.data(), t.state.get(), sizeof(TrackState), hipMemcpyDeviceToHost, h->stream));
    GV_HIP(hipStreamSynchronize(h->stream));
  }
  const int32_t live = track_state_live(st[0], out, cap);
  if (n) *n = live;
  if (next_id) *next_id = st[0].next_id;
  return live <= cap ? GV_OK : GV_ERR_BAD_ARG;
  GV_CATCH
}

// One kernel on the public stream; with GV_TRACK_FEED_DYNAMIC it also writes the slot of X13's object table that is not
// the current one -- every kernel that was given that slot is ahead of it on the stream -- and the slot is the current
// one for the calls enqueued from now on, with its count on the device.
int gv_track_update_async(gv_handle h, const gv_lshape_pose *dets, int32_t n, double dt, const gv_transform *motion,
                          uint32_t flags, gv_track_info *info, gv_track *tracks)
{
  if (!h) return GV_ERR_BAD_ARG;
  GV_TRY
  if (!track_update_ok(dets, n, dt, motion) || (flags & ~(uint32_t)(GV_TRACK_DEVICE_DETS | GV_TRACK_FEED_DYNAMIC)) != 0)
    return GV_ERR_BAD_ARG;
  gv_context::Track &t = h->trk;
  gv_context::DynScore &d = h->dyn;
  if (!t.set) {
    h->err = "gv_track_update: no configuration set (gv_set_track_config)";
    return GV_ERR_STATE;
  }
  const bool feed = (flags & GV_TRACK_FEED_DYNAMIC) != 0;
  const int k = d.objs.slot ^ 1;
  int rc = GV_OK;
  if ((rc = set_device_only(h)) || (rc = t.state.reserve(h, 1)) || (feed && (rc = d.objs.dev[k].reserve(h, kDynSlotBytes)))) return rc;
  TrackArgs a{};
  a.p = track_params(t.cfg);
  a.ego = track_ego(motion);
  a.dt = dt;
  a.fresh = t.fresh ? 1 : 0;
  a.n = n;
  a.dets = dets;
  if (n > 0 && !(flags & GV_TRACK_DEVICE_DETS)) {
    if ((rc = upload_slot(h, t.dets, dets, (size_t)n * sizeof(gv_lshape_pose), (size_t)kTrackSlots * sizeof(gv_lshape_pose)))) return rc;
    a.dets = reinterpret_cast<const gv_lshape_pose *>(t.dets.dev[t.dets.slot].get());
  }
  a.state = t.state;
  ResultDest<gv_track_info> to_info;   // each stays closed (null, no copy) when the caller passes null
  ResultDest<gv_track> to_tracks;
  if ((info && (rc = to_info.open(h, info, 1, 8, t.d_info))) || (tracks && (rc = to_tracks.open(h, tracks, (size_t)kTrackSlots, 8, t.d_tracks))))
    return rc;
  a.info = to_info.dev;
  a.tracks = to_tracks.dev;
  if (feed) {
    a.feed_objs = reinterpret_cast<DynObject *>(d.objs.dev[k].get());
    a.feed_n = reinterpret_cast<int32_t *>(d.objs.dev[k].get() + kDynRowsBytes);
  }
  launch_track_update(a, h->stream);
  GV_HIP(hipGetLastError());
  t.fresh = false;
  if (feed) {
    d.objs.slot = k;
    d.n_obj = kDynMaxObjects;   // the host does not learn the count: up to 128
    d.n_obj_dev = a.feed_n;
  }
  if ((rc = to_info.copy_back(h)) || (rc = to_tracks.copy_back(h))) return rc;
  return GV_OK;
  GV_CATCH
}

int gv_track_update(gv_handle h, const gv_lshape_pose *dets, int32_t n, double dt, const gv_transform *motion, uint32_t flags,
                    gv_track_info *info, gv_track *tracks)
{
  return wait_scored(h, gv_track_update_async(h, dets, n, dt, motion, flags, info, tracks), 1);
}

// host only: gv_track.hpp's text, the association as a literal sort
int gv_track_step(const gv_track_config *cfg, gv_track *tracks, int32_t *n_tracks, uint32_t *next_id, const gv_lshape_pose *dets,
                  int32_t n, double dt, const gv_transform *motion, gv_track_info *info, gv_moving_object *objs, int32_t *n_objs)
{
  gv_context *h = nullptr;
  if (!cfg || !track_config_valid(*cfg) || !tracks || !n_tracks || !next_id || !track_update_ok(dets, n, dt, motion) ||
      (objs != nullptr) != (n_objs != nullptr))
    return GV_ERR_BAD_ARG;
  GV_TRY
  std::vector<TrackState> st(1);
  if (!track_state_from(tracks, *n_tracks, *next_id, st[0])) return GV_ERR_BAD_ARG;
  track_step(track_params(*cfg), st[0], dets, n, dt, motion, info, objs, n_objs);
  *n_tracks = track_state_live(st[0], tracks, kTrackSlots);
  *next_id = st[0].next_id;
  return GV_OK;
  GV_CATCH
}

}  // extern "C"
