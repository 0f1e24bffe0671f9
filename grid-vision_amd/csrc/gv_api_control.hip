// gv_api_control.hip -- the controller side of the C ABI, what runs over the layers gv_api_planner.hip makes and samples:
//   [EXTENSION] X10 the rollout and the control step (gv_set_motion_model, gv_rollout*, gv_control_step*),
//   [EXTENSION] X11, X12 MPPI's two ends around them and their limits (gv_set_mppi, gv_set_mppi_limits, gv_mppi_*),
//   [EXTENSION] X13 the configuration and the object set of the dyn sampler (gv_set_dyn_config, gv_set_moving_objects),
//   [EXTENSION] X14 the tracker that can feed that set on the device (gv_set_track_config, gv_*_tracks, gv_track_update*).
// The kernels are gv_rollout.hip, gv_mppi.hip and gv_track.hip; the samplers a control step and an MPPI update run are
// gv_api_planner.hip's (enqueue_control_scores), the host twins gv_api_planner_host.hip's.
#include <cstring>
#include <vector>

#include "gv_context.hpp"
#include "gv_mppi.hpp"
#include "gv_planner_rules.hpp"

namespace {

// A slot of X13's object table: the rows, and behind them the count that a fed gv_track_update (X14) writes.
constexpr size_t kDynRowsBytes = (size_t)kDynMaxObjects * sizeof(DynObject);
constexpr size_t kDynSlotBytes = kDynRowsBytes + 16;

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
  return why ? state_error(h, call, why) : GV_OK;
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
  return why ? state_error(h, call, why) : GV_OK;
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

// ---- [EXTENSION] X10: rollout and control step ----
// handle configuration only; every rollout copies h->roll.model into its kernel arguments
int gv_set_motion_model(gv_handle h, const gv_motion_model *m)
{
  return h ? set_config(m, m && motion_model_valid(*m), h->roll.model, h->roll.set) : GV_ERR_BAD_ARG;
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
  if (!r.set) return state_error(h, "gv_rollout", "no motion model set (gv_set_motion_model)");
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

// The samplers over the resident rollout and the selection (enqueue_control_scores), then a copy per result the
// selection cannot write in place, all on the public stream.
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
  return (rc = to_result.copy_back(h)) ? rc : to_totals.copy_back(h);
  GV_CATCH
}

int gv_control_step(gv_handle h, const gv_critic_weights *w, uint32_t flags, gv_control_result *result, uint64_t *totals)
{
  return wait_scored(h, gv_control_step_async(h, w, flags, result, totals), 1);
}

// ---- [EXTENSION] X11: MPPI sampling and softmax update ----
// handle configuration only; every sampling and update copies h->mppi.cfg into its kernel arguments
int gv_set_mppi(gv_handle h, const gv_mppi_config *cfg)
{
  return h ? set_config(cfg, cfg && mppi_config_valid(*cfg, 3), h->mppi.cfg, h->mppi.set) : GV_ERR_BAD_ARG;
}

// One copy on the public stream and the wait for it: the caller's array is free on return.
int gv_mppi_set_nominal(gv_handle h, const float *nominal, int32_t P)
{
  if (!h) return GV_ERR_BAD_ARG;
  GV_TRY
  if (!nominal || !shape_ok(0, P, false)) return GV_ERR_BAD_ARG;
  if (!h->roll.set) return state_error(h, "gv_mppi_set_nominal", "no motion model set (gv_set_motion_model)");
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

// One kernel on the public stream.  The controls buffer grows by DevBuf::reserve, like the rollout's.  K is checked
// alone first: P is the nominal's, which the state rules vouch for.
int gv_mppi_sample_async(gv_handle h, int32_t K, uint64_t seed, uint64_t iteration, uint32_t flags)
{
  if (!h) return GV_ERR_BAD_ARG;
  GV_TRY
  if (!shape_ok(K, 1, false) || (flags & ~(uint32_t)GV_MPPI_SHIFT) != 0) return GV_ERR_BAD_ARG;
  int rc = mppi_sample_refused(h, "gv_mppi_sample");
  if (rc) return rc;
  if (!shape_ok(K, h->mppi.P, true)) return GV_ERR_BAD_ARG;
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
  if (!start || !std::isfinite(start[0]) || !std::isfinite(start[1]) || !std::isfinite(start[2]) || !shape_ok(K, 1, false) ||
      (sample_flags & ~(uint32_t)GV_MPPI_SHIFT) != 0 || !control_args_ok(w, flags, result, totals))
    return GV_ERR_BAD_ARG;
  int rc = mppi_sample_refused(h, "gv_mppi_cycle");
  if (rc || (rc = mppi_update_refused(h, "gv_mppi_cycle", *w, true))) return rc;
  if (!shape_ok(K, h->mppi.P, true)) return GV_ERR_BAD_ARG;
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

// ---- [EXTENSION] X12: limits on the samples, control cost ----
// handle configuration only, like gv_set_mppi
int gv_set_mppi_limits(gv_handle h, const gv_mppi_limits *lim)
{
  return h ? set_config(lim, lim && mppi_limits_valid(*lim), h->mppi.lim, h->mppi.lim_set) : GV_ERR_BAD_ARG;
}

int gv_get_mppi_control_costs(gv_handle h, double *out)
{
  if (!h || !out) return GV_ERR_BAD_ARG;
  const gv_context::Mppi &m = h->mppi;
  if (!m.have_costs) return GV_ERR_STATE;
  return copy_out(h, out, m.cost, (size_t)m.costK * sizeof(double));
}

// ---- [EXTENSION] X13: the configuration and the object set ----
// handle configuration: the table is built here on the host and reaches the device with the next call that scores
// (dyn_kernel_args, gv_api_planner.hip).  A rejected configuration leaves the one in force alone.
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

// The object table is built on the host and goes to the device through `objs`' slots: the calls enqueued before it
// read the slot they were given, the calls after it the new one.
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

// ---- [EXTENSION] X14: the tracker over the tick's boxes ----
// handle configuration: it travels in the kernel arguments of the updates enqueued from now on.  Turning it off makes
// the state the one after gv_create without touching the device: the next update is told to ignore the block.
int gv_set_track_config(gv_handle h, const gv_track_config *cfg)
{
  if (!h) return GV_ERR_BAD_ARG;
  if (!cfg) h->trk.fresh = true;
  return set_config(cfg, cfg && track_config_valid(*cfg), h->trk.cfg, h->trk.set);
}

// The block is built on the host and replaces the resident one through `up`'s staging slots, behind the updates
// enqueued before it.
int gv_set_tracks(gv_handle h, const gv_track *tracks, int32_t n, uint32_t next_id)
{
  if (!h) return GV_ERR_BAD_ARG;
  GV_TRY
  TrackState st;
  if (!track_state_from(tracks, n, next_id, st)) return GV_ERR_BAD_ARG;
  gv_context::Track &t = h->trk;
  int rc = GV_OK;
  if ((rc = set_device_only(h)) || (rc = t.state.reserve(h, 1)) || (rc = stage_upload(h, t.up, &st, sizeof(st), sizeof(st), t.state.get())))
    return rc;
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
// the current one, which is the current one for the calls enqueued from now on, with its count on the device
// (gv_context::UploadSlots).
int gv_track_update_async(gv_handle h, const gv_lshape_pose *dets, int32_t n, double dt, const gv_transform *motion,
                          uint32_t flags, gv_track_info *info, gv_track *tracks)
{
  if (!h) return GV_ERR_BAD_ARG;
  GV_TRY
  if (!track_update_ok(dets, n, dt, motion) || !track_update_flags_ok(flags, dets, n)) return GV_ERR_BAD_ARG;
  gv_context::Track &t = h->trk;
  gv_context::DynScore &d = h->dyn;
  if (!t.set) return state_error(h, "gv_track_update", "no configuration set (gv_set_track_config)");
  // [EXTENSION] X15: the list of the most recently enqueued tick, pending or waited for; its count stays on the device
  const bool from_tick = (flags & GV_TRACK_TICK_DETS) != 0;
  if (from_tick && !h->tick.dets_live)
    return state_error(h, "gv_track_update", "GV_TRACK_TICK_DETS: the last tick enqueued did not carry GV_TICK_KEEP_DETS");
  const bool feed = (flags & GV_TRACK_FEED_DYNAMIC) != 0;
  const int k = d.objs.st.slot ^ 1;
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
    a.dets = reinterpret_cast<const gv_lshape_pose *>(t.dets.current());
  }
  if (from_tick) {
    a.n = 0;
    a.dets = h->tick.dets.get()->p;
    a.n_dev = &h->tick.dets.get()->n;
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
    d.objs.st.slot = k;
    d.n_obj = kDynMaxObjects;   // the host does not learn the count: up to 128
    d.n_obj_dev = a.feed_n;
  }
  return (rc = to_info.copy_back(h)) ? rc : to_tracks.copy_back(h);
  GV_CATCH
}

int gv_track_update(gv_handle h, const gv_lshape_pose *dets, int32_t n, double dt, const gv_transform *motion, uint32_t flags,
                    gv_track_info *info, gv_track *tracks)
{
  return wait_scored(h, gv_track_update_async(h, dets, n, dt, motion, flags, info, tracks), 1);
}

}  // extern "C"
