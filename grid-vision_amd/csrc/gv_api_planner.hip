// gv_api_planner.hip -- the planner side of the C ABI, everything that makes or samples a map layer:
//   [EXTENSION] X6  the inflated costmap layer (gv_set_inflation, gv_inflate, its getters and publisher),
//   [EXTENSION] X7  footprint scoring of trajectories against it (gv_set_footprint, gv_score_trajectories*),
//   [EXTENSION] X9  the goal / path distance field over it (gv_set_nav_config, gv_nav_field and its getters) and its
//                   sampler along trajectories (gv_score_nav*),
//   [EXTENSION] X13 the third sampler, against predicted moving objects (gv_score_dynamic*).
// The kernels are gv_inflate.hip, gv_trajscore.hip, gv_navfield.hip (which also argues why the rounds end at the exact
// field) and gv_dynscore.hip.  What the calls here and the controller's (gv_api_control.hip) do alike is written once,
// in front of the entry points: the refusals, the upload through alternating slots, a sampler's call, and the samplers
// over the resident rollout.  The host-only twins are gv_api_planner_host.hip's.
#include <algorithm>
#include <cstring>
#include <string>

#include "gv_context.hpp"
#include "gv_planner_rules.hpp"

namespace {

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

// What every launch of a sampler carries from the handle; the caller adds the poses, K, P and the destinations.  The
// dyn sampler's takes the configuration and the set in force now, and a changed cost table goes to the device first.
TrajArgs traj_args(const gv_context *h)
{
  TrajArgs a{};
  a.g = h->g;
  a.fp = h->traj.fp;
  a.cost = h->infl.cost;
  return a;
}

NavScoreArgs nav_args(const gv_context *h)
{
  NavScoreArgs a{};
  a.g = h->g;
  a.field = h->nav.field;
  return a;
}

int dyn_kernel_args(gv_context *h, DynArgs &a)
{
  gv_context::DynScore &d = h->dyn;
  if (d.dirty) {
    if (int rc = upload_slot(h, d.table, d.tab.cost.data(), d.tab.cost.size(), host::kTableBytes)) return rc;
    d.dirty = false;
  }
  a.p = dyn_params(d.cfg, d.tab.d2max + 1);
  a.objs = reinterpret_cast<const DynObject *>(d.objs.current());
  a.n_obj = d.n_obj;
  a.n_obj_dev = d.n_obj_dev;
  a.table = d.table.current();
  return GV_OK;
}

// A sampler's call once its rules hold, all on the public stream: a copy of the poses (host poses only), one kernel over
// `a` (which has K and P), and a copy per result the kernel cannot write in place.  The records' pinned view is aligned
// to `align`, d_scores / d_pose_cost are the landing buffers; pose_cost null (no copy): the kernel keeps none, and a
// sampler that never does names no argument for it.
template <typename Args, typename Score>
int enqueue_sampler(gv_context *h, Args &a, void (*launch)(const Args &, hipStream_t), const float *poses, uint32_t flags,
                    Score *scores, size_t align, DevBuf<Score> &d_scores, uint8_t *pose_cost = nullptr,
                    uint8_t *Args::*pose_cost_arg = nullptr, DevBuf<uint8_t> *d_pose_cost = nullptr)
{
  const size_t n_poses = (size_t)a.K * (size_t)a.P;
  ResultDest<Score> to_scores;
  ResultDest<uint8_t> to_pose_cost;
  int rc = GV_OK;
  if ((rc = stage_poses(h, poses, n_poses, flags, &a.poses)) || (rc = to_scores.open(h, scores, (size_t)a.K, align, d_scores)) ||
      (pose_cost && (rc = to_pose_cost.open(h, pose_cost, n_poses, 1, *d_pose_cost))))
    return rc;
  a.scores = to_scores.dev;
  if (pose_cost) a.*pose_cost_arg = to_pose_cost.dev;
  launch(a, h->stream);
  GV_HIP(hipGetLastError());
  return (rc = to_scores.copy_back(h)) ? rc : to_pose_cost.copy_back(h);
}

}  // namespace

namespace gv_internal __attribute__((visibility("hidden"))) {

// every GV_ERR_STATE of the planner and controller calls: h->err says which call refused and why
int state_error(gv_context *h, const char *call, const char *why)
{
  h->err = std::string(call) + ": " + why;
  return GV_ERR_STATE;
}

// What a call refuses with GV_ERR_STATE, checked in this order: `missing` (the call's own configuration is not set:
// the caller passes the text, or null), a rollout or a layer in `needs` that no call has made since gv_create (the
// rollout) or gv_create / gv_reset (the layers), and a communicator of more than one rank (`sharded`: why a row band
// of the grid will not do).
int refuse_state(gv_context *h, const char *call, const char *missing, unsigned needs, const char *sharded)
{
  std::string why;
  if (missing) why = missing;
  else if ((needs & kNeedRollout) && !h->roll.have) why = "no rollout (gv_rollout)";
  else if ((needs & kNeedCostmap) && !h->infl.have_cost) why = "no costmap (gv_inflate)";
  else if ((needs & kNeedField) && !h->nav.have_field) why = "no distance field (gv_nav_field)";
  else if (h->sh.world > 1) why = std::string("ranks own row bands of the grid, ") + sharded;
  else return GV_OK;
  return state_error(h, call, why.c_str());
}

// `bytes` (> 0) of host data to `dst` on the device through the staging slot of `s` that is not the current one, of
// `cap` bytes: the wait for that slot's last copy, the memcpy, one copy command on the public stream, its event.
int stage_upload(gv_context *h, gv_context::StageSlots &s, const void *src, size_t bytes, size_t cap, void *dst)
{
  const int k = s.slot ^ 1;
  if (int rc = s.stage[k].reserve(h, cap, hipHostMallocDefault)) return rc;
  if (!s.staged[k]) GV_HIP(s.staged[k].create(hipEventDisableTiming));
  if (s.staged_used[k]) GV_HIP(hipEventSynchronize(s.staged[k]));
  std::memcpy(s.stage[k].get(), src, bytes);
  GV_HIP(hipMemcpyAsync(dst, s.stage[k].get(), bytes, hipMemcpyHostToDevice, h->stream));
  GV_HIP(hipEventRecord(s.staged[k], h->stream));
  s.staged_used[k] = true;
  s.slot = k;
  return GV_OK;
}

// ... into the device slot of `u` that is not the current one; that slot is the current one afterwards
int upload_slot(gv_context *h, gv_context::UploadSlots &u, const void *src, size_t bytes, size_t cap)
{
  DevBuf<uint8_t> &dev = u.dev[u.st.slot ^ 1];
  if (int rc = dev.reserve(h, cap)) return rc;
  return stage_upload(h, u.st, src, bytes, cap, dev.get());
}

// the synchronous form of a call: rc is what its asynchronous form returned
int wait_scored(gv_context *h, int rc, int32_t K)
{
  if (rc || K == 0) return rc;
  GV_HIP(hipStreamSynchronize(h->stream));
  return GV_OK;
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
  TrajArgs t = traj_args(h);
  t.poses = r.poses;
  t.K = K; t.P = P;
  t.scores = h->traj.d_scores;
  launch_score_trajectories(t, h->stream);
  if (nav_used) {
    NavScoreArgs n = nav_args(h);
    n.poses = r.poses;
    n.K = K; n.P = P;
    n.scores = h->nav.d_scores;
    launch_score_nav(n, h->stream);
  }
  if (dyn_used) {
    DynArgs d{};
    if ((rc = dyn_kernel_args(h, d))) return rc;
    d.poses = r.poses;
    d.K = K; d.P = P;
    d.scores = h->dyn.d_scores;
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

// What gv_nav_field and gv_nav_field_from_path do alike before their seeds: the refusals, the buffers (room for
// `seed_room` host seeds in the staging block), the kernel arguments of this grid, costmap and configuration, and the
// flags and the seed counter zeroed on the public stream.  The field counts as absent until nav_field_relax has converged.
int nav_field_begin(gv_context *h, const char *call, size_t seed_room, NavArgs &a)
{
  gv_context::NavField &f = h->nav;
  int rc = refuse_state(h, call, f.set ? nullptr : "no configuration set (gv_set_nav_config)", kNeedCostmap,
                        "there is no whole costmap");
  if (rc || (rc = set_device_only(h))) return rc;
  constexpr int kBatchMax = gv_context::NavField::kBatchMax;
  static_assert((1 + kBatchMax) * sizeof(uint32_t) <= kNavSeedOff, "the counters fit in front of the seeds");
  const int32_t G = h->g.G;
  const int32_t tiles_x = (h->g.nx + kNavTile - 1) / kNavTile, tiles_y = (h->g.ny + kNavTile - 1) / kNavTile;
  const size_t n_tiles = (size_t)tiles_x * (size_t)tiles_y;
  if ((rc = f.field.reserve(h, ((size_t)G + 3) / 4 * 4))) return rc;
  if ((rc = f.flags.reserve(h, 2 * n_tiles))) return rc;
  if ((rc = f.counters.reserve(h, 1 + kBatchMax))) return rc;
  if (seed_room && (rc = f.d_seeds.reserve(h, seed_room))) return rc;
  if ((rc = f.stage.reserve(h, kNavSeedOff + seed_room * sizeof(int32_t), hipHostMallocDefault))) return rc;
  if (!f.done) GV_HIP(f.done.create(hipEventDisableTiming));
  f.have_field = false;   // until this call has converged

  a = NavArgs{};
  a.nx = h->g.nx; a.ny = h->g.ny; a.G = G;
  a.tiles_x = tiles_x; a.tiles_y = tiles_y;
  a.step = NavStep{f.cfg.obstacle_cost, f.cfg.cost_weight};
  a.pass_cap = h->tune.nav_pass_cap;
  a.cost = h->infl.cost;
  a.field = f.field;
  a.flags_out = f.flags;          // round 0 reads the first half
  a.counter = f.counters;         // [0]: seeds used
  GV_HIP(hipMemsetAsync(f.flags, 0, 2 * n_tiles * sizeof(uint32_t), h->stream));
  GV_HIP(hipMemsetAsync(f.counters, 0, sizeof(uint32_t), h->stream));
  return GV_OK;
}

// The relaxation behind the seeds: rounds in batches of 4, 8, .. kBatchMax launches; a batch ends with its counters
// copied into the pinned block and one event wait, and the loop stops after the first round whose counter is 0 (the
// rounds behind it in the batch found no active tile and did nothing).
int nav_field_relax(gv_context *h, const char *call, NavArgs &a, gv_nav_info *info)
{
  gv_context::NavField &f = h->nav;
  constexpr int kBatchMax = gv_context::NavField::kBatchMax;
  const size_t n_tiles = (size_t)a.tiles_x * (size_t)a.tiles_y;
  const volatile uint32_t *landed = reinterpret_cast<const volatile uint32_t *>(f.stage.get());
  const int64_t max_rounds = (int64_t)a.G + 2;
  int64_t rounds = 0;
  int batch = 4;
  for (bool converged = false; !converged;) {
    if (rounds >= max_rounds) return state_error(h, call, "no convergence within G + 2 rounds");
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
}

}  // namespace gv_internal

extern "C" {

// [EXTENSION] X6: handle configuration, the table is built here on the host and reaches the device with the next
// gv_inflate (gv_context::Inflation).  A rejected configuration leaves the one in force alone.

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
  if (f.dirty) {
    if ((rc = upload_slot(h, f.table, f.tab.cost.data(), f.tab.cost.size(), host::kTableBytes))) return rc;
    f.dirty = false;
  }
  InflateArgs a{};
  a.nx = h->g.nx; a.ny = h->g.ny;
  a.row_words = row_words;
  a.thr = f.thr;
  a.rc = f.tab.rc; a.d2max = f.tab.d2max;
  a.i8 = h->occ_i8;
  a.bits = f.bits;
  a.table = f.table.current();
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
  const int rc = set_config(fp, fp && host::footprint_valid(*fp), h->traj.fp, h->traj.set);
  if (fp && !rc)
    for (int32_t i = fp->n_vertices; i < host::kFootprintMaxVertices; ++i) h->traj.fp.vx[i] = h->traj.fp.vy[i] = 0.0;
  return rc;
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
  TrajArgs a = traj_args(h);
  a.K = K; a.P = P;
  return enqueue_sampler(h, a, launch_score_trajectories, poses, flags, scores, 16, t.d_scores, keep ? pose_cost : nullptr,
                         &TrajArgs::pose_cost, &t.d_pose_cost);
  GV_CATCH
}

int gv_score_trajectories(gv_handle h, const float *poses, int32_t K, int32_t P, uint32_t flags, gv_traj_score *scores,
                          uint8_t *pose_cost)
{
  return wait_scored(h, gv_score_trajectories_async(h, poses, K, P, flags, scores, pose_cost), K);
}

// ---- [EXTENSION] X9: the distance field and its sampler ----
// handle configuration only; gv_nav_field copies it into its kernel arguments
int gv_set_nav_config(gv_handle h, const gv_nav_config *cfg)
{
  if (!h) return GV_ERR_BAD_ARG;
  return set_config(cfg, cfg && host::nav_config_valid(*cfg) && host::nav_config_fits(*cfg, h->g.G), h->nav.cfg, h->nav.set);
}

// Everything goes on the public stream, behind what was enqueued before (a pending tick's grid pass and inflate
// included).  Seeds become field entries here on the host (the exact getIndex); whether a seed's cell is blocked only
// the device knows, so k_nav_seeds drops those and counts the rest.  Then the rounds (nav_field_relax).
int gv_nav_field(gv_handle h, const float *seeds_xy, int32_t S, gv_nav_info *info)
{
  if (!h) return GV_ERR_BAD_ARG;
  GV_TRY
  if (!seeds_xy || S < 1 || S > 65536) return GV_ERR_BAD_ARG;
  gv_context::NavField &f = h->nav;
  NavArgs a{};
  if (int rc = nav_field_begin(h, "gv_nav_field", (size_t)S, a)) return rc;
  int32_t *cells = reinterpret_cast<int32_t *>(f.stage.get() + kNavSeedOff);
  int32_t n = 0;
  for (int32_t i = 0; i < S; ++i) {
    const int32_t e = host::nav_seed_entry(h->g, seeds_xy[2 * i], seeds_xy[2 * i + 1]);
    if (e >= 0) cells[n++] = e;
  }
  a.seeds = f.d_seeds;
  a.n_seeds = n;
  if (n > 0) GV_HIP(hipMemcpyAsync(f.d_seeds, cells, (size_t)n * sizeof(int32_t), hipMemcpyHostToDevice, h->stream));
  launch_nav_init(a, h->stream);
  launch_nav_seeds(a, h->stream);
  GV_HIP(hipGetLastError());
  return nav_field_relax(h, "gv_nav_field", a, info);
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

int gv_score_nav_async(gv_handle h, const float *poses, int32_t K, int32_t P, uint32_t flags, gv_nav_score *scores)
{
  if (!h) return GV_ERR_BAD_ARG;
  GV_TRY
  if (!batch_ok(poses, scores, K, P, flags, GV_TRAJ_DEVICE_POSES)) return GV_ERR_BAD_ARG;
  int rc = refuse_state(h, "gv_score_nav", nullptr, kNeedField, "there is no whole field");
  if (rc || K == 0 || (rc = set_device_only(h))) return rc;
  NavScoreArgs a = nav_args(h);
  a.K = K; a.P = P;
  return enqueue_sampler(h, a, launch_score_nav, poses, flags, scores, 8, h->nav.d_scores);
  GV_CATCH
}

int gv_score_nav(gv_handle h, const float *poses, int32_t K, int32_t P, uint32_t flags, gv_nav_score *scores)
{
  return wait_scored(h, gv_score_nav_async(h, poses, K, P, flags, scores), K);
}

// ---- [EXTENSION] X13: the sampler against predicted moving objects; no grid and no costmap is read ----
int gv_score_dynamic_async(gv_handle h, const float *poses, int32_t K, int32_t P, uint32_t flags, gv_dyn_score *scores,
                           uint8_t *pose_cost)
{
  if (!h) return GV_ERR_BAD_ARG;
  GV_TRY
  const bool keep = (flags & GV_TRAJ_KEEP_POSE_COST) != 0;
  if (!batch_ok(poses, scores, K, P, flags, host::kTrajFlags) || (keep && !pose_cost)) return GV_ERR_BAD_ARG;
  gv_context::DynScore &d = h->dyn;
  if (!d.set) return state_error(h, "gv_score_dynamic", "no configuration set (gv_set_dyn_config)");
  int rc = GV_OK;
  DynArgs a{};
  a.K = K; a.P = P;
  if (K == 0 || (rc = set_device_only(h)) || (rc = dyn_kernel_args(h, a))) return rc;   // the table in front of the poses
  return enqueue_sampler(h, a, launch_score_dynamic, poses, flags, scores, 8, d.d_scores, keep ? pose_cost : nullptr,
                         &DynArgs::pose_cost, &d.d_pose_cost);
  GV_CATCH
}

int gv_score_dynamic(gv_handle h, const float *poses, int32_t K, int32_t P, uint32_t flags, gv_dyn_score *scores,
                     uint8_t *pose_cost)
{
  return wait_scored(h, gv_score_dynamic_async(h, poses, K, P, flags, scores, pose_cost), K);
}

}  // extern "C"
