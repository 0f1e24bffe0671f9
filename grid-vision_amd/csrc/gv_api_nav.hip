// gv_api_nav.hip -- [EXTENSION] X9: the goal / path distance field over the resident costmap (gv_set_nav_config,
// gv_nav_field and its getters) and its sampler along trajectories (gv_score_nav*).  The kernels and the argument why
// the rounds end at the exact field are in gv_navfield.hip.
#include <algorithm>
#include <cstring>

#include "gv_context.hpp"

extern "C" {

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
  if (!f.set) { h->err = "gv_nav_field: no configuration set (gv_set_nav_config)"; return GV_ERR_STATE; }
  if (!h->infl.have_cost) { h->err = "gv_nav_field: no costmap (gv_inflate)"; return GV_ERR_STATE; }
  if (h->world > 1) { h->err = "gv_nav_field: ranks own row bands of the grid, there is no whole costmap"; return GV_ERR_STATE; }
  int rc = set_device_only(h);
  if (rc) return rc;
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

// gv_score_trajectories_async with another kernel and another record: a copy of host poses, one kernel, a copy of the
// records the kernel cannot write in place, all on the public stream.
int gv_score_nav_async(gv_handle h, const float *poses, int32_t K, int32_t P, uint32_t flags, gv_nav_score *scores)
{
  if (!h) return GV_ERR_BAD_ARG;
  GV_TRY
  if (!poses || !scores || P < 1 || P > 4096 || K < 0 || K > (1 << 20) || (flags & ~(uint32_t)GV_TRAJ_DEVICE_POSES) != 0)
    return GV_ERR_BAD_ARG;
  gv_context::NavField &f = h->nav;
  if (!f.have_field) { h->err = "gv_score_nav: no distance field (gv_nav_field)"; return GV_ERR_STATE; }
  if (h->world > 1) { h->err = "gv_score_nav: ranks own row bands of the grid, there is no whole field"; return GV_ERR_STATE; }
  if (K == 0) return GV_OK;
  int rc = set_device_only(h);
  if (rc) return rc;
  const size_t n_poses = (size_t)K * (size_t)P;
  NavScoreArgs a{};
  a.g = h->g;
  a.K = K; a.P = P;
  a.field = f.field;
  if (flags & GV_TRAJ_DEVICE_POSES) {
    a.poses = poses;
  } else {
    if ((rc = f.d_poses.reserve(h, n_poses * 3))) return rc;
    GV_HIP(hipMemcpyAsync(f.d_poses, poses, n_poses * 3 * sizeof(float), hipMemcpyHostToDevice, h->stream));
    a.poses = f.d_poses;
  }
  a.scores = static_cast<gv_nav_score *>(pinned_device_view(scores, 8));
  const bool copy_scores = a.scores == nullptr;
  if (copy_scores) {
    if ((rc = f.d_scores.reserve(h, (size_t)K))) return rc;
    a.scores = f.d_scores;
  }
  launch_score_nav(a, h->stream);
  GV_HIP(hipGetLastError());
  if (copy_scores) GV_HIP(hipMemcpyAsync(scores, a.scores, (size_t)K * sizeof(gv_nav_score), hipMemcpyDeviceToHost, h->stream));
  return GV_OK;
  GV_CATCH
}

int gv_score_nav(gv_handle h, const float *poses, int32_t K, int32_t P, uint32_t flags, gv_nav_score *scores)
{
  const int rc = gv_score_nav_async(h, poses, K, P, flags, scores);
  if (rc || K == 0) return rc;
  GV_HIP(hipStreamSynchronize(h->stream));
  return GV_OK;
}

}  // extern "C"
