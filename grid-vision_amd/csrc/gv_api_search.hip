// gv_api_search.hip -- [EXTENSION] X18 wide-window scan matching by branch and bound behind the C ABI of
// include/gridvision_hip_search.h: the handle's configuration, the device call (gv_match_search_async /
// gv_match_search: X16's point pass and the kernels of gv_search.hip on the public stream) and the host twin
// gv_match_search_host (gv_match.hpp's and gv_search.hpp's text in sequential loops: what the GPU tests hold the
// device call to).  Under a host compiler alone (no __HIPCC__) only the twin is built: it needs no HIP header.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

#ifdef __HIPCC__
#include "gv_context.hpp"
#else
#include "gv_host_math.hpp"
#include "gv_search.hpp"
using namespace gv;
#endif

namespace {

bool search_config_valid(const gv_search_config &c)
{
  const auto half_ok = [](int32_t w, int32_t most) { return w >= 0 && w <= most; };
  return half_ok(c.wx, kSearchMaxHalf) && half_ok(c.wy, kSearchMaxHalf) && half_ok(c.wt, kMatchMaxHalf) &&
         std::isfinite(c.yaw_step) && c.yaw_step >= 0.0 && (c.wt == 0 || c.yaw_step > 0.0) && c.stride >= 1 &&
         c.stride <= kMatchMaxStride && c.min_points >= 1 && (c.flags & ~(uint32_t)GV_SEARCH_USE_BAND) == 0 && c.block_log2 >= 1 &&
         c.block_log2 <= kSearchMaxBlockLog2 && c.reserved == 0;
}

// what every form of the call refuses alike
bool search_call_ok(const gv_match_guess *q, uint32_t flags, const gv_match_result *result)
{
  return q && std::isfinite(q->x) && std::isfinite(q->y) && std::isfinite(q->yaw) && result && flags == 0u;
}

SearchParams search_params(const gv_search_config &c, const gv_match_guess &q)
{
  SearchParams sp{};
  sp.p.wx = c.wx; sp.p.wy = c.wy; sp.p.wt = c.wt;
  sp.p.stride = c.stride;
  sp.p.min_points = c.min_points;
  sp.p.use_band = (c.flags & GV_SEARCH_USE_BAND) ? 1u : 0u;
  sp.p.x = q.x; sp.p.y = q.y; sp.p.yaw = q.yaw;
  sp.p.yaw_step = c.yaw_step;
  sp.block_log2 = c.block_log2;
  return sp;
}

// (c_t, s_t): libm in fp64, rounded once (gv_match_rotations' table)
void search_rotations(const MatchParams &p, float *table)
{
  for (int32_t t = 0; t < match_nt(p); ++t) {
    const double th = match_theta(p, t);
    table[2 * t] = (float)std::cos(th);
    table[2 * t + 1] = (float)std::sin(th);
  }
}

size_t search_selected(size_t n, int32_t stride) { return (n + (size_t)stride - 1) / (size_t)stride; }

}  // namespace

extern "C" {

#ifdef __HIPCC__
// handle configuration only; every call copies it into its kernel arguments
int gv_set_search_config(gv_handle h, const gv_search_config *cfg)
{
  if (!h) return GV_ERR_BAD_ARG;
  if (cfg && !search_config_valid(*cfg)) return GV_ERR_BAD_ARG;
  if (cfg) h->search.cfg = *cfg;
  h->search.set = cfg != nullptr;
  return GV_OK;
}

// One memset, ten kernels and a copy per destination the device cannot write in place, all on the public stream:
// behind the last gv_inflate, and behind the upload of the cloud it reads, as gv_match_scan_async.
int gv_match_search_async(gv_handle h, const gv_match_guess *guess, uint32_t flags, gv_match_result *result, gv_search_stats *stats)
{
  if (!h) return GV_ERR_BAD_ARG;
  GV_TRY
  if (!search_call_ok(guess, flags, result)) return GV_ERR_BAD_ARG;
  if (!h->has_bl) return GV_ERR_TF;
  gv_context::Search &m = h->search;
  const char *missing = !m.set ? "no configuration set (gv_set_search_config)" : (h->n == 0 ? "no cloud" : nullptr);
  int rc = refuse_state(h, "gv_match_search", missing, kNeedCostmap, "there is no whole costmap");
  if (rc) return rc;
  const size_t n_sel = search_selected(h->n, m.cfg.stride);
  if (n_sel > (size_t)kMatchMaxSelected) return state_error(h, "gv_match_search", "more than 2^24 selected points");
  if ((rc = set_device_only(h))) return rc;

  SearchArgs a{};
  a.g = h->g;
  a.sp = search_params(m.cfg, *guess);
  a.n_sel = (uint32_t)n_sel;
  a.n_blocks = search_blocks(a.sp);
  search_rotations(a.sp.p, a.rot);
  const int32_t S = search_s(a.sp);
  const size_t words = (size_t)kSearchBounds + (size_t)a.n_blocks;
  const size_t pw = (size_t)search_pool_w(a.g, S), ph = (size_t)search_pool_h(a.g, S);
  ResultDest<gv_match_result> to_result;
  ResultDest<gv_search_stats> to_stats;
  if ((rc = m.pts.reserve(h, n_sel)) || (rc = m.head.reserve(h, words)) || (rc = m.rows.reserve(h, pw * (size_t)a.g.ny)) ||
      (rc = m.pool.reserve(h, pw * ph)) || (rc = m.list.reserve(h, (size_t)a.n_blocks)) ||
      (rc = m.slots.reserve(h, (size_t)a.n_blocks * (size_t)S * (size_t)S)) || (rc = to_result.open(h, result, 1, 8, m.d_result)))
    return rc;
  if (stats) {
    if ((rc = to_stats.open(h, stats, 1, 8, m.d_stats))) return rc;
  } else {
    if ((rc = m.d_stats.reserve(h, 1))) return rc;
    to_stats.dev = m.d_stats;
  }
  gv_context::Match &mm = h->match;   // the cloud's readers: one event and one mask for both matchers
  if (!mm.read) GV_HIP(mm.read.create(hipEventDisableTiming));
  a.pts = m.pts;
  a.head = m.head;
  a.cost = h->infl.cost;
  a.rows = m.rows;
  a.pool = m.pool;
  a.list = m.list;
  a.slots = m.slots;
  a.result = to_result.dev;
  a.stats = to_stats.dev;

  MatchArgs pa{};   // X16's point pass over this call's block
  pa.g = a.g;
  pa.p = a.sp.p;
  pa.m_base = h->m_base;
  pa.band = h->band;
  pa.x = h->cx; pa.y = h->cy; pa.z = h->cz;
  pa.n = (uint32_t)h->n;
  pa.n_sel = a.n_sel;
  pa.pts = m.pts;
  pa.head = m.head;

  CloudSet &C = h->cloud[h->cloud_cur];
  if (!(C.seen & 1u)) {   // the public stream reads this cloud for the first time: behind its upload
    GV_HIP(hipStreamWaitEvent(h->stream, C.ready, 0));
    C.seen |= 1u;
    h->sb[0].lane_clean = false;
  }
  GV_HIP(hipMemsetAsync(m.head, 0, words * sizeof(uint32_t), h->stream));
  launch_match_points(pa, h->stream);
  GV_HIP(hipEventRecord(mm.read, h->stream));   // the cloud's last reader of this call: an upload into the set waits for it
  mm.clouds |= 1u << h->cloud_cur;
  launch_search_pool(a, h->stream);
  launch_search_bound(a, h->stream);
  launch_search_seed(a, h->stream);
  launch_search_fine(a, true, h->stream);
  launch_search_prune(a, h->stream);
  launch_search_fine(a, false, h->stream);
  launch_search_select(a, h->stream);
  GV_HIP(hipGetLastError());
  if ((rc = to_result.copy_back(h)) || (rc = to_stats.copy_back(h))) return rc;
  return GV_OK;
  GV_CATCH
}

int gv_match_search(gv_handle h, const gv_match_guess *guess, uint32_t flags, gv_match_result *result, gv_search_stats *stats)
{
  return wait_scored(h, gv_match_search_async(h, guess, flags, result, stats), 1);
}

#endif  // __HIPCC__

// ---- host only: no handle, nothing enqueued

// The definition in sequential loops: the used points in index order and their cells under every yaw candidate; M by
// its two passes; every bound; the seed; its exact scores and L; the survivors' exact scores and the centre's; the
// selection.
int gv_match_search_host(uint8_t grid_x, uint8_t grid_y, double resolution, const uint8_t *cost, const float *x, const float *y,
                         const float *z, size_t n, const gv_transform *base_from_lidar, const gv_height_band *band,
                         const gv_search_config *cfg, const gv_match_guess *guess, uint32_t flags, gv_match_result *result,
                         gv_search_stats *stats)
{
  if (!cost || (n && (!x || !y || !z)) || !base_from_lidar || !cfg || !search_config_valid(*cfg) || !search_call_ok(guess, flags, result))
    return GV_ERR_BAD_ARG;
  if (band && (std::isnan(band->z_ground) || std::isnan(band->z_max) || band->z_ground > band->z_max)) return GV_ERR_BAD_ARG;
  try {
    GridParams g{};
    if (!host::grid_params(grid_x, grid_y, resolution, g)) return GV_ERR_BAD_ARG;
    if (search_selected(n, cfg->stride) > (size_t)kMatchMaxSelected) return GV_ERR_BAD_ARG;
    const SearchParams sp = search_params(*cfg, *guess);
    const MatchParams &p = sp.p;
    const Mat34f mb = host::pcl_matrix_from_tf(*base_from_lidar);
    const HeightBand hb = band ? HeightBand{band->z_ground, band->z_max, 0} : HeightBand{-INFINITY, INFINITY, 0};
    std::vector<float> bxs, bys;
    for (size_t i = 0; i < n; i += (size_t)p.stride) {
      float bx, by, bz;
      match_base_point(mb, x[i], y[i], z[i], bx, by, bz);
      if (match_used(bx, by, bz, p.use_band, hb)) {
        bxs.push_back(bx);
        bys.push_back(by);
      }
    }
    const int32_t NT = match_nt(p), S = search_s(sp), S2 = S * S, nbx = search_nbx(sp), nby = search_nby(sp);
    const uint32_t n_blocks = search_blocks(sp);
    float rot[2 * kMatchMaxSide];
    search_rotations(p, rot);

    // the cells of every (t, point); uy == INT32_MIN: the point contributes to no candidate
    const size_t np = bxs.size();
    std::vector<int32_t> cx((size_t)NT * np), cy((size_t)NT * np);
    for (int32_t t = 0; t < NT; ++t)
      for (size_t q = 0; q < np; ++q) {
        int32_t ux = 0, uy = 0;
        const bool ok = match_cell(g, p, rot[2 * t], rot[2 * t + 1], bxs[q], bys[q], ux, uy);
        cx[(size_t)t * np + q] = ux;
        cy[(size_t)t * np + q] = ok ? uy : INT32_MIN;
      }

    // M: along x, then along y
    const int32_t pw = search_pool_w(g, S), ph = search_pool_h(g, S);
    std::vector<uint8_t> rows((size_t)pw * (size_t)g.ny), pool((size_t)pw * (size_t)ph);
    for (int32_t iy = 0; iy < g.ny; ++iy)
      for (int32_t ix = -(S - 1); ix < g.nx; ++ix) {
        uint32_t m = 0u;
        for (int32_t dx = 0; dx < S; ++dx) m = std::max(m, match_cost(g, cost, ix + dx, iy));
        rows[(size_t)iy * (size_t)pw + (size_t)(ix + S - 1)] = (uint8_t)m;
      }
    for (int32_t iy = -(S - 1); iy < g.ny; ++iy)
      for (int32_t c = 0; c < pw; ++c) {
        uint32_t m = 0u;
        for (int32_t dy = 0; dy < S; ++dy)
          if (iy + dy >= 0 && iy + dy < g.ny) m = std::max(m, (uint32_t)rows[(size_t)(iy + dy) * (size_t)pw + (size_t)c]);
        pool[(size_t)(iy + S - 1) * (size_t)pw + (size_t)c] = (uint8_t)m;
      }

    // the bounds, the seed, bound_sum
    std::vector<uint32_t> B(n_blocks, 0u);
    for (int32_t t = 0; t < NT; ++t) {
      uint32_t *Bt = B.data() + (size_t)t * (size_t)(nby * nbx);
      for (size_t q = 0; q < np; ++q) {
        const int32_t ux = cx[(size_t)t * np + q], uy = cy[(size_t)t * np + q];
        if (uy == INT32_MIN) continue;
        for (int32_t J = 0; J < nby; ++J) {
          const int32_t iy = uy + search_jb(sp, J);
          if (iy <= -S || iy >= g.ny) continue;
          for (int32_t I = 0; I < nbx; ++I) Bt[J * nbx + I] += search_pooled(g, S, pool.data(), ux + search_ib(sp, I), iy);
        }
      }
    }
    uint64_t seed = 0, bound_sum = 0;
    for (uint32_t b = 0; b < n_blocks; ++b) {
      seed = std::max(seed, search_seed_key(sp, B[b], b));
      bound_sum += B[b];
    }

    // the exact scores of one block, S * S words (those outside the window stay 0)
    const auto score_block = [&](uint32_t blk, uint32_t *out) {
      int32_t t, J, I;
      search_block_of(sp, blk, t, J, I);
      std::fill(out, out + S2, 0u);
      const int32_t jb = search_jb(sp, J), ib = search_ib(sp, I), nr = search_rows(sp, J), nc = search_cols(sp, I);
      for (size_t q = 0; q < np; ++q) {
        const int32_t ux = cx[(size_t)t * np + q], uy = cy[(size_t)t * np + q];
        if (uy == INT32_MIN) continue;
        for (int32_t jj = 0; jj < nr; ++jj)
          for (int32_t ii = 0; ii < nc; ++ii) out[jj * S + ii] += match_cost(g, cost, ux + ib + ii, uy + jb + jj);
      }
    };
    uint32_t slot[kSearchMaxS2];
    score_block(search_key_block(seed), slot);
    uint32_t lower = 0u;
    for (int32_t c = 0; c < S2; ++c) lower = std::max(lower, slot[c]);

    score_block(search_centre_block(sp), slot);
    const uint32_t guess_score = slot[(p.wy & (S - 1)) * S + (p.wx & (S - 1))];
    uint64_t best = match_key(guess_score, 0, 0, 0, search_centre_lin(sp));
    uint32_t n_survivors = 0, n_scored = 0;
    for (uint32_t b = 0; b < n_blocks; ++b) {
      if (!search_survives(B[b], lower)) continue;
      int32_t t, J, I;
      search_block_of(sp, b, t, J, I);
      const int32_t nr = search_rows(sp, J), nc = search_cols(sp, I);
      ++n_survivors;
      n_scored += (uint32_t)(nr * nc);
      score_block(b, slot);
      for (int32_t jj = 0; jj < nr; ++jj)
        for (int32_t ii = 0; ii < nc; ++ii)
          best = std::max(best, match_key(slot[jj * S + ii], t - p.wt, search_jb(sp, J) + jj, search_ib(sp, I) + ii,
                                          search_lin(sp, t, J, I, jj, ii)));
    }
    *result = match_record(g, p, match_key_lin(best), match_key_score(best), guess_score, (uint32_t)np);
    if (stats)
      *stats = gv_search_stats{n_blocks, n_survivors, n_scored, search_key_block(seed), lower, search_key_bound(seed), bound_sum};
    return GV_OK;
  } catch (...) {
    return GV_ERR_HIP;
  }
}

}  // extern "C"
