// gv_api_match_host.hip -- the host-only entry points of the two scan matchers (include/gridvision_hip_match.h,
// include/gridvision_hip_search.h): the twins gv_match_scan_host and gv_match_search_host (gv_match.hpp's and
// gv_search.hpp's text in sequential loops: what the GPU tests hold the device calls to), the rotation table and the
// motion of a result.  None takes a handle or enqueues anything; plain C++17 without a HIP header, so a host compiler
// alone builds it too.  What the twins check and derive as the device calls do is gv_match_rules.hpp's.
#include <algorithm>
#include <cstring>
#include <vector>

#include "gv_match_rules.hpp"

using namespace gv;
using namespace gv_internal;

// what both twins refuse alike, beside their own configuration and call rules
static bool host_inputs_ok(const uint8_t *cost, const float *x, const float *y, const float *z, size_t n, const gv_transform *base_from_lidar,
                           const gv_height_band *band)
{
  return cost && (!n || (x && y && z)) && base_from_lidar && match_band_valid(band);
}

extern "C" {

// The definition in sequential loops: the used points in index order; for every yaw candidate their cells, and every
// point adds its window into the volume, row by row (a window that lies on the map whole needs no test per cell);
// then the selection over the volume in linear order.
int gv_match_scan_host(uint8_t grid_x, uint8_t grid_y, double resolution, const uint8_t *cost, const float *x, const float *y,
                       const float *z, size_t n, const gv_transform *base_from_lidar, const gv_height_band *band,
                       const gv_match_config *cfg, const gv_match_guess *guess, uint32_t flags, gv_match_result *result,
                       uint32_t *scores)
{
  if (!host_inputs_ok(cost, x, y, z, n, base_from_lidar, band) || !cfg || !match_config_valid(*cfg) ||
      !match_call_ok(guess, flags, result, scores))
    return GV_ERR_BAD_ARG;
  try {
    const MatchParams p = match_params(*cfg, *guess);
    GridParams g{};
    std::vector<float> bxs, bys;
    if (!scan_prelude(grid_x, grid_y, resolution, x, y, z, n, *base_from_lidar, band, p, g, bxs, bys)) return GV_ERR_BAD_ARG;
    const int32_t NT = match_nt(p), NY = match_ny(p), NX = match_nx(p);
    float rot[2 * kMatchMaxSide];
    match_rotations(p, rot);
    std::vector<uint32_t> vol((size_t)NT * (size_t)NY * (size_t)NX, 0u);
    for (int32_t t = 0; t < NT; ++t) {
      uint32_t *v = vol.data() + (size_t)t * (size_t)NY * (size_t)NX;
      for (size_t q = 0; q < bxs.size(); ++q) {
        int32_t ux = 0, uy = 0;
        if (!match_cell(g, p, rot[2 * t], rot[2 * t + 1], bxs[q], bys[q], ux, uy)) continue;
        const bool inside = ux - p.wx >= 0 && uy - p.wy >= 0 && ux + p.wx < g.nx && uy + p.wy < g.ny;
        for (int32_t j = -p.wy; j <= p.wy; ++j) {
          uint32_t *row = v + (size_t)(j + p.wy) * (size_t)NX + (size_t)p.wx;
          if (inside) {
            const uint8_t *c = cost + data_entry(g, ux, uy + j);   // cell (ux + i, uy + j) is entry c[-i]
            for (int32_t i = -p.wx; i <= p.wx; ++i) row[i] += (uint32_t)c[-i];
          } else {
            for (int32_t i = -p.wx; i <= p.wx; ++i) row[i] += match_cost(g, cost, ux + i, uy + j);
          }
        }
      }
    }
    uint64_t best = 0;
    for (uint32_t lin = 0; lin < (uint32_t)vol.size(); ++lin) {
      const int32_t t = (int32_t)(lin / (uint32_t)(NY * NX)), r = (int32_t)(lin % (uint32_t)(NY * NX));
      const uint64_t key = match_key(vol[lin], t - p.wt, r / NX - p.wy, r % NX - p.wx, lin);
      if (key > best) best = key;
    }
    const size_t centre = ((size_t)p.wt * (size_t)NY + (size_t)p.wy) * (size_t)NX + (size_t)p.wx;
    *result = match_record(g, p, match_key_lin(best), match_key_score(best), vol[centre], (uint32_t)bxs.size());
    if (flags & GV_MATCH_KEEP_SCORES) std::memcpy(scores, vol.data(), vol.size() * sizeof(uint32_t));
    return GV_OK;
  } catch (...) {
    return GV_ERR_HIP;
  }
}

// The definition in sequential loops: the used points in index order and their cells under every yaw candidate; M by
// its two passes; every bound; the seed; its exact scores and L; the survivors' exact scores and the centre's; the
// selection.
int gv_match_search_host(uint8_t grid_x, uint8_t grid_y, double resolution, const uint8_t *cost, const float *x, const float *y,
                         const float *z, size_t n, const gv_transform *base_from_lidar, const gv_height_band *band,
                         const gv_search_config *cfg, const gv_match_guess *guess, uint32_t flags, gv_match_result *result,
                         gv_search_stats *stats)
{
  if (!host_inputs_ok(cost, x, y, z, n, base_from_lidar, band) || !cfg || !search_config_valid(*cfg) || !search_call_ok(guess, flags, result))
    return GV_ERR_BAD_ARG;
  try {
    const SearchParams sp = search_params(*cfg, *guess);
    const MatchParams &p = sp.p;
    GridParams g{};
    std::vector<float> bxs, bys;
    if (!scan_prelude(grid_x, grid_y, resolution, x, y, z, n, *base_from_lidar, band, p, g, bxs, bys)) return GV_ERR_BAD_ARG;
    const int32_t NT = match_nt(p), S = search_s(sp), S2 = S * S, nbx = search_nbx(sp), nby = search_nby(sp);
    const uint32_t n_blocks = search_blocks(sp);
    float rot[2 * kMatchMaxSide];
    match_rotations(p, rot);

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

int gv_match_rotations(const gv_match_config *cfg, const gv_match_guess *guess, float *table)
{
  if (!cfg || !match_config_valid(*cfg) || !match_guess_valid(guess) || !table) return GV_ERR_BAD_ARG;
  match_rotations(match_params(*cfg, *guess), table);
  return GV_OK;
}

int gv_match_motion(const gv_match_result *result, gv_transform *out)
{
  if (!result || !out || !std::isfinite(result->x) || !std::isfinite(result->y) || !std::isfinite(result->yaw)) return GV_ERR_BAD_ARG;
  const double half = result->yaw / 2.0;
  *out = gv_transform{0.0, 0.0, std::sin(half), std::cos(half), result->x, result->y, 0.0};
  return GV_OK;
}

}  // extern "C"
