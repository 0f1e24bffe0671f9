// gv_match_rules.hpp -- what the two scan matchers' device calls (gv_api_match.hip: X16 gv_match_scan*, X18
// gv_match_search*) and their host-only twins (gv_api_match_host.hip) check and derive alike: the one text of the
// configuration and argument rules, of MatchParams, the rotation table and the selected-points count, and the twins'
// shared prelude.  Plain C++: no HIP header, no handle.
#pragma once

#include <cmath>
#include <vector>

#include "gv_host_math.hpp"
#include "gv_search.hpp"   // and gv_match.hpp

namespace gv_internal __attribute__((visibility("hidden"))) {
using namespace gv;

static_assert((uint32_t)GV_MATCH_USE_BAND == (uint32_t)GV_SEARCH_USE_BAND, "one flag bit for both configurations");

// what gv_match_config and gv_search_config hold alike (same field names): the window with wx, wy up to `most`, the yaw
// step, the stride, min_points and the flag word
template <typename Cfg>
bool scan_config_valid(const Cfg &c, int32_t most)
{
  const auto half_ok = [](int32_t w, int32_t m) { return w >= 0 && w <= m; };
  return half_ok(c.wx, most) && half_ok(c.wy, most) && half_ok(c.wt, kMatchMaxHalf) && std::isfinite(c.yaw_step) &&
         c.yaw_step >= 0.0 && (c.wt == 0 || c.yaw_step > 0.0) && c.stride >= 1 && c.stride <= kMatchMaxStride && c.min_points >= 1 &&
         (c.flags & ~(uint32_t)GV_MATCH_USE_BAND) == 0;
}
inline bool match_config_valid(const gv_match_config &c) { return scan_config_valid(c, kMatchMaxHalf); }
inline bool search_config_valid(const gv_search_config &c)
{
  return scan_config_valid(c, kSearchMaxHalf) && c.block_log2 >= 1 && c.block_log2 <= kSearchMaxBlockLog2 && c.reserved == 0;
}

inline bool match_guess_valid(const gv_match_guess *q) { return q && std::isfinite(q->x) && std::isfinite(q->y) && std::isfinite(q->yaw); }

// what every form of a call refuses alike
inline bool match_call_ok(const gv_match_guess *guess, uint32_t flags, const gv_match_result *result, const uint32_t *scores)
{
  return match_guess_valid(guess) && result && (flags & ~(uint32_t)GV_MATCH_KEEP_SCORES) == 0 &&
         (!(flags & GV_MATCH_KEEP_SCORES) || scores);
}
inline bool search_call_ok(const gv_match_guess *guess, uint32_t flags, const gv_match_result *result)
{
  return match_guess_valid(guess) && result && flags == 0u;
}

// a band gv_set_height_band would take, or none
inline bool match_band_valid(const gv_height_band *band)
{
  return !band || !(std::isnan(band->z_ground) || std::isnan(band->z_max) || band->z_ground > band->z_max);
}

// either configuration (valid) and the guess as a call carries them
template <typename Cfg>
MatchParams match_params(const Cfg &c, const gv_match_guess &q)
{
  MatchParams p{};
  p.wx = c.wx; p.wy = c.wy; p.wt = c.wt;
  p.stride = c.stride;
  p.min_points = c.min_points;
  p.use_band = (c.flags & GV_MATCH_USE_BAND) ? 1u : 0u;
  p.x = q.x; p.y = q.y; p.yaw = q.yaw;
  p.yaw_step = c.yaw_step;
  return p;
}
inline SearchParams search_params(const gv_search_config &c, const gv_match_guess &q) { return SearchParams{match_params(c, q), c.block_log2, 0}; }

// (c_t, s_t): libm in fp64, rounded once
inline void match_rotations(const MatchParams &p, float *table)
{
  for (int32_t t = 0; t < match_nt(p); ++t) {
    const double th = match_theta(p, t);
    table[2 * t] = (float)std::cos(th);
    table[2 * t + 1] = (float)std::sin(th);
  }
}

// the selected points: every stride-th of n
inline size_t match_selected(size_t n, int32_t stride) { return (n + (size_t)stride - 1) / (size_t)stride; }

// The twins' common start, given a valid configuration's `p`, a band that passed the test above and arrays of n points:
// the geometry gv_create gives and the used points' (bx, by) in index order.  False: a geometry gv_create rejects, or
// more than 2^24 selected points.
inline bool scan_prelude(uint8_t grid_x, uint8_t grid_y, double resolution, const float *x, const float *y, const float *z, size_t n,
                         const gv_transform &base_from_lidar, const gv_height_band *band, const MatchParams &p, GridParams &g,
                         std::vector<float> &bxs, std::vector<float> &bys)
{
  if (!host::grid_params(grid_x, grid_y, resolution, g)) return false;
  if (match_selected(n, p.stride) > (size_t)kMatchMaxSelected) return false;
  const Mat34f mb = host::pcl_matrix_from_tf(base_from_lidar);
  const HeightBand hb = band ? HeightBand{band->z_ground, band->z_max, 0} : HeightBand{-INFINITY, INFINITY, 0};
  for (size_t i = 0; i < n; i += (size_t)p.stride) {
    float bx, by, bz;
    match_base_point(mb, x[i], y[i], z[i], bx, by, bz);
    if (match_used(bx, by, bz, p.use_band, hb)) {
      bxs.push_back(bx);
      bys.push_back(by);
    }
  }
  return true;
}

}  // namespace gv_internal
