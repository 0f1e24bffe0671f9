// gv_gain.hpp -- [EXTENSION] X20 information gain of exploration goals (gvx2_*): the arithmetic of the definition in
// include/gridvision_hip_gain.h, one text for the kernels (gv_gain.hip) and for the host twin (gvx2_gain_host,
// gv_api_gain_host.hip), as gv_frontier.hpp is for the clusters.  Plain C++ under GV_HD: the rules of the configuration
// and of a call, the ring, the walk of one ray over whatever answers "is this cell opaque" and takes "this cell is seen",
// the window bitmaps' geometry, a record from its counts, and the key of `best`.
#pragma once

#include "../../include/gridvision_hip_gain.h"
#include "gv_frontier.hpp"   // frontier_class, FrontierRule: the classes are X19's test over this configuration's bounds
#include "gv_line.hpp"       // line_cell: cell i of a ray in closed form
#include "gv_types.hpp"

namespace gv {

constexpr int32_t kGainMaxN = GVX2_GAIN_MAX_N;
constexpr int32_t kGainMaxRadius = GVX2_GAIN_MAX_RADIUS;
constexpr uint32_t kGainNoOpaque = GVX2_GAIN_NO_OPAQUE;
constexpr uint32_t kGainListFlags = GVX2_GAIN_USE_FIELD | GVX2_GAIN_DEVICE_ENTRIES;

GV_HD bool gain_config_valid(const gvx2_gain_config &c)
{
  return c.free_max >= 0 && c.free_max <= 100 && c.unknown_min >= 0 && c.unknown_min <= 100 && c.unknown_max >= 0 &&
         c.unknown_max <= 100 && c.free_max < c.unknown_min && c.unknown_min <= c.unknown_max && c.radius >= 1 &&
         c.radius <= kGainMaxRadius && c.min_gain >= 0 && c.min_gain <= (1 << 20) && c.w_gain >= 0 && c.w_gain <= 65535 &&
         c.w_dist >= 0 && c.w_dist <= 65535 && c.reserved == 0u;
}

GV_HD bool gain_call_ok(int32_t n, uint32_t flags, uint32_t allowed) { return n >= 1 && n <= kGainMaxN && (flags & ~allowed) == 0u; }

// what the kernels and the twin read of a configuration
struct GainRule {
  FrontierRule cls;    // the class bounds (max_cost and min_cells are not read)
  int32_t radius, min_gain, w_gain, w_dist;
};
GV_HD GainRule gain_rule(const gvx2_gain_config &c)
{
  return GainRule{FrontierRule{c.free_max, c.unknown_min, c.unknown_max, 256, 1}, c.radius, c.min_gain, c.w_gain, c.w_dist};
}

// the offset of ray r (0 .. 8R-1) of the square ring at Chebyshev distance R
GV_HD void gain_ray_offset(int32_t R, int32_t r, int32_t &ox, int32_t &oy)
{
  const int32_t side = r / (2 * R), j = r - side * 2 * R;
  ox = side == 0 ? -R + j : side == 1 ? R : side == 2 ? R - j : -R;
  oy = side == 0 ? -R : side == 1 ? -R + j : side == 2 ? R : R - j;
}

enum : int32_t { kGainRayOpaque = 0, kGainRayOffMap = 1, kGainRayRange = 2 };   // how a ray ended: the index of its counter

// The walk of ray r from (cx, cy): cells 1 .. R of the line to the ring cell, in order; returns how the ray ended and, when
// on an opaque cell, that cell's d2.  seen(x, y) is told every cell the ray sees, opaque(x, y) is asked about each of them;
// both get cells on the map within the radius only, so |x - cx| and |y - cy| are at most R.
template <class Opaque, class Seen>
GV_HD int32_t gain_walk(int32_t nx, int32_t ny, int32_t cx, int32_t cy, int32_t R, int32_t r, Opaque &&opaque, Seen &&seen, uint32_t &opaque_d2)
{
  int32_t ox, oy;
  gain_ray_offset(R, r, ox, oy);
  const int32_t ex = cx + ox, ey = cy + oy;
  for (int32_t i = 1; i <= R; ++i) {
    int32_t x, y;
    line_cell(cx, cy, ex, ey, (uint32_t)i, x, y);
    if (x < 0 || x >= nx || y < 0 || y >= ny) return kGainRayOffMap;
    const int32_t dx = x - cx, dy = y - cy;
    const uint32_t d2 = (uint32_t)(dx * dx + dy * dy);
    if (d2 > (uint32_t)(R * R)) return kGainRayRange;
    seen(x, y);
    if (opaque(x, y)) {
      opaque_d2 = d2;
      return kGainRayOpaque;
    }
  }
  return kGainRayRange;
}

// The window of a candidate as bitmaps: (2R + 1) rows of gain_row_words(R) 32-bit words, bit wx % 32 of word wx / 32 of row
// wy for the cell (cx - R + wx, cy - R + wy).  Three of them (UNKNOWN, OPAQUE, SEEN) are a workgroup's LDS.
GV_HD int32_t gain_row_words(int32_t R) { return (2 * R + 1 + 31) / 32; }
GV_HD int32_t gain_bitmap_words(int32_t R) { return (2 * R + 1) * gain_row_words(R); }
GV_HD size_t gain_lds_bytes(int32_t R) { return 3u * (size_t)gain_bitmap_words(R) * sizeof(uint32_t); }

// what the rays of one candidate found
struct GainCounts {
  int32_t n_unknown, n_free, n_opaque;
  int32_t rays[3];               // by kGainRay*
  uint32_t nearest_opaque_d2;
};

GV_HD gvx2_gain_record gain_record_zero()
{
  gvx2_gain_record r;
  r.entry = 0;
  r.status = 0u;
  r.n_unknown = r.n_free = r.n_opaque = 0;
  r.rays_opaque = r.rays_off_map = r.rays_range = 0;
  r.nearest_opaque_d2 = 0u;
  r.dist = 0u;
  r.score = 0;
  return r;
}

GV_HD bool gain_entry_valid(int32_t entry, int32_t G) { return entry >= 0 && entry < G; }

GV_HD gvx2_gain_record gain_record_invalid(int32_t entry)
{
  gvx2_gain_record r = gain_record_zero();
  r.entry = entry;
  r.status = GVX2_GAIN_INVALID;
  return r;
}

// the record of a valid candidate; field_value is read only with use_field
GV_HD gvx2_gain_record gain_record(const GainRule &g, int32_t entry, const GainCounts &c, bool use_field, uint32_t field_value)
{
  gvx2_gain_record r;
  r.entry = entry;
  const bool lost = use_field && field_value >= (uint32_t)GV_NAV_UNREACHABLE;
  r.status = (lost ? GVX2_GAIN_UNREACHABLE : 0u) | (c.n_unknown < g.min_gain ? GVX2_GAIN_BELOW_MIN : 0u);
  r.n_unknown = c.n_unknown;
  r.n_free = c.n_free;
  r.n_opaque = c.n_opaque;
  r.rays_opaque = c.rays[kGainRayOpaque];
  r.rays_off_map = c.rays[kGainRayOffMap];
  r.rays_range = c.rays[kGainRayRange];
  r.nearest_opaque_d2 = c.nearest_opaque_d2;
  r.dist = use_field ? field_value : 0u;
  r.score = lost ? 0 : (int64_t)g.w_gain * (int64_t)c.n_unknown - (int64_t)g.w_dist * (int64_t)r.dist;
  return r;
}

// The key of `best` over the ranked records, LARGEST wins: (score, ~index).  |score| < 2^48 + 2^36 (w_dist * dist against
// w_gain * n_unknown), so score + 2^50 is in (0, 2^51) and stands in front of 12 bits of 4095 - index; 0: no record.
constexpr uint64_t kGainNoKey = 0ull;
GV_HD uint64_t gain_best_key(const gvx2_gain_record &r, int32_t index)
{
  if (r.status != 0u) return kGainNoKey;
  return ((uint64_t)(r.score + ((int64_t)1 << 50)) << 12) | (uint64_t)(uint32_t)(kGainMaxN - 1 - index);
}
GV_HD int32_t gain_best_index(uint64_t key) { return key == kGainNoKey ? -1 : kGainMaxN - 1 - (int32_t)(key & (uint64_t)(kGainMaxN - 1)); }

GV_HD gvx2_gain_info gain_info(int32_t n_candidates, int32_t n_ranked, uint64_t best_key, const gvx2_gain_record *rec, uint32_t flags, int32_t radius)
{
  gvx2_gain_info I;
  I.n_candidates = n_candidates;
  I.n_ranked = n_ranked;
  I.best = gain_best_index(best_key);
  I.best_entry = I.best >= 0 ? rec[I.best].entry : -1;
  I.best_score = I.best >= 0 ? rec[I.best].score : 0;
  I.flags = flags;
  I.radius = radius;
  return I;
}

}  // namespace gv
