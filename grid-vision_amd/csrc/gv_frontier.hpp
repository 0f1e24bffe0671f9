// gv_frontier.hpp -- [EXTENSION] X19 frontier clusters (gvx_frontier*): the arithmetic of the definition in
// include/gridvision_hip_frontier.h, one text for the kernels (gv_frontier.hip) and for the host twin (gvx_frontier_host,
// gv_api_frontier_host.hip), as gv_navpath.hpp is for the paths.  Plain C++ under GV_HD: the class test, the rules of
// the configuration and of a call, the 64-bit keys of the two minima and of `best`, and the last step of a record.
#pragma once

#include "../../include/gridvision_hip_frontier.h"
#include "gv_navpath.hpp"   // path_centre: the goal's cell centre is X17's formula, the same text
#include "gv_types.hpp"

namespace gv {

constexpr int32_t kFrontierMaxCap = GVX_FRONTIER_MAX_CAP;
constexpr int32_t kFrontierMaxSide = 65535;   // (x - cx)^2 + (y - cy)^2 < 2^33 stands in front of an entry < 2^30 in one key
constexpr uint32_t kFrontierNone = GVX_FRONTIER_NONE;
constexpr uint64_t kFrontierNoKey = ~0ull;

enum : int32_t { kFrontierNeither = 0, kFrontierFree = 1, kFrontierUnknown = 2 };

GV_HD bool frontier_config_valid(const gvx_frontier_config &c)
{
  return c.free_max >= 0 && c.free_max <= 100 && c.unknown_min >= 0 && c.unknown_min <= 100 && c.unknown_max >= 0 &&
         c.unknown_max <= 100 && c.free_max < c.unknown_min && c.unknown_min <= c.unknown_max && c.max_cost >= 1 &&
         c.max_cost <= 256 && c.min_cells >= 1 && c.min_cells <= (1 << 20) && c.flags == 0u && c.reserved[0] == 0u &&
         c.reserved[1] == 0u;
}

GV_HD bool frontier_call_ok(int32_t cap, uint32_t flags)
{
  return cap >= 1 && cap <= kFrontierMaxCap && (flags & ~(uint32_t)GVX_FRONTIER_USE_FIELD) == 0u;
}

GV_HD bool frontier_grid_ok(int32_t nx, int32_t ny) { return nx <= kFrontierMaxSide && ny <= kFrontierMaxSide; }

// what the kernels and the twin read of a configuration
struct FrontierRule {
  int32_t free_max, unknown_min, unknown_max;
  int32_t max_cost;    // 256: the costmap is not read
  int32_t min_cells;
};
GV_HD FrontierRule frontier_rule(const gvx_frontier_config &c)
{
  return FrontierRule{c.free_max, c.unknown_min, c.unknown_max, c.max_cost, c.min_cells};
}

GV_HD int32_t frontier_class(const FrontierRule &r, int8_t v)
{
  const int32_t i = (int32_t)v;
  return (i >= 0 && i <= r.free_max) ? kFrontierFree : (i >= r.unknown_min && i <= r.unknown_max) ? kFrontierUnknown : kFrontierNeither;
}

// the costmap gate of a frontier cell; `cost` is read only when the rule asks for it
GV_HD bool frontier_cost_ok(const FrontierRule &r, const uint8_t *cost, size_t e)
{
  return r.max_cost >= 256 || (int32_t)cost[e] < r.max_cost;
}

// ((x - cx)^2 + (y - cy)^2, entry): the smallest key is the centre cell's
GV_HD uint64_t frontier_centre_key(int32_t x, int32_t y, int64_t cx, int64_t cy, int32_t e)
{
  const int64_t dx = (int64_t)x - cx, dy = (int64_t)y - cy;
  return ((uint64_t)(dx * dx + dy * dy) << 30) | (uint64_t)(uint32_t)e;
}
GV_HD int32_t frontier_centre_key_entry(uint64_t key) { return (int32_t)(key & ((1ull << 30) - 1ull)); }

// (value, entry): the smallest key over the cells below GV_NAV_UNREACHABLE is the field cell's
GV_HD uint64_t frontier_field_key(uint32_t value, int32_t e) { return ((uint64_t)value << 32) | (uint64_t)(uint32_t)e; }

// the key of `best` over the written records, smallest wins: with the field (field_min, index) of the records that
// have a field cell, else (~n_cells, index); kFrontierNoKey: the record does not take part
GV_HD uint64_t frontier_best_key(const gvx_frontier_record &r, int32_t index, bool use_field)
{
  if (use_field) return r.field_entry >= 0 ? ((uint64_t)r.field_min << 32) | (uint64_t)(uint32_t)index : kFrontierNoKey;
  return ((uint64_t)(0x7FFFFFFFu - (uint32_t)r.n_cells) << 32) | (uint64_t)(uint32_t)index;
}
GV_HD int32_t frontier_best_index(uint64_t key) { return key == kFrontierNoKey ? -1 : (int32_t)(key & 0xFFFFFFFFull); }

// the beginning of a record: what the cluster's root knows; the extrema at their identities
GV_HD gvx_frontier_record frontier_record_begin(int32_t label, int32_t n_cells)
{
  gvx_frontier_record r;
  r.label = label;
  r.n_cells = n_cells;
  r.min_x = r.min_y = 0x7FFFFFFF;
  r.max_x = r.max_y = -1;
  r.sum_x = r.sum_y = 0ull;
  r.centre_entry = -1;
  r.field_entry = -1;
  r.field_min = GV_NAV_UNREACHABLE;
  r.goal_entry = -1;
  r.goal_x = r.goal_y = 0.0f;
  return r;
}

// the last step of a record: the two keys become its centre, field and goal fields
GV_HD void frontier_record_finish(const GridParams &g, uint64_t centre_key, uint64_t field_key, gvx_frontier_record &r)
{
  r.centre_entry = frontier_centre_key_entry(centre_key);
  const bool have = field_key != kFrontierNoKey;
  r.field_entry = have ? (int32_t)(field_key & 0xFFFFFFFFull) : -1;
  r.field_min = have ? (uint32_t)(field_key >> 32) : (uint32_t)GV_NAV_UNREACHABLE;
  r.goal_entry = r.field_entry >= 0 ? r.field_entry : r.centre_entry;
  const int32_t gy = r.goal_entry / g.nx, gx = r.goal_entry - gy * g.nx;
  r.goal_x = path_centre(g.pos_x, g.off_x, g.res, g.nx, gx);
  r.goal_y = path_centre(g.pos_y, g.off_y, g.res, g.ny, gy);
}

GV_HD gvx_frontier_record frontier_record_zero()
{
  gvx_frontier_record r;
  r.label = r.n_cells = r.min_x = r.max_x = r.min_y = r.max_y = 0;
  r.sum_x = r.sum_y = 0ull;
  r.centre_entry = r.field_entry = 0;
  r.field_min = 0u;
  r.goal_entry = 0;
  r.goal_x = r.goal_y = 0.0f;
  return r;
}

}  // namespace gv
