// gv_shortcut.hpp -- [EXTENSION] X21 line-of-sight shortcuts and waypoints of resident paths (gvx3_*): the arithmetic of
// the definition in include/gridvision_hip_shortcut.h, one text for the kernels (gv_shortcut.hip) and for the host twin
// (gvx3_shortcut_host, gv_api_shortcut_host.hip), as gv_navpath.hpp is for the walk.  Plain C++ under GV_HD: the rules of
// the configuration and of a call, the line iterator's stepping loop as a struct of registers, a chunk of a visibility
// walk over whatever answers "the cost of this cell", the waypoints of a segment in closed form, and the record.  Every
// translation unit that includes it is built with -ffp-contract=off (the centres are gv_navpath.hpp's path_centre).
#pragma once

#include "../../include/gridvision_hip_shortcut.h"
#include "gv_line.hpp"      // line_cell: cell i of a segment in closed form
#include "gv_navpath.hpp"   // path_centre, kPathMaxStarts, kPathMaxCap, kPathMaxCells
#include "gv_types.hpp"

namespace gv {

constexpr int32_t kShortcutMaxWindow = GVX3_SHORTCUT_MAX_WINDOW;
constexpr int32_t kShortcutMaxSpacing = GVX3_SHORTCUT_MAX_SPACING;
constexpr int32_t kShortcutMaxWcap = GVX3_SHORTCUT_MAX_WCAP;
constexpr int32_t kShortcutMaxCells = GVX3_SHORTCUT_MAX_CELLS;
constexpr int32_t kShortcutChunk = 4;   // cells of a line a visibility walk takes between two looks at "go on?"

GV_HD bool shortcut_config_valid(const gvx3_shortcut_config &c)
{
  return c.max_cost >= 0 && c.max_cost <= 254 && c.window >= 1 && c.window <= kShortcutMaxWindow && c.spacing >= 0 &&
         c.spacing <= kShortcutMaxSpacing && (c.reserved[0] | c.reserved[1] | c.reserved[2] | c.reserved[3] | c.reserved[4]) == 0u;
}

// what a call checks before it knows S
GV_HD bool shortcut_call_ok(int32_t wcap, uint32_t flags)
{
  return wcap >= 1 && wcap <= kShortcutMaxWcap && (flags & ~(uint32_t)GVX3_SHORTCUT_NO_CORNER) == 0u;
}
// ... and once it does
GV_HD bool shortcut_room_ok(int32_t S, int32_t wcap) { return (int64_t)S * (int64_t)wcap <= (int64_t)kShortcutMaxCells; }

// what the kernel and the twin read of a configuration and a call's flags
struct ShortcutRule {
  int32_t max_cost, window, spacing;
  uint32_t no_corner;
};
GV_HD ShortcutRule shortcut_rule(const gvx3_shortcut_config &c, uint32_t flags)
{
  return ShortcutRule{c.max_cost, c.window, c.spacing, flags & GVX3_SHORTCUT_NO_CORNER};
}

// The iterator's stepping loop from p to q, cell 0 = p: the state a lane keeps in registers.  (x, y) is cell i; step()
// goes to cell i + 1 and must not be called at i == major.
struct LineWalk {
  int32_t x, y, i;
  int32_t num, major, minor;
  int32_t sx, sy;
  bool x_major;
};
GV_HD LineWalk line_walk(int32_t px, int32_t py, int32_t qx, int32_t qy)
{
  LineWalk w;
  const int32_t ddx = qx >= px ? qx - px : px - qx, ddy = qy >= py ? qy - py : py - qy;
  w.x = px; w.y = py; w.i = 0;
  w.x_major = ddx >= ddy;
  w.major = w.x_major ? ddx : ddy;
  w.minor = w.x_major ? ddy : ddx;
  w.num = w.major / 2;
  w.sx = qx >= px ? 1 : -1;
  w.sy = qy >= py ? 1 : -1;
  return w;
}
GV_HD void line_step(LineWalk &w)
{
  w.num += w.minor;
  const bool m = w.num >= w.major;
  w.num -= m ? w.major : 0;
  w.x += (w.x_major || m) ? w.sx : 0;
  w.y += (!w.x_major || m) ? w.sy : 0;
  ++w.i;
}

// Up to kShortcutChunk further cells of a visibility walk: `ok` says whether every cell so far was CLEAR; cell 0 is the
// caller's (the anchor is the same for every candidate).  cost(x, y) is the cost byte of a cell on the map.  All the
// chunk's reads come first and none depends on another, so the kernel has them in flight together; a walk that has
// failed or reached its last cell stands still, reads the cell it stands on again and changes nothing.  With no_corner
// the two flanking cells (x_{i-1}, y_i) and (x_i, y_{i-1}) of EVERY step are read and must be CLEAR: those of a step
// along one axis are the step's own two cells, which must be CLEAR anyway, so the outcome is the definition's.
// Returns whether the walk goes on: ok, and cells are left.
template <class Cost>
GV_HD bool shortcut_visible_chunk(const Cost &cost, const ShortcutRule &r, LineWalk &w, bool &ok)
{
  int32_t c[kShortcutChunk], f0[kShortcutChunk], f1[kShortcutChunk];
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
  for (int k = 0; k < kShortcutChunk; ++k) {
    const int32_t xp = w.x, yp = w.y;
    if (ok && w.i < w.major) line_step(w);
    c[k] = (int32_t)cost(w.x, w.y);
    f0[k] = f1[k] = 0;
    if (r.no_corner) {
      f0[k] = (int32_t)cost(xp, w.y);
      f1[k] = (int32_t)cost(w.x, yp);
    }
    // (the reads above are issued whatever ok is; the decision below uses this chunk's earlier cells only through ok,
    // which is folded in after the loop, so that no read waits for a compare)
  }
  bool all = true;
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
  for (int k = 0; k < kShortcutChunk; ++k) all = all && c[k] <= r.max_cost && f0[k] <= r.max_cost && f1[k] <= r.max_cost;
  ok = ok && all;
  return ok && w.i < w.major;
}

// how many waypoints segment (a, b) of major m emits: its first anchor and the cells spacing, 2 * spacing, ... < m
GV_HD int32_t shortcut_segment_waypoints(int32_t m, int32_t spacing) { return 1 + (spacing > 0 && m > 0 ? (m - 1) / spacing : 0); }

// waypoint t (0 .. shortcut_segment_waypoints - 1) of the segment from p to q: the cell t * spacing of its line
GV_HD void shortcut_waypoint(int32_t px, int32_t py, int32_t qx, int32_t qy, int32_t spacing, int32_t t, int32_t &x, int32_t &y)
{
  line_cell(px, py, qx, qy, (uint32_t)(t * spacing), x, y);
}

GV_HD gvx3_shortcut_info shortcut_info_empty()
{
  gvx3_shortcut_info r;
  r.status = GVX3_SHORTCUT_EMPTY;
  r.n_waypoints = r.n_anchors = r.n_src = r.n_steps = r.n_diag_steps = r.max_cost_seen = 0;
  r.end_entry = -1;
  return r;
}

}  // namespace gv
