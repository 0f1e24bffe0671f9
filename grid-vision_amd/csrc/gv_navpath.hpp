// gv_navpath.hpp -- [EXTENSION] X17 path extraction from the distance field (gv_nav_path*): the arithmetic of the
// definition in include/gridvision_hip_path.h, one text for the kernel (gv_navpath.hip) and for the host twin
// (gv_nav_path_host, gv_api_planner_host.hip), as gv_match.hpp is for the matcher.  Plain C++ under GV_HD; every translation
// unit that includes it is built with -ffp-contract=off, so each operation below is rounded on its own, on the host and
// on the device.
#pragma once

#include "../../include/gridvision_hip_path.h"
#include "gv_types.hpp"

namespace gv {

constexpr int32_t kPathMaxStarts = 256;
constexpr int32_t kPathMaxCap = 65536;
constexpr int32_t kPathMaxCells = 1 << 20;   // S * cap

GV_HD bool path_call_ok(int32_t S, int32_t cap, uint32_t flags)
{
  return S >= 1 && S <= kPathMaxStarts && cap >= 1 && cap <= kPathMaxCap && (int64_t)S * (int64_t)cap <= (int64_t)kPathMaxCells &&
         (flags & ~(uint32_t)GV_PATH_DIAGONAL) == 0u;
}

// One step of the descent from cell (x, y) of value v.  `f(x, y)` is the field at a cell: the kernel's LDS window and
// the twin's array are two such accessors of this one text.  All eight reads come first and none depends on another,
// so the kernel has them in flight together and a step costs one round trip to LDS, not eight; for that `f` is asked
// for cells up to one step OFF the map too, must not fault there, and may answer anything: what it says about such a
// cell is replaced before it is looked at.  Everything after the reads is compares and selects in the order of the
// header: the four straight candidates, then the four diagonal ones, a candidate counting when it is strictly smaller
// than the best so far.  A diagonal whose flank is GV_NAV_BLOCKED is itself made GV_NAV_BLOCKED, which is smaller than
// nothing; a flank off the map is one, so a diagonal off the map never counts either.
// true: a candidate counted, (x, y, v) are the next cell's and `diag` says whether the move was diagonal; false: none
// is smaller, nothing changed.
GV_HD void path_take(uint32_t cand, int32_t cx, int32_t cy, bool cd, uint32_t &best, int32_t &x, int32_t &y, bool &diag)
{
  const bool t = cand < best;
  best = t ? cand : best;
  x = t ? cx : x;
  y = t ? cy : y;
  diag = t ? cd : diag;
}

template <class Field>
GV_HD bool path_next(const Field &f, int32_t nx, int32_t ny, bool diagonal, int32_t &x, int32_t &y, uint32_t &v, bool &diag)
{
  const uint32_t kOff = GV_NAV_BLOCKED;
  const int32_t cx = x, cy = y;
  uint32_t w = f(cx - 1, cy), e = f(cx + 1, cy), n = f(cx, cy - 1), s = f(cx, cy + 1);
  uint32_t nw = kOff, ne = kOff, sw = kOff, se = kOff;
  if (diagonal) {
    nw = f(cx - 1, cy - 1);
    ne = f(cx + 1, cy - 1);
    sw = f(cx - 1, cy + 1);
    se = f(cx + 1, cy + 1);
  }
  w = cx > 0 ? w : kOff;
  e = cx + 1 < nx ? e : kOff;
  n = cy > 0 ? n : kOff;
  s = cy + 1 < ny ? s : kOff;
  nw = ((w != kOff) & (n != kOff)) ? nw : kOff;
  ne = ((e != kOff) & (n != kOff)) ? ne : kOff;
  sw = ((w != kOff) & (s != kOff)) ? sw : kOff;
  se = ((e != kOff) & (s != kOff)) ? se : kOff;
  uint32_t best = v;
  diag = false;
  path_take(w, cx - 1, cy, false, best, x, y, diag);
  path_take(e, cx + 1, cy, false, best, x, y, diag);
  path_take(n, cx, cy - 1, false, best, x, y, diag);
  path_take(s, cx, cy + 1, false, best, x, y, diag);
  path_take(nw, cx - 1, cy - 1, true, best, x, y, diag);
  path_take(ne, cx + 1, cy - 1, true, best, x, y, diag);
  path_take(sw, cx - 1, cy + 1, true, best, x, y, diag);
  path_take(se, cx + 1, cy + 1, true, best, x, y, diag);
  const bool found = best < v;
  v = best;
  return found;
}

// the record of a start that writes no cell, or the beginning of one that does (status and the end fields follow)
GV_HD gv_nav_path_info path_record_begin(int32_t start_entry, uint32_t start_value)
{
  gv_nav_path_info r;
  r.status = start_entry < 0              ? GV_PATH_OFF_MAP
             : start_value == GV_NAV_BLOCKED     ? GV_PATH_BLOCKED
             : start_value == GV_NAV_UNREACHABLE ? GV_PATH_UNREACHABLE
                                                 : GV_PATH_REACHED;
  r.n_cells = 0;
  r.start_value = start_value;
  r.end_value = start_value;
  r.start_entry = start_entry;
  r.end_entry = -1;
  r.n_diagonal = 0;
  r.reserved = 0u;
  return r;
}

// the centre of the cell behind data-order entry coordinate `i` of an axis of n cells: (pos + off) - (ix + 0.5) * res
// with ix = n - 1 - i, in fp64, rounded once
GV_HD float path_centre(double pos, double off, double res, int32_t n, int32_t i)
{
  return (float)((pos + off) - ((double)(n - 1 - i) + 0.5) * res);
}

}  // namespace gv
