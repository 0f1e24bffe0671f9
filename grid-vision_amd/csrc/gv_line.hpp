// gv_line.hpp -- cell i of grid_map::LineIterator(start, end) in closed form, compiled for the host (footprint_cells,
// gv_host_math.hpp) and for the device (gv_trajscore.hip) from this one text.
//
// The iterator (oracle/extension.c restates it): the major axis -- x when ddx >= ddy -- steps every cell, major + 1
// cells in all; num = major / 2, then after every cell num += minor and, when num >= major, num -= major and the minor
// axis steps.  minor <= major, so num < major holds between cells and one subtraction per cell is enough: after i
// cells the minor axis has stepped floor((major / 2 + i * minor) / major) times.  That is the whole closed form:
//   major coordinate  s + i * step
//   minor coordinate  s + step * ((major / 2 + i * minor) / major)
// Cell i needs no cell before it, so the lanes of a wavefront take the cells of an outline side by side.
#pragma once

#include <stdint.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define GV_HD __host__ __device__ __forceinline__
#else
#define GV_HD inline
#endif

namespace gv {

// floor(a / d) exactly, for 1 <= d, a < 2^31 and a / d < 2^20, without an integer division: the fp32 product
// (float)a * (1 / (float)d) carries two roundings of 2^-24 and the reciprocal's error (correctly rounded on the host,
// v_rcp_f32's one ulp on the device), 2^-22 relative in all and under 0.3 absolute at a quotient below 2^20, so its
// truncation is the quotient or one beside it, and the remainder says which.
// (Major and minor are different axes of the map: i * minor <= (nx - 1) * (ny - 1) < G <= 2^30, the quotient is at
// most minor + 1, and no side of a map gv_create accepts reaches 2^20.)
GV_HD uint32_t div_floor_small(uint32_t a, uint32_t d)
{
#if defined(__HIP_DEVICE_COMPILE__)
  const float r_d = __builtin_amdgcn_rcpf((float)d);
#else
  const float r_d = 1.0f / (float)d;
#endif
  uint32_t q = (uint32_t)((float)a * r_d);
  int32_t r = (int32_t)(a - q * d);
  if (r < 0) { --q; r += (int32_t)d; }
  if (r >= (int32_t)d) ++q;
  return q;
}

// number of cells of the line: major + 1
GV_HD int32_t line_cells(int32_t sx, int32_t sy, int32_t ex, int32_t ey)
{
  const int32_t ddx = ex >= sx ? ex - sx : sx - ex, ddy = ey >= sy ? ey - sy : sy - ey;
  return (ddx >= ddy ? ddx : ddy) + 1;
}

// cell i (0 .. line_cells - 1) of the line from (sx, sy) to (ex, ey)
GV_HD void line_cell(int32_t sx, int32_t sy, int32_t ex, int32_t ey, uint32_t i, int32_t &cx, int32_t &cy)
{
  const uint32_t ddx = (uint32_t)(ex >= sx ? ex - sx : sx - ex), ddy = (uint32_t)(ey >= sy ? ey - sy : sy - ey);
  const int32_t stepx = ex >= sx ? 1 : -1, stepy = ey >= sy ? 1 : -1;
  const bool x_major = ddx >= ddy;
  const uint32_t den = x_major ? ddx : ddy, add = x_major ? ddy : ddx;
  const int32_t minor = den ? (int32_t)div_floor_small(den / 2 + i * add, den) : 0;   // den == 0: the line is one cell
  cx = sx + stepx * (x_major ? (int32_t)i : minor);
  cy = sy + stepy * (x_major ? minor : (int32_t)i);
}

}  // namespace gv
