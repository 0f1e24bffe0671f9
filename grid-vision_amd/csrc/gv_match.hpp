// gv_match.hpp -- [EXTENSION] X16 scan-to-costmap matching (gv_match_scan*): the arithmetic of the definition in
// include/gridvision_hip_match.h, one text for the kernels (gv_match.hip) and for the host twin (gv_match_scan_host,
// gv_api_match_host.hip), as gv_track.hpp is for the tracker.  Plain C++ under GV_HD; every translation unit that includes
// it is built with -ffp-contract=off, so each operation below is rounded on its own, on the host and on the device.
#pragma once

#include <math.h>
#include <string.h>

#include "../../include/gridvision_hip_match.h"
#include "gv_types.hpp"

namespace gv {

constexpr int32_t kMatchMaxHalf = 32;                 // wx, wy, wt
constexpr int32_t kMatchMaxSide = 2 * kMatchMaxHalf + 1;
constexpr int32_t kMatchMaxStride = 1024;
constexpr uint32_t kMatchMaxSelected = 1u << 24;      // 2^24 points of cost <= 255: the uint32 sums cannot wrap
#ifndef GV_MATCH_CHUNK
#define GV_MATCH_CHUNK 512
#endif
constexpr int32_t kMatchChunk = GV_MATCH_CHUNK;       // points of one workgroup of the score pass (A/B builds: -DGV_MATCH_CHUNK=)
constexpr double kMatchCellLimit = 1073741824.0;      // 2^30: a cell index of this magnitude or more takes no part

// configuration + guess as a call carries them (kernel arguments, the twin's locals)
struct MatchParams {
  int32_t wx, wy, wt;
  int32_t stride;
  int32_t min_points;
  uint32_t use_band;
  double x, y, yaw;        // the guess
  double yaw_step;
};

GV_HD int32_t match_nt(const MatchParams &p) { return 2 * p.wt + 1; }
GV_HD int32_t match_ny(const MatchParams &p) { return 2 * p.wy + 1; }
GV_HD int32_t match_nx(const MatchParams &p) { return 2 * p.wx + 1; }

GV_HD bool match_finite(float v)
{
  uint32_t b;
  memcpy(&b, &v, sizeof(b));
  return (b & 0x7f800000u) != 0x7f800000u;
}

// the map update's transform (pcl's SSE form, xform34 of gv_device.hpp): x*c0 + (y*c1 + (z*c2 + c3))
GV_HD void match_base_point(const Mat34f &m, float px, float py, float pz, float &bx, float &by, float &bz)
{
  bx = px * m.m[0] + (py * m.m[1] + (pz * m.m[2] + m.m[3]));
  by = px * m.m[4] + (py * m.m[5] + (pz * m.m[6] + m.m[7]));
  bz = px * m.m[8] + (py * m.m[9] + (pz * m.m[10] + m.m[11]));
}

// a selected point is used: finite, and inside the band when the configuration asks for it (X4's compares)
GV_HD bool match_used(float bx, float by, float bz, uint32_t use_band, const HeightBand &hb)
{
  if (!(match_finite(bx) && match_finite(by) && match_finite(bz))) return false;
  return !use_band || (!(bz < hb.z_ground) && !(bz > hb.z_max));
}

// theta_t
GV_HD double match_theta(const MatchParams &p, int32_t t) { return p.yaw + (double)(t - p.wt) * p.yaw_step; }

// the cell (ux, uy) of a used point under yaw candidate (c, s); false: it contributes to no candidate
GV_HD bool match_cell(const GridParams &g, const MatchParams &p, float c, float s, float bx, float by, int32_t &ux, int32_t &uy)
{
  const float cx = c * bx, sy = s * by, sx = s * bx, cy = c * by;
  const float rx = cx - sy;
  const float ry = sx + cy;
  const double gx = (double)rx + p.x;
  const double gy = (double)ry + p.y;
  const double vx = ((gx - g.off_x) - g.pos_x) / g.res;
  const double vy = ((gy - g.off_y) - g.pos_y) / g.res;
  const double fx = floor(-vx), fy = floor(-vy);
  if (!(fabs(fx) < kMatchCellLimit) || !(fabs(fy) < kMatchCellLimit)) return false;   // NaN lands here too
  ux = (int32_t)fx;
  uy = (int32_t)fy;
  return true;
}

// C(ix, iy)
GV_HD uint32_t match_cost(const GridParams &g, const uint8_t *cost, int32_t ix, int32_t iy)
{
  if (ix < 0 || iy < 0 || ix >= g.nx || iy >= g.ny) return 0u;
  return (uint32_t)cost[data_entry(g, ix, iy)];
}

// The selection's order as one 64-bit key, larger is better: the score, then the smaller Chebyshev distance (<= 32),
// then the smaller linear index (< 65^3 < 2^24).
GV_HD uint64_t match_key(uint32_t score, int32_t dt, int32_t j, int32_t i, uint32_t lin)
{
  const int32_t a = dt < 0 ? -dt : dt, b = j < 0 ? -j : j, c = i < 0 ? -i : i;
  const int32_t cheb = a > b ? (a > c ? a : c) : (b > c ? b : c);
  return ((uint64_t)score << 32) | ((uint64_t)(255 - cheb) << 24) | (uint64_t)(0xFFFFFFu - lin);
}
GV_HD uint32_t match_key_lin(uint64_t key) { return 0xFFFFFFu - (uint32_t)(key & 0xFFFFFFu); }
GV_HD uint32_t match_key_score(uint64_t key) { return (uint32_t)(key >> 32); }

// the record of the best candidate `lin` (linear index) with its score
GV_HD gv_match_result match_record(const GridParams &g, const MatchParams &p, uint32_t lin, uint32_t best_score, uint32_t guess_score,
                                   uint32_t n_used)
{
  const int32_t NX = match_nx(p), NY = match_ny(p);
  const int32_t t = (int32_t)(lin / (uint32_t)(NY * NX));
  const int32_t r = (int32_t)(lin % (uint32_t)(NY * NX));
  const int32_t j = r / NX - p.wy, i = r % NX - p.wx;
  gv_match_result o;
  o.best_t = t - p.wt;
  o.best_j = j;
  o.best_i = i;
  o.valid = ((int64_t)n_used >= (int64_t)p.min_points && best_score > 0u) ? 1 : 0;
  o.n_used = n_used;
  o.best_score = best_score;
  o.guess_score = guess_score;
  o.reserved = 0u;
  o.x = p.x - (double)i * g.res;
  o.y = p.y - (double)j * g.res;
  o.yaw = match_theta(p, t);
  o.reserved2 = 0u;
  return o;
}

}  // namespace gv
