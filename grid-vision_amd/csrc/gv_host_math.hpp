// gv_host_math.hpp -- small host-side arithmetic of the hot path: what the
// reference delegates to tf2, pcl_ros and Eigen around its per-frame loop.
// Product code (no dependency on oracle/).  Compiled with -ffp-contract=off.
#pragma once

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <vector>

#include "gv_line.hpp"
#include "gv_pose_math.hpp"
#include "gv_types.hpp"

namespace gv {
namespace host {

// Quat, Basis, xform_from_tf, apply, transform_pose: gv_pose_math.hpp (one text for the host and the device)

// pcl_ros::transformPointCloud(in, out, tf2::Transform) matrix construction:
// quaternion read back from the tf2 basis, narrowed to fp32,
// Eigen::Quaternionf::toRotationMatrix, translation narrowed to fp32.
inline Mat34f pcl_matrix_from_tf(const gv_transform &t)
{
  const Quat q = Basis::from_quat(Quat{t.qx, t.qy, t.qz, t.qw}).to_quat();
  const float x = (float)q.x, y = (float)q.y, z = (float)q.z, w = (float)q.w;
  const float tx = 2.0f * x, ty = 2.0f * y, tz = 2.0f * z;
  const float twx = tx * w, twy = ty * w, twz = tz * w;
  const float txx = tx * x, txy = ty * x, txz = tz * x;
  const float tyy = ty * y, tyz = tz * y, tzz = tz * z;
  Mat34f m;
  m.m[0] = 1.0f - (tyy + tzz); m.m[1] = txy - twz;          m.m[2] = txz + twy;           m.m[3] = (float)t.tx;
  m.m[4] = txy + twz;          m.m[5] = 1.0f - (txx + tzz); m.m[6] = tyz - twx;           m.m[7] = (float)t.ty;
  m.m[8] = txz - twy;          m.m[9] = tyz + twx;          m.m[10] = 1.0f - (txx + tyy); m.m[11] = (float)t.tz;
  return m;
}

// tf2::Quaternion::setRPY
inline Quat quat_from_rpy(double roll, double pitch, double yaw)
{
  const double hy = yaw * 0.5, hp = pitch * 0.5, hr = roll * 0.5;
  const double cy = std::cos(hy), sy = std::sin(hy);
  const double cp = std::cos(hp), sp = std::sin(hp);
  const double cr = std::cos(hr), sr = std::sin(hr);
  return quat_from_half_angles(cr, sr, cp, sp, cy, sy);
}

// setIntrinsicMatrix / K.inverse() (Eigen 3x3 cofactor inverse)
inline void intrinsics(double fx, double fy, double cx, double cy, double K[9], double Ki[9])
{
  const double k[9] = {fx, 0, cx, 0, fy, cy, 0, 0, 1};
  for (int i = 0; i < 9; ++i) K[i] = k[i];
  auto M = [&](int r, int c) { return k[r * 3 + c]; };
  double cof[9];
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) {
      const int i1 = (i + 1) % 3, i2 = (i + 2) % 3, j1 = (j + 1) % 3, j2 = (j + 2) % 3;
      cof[i * 3 + j] = M(i1, j1) * M(i2, j2) - M(i1, j2) * M(i2, j1);
    }
  const double det = (cof[0] * M(0, 0) + cof[3] * M(1, 0)) + cof[6] * M(2, 0);
  const double invdet = 1.0 / det;
  for (int r = 0; r < 3; ++r)
    for (int c = 0; c < 3; ++c) Ki[r * 3 + c] = cof[c * 3 + r] * invdet;
}

// ---- object_detection post-processing (src/object_detection.cpp:94-269) ----
inline int32_t object_class(int32_t label) { return (label >= 0 && label <= 9) ? label : 10; }

inline float iou(const gv_bbox &box, const float r[4])
{
  const float bx0 = (float)box.x_min, by0 = (float)box.y_min, bx1 = (float)box.x_max, by1 = (float)box.y_max;
  const float x1 = std::max(r[0], bx0), y1 = std::max(r[1], by0);
  const float x2 = std::min(r[2], bx1), y2 = std::min(r[3], by1);
  const float w = std::max(x2 - x1, 0.0f), h = std::max(y2 - y1, 0.0f);
  const float inter = w * h;
  const float area1 = (r[2] - r[0]) * (r[3] - r[1]);
  const float area2 = (float)((box.x_max - box.x_min) * (box.y_max - box.y_min));
  return inter / ((area1 + area2) - inter);
}

// fast_non_max_suppression :166-211 (stable sort: equal confidences keep input order)
inline std::vector<gv_bbox> nms(std::vector<gv_bbox> b, float iou_threshold)
{
  std::vector<gv_bbox> out;
  if (b.empty()) return out;
  std::stable_sort(b.begin(), b.end(), [](const gv_bbox &a, const gv_bbox &c) { return a.confidence > c.confidence; });
  const size_t n = b.size();
  std::vector<float> mat(n * 4);
  std::vector<char> keep(n, 1);
  for (size_t i = 0; i < n; ++i) {
    mat[i * 4 + 0] = (float)b[i].x_min; mat[i * 4 + 1] = (float)b[i].y_min;
    mat[i * 4 + 2] = (float)b[i].x_max; mat[i * 4 + 3] = (float)b[i].y_max;
  }
  for (size_t i = 0; i < n; ++i) {
    if (!keep[i]) continue;
    out.push_back(b[i]);
    for (size_t j = i + 1; j < n; ++j)
      if (iou(b[i], &mat[j * 4]) > iou_threshold) keep[j] = 0;
  }
  return out;
}

// denormalizeAndScaleBoundingBox :226-239
inline void denormalize(std::vector<gv_bbox> &b, int orig_w, int orig_h, int resize)
{
  const float scale_x = static_cast<float>(orig_w) / resize;
  const float scale_y = static_cast<float>(orig_h) / resize;
  for (auto &box : b) {
    box.x_min = static_cast<int>(box.x_min * resize * scale_x);
    box.y_min = static_cast<int>(box.y_min * resize * scale_y);
    box.x_max = static_cast<int>(box.x_max * resize * scale_x);
    box.y_max = static_cast<int>(box.y_max * resize * scale_y);
  }
}

// (double)u >= lo  <=>  u >= ceil_f(lo);   (double)u <= hi  <=>  u <= floor_f(hi)
// for every float u (NaN bounds stay NaN: both forms are then always false).
inline float ceil_to_float(double v)
{
  float f = (float)v;
  if ((double)f < v) f = std::nextafterf(f, INFINITY);
  return f;
}
inline float floor_to_float(double v)
{
  float f = (float)v;
  if ((double)f > v) f = std::nextafterf(f, -INFINITY);
  return f;
}

// grid_map::GridMap::setGeometry + setPosition as the constructor calls them (src/occupancy_grid.cpp:10-11): the
// geometry gv_create gives a handle.  false for what gv_create rejects.
inline bool grid_params(uint8_t grid_x, uint8_t grid_y, double resolution, GridParams &g)
{
  if (grid_x == 0 || grid_y == 0 || !(resolution > 0.0)) return false;
  g.res = resolution;
  g.inv_res = 1.0 / resolution;
  const double sx = std::round((double)grid_x / resolution), sy = std::round((double)grid_y / resolution);
  if (!(sx >= 1.0 && sy >= 1.0) || sx * sy > (double)(1 << 30)) return false;
  g.nx = (int32_t)sx;
  g.ny = (int32_t)sy;
  g.G = g.nx * g.ny;
  g.len_x = (double)g.nx * resolution;
  g.len_y = (double)g.ny * resolution;
  g.pos_x = (double)(grid_x / 3);   // uint8_t / int: integer division (:11)
  g.pos_y = 0.0;
  g.off_x = 0.5 * g.len_x;
  g.off_y = 0.5 * g.len_y;
  return true;
}

// ---- [EXTENSION] X7 trajectory scoring (gv_score_trajectories): the footprint's rules and the host twin of the
// kernel's geometry (include/gridvision_hip.h has the definition) ----
constexpr int32_t kFootprintMaxVertices = 16;
constexpr uint32_t kTrajFlags = GV_TRAJ_KEEP_POSE_COST | GV_TRAJ_DEVICE_POSES;

// what gv_set_footprint accepts
inline bool footprint_valid(const gv_footprint &f)
{
  if (f.n_vertices != 0 && (f.n_vertices < 3 || f.n_vertices > kFootprintMaxVertices)) return false;
  for (int32_t i = 0; i < f.n_vertices; ++i)
    if (!std::isfinite(f.vx[i]) || !std::isfinite(f.vy[i])) return false;
  return f.collision_cost >= 1 && f.collision_cost <= 255 && f.off_map_cost >= 0 && f.off_map_cost <= 255 && f.flags == 0;
}

// The cells one pose tests, as iy * nx + ix: the centre, then every edge's line (gv_line.hpp, the closed form the
// kernel evaluates a lane per cell) from vertex i to vertex (i + 1) % n.  false: the pose is off the map (out untouched).
inline bool footprint_cells(const GridParams &g, const gv_footprint &f, float x, float y, float yaw, std::vector<int32_t> &out)
{
  int cx[kFootprintMaxVertices + 1], cy[kFootprintMaxVertices + 1];
  const double px = (double)x, py = (double)y;
  if (!get_index(g, px, py, cx[0], cy[0])) return false;
  const int32_t n = f.n_vertices;
  if (n > 0) {
    const double c = std::cos((double)yaw), s = std::sin((double)yaw);
    for (int32_t i = 0; i < n; ++i) {
      const double wx = px + (c * f.vx[i] - s * f.vy[i]);
      const double wy = py + (s * f.vx[i] + c * f.vy[i]);
      if (!get_index(g, wx, wy, cx[i + 1], cy[i + 1])) return false;
    }
  }
  std::vector<int32_t> cells;
  cells.push_back(cy[0] * g.nx + cx[0]);
  for (int32_t e = 0; e < n; ++e) {
    const int32_t a = 1 + e, b = 1 + (e + 1 == n ? 0 : e + 1);
    const int32_t m = line_cells(cx[a], cy[a], cx[b], cy[b]);
    for (int32_t i = 0; i < m; ++i) {
      int32_t lx, ly;
      line_cell(cx[a], cy[a], cx[b], cy[b], (uint32_t)i, lx, ly);
      cells.push_back(ly * g.nx + lx);
    }
  }
  out = std::move(cells);
  return true;
}

// ---- [EXTENSION] X9 goal / path distance field (gv_nav_field) ----
// what gv_nav_step_table accepts; gv_set_nav_config adds nav_config_fits
inline bool nav_config_valid(const gv_nav_config &c)
{
  return c.obstacle_cost >= 1 && c.obstacle_cost <= 255 && c.cost_weight >= 0 && c.cost_weight <= 255 && c.flags == 0;
}

// the longest simple path, G - 1 cells entered at the largest step, stays below the two sentinels
inline bool nav_config_fits(const gv_nav_config &c, int32_t G)
{
  const uint64_t max_step = 1u + (uint64_t)c.cost_weight * (uint64_t)(c.obstacle_cost - 1);
  return max_step * (uint64_t)(G - 1) <= 0xFFFFFFFDull;
}

inline void nav_step_table(const gv_nav_config &c, uint32_t table[256])
{
  const NavStep s{c.obstacle_cost, c.cost_weight};
  for (uint32_t v = 0; v < 256; ++v) table[v] = nav_step(s, v);
}

// the field entry (data_entry) of a seed, through the grid's own getIndex (gv_types.hpp: the kernels' text); -1 off the map or non-finite
inline int32_t nav_seed_entry(const GridParams &g, float x, float y)
{
  int ix = 0, iy = 0;
  if (!get_index(g, (double)x, (double)y, ix, iy)) return -1;
  return data_entry(g, ix, iy);
}

// ---- [EXTENSION] ego-motion compensation (gv_grid_move) ----
// Planar rigid motion (yaw, x, y) in fp64.
struct Se2 {
  double yaw, x, y;
};

// (-pi, pi] for an angle in (-2pi, 2pi] (the sum of two wrapped angles)
constexpr double kPi = 3.14159265358979323846;
inline double wrap_pi(double a)
{
  if (a > kPi) a -= 2.0 * kPi;
  else if (a <= -kPi) a += 2.0 * kPi;
  return a;
}

// a o b: rotation a.yaw + b.yaw, translation a.t + R(a.yaw) b.t
inline Se2 se2_compose(const Se2 &a, const Se2 &b)
{
  const double c = std::cos(a.yaw), s = std::sin(a.yaw);
  return Se2{wrap_pi(a.yaw + b.yaw), a.x + (c * b.x - s * b.y), a.y + (s * b.x + c * b.y)};
}

// The planar part of a motion: yaw of the fp64-normalised quaternion, tx, ty (z, roll and pitch are dropped).
// false when a field, or the result, is not finite (a zero quaternion among them).
inline bool se2_from_motion(const gv_transform &m, Se2 &out)
{
  const double f[7] = {m.qx, m.qy, m.qz, m.qw, m.tx, m.ty, m.tz};
  for (double v : f)
    if (!std::isfinite(v)) return false;
  const double n = std::sqrt(((m.qx * m.qx + m.qy * m.qy) + m.qz * m.qz) + m.qw * m.qw);
  const double qx = m.qx / n, qy = m.qy / n, qz = m.qz / n, qw = m.qw / n;
  const double yaw = std::atan2(2.0 * (qw * qz + qx * qy), 1.0 - 2.0 * (qy * qy + qz * qz));
  if (!std::isfinite(yaw)) return false;
  out = Se2{yaw, m.tx, m.ty};
  return true;
}

// Largest distance from the base origin to a map corner (pos +- len/2).
inline double map_corner_radius(const GridParams &g)
{
  double r = 0.0;
  for (int i = 0; i < 4; ++i) {
    const double x = (i & 1) ? g.pos_x + g.off_x : g.pos_x - g.off_x;
    const double y = (i & 2) ? g.pos_y + g.off_y : g.pos_y - g.off_y;
    r = std::max(r, std::sqrt(x * x + y * y));
  }
  return r;
}

// One gv_grid_move: the resample S the layers take and the residue left for the next call.
struct GridMoveStep {
  bool applied;        // S is not the identity
  double yaw;          // S's rotation ...
  double c, s;         // ... as the kernel uses it: cos / sin (exactly 1, 0 without rotation)
  double tx, ty;       // S's translation: whole multiples of res
  Se2 residue;         // E after the call
};

// residue E = L <- base_prev, motion D = base_prev <- base_now.  E <- E o D; S = (yaw_s, t_s) with yaw_s = yaw_E where
// |yaw_E| * r_max >= res/2 (the rotation moves some cell centre of the map by half a cell) and 0 otherwise,
// t_s = res * round(t_E / res); then E <- S^-1 o E.  Motion below a cell stays in E until it adds up.
inline GridMoveStep plan_grid_move(const Se2 &residue, const Se2 &motion, const GridParams &g)
{
  const Se2 e = se2_compose(residue, motion);
  GridMoveStep st;
  st.yaw = (std::fabs(e.yaw) * map_corner_radius(g) >= 0.5 * g.res) ? e.yaw : 0.0;
  st.tx = g.res * std::round(e.x / g.res);
  st.ty = g.res * std::round(e.y / g.res);
  st.c = st.yaw == 0.0 ? 1.0 : std::cos(st.yaw);
  st.s = st.yaw == 0.0 ? 0.0 : std::sin(st.yaw);
  st.applied = st.yaw != 0.0 || st.tx != 0.0 || st.ty != 0.0;
  // S^-1 o E: rotation yaw_E - yaw_s, translation R(-yaw_s) (t_E - t_s)
  const double dx = e.x - st.tx, dy = e.y - st.ty;
  st.residue = Se2{wrap_pi(e.yaw - st.yaw), st.c * dx + st.s * dy, st.c * dy - st.s * dx};
  return st;
}

// [EXTENSION] X6 inflated costmap (gv_inflate): the cost table of include/gridvision_hip.h, built once per
// configuration in fp64.  cost[q], q = 0 .. d2max, from dist = sqrt((double)q) * res; d2max is the largest q whose dist
// is within the inflation radius, rc = isqrt(d2max) is how far the kernels search along a row and across rows.
constexpr int32_t kInflateMaxRc = 63;
constexpr size_t kTableBytes = (size_t)(kInflateMaxRc + 1) * (kInflateMaxRc + 1);   // room of a table's device and staging slot
constexpr int32_t kInflateFlags = GV_INFLATE_KEEP_DIST2 | GV_INFLATE_OCCUPANCY_SCALE;

struct InflationTable {
  int32_t d2max = -1, rc = 0;
  std::vector<uint8_t> cost;   // d2max + 1 entries
};

// false (out untouched) for anything gv_set_inflation rejects
inline bool inflation_table(const gv_inflation &c, double res, InflationTable &out)
{
  if (!std::isfinite(c.inscribed_radius) || !std::isfinite(c.inflation_radius) || !std::isfinite(c.cost_scaling_factor) ||
      !std::isfinite(res) || !(res > 0.0))
    return false;
  if (c.inscribed_radius < 0.0 || c.inflation_radius < c.inscribed_radius || c.cost_scaling_factor < 0.0) return false;
  if (c.lethal_threshold < 1 || c.lethal_threshold > 100 || (c.flags & ~kInflateFlags) != 0) return false;
  const int32_t q_end = (kInflateMaxRc + 1) * (kInflateMaxRc + 1);   // the first q with isqrt(q) > 63
  int32_t d2max = 0;
  while (d2max + 1 <= q_end && std::sqrt((double)(d2max + 1)) * res <= c.inflation_radius) ++d2max;
  if (d2max >= q_end) return false;
  InflationTable t;
  t.d2max = d2max;
  while ((t.rc + 1) * (t.rc + 1) <= d2max) ++t.rc;
  t.cost.resize((size_t)d2max + 1);
  for (int32_t q = 0; q <= d2max; ++q) {
    const double dist = std::sqrt((double)q) * res;
    uint8_t v;
    if (q == 0) v = 254;
    else if (dist <= c.inscribed_radius) v = 253;
    else if (dist > c.inflation_radius) v = 0;
    else v = (uint8_t)(252.0 * std::exp(-c.cost_scaling_factor * (dist - c.inscribed_radius)));
    if (c.flags & GV_INFLATE_OCCUPANCY_SCALE)
      v = v == 0 ? 0 : v == 253 ? 99 : v == 254 ? 100 : (uint8_t)(1 + (97 * ((int)v - 1)) / 251);
    t.cost[(size_t)q] = v;
  }
  out = std::move(t);
  return true;
}

// [EXTENSION] SURVEY 8(e)-2 the frame sharded by points over `world` GPUs: who owns which rows of the grid and how large
// the two exchanges are.  THE band rule: rank q finalises the whole 64-row blocks [blk(q), blk(q + 1)) of the padded grid,
// blk(q) = q * (ny_pad / 64) / world, clipped to ny.  (Device twin: band_block in gv_shard.hip, which packs by that rule.)
inline int shard_band_block(int q, int nblk, int world) { return (int)((long long)q * nblk / world); }
inline void shard_band_rows(int rank, int world, int ny, int ny_pad, int32_t &y0, int32_t &y1)
{
  y0 = std::min(ny, 64 * shard_band_block(rank, ny_pad / 64, world));
  y1 = std::min(ny, 64 * shard_band_block(rank + 1, ny_pad / 64, world));
}

// words of one of `world` equal slices that cover `words` bitmap words: a multiple of 4 (16-byte vectors)
inline size_t shard_slice_words(size_t words, int world)
{
  return (((words + (size_t)world - 1) / (size_t)world) + 3) & ~(size_t)3;
}

struct ShardPlan {
  struct Band {
    int32_t y0 = 0, y1 = 0;   // rows [y0, y1)
    size_t b = 0, e = 0;      // cells [b, e) = [y0 * nx, y1 * nx)
  };
  int32_t world = 1;
  int32_t nxw = 0, nx_pad = 0, ny_pad = 0;   // the bitmaps' geometry (the band packing kernels take it)
  size_t slice = 0;           // exchange 1: words of one rank's slice of the end bitmaps
  size_t chunk = 0;           // exchange 2: words of one packed free-cell band (the longest one's, a multiple of 4)
  std::vector<Band> bands;    // per rank
  // one ncclReduceScatter of cnt0 cells per rank serves the hit counts: every band has cnt0 cells and band r starts at
  // cell r * cnt0 (otherwise: one ncclReduce per band)
  bool equal_bands = true;
  size_t cnt0 = 0;

  ShardPlan() = default;
  ShardPlan(int32_t nx, int32_t ny, int32_t nx_pad_, int32_t ny_pad_, int32_t nxw_, size_t ends_words, int32_t world_)
      : world(world_), nxw(nxw_), nx_pad(nx_pad_), ny_pad(ny_pad_), slice(shard_slice_words(ends_words, world_)),
        bands((size_t)world_)
  {
    int32_t rows_max = 0;
    for (int r = 0; r < world; ++r) {
      Band &B = bands[(size_t)r];
      shard_band_rows(r, world, ny, ny_pad, B.y0, B.y1);
      B.b = (size_t)B.y0 * (size_t)nx;
      B.e = (size_t)B.y1 * (size_t)nx;
      if (r == 0) cnt0 = B.e - B.b;
      equal_bands = equal_bands && B.e - B.b == cnt0 && B.b == (size_t)r * cnt0;
      // (a packed band holds every row of its blocks, also those of the padding behind ny)
      rows_max = std::max(rows_max, 64 * (shard_band_block(r + 1, ny_pad / 64, world) - shard_band_block(r, ny_pad / 64, world)));
    }
    // (equal bands are never empty: the bands cover [0, ny) and ny >= 1)
    chunk = ((size_t)nxw * (size_t)rows_max + (size_t)(rows_max / 32) * (size_t)nx_pad + 3) & ~(size_t)3;
  }
  // words the exchange scratch holds: `world` received slices, or the packed bands and behind them the received ones
  size_t scratch_words() const { return std::max(slice * (size_t)world, 2 * chunk * (size_t)world) + 16; }
};

// [EXTENSION] X2 the sector ray stage (k_ray_sectors, gv_raysector.hip): how the eight wedges around the origin cell are
// cut into workgroups.  Built per frame from the grid, the origin cell and the cloud's size; the launcher and the
// argument block (SectorArgs) only copy it.  violations() is THE list of what the kernel relies on.
constexpr size_t kMaxStatSlots = 8u << 12;        // one (rays, visits) slot per sector workgroup
constexpr size_t kSectorLdsMax = 160u * 1024u;    // LDS of a gfx950 CU: the most hipFuncAttributeMaxDynamicSharedMemorySize grants

// the knobs of Tuning (gv_context.hpp) the plan reads; read_tuning fills them with the rest
struct SectorTuning {
  int32_t log2s = 0, cap = 0, log2m = 0;   // GV_LOG2S / GV_CAP / GV_LOG2M (sweeps)
  int32_t log2s_oct[8] = {0, 0, 0, 0, 0, 0, 0, 0};   // GV_LOG2S_OCT="a,b,..." per octant index (sweeps)
  int32_t sector_rev = -1;                 // GV_SECTOR_REV (sweeps)
  int reorder = 1;                         // GV_SECTOR_REORDER=0: workgroups in natural (octant, sector) order
  int helpers = -1;                        // GV_SECTOR_HELPERS: -1 automatic, 0 off, 1 on
  int32_t flat_k = 8;                      // GV_FLAT_K: exact-cell : marched-cell cost ratio (0 = always march)
  uint32_t march_limit = 64u * 512u;       // GV_MARCH_LIMIT
  uint32_t flat_direct = 2048;             // GV_FLAT_DIRECT
};

struct SectorPlan {
  // one bit per precondition of k_ray_sectors (names: the kernel's own lambdas and variables, gv_raysector.hip)
  enum : uint32_t {
    kWideColumn = 1u << 0,      // a column of a sector is one 32-bit word of cell bits (w = bhi - blo + 1 of col_bounds and
                                // the mask wm made of it, in scan_columns and in scan_row)
    kSectorCount = 1u << 1,     // S <= 2^12: S << log2m stays in 32 bits (SM, the lattice-gap buckets)
    kWorkgroups = 1u << 2,      // wg_base[] is 16 bits wide and there is one statistics slot per workgroup (bid and stat_slot in
                                // the dispatch-order decode at the top of k_ray_sectors)
    kLog2m = 1u << 3,           // M = 1 << log2m <= 512 slope buckets: eight blocks of 64 (s_blkmax[8]); 4 is the knob's least
    kCap = 1u << 4,             // cap >= 2048: the ends of one wavefront's 64 columns fit a chunk (next_group's per-wavefront
                                // groups); <= 65536: an overflow entry holds a 16-bit index into raw (L.over, sector_lds_layout)
    kMarksWords = 1u << 5,      // marks[]: one word per wedge column 0 .. imax (cleared up to oc.imax); even: what follows it stays 8-byte aligned
    kLds = 1u << 6,             // sector_lds_layout fits the LDS of a CU
  };
  struct Workgroup {
    int32_t octant, sector, helper, part, nparts, stat_slot, idle;
  };

  int32_t len[8] = {}, imax = 0;   // wedge length of octant o (xmaj = bit 2, smaj = bit 1): cells to the map edge along the major axis
  uint8_t log2s_oct[8] = {};
  uint16_t rev_oct[8] = {};
  int32_t cap = 0, log2m = 0, marks_words = 0;
  uint32_t oct_perm = 0;
  int32_t reorder = 0;
  uint32_t wg_base[9] = {};        // (SectorArgs holds them in 16 bits: kWorkgroups)
  int32_t n_helpers = 0;
  int32_t flat_k = 0;              // the tail parameters
  uint32_t march_limit = 0, flat_direct = 0;
  int32_t ch = 4;                  // k_ray_sectors<ch>: every wedge column lives in a register slot of one thread, ch * 512 >= imax
  size_t lds_bytes = 0;
  uint32_t total_workgroups = 0;   // the dispatch: helpers first, then the octants' sectors
  size_t stat_slots = 0;

  SectorPlan() = default;
  SectorPlan(int32_t nx, int32_t ny, int32_t cx, int32_t cy, size_t n_points, const SectorTuning &tune)
  {
    imax = std::max(std::max(cx, nx - 1 - cx), std::max(cy, ny - 1 - cy));
    int ord[8];
    for (int o = 0; o < 8; ++o) {
      const bool xmaj = (o >> 2) & 1, pos = (o >> 1) & 1;
      len[o] = xmaj ? (pos ? nx - 1 - cx : cx) : (pos ? ny - 1 - cy : cy);
      ord[o] = o;
    }
    // Sectors per octant: the far end of a wedge about 16 cells wide (len <= 16*S; the kernel needs
    // <= 32) and an estimated <= 12000 ends per sector (the estimate runs ~2x high; above one LDS chunk
    // of 4096 ends a wedge is processed in row groups, which measured better on config 5 -- 10 M points,
    // 160 vs 390 us -- than four times as many, thinner wedges).  Measured on
    // config 3 (tools/sweep_oct.sh, tools/sweep_sectors.sh): the kernel is bound by per-workgroup
    // latency chains, so fewer, fatter wedges win as long as those two hold, and an octant whose wedge
    // is short (origin near that map edge) gets proportionally fewer sectors: 128/64/32 sectors for
    // wedges of 1660/1000/340 columns instead of 128 everywhere does the same frame in 576 instead of
    // 1024 workgroups, 84 -> 76 us pipelined.  Wider wedges (S = 16 for 340 columns) lose again.
    const double G = (double)nx * (double)ny;
    const double dens = std::min((double)n_points, G) / G;
    double est_max = 0.0;
    for (int o = 0; o < 8; ++o) {
      int l2 = 3;   // the gap-sector logic wants S >= 8
      while ((16 << l2) < len[o]) ++l2;
      double est = 1.5 * dens * (double)len[o] * (double)len[o] / (double)(2 << l2);
      while (est > 12000.0 && l2 < 12) {
        ++l2;
        est *= 0.5;
      }
      if (tune.log2s > 0) { l2 = tune.log2s; est = 1.5 * dens * (double)len[o] * (double)len[o] / (double)(2 << l2); }
      if (tune.log2s_oct[o] > 0) { l2 = tune.log2s_oct[o]; est = 1.5 * dens * (double)len[o] * (double)len[o] / (double)(2 << l2); }
      log2s_oct[o] = (uint8_t)l2;
      est_max = std::max(est_max, est);
    }
    // Rows of 512 columns, 8 blocks of 64 each, one block per wavefront: a row goes to the wavefronts in ascending or in
    // descending order, whichever keeps the fullest wavefront lightest (far columns are wider: weight ~ column number),
    // rows taken from the heaviest (last) one down.  GV_SECTOR_REV=0 / 1: never / always alternate (experiments).
    for (int o = 0; o < 8; ++o) {
      const int rows = (len[o] + 511) / 512;
      double load[8] = {0, 0, 0, 0, 0, 0, 0, 0};
      uint16_t mask = 0;
      const double wbase = (double)(1 << log2s_oct[o]);   // a column's cost: its cells (a / S + 1), times S
      for (int r = std::min(rows, 16) - 1; r >= 0; --r) {
        double w[8];
        for (int b = 0; b < 8; ++b) {
          const int a0 = 512 * r + 64 * b + 1, a1 = std::min(a0 + 63, len[o]);
          w[b] = a1 >= a0 ? (double)(a1 - a0 + 1) * (0.5 * (double)(a0 + a1) + wbase) : 0.0;
        }
        double up = 0.0, down = 0.0;
        for (int b = 0; b < 8; ++b) { up = std::max(up, load[b] + w[b]); down = std::max(down, load[b] + w[7 - b]); }
        bool rev = down < up;
        if (tune.sector_rev == 0) rev = false;
        if (tune.sector_rev == 1) rev = (r & 1) != 0;
        if (rev) mask |= (uint16_t)(1u << r);
        for (int b = 0; b < 8; ++b) load[b] += rev ? w[7 - b] : w[b];
      }
      rev_oct[o] = mask;
    }
    cap = tune.cap > 0 ? std::max(2048, tune.cap) : ((est_max <= 1700.0 && tune.log2s <= 0) ? 2048 : 4096);
    flat_k = tune.flat_k;
    march_limit = tune.march_limit;
    flat_direct = tune.flat_direct;
    log2m = tune.log2m > 0 ? tune.log2m : 9;
    marks_words = (imax + 3) & ~1;   // one word per wedge column, 0..imax
    std::stable_sort(ord, ord + 8, [&](int a, int b) { return len[a] > len[b]; });
    reorder = tune.reorder;
    uint32_t base = 0;
    for (int k = 0; k < 8; ++k) {
      oct_perm |= (uint32_t)ord[k] << (3 * k);
      wg_base[k] = base;
      base += 1u << std::min<int>(log2s_oct[reorder ? ord[k] : k], 28);   // (beyond 2^12: kSectorCount)
    }
    wg_base[8] = base;
    // second workgroups for the axis / diagonal sectors of every octant once the wedges are long enough to have
    // heavy tails (GV_SECTOR_HELPERS=0 / 1 forces them off / on)
    n_helpers = (tune.helpers >= 0) ? (tune.helpers ? 16 : 0) : (imax >= 512 ? 16 : 0);
    ch = imax <= 4 * kSecThreads ? 4 : imax <= 8 * kSecThreads ? 8 : 16;
    lds_bytes = sector_lds_layout(cap, marks_words, std::min(log2m, 30)).total;
    total_workgroups = wg_base[8] + (uint32_t)n_helpers;
    stat_slots = (size_t)total_workgroups;
  }

  uint32_t violations() const
  {
    uint32_t v = 0;
    for (int o = 0; o < 8; ++o) {
      // the widest column of a wedge is the last sector's, at column len, in an x-major octant: floor(len / S) + 1
      // cells (col_bounds: bhi = len, blo = ceil(len * (S - 1) / S)); no other sector or column is wider
      if (len[o] >= 1 && (len[o] >> std::min<int>(log2s_oct[o], 30)) + 1 > 32) v |= kWideColumn;
      if (log2s_oct[o] > 12) v |= kSectorCount;
    }
    if (wg_base[8] > 65535u || (size_t)total_workgroups > kMaxStatSlots) v |= kWorkgroups;
    if (log2m < 4 || log2m > 9) v |= kLog2m;
    if (cap < 2048 || cap > 65536) v |= kCap;
    if (marks_words < imax + 1 || (marks_words & 1)) v |= kMarksWords;
    if (lds_bytes > kSectorLdsMax) v |= kLds;
    return v;
  }
  // what the first violated condition is called in an error message
  static const char *violation_name(uint32_t v)
  {
    return (v & kWideColumn)    ? "sector ray stage: a wedge column is wider than 32 cells (GV_LOG2S / GV_LOG2S_OCT too small for this grid)"
           : (v & kSectorCount) ? "sector ray stage: more than 4096 sectors in an octant"
           : (v & kWorkgroups)  ? "too many sector workgroups"
           : (v & kLog2m)       ? "sector ray stage: log2m outside 4 .. 9"
           : (v & kCap)         ? "sector ray stage: cap outside 2048 .. 65536"
           : (v & kMarksWords)  ? "sector ray stage: marks_words below imax + 1 or odd"
           : (v & kLds)         ? "sector ray stage: the LDS layout exceeds 160 KiB"
                                : "";
  }

  // Host twin of the kernel's decode of its place in the dispatch order (the dispatch-order decode at the top of
  // k_ray_sectors, gv_raysector.hip, which stays a device copy): helpers first, then the octants with the longest wedges, and inside an octant the
  // sectors next to the slopes 0, 1/2, 1 first.  idle: the odd helper of a one-sector octant, which returns at once.
  Workgroup workgroup(int bid_all) const
  {
    const bool helper = bid_all < n_helpers;
    const int bid = helper ? (int)wg_base[bid_all >> 1] : bid_all - n_helpers;   // (helpers: only k_oct is taken from it)
    int k_oct = 0;
    for (int k = 1; k < 8; ++k) k_oct += (bid >= (int)wg_base[k]) ? 1 : 0;
    const int o = reorder ? ((int)(oct_perm >> (3 * k_oct)) & 7) : k_oct;
    const int S = 1 << log2s_oct[o];
    int s = bid - (int)wg_base[k_oct];
    if (reorder && S >= 8) {
      const int r = s;
      if (r < 4) s = (r == 0) ? 0 : (r == 1) ? (S >> 1) - 1 : (r == 2) ? S - 1 : (S >> 1);
      else s = (r - 4 < (S >> 1) - 2) ? r - 3 : r - 1;
    }
    bool idle = false;
    if (helper) {
      s = (bid_all & 1) ? S - 1 : 0;
      idle = S < 2 && (bid_all & 1);   // one sector only: it has one helper
    }
    // column share: workgroup `part` of `nparts` evaluates the columns i with i % nparts == part
    const int nparts = (n_helpers > 0 && (s == 0 || s == S - 1)) ? 2 : 1;
    return {o, s, helper ? 1 : 0, helper ? 1 : 0, nparts, helper ? (int)wg_base[8] + bid_all : bid, idle ? 1 : 0};
  }
};

}  // namespace host
}  // namespace gv
