// gv_dyn.hpp -- [EXTENSION] X13 the arithmetic of scoring poses against predicted moving objects, compiled for the host
// (gv_dyn_score_poses) and for the device (gv_dynscore.hip) from this one text, like gv_motion.hpp:
//   dyn_object        a row of the object table from a gv_moving_object (host, once per gv_set_moving_objects);
//   dyn_time, dyn_centre, dyn_object_at, dyn_d2   the pieces of one (pose, circle, object) test;
//   dyn_cost          the pose cost from the smallest d2;
//   dyn_take          (d2, j) against the best so far: the lexicographic minimum, which no order of visits changes.
// Every operation is one fp64 operation in the header's order (include/gridvision_hip.h has the definition); the build
// never contracts (-ffp-contract=off).
#pragma once

#include <math.h>
#include <stdint.h>

#include "gv_types.hpp"   // the public structs, GV_HD

namespace gv {

constexpr int32_t kDynMaxObjects = 128;
constexpr int32_t kDynMaxCircles = 8;

// One row of the object table: 8 doubles, 64 bytes.
struct DynObject {
  double x, y, vx, vy;   // position at t = 0, velocity
  double c, s;           // the yaw terms of the quaternion, as given
  double hl, hw;         // half length (along the heading), half width
};
static_assert(sizeof(DynObject) == 64, "a row is four 16-byte LDS reads");

// What a kernel launch carries of a gv_dyn_config, by value: an enqueued call keeps what it was enqueued with.
struct DynParams {
  int32_t n_circles;
  int32_t need_yaw;              // some off_x[i] != 0.0 among the first n_circles
  double off_x[kDynMaxCircles];
  double t0, dt;
  double inv_q2;                 // 1.0 / (quantum * quantum)
  int32_t T;                     // entries of the cost table
  int32_t collision_cost;
};

GV_HD DynObject dyn_object(const gv_moving_object &m)
{
  const gv_lshape_pose &q = m.pose;
  DynObject o;
  o.x = q.px; o.y = q.py;
  o.vx = m.vx; o.vy = m.vy;
  o.c = 1.0 - 2.0 * (q.qy * q.qy + q.qz * q.qz);
  o.s = 2.0 * (q.qw * q.qz + q.qx * q.qy);
  o.hl = 0.5 * q.length;
  o.hw = 0.5 * q.width;
  return o;
}

GV_HD DynParams dyn_params(const gv_dyn_config &c, int32_t T)
{
  DynParams p;
  p.n_circles = c.n_circles;
  p.need_yaw = 0;
  for (int32_t i = 0; i < kDynMaxCircles; ++i) {
    p.off_x[i] = i < c.n_circles ? c.off_x[i] : 0.0;
    if (p.off_x[i] != 0.0) p.need_yaw = 1;
  }
  p.t0 = c.t0; p.dt = c.dt;
  p.inv_q2 = 1.0 / (c.quantum * c.quantum);
  p.T = T;
  p.collision_cost = c.collision_cost;
  return p;
}

GV_HD double dyn_time(const DynParams &c, int32_t p) { return c.t0 + (double)p * c.dt; }

// the centre of the circle at `off` on the robot's x axis; cy, sy are read only when off != 0.0
GV_HD void dyn_centre(double x, double y, double cy, double sy, double off, double &ax, double &ay)
{
  if (off == 0.0) {
    ax = x;
    ay = y;
  } else {
    ax = x + cy * off;
    ay = y + sy * off;
  }
}

GV_HD void dyn_object_at(const DynObject &o, double t, double &ox, double &oy)
{
  ox = o.x + o.vx * t;
  oy = o.y + o.vy * t;
}

// squared distance from the circle centre (ax, ay) to the rectangle of o centred at (ox, oy); never NaN
GV_HD double dyn_d2(const DynObject &o, double ox, double oy, double ax, double ay)
{
  const double dx = ax - ox, dy = ay - oy;
  const double lx = o.c * dx + o.s * dy, ly = o.c * dy - o.s * dx;
  double ex = fabs(lx) - o.hl;
  ex = ex > 0.0 ? ex : 0.0;
  double ey = fabs(ly) - o.hw;
  ey = ey > 0.0 ? ey : 0.0;
  return ex * ex + ey * ey;
}

GV_HD int32_t dyn_cost(const DynParams &c, const uint8_t *table, double m2)
{
  const double u = m2 * c.inv_q2;
  return u < (double)c.T ? (int32_t)table[(uint32_t)u] : 0;
}

// (d2, j) of one test against the best so far (best_j < 0: none yet)
GV_HD void dyn_take(double d2, int32_t j, double &best, int32_t &best_j)
{
  if (j >= 0 && (best_j < 0 || d2 < best || (d2 == best && j < best_j))) {
    best = d2;
    best_j = j;
  }
}

// One pose against objects j0, j0 + step, ..: the lexicographic minimum of (d2, j) over them and all circles into
// (best, best_j), which the caller starts at (+inf, -1).  The host passes (0, 1), a wavefront its share.
GV_HD void dyn_pose_min(const DynParams &c, const DynObject *objs, int32_t n_obj, int32_t j0, int32_t step, const float *q, int32_t p,
                        double &best, int32_t &best_j)
{
  const double t = dyn_time(c, p);
  const double x = (double)q[0], y = (double)q[1];
  double cy = 0.0, sy = 0.0;
  if (c.need_yaw) {
#if defined(__HIP_DEVICE_COMPILE__)
    sincos((double)q[2], &sy, &cy);
#else
    cy = cos((double)q[2]);
    sy = sin((double)q[2]);
#endif
  }
  double ax[kDynMaxCircles], ay[kDynMaxCircles];
#pragma unroll
  for (int32_t i = 0; i < kDynMaxCircles; ++i) dyn_centre(x, y, cy, sy, c.off_x[i], ax[i], ay[i]);
  for (int32_t j = j0; j < n_obj; j += step) {
    const DynObject o = objs[j];
    double ox, oy;
    dyn_object_at(o, t, ox, oy);
    double m = INFINITY;
#pragma unroll
    for (int32_t i = 0; i < kDynMaxCircles; ++i)
      if (i < c.n_circles) {
        const double d2 = dyn_d2(o, ox, oy, ax[i], ay[i]);
        m = d2 < m ? d2 : m;
      }
    dyn_take(m, j, best, best_j);
  }
}

// a trajectory's record while it is being made: maxima, minima and integer sums only
struct DynAccum {
  int32_t max_cost = 0, first = -1;
  uint32_t sum = 0;
  double best = INFINITY;
  int32_t best_j = -1;
};

GV_HD void dyn_accumulate(const DynParams &c, int32_t p, int32_t cost, double m2, int32_t j, DynAccum &a)
{
  a.max_cost = cost > a.max_cost ? cost : a.max_cost;
  if (cost >= c.collision_cost && (a.first < 0 || p < a.first)) a.first = p;
  a.sum += (uint32_t)cost;
  dyn_take(m2, j, a.best, a.best_j);
}

GV_HD gv_dyn_score dyn_record(const DynAccum &a)
{
  gv_dyn_score r;
  r.max_cost = a.max_cost;
  r.first_collision = a.first;
  r.cost_sum = a.sum;
  r.nearest_object = a.best_j;
  r.min_dist2 = a.best;
  return r;
}

}  // namespace gv
