// gv_pose_math.hpp -- the fp64 rotation arithmetic the reference delegates to tf2 (Matrix3x3::setRotation / getRotation,
// Transform::operator(), Quaternion::setRPY, doTransform(Pose)), compiled for the host (gv_host_math.hpp's callers) and
// for the device (k_tick_dets, gv_track.hip) from this one text, like gv_track.hpp and gv_motion.hpp.  Every operation
// is one fp64 operation in the order written; the build never contracts (-ffp-contract=off).
//   Quat, Basis (from_quat, to_quat, operator*), xform_from_tf, apply, quat_from_half_angles, transform_pose;
//   [EXTENSION] X15 the tick's detection list: tick_vision_pose, tick_dets_empty, tick_det_take.
#pragma once

#include <math.h>
#include <stdint.h>

#include "gv_types.hpp"   // the public structs, Xform64, VisionOut, GV_HD

namespace gv {
namespace host {

struct Quat {
  double x, y, z, w;
};

// 3x3 fp64 rotation, row-major (tf2::Matrix3x3)
struct Basis {
  double m[9];

  // tf2::Matrix3x3::setRotation(const Quaternion&)
  static GV_HD Basis from_quat(const Quat &q)
  {
    const double d = ((q.x * q.x + q.y * q.y) + q.z * q.z) + q.w * q.w;
    const double s = 2.0 / d;
    const double xs = q.x * s, ys = q.y * s, zs = q.z * s;
    const double wx = q.w * xs, wy = q.w * ys, wz = q.w * zs;
    const double xx = q.x * xs, xy = q.x * ys, xz = q.x * zs;
    const double yy = q.y * ys, yz = q.y * zs, zz = q.z * zs;
    Basis b;
    b.m[0] = 1.0 - (yy + zz); b.m[1] = xy - wz;         b.m[2] = xz + wy;
    b.m[3] = xy + wz;         b.m[4] = 1.0 - (xx + zz); b.m[5] = yz - wx;
    b.m[6] = xz - wy;         b.m[7] = yz + wx;         b.m[8] = 1.0 - (xx + yy);
    return b;
  }

  // tf2::Matrix3x3::getRotation(Quaternion&)
  GV_HD Quat to_quat() const
  {
    const double trace = (m[0] + m[4]) + m[8];
    double t[4];
    if (trace > 0.0) {
      double s = sqrt(trace + 1.0);
      t[3] = s * 0.5;
      s = 0.5 / s;
      t[0] = (m[7] - m[5]) * s;
      t[1] = (m[2] - m[6]) * s;
      t[2] = (m[3] - m[1]) * s;
    } else {
      const int i = m[0] < m[4] ? (m[4] < m[8] ? 2 : 1) : (m[0] < m[8] ? 2 : 0);
      const int j = (i + 1) % 3, k = (i + 2) % 3;
      double s = sqrt(((m[i * 3 + i] - m[j * 3 + j]) - m[k * 3 + k]) + 1.0);
      t[i] = s * 0.5;
      s = 0.5 / s;
      t[3] = (m[k * 3 + j] - m[j * 3 + k]) * s;
      t[j] = (m[j * 3 + i] + m[i * 3 + j]) * s;
      t[k] = (m[k * 3 + i] + m[i * 3 + k]) * s;
    }
    return Quat{t[0], t[1], t[2], t[3]};
  }

  GV_HD Basis operator*(const Basis &o) const
  {
    Basis r;
    for (int i = 0; i < 3; ++i)
      for (int j = 0; j < 3; ++j)
        r.m[i * 3 + j] = (m[i * 3 + 0] * o.m[0 * 3 + j] + m[i * 3 + 1] * o.m[1 * 3 + j]) + m[i * 3 + 2] * o.m[2 * 3 + j];
    return r;
  }
};

GV_HD Xform64 xform_from_tf(const gv_transform &t)
{
  const Basis b = Basis::from_quat(Quat{t.qx, t.qy, t.qz, t.qw});
  Xform64 x;
  for (int i = 0; i < 9; ++i) x.b[i] = b.m[i];
  x.o[0] = t.tx; x.o[1] = t.ty; x.o[2] = t.tz;
  return x;
}

// tf2::Transform::operator()(Vector3): basis[r].dot(v) + origin[r]
GV_HD void apply(const Xform64 &x, const double v[3], double out[3])
{
  for (int r = 0; r < 3; ++r) out[r] = ((x.b[r * 3] * v[0] + x.b[r * 3 + 1] * v[1]) + x.b[r * 3 + 2] * v[2]) + x.o[r];
}

// tf2::Quaternion::setRPY from the cosines and sines of the three half angles
GV_HD Quat quat_from_half_angles(double cr, double sr, double cp, double sp, double cy, double sy)
{
  return Quat{sr * cp * cy - cr * sp * sy, cr * sp * cy + sr * cp * sy, cr * cp * sy - sr * sp * cy,
              cr * cp * cy + sr * sp * sy};
}

// tf2::doTransform(Pose): Transform(t) * Transform(r, v)
GV_HD void transform_pose(const gv_transform &t, gv_lshape_pose &p)
{
  const Xform64 x = xform_from_tf(t);
  const double v[3] = {p.px, p.py, p.pz};
  double o[3];
  apply(x, v, o);
  const Basis prod = Basis::from_quat(Quat{t.qx, t.qy, t.qz, t.qw}) * Basis::from_quat(Quat{p.qx, p.qy, p.qz, p.qw});
  const Quat q = prod.to_quat();
  p.px = o[0]; p.py = o[1]; p.pz = o[2];
  p.qx = q.x; p.qy = q.y; p.qz = q.z; p.qw = q.w;
}

}  // namespace host

// ---- [EXTENSION] X15 the tick's detection list (include/gridvision_hip.h, GV_TICK_KEEP_DETS) ----
constexpr int32_t kTickDets = 128;          // records of the list
constexpr int32_t kTickDetCandidates = 16383;   // boxes of a tick (gv_tick_enqueue)

// The list as it lies in device memory: the records, then the two counts.
struct TickDetList {
  gv_lshape_pose p[kTickDets];
  int32_t n, n_total;     // records used (0 .. 128); poses found
  int32_t pad[2];
};
static_assert(sizeof(TickDetList) == 128 * 80 + 16, "no padding: the hook copies it as bytes");

// camera-frame pose of one VisionOut (vision_orientation.cpp:432-444) from cp = cos(-orient / 2), sp = sin(-orient / 2):
// setRPY(0, -orient, 0), whose roll and yaw half angles have cosine 1 and sine 0
GV_HD gv_lshape_pose tick_vision_pose(const VisionOut &vo, double cp, double sp)
{
  gv_lshape_pose p;
  p.px = vo.loc[0]; p.py = vo.loc[1]; p.pz = vo.loc[2];     // :434-436
  const host::Quat q = host::quat_from_half_angles(1.0, 0.0, cp, sp, 1.0, 0.0);   // :440
  p.qx = q.x; p.qy = q.y; p.qz = q.z; p.qw = q.w;
  p.length = vo.dims[0]; p.width = vo.dims[1]; p.height = vo.dims[2];
  return p;
}

// "empty segmented cloud": no plane, no ground point, or nothing but ground among the n points -> the reference returns {}
// (cloud_detections.cpp:307-309)
GV_HD bool tick_dets_empty(uint32_t best_count, uint64_t n_inliers, uint64_t n)
{
  const uint64_t m = best_count ? n_inliers : 0;
  return m == 0 || m == n;
}

// Candidate c of a tick is a detection iff this holds; its rank among those is its place in the list.
GV_HD bool tick_det_take(bool empty, int32_t valid) { return !empty && valid != 0; }

// Record `rank` of the list: the camera-frame pose in the base frame (transformLShapeObjects, grid_vision_node.cpp:204, :227)
GV_HD gv_lshape_pose tick_det_record(const gv_transform &tf_bc, gv_lshape_pose cam)
{
  host::transform_pose(tf_bc, cam);
  return cam;
}

// Host only: the selection in sequence.  out has room for kTickDets records.
inline void tick_dets_host(const gv_lshape_pose *cam, const uint8_t *valid, int32_t n_cand, bool empty, const gv_transform &tf_bc,
                           gv_lshape_pose *out, int32_t &n, int32_t &n_total)
{
  int32_t m = 0;
  for (int32_t c = 0; c < n_cand; ++c) {
    if (!tick_det_take(empty, valid[c])) continue;
    if (m < kTickDets) out[m] = tick_det_record(tf_bc, cam[c]);
    ++m;
  }
  n_total = m;
  n = m < kTickDets ? m : kTickDets;
  for (int32_t i = n; i < kTickDets; ++i) out[i] = gv_lshape_pose{};
}

}  // namespace gv
