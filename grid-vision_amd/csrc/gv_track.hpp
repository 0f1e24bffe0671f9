// gv_track.hpp -- [EXTENSION] X14 the arithmetic of the multi-object tracker over the tick's boxes, compiled for the
// host (gv_track_step) and for the device (gv_track.hip) from this one text, like gv_dyn.hpp:
//   track_params, track_ego       what one update computes once from the configuration and the motion;
//   track_move, track_predict     steps 1 and 2 on one live track;
//   track_det_valid, track_d2     steps 3 and 4: a detection's validity, a pair's squared distance;
//   track_match, track_miss, track_birth   steps 5 to 7 on one slot;
//   track_exported, track_export  step 8: whether a track leaves, and as what;
//   track_step                    host only: the eight steps in sequence, the association as a literal sort.
// Every operation is one fp64 operation in the header's order (include/gridvision_hip.h has the definition); the build
// never contracts (-ffp-contract=off).
#pragma once

#include <math.h>
#include <stdint.h>

#include <algorithm>
#include <vector>

#include "gv_dyn.hpp"   // dyn_object: the row an exported track becomes

namespace gv {

constexpr int32_t kTrackSlots = 128;
static_assert(sizeof(gv_track) == 128 && sizeof(gv_track_info) == 40, "the X14 records");
static_assert(kTrackSlots == kDynMaxObjects, "every exported track has a row in X13's table");

// What a kernel launch carries of a gv_track_config, by value.
struct TrackParams {
  double q, r, v0, gate2, min2;
  int32_t confirm_hits, max_misses;
};

// base_prev <- base_now as the tracks read it: the yaw terms and the translation, and the conjugate quaternion
struct TrackEgo {
  int32_t on;
  double ce, se, tx, ty;
  double ax, ay, az, aw;
};

GV_HD bool track_finite(double v) { return v - v == 0.0; }   // false for NaN and both infinities

GV_HD bool track_config_valid(const gv_track_config &c)
{
  return track_finite(c.gate) && c.gate > 0.0 && track_finite(c.sigma_accel) && c.sigma_accel >= 0.0 &&
         track_finite(c.sigma_meas) && c.sigma_meas > 0.0 && track_finite(c.sigma_v0) && c.sigma_v0 >= 0.0 &&
         track_finite(c.min_speed) && c.min_speed >= 0.0 && c.confirm_hits >= 1 && c.confirm_hits <= 255 &&
         c.max_misses >= 0 && c.max_misses <= 255 && c.flags == 0u;
}

GV_HD TrackParams track_params(const gv_track_config &c)
{
  TrackParams p;
  p.q = c.sigma_accel * c.sigma_accel;
  p.r = c.sigma_meas * c.sigma_meas;
  p.v0 = c.sigma_v0 * c.sigma_v0;
  p.gate2 = c.gate * c.gate;
  p.min2 = c.min_speed * c.min_speed;
  p.confirm_hits = c.confirm_hits;
  p.max_misses = c.max_misses;
  return p;
}

GV_HD TrackEgo track_ego(const gv_transform *m)
{
  TrackEgo e{};
  if (!m) return e;
  e.on = 1;
  e.ce = 1.0 - 2.0 * (m->qy * m->qy + m->qz * m->qz);
  e.se = 2.0 * (m->qw * m->qz + m->qx * m->qy);
  e.tx = m->tx; e.ty = m->ty;
  e.ax = -m->qx; e.ay = -m->qy; e.az = -m->qz; e.aw = m->qw;
  return e;
}

GV_HD int32_t track_inc(int32_t v) { return v < INT32_MAX ? v + 1 : v; }

// The state, on the device and in the host twin alike: slot s is live iff live[s] != 0; a dead slot's record is not read.
struct TrackState {
  gv_track t[kTrackSlots];
  int32_t live[kTrackSlots];
  uint32_t next_id, reserved;
};
static_assert(sizeof(TrackState) == 128 * 128 + 128 * 4 + 8, "no padding: the block is copied as bytes");

// step 1
GV_HD void track_move(const TrackEgo &e, gv_track &t)
{
  const double dx = t.x - e.tx, dy = t.y - e.ty;
  t.x = e.ce * dx + e.se * dy;
  t.y = e.ce * dy - e.se * dx;
  const double vx = e.ce * t.vx + e.se * t.vy, vy = e.ce * t.vy - e.se * t.vx;
  t.vx = vx; t.vy = vy;
  const double bx = t.qx, by = t.qy, bz = t.qz, bw = t.qw;
  t.qw = e.aw * bw - e.ax * bx - e.ay * by - e.az * bz;
  t.qx = e.aw * bx + e.ax * bw + e.ay * bz - e.az * by;
  t.qy = e.aw * by - e.ax * bz + e.ay * bw + e.az * bx;
  t.qz = e.aw * bz + e.ax * by - e.ay * bx + e.az * bw;
}

// step 2
GV_HD void track_predict(const TrackParams &p, double dt, gv_track &t)
{
  const double dt2 = dt * dt;
  t.x = t.x + t.vx * dt;
  t.y = t.y + t.vy * dt;
  const double p00 = ((t.p00 + (2.0 * dt) * t.p01) + dt2 * t.p11) + p.q * (0.25 * (dt2 * dt2));
  const double p01 = (t.p01 + dt * t.p11) + p.q * (0.5 * (dt2 * dt));
  const double p11 = t.p11 + p.q * dt2;
  t.p00 = p00; t.p01 = p01; t.p11 = p11;
  t.age = track_inc(t.age);
  t.det = -1;
}

// step 3
GV_HD bool track_det_valid(const gv_lshape_pose &d)
{
  return track_finite(d.px) && track_finite(d.py) && track_finite(d.qx) && track_finite(d.qy) && track_finite(d.qz) &&
         track_finite(d.qw) && track_finite(d.length) && track_finite(d.width) && d.length >= 0.0 && d.width >= 0.0;
}

// step 4: the pair is a candidate iff this is <= gate2 (a NaN fails)
GV_HD double track_d2(double x, double y, double px, double py)
{
  const double ex = px - x, ey = py - y;
  return ex * ex + ey * ey;
}

// step 5
GV_HD void track_match(const TrackParams &p, const gv_lshape_pose &z, int32_t d, gv_track &t)
{
  const double ex = z.px - t.x, ey = z.py - t.y;
  const double S = t.p00 + p.r, k0 = t.p00 / S, k1 = t.p01 / S;
  t.x = t.x + k0 * ex; t.vx = t.vx + k1 * ex;
  t.y = t.y + k0 * ey; t.vy = t.vy + k1 * ey;
  const double p11 = t.p11 - k1 * t.p01, p01 = t.p01 - k1 * t.p00, p00 = t.p00 - k0 * t.p00;
  t.p00 = p00; t.p01 = p01; t.p11 = p11;
  t.qx = z.qx; t.qy = z.qy; t.qz = z.qz; t.qw = z.qw;
  t.length = z.length; t.width = z.width;
  t.hits = track_inc(t.hits);
  t.misses = 0;
  t.det = d;
}

// step 6: true when the slot is freed
GV_HD bool track_miss(const TrackParams &p, gv_track &t)
{
  t.misses = track_inc(t.misses);
  return t.misses > p.max_misses;
}

// step 7
GV_HD gv_track track_birth(const TrackParams &p, const gv_lshape_pose &z, int32_t d, uint32_t id, int32_t slot)
{
  gv_track t;
  t.id = id; t.slot = slot; t.hits = 1; t.misses = 0; t.age = 0; t.det = d;
  t.x = z.px; t.y = z.py; t.vx = 0.0; t.vy = 0.0;
  t.qx = z.qx; t.qy = z.qy; t.qz = z.qz; t.qw = z.qw;
  t.length = z.length; t.width = z.width;
  t.p00 = p.r; t.p01 = 0.0; t.p11 = p.v0;
  return t;
}

// step 8
GV_HD bool track_confirmed(const TrackParams &p, const gv_track &t) { return t.hits >= p.confirm_hits; }
GV_HD bool track_exported(const TrackParams &p, const gv_track &t)
{
  return track_confirmed(p, t) && track_finite(t.x) && track_finite(t.y) && track_finite(t.vx) && track_finite(t.vy);
}
GV_HD gv_moving_object track_export(const TrackParams &p, const gv_track &t)
{
  const double sp2 = t.vx * t.vx + t.vy * t.vy;
  const bool still = sp2 < p.min2;
  gv_moving_object m;
  m.pose.px = t.x; m.pose.py = t.y; m.pose.pz = 0.0;
  m.pose.qx = t.qx; m.pose.qy = t.qy; m.pose.qz = t.qz; m.pose.qw = t.qw;
  m.pose.length = t.length; m.pose.width = t.width; m.pose.height = 0.0;
  m.vx = still ? 0.0 : t.vx;
  m.vy = still ? 0.0 : t.vy;
  return m;
}

// Host only.  One update, steps 1 to 8 in sequence (n in 0..128, dt and the motion checked by the caller).  objs (room for 128) and
// n_objs may be null together; info may be null.
inline void track_step(const TrackParams &p, TrackState &st, const gv_lshape_pose *dets, int32_t n, double dt,
                       const gv_transform *motion, gv_track_info *info, gv_moving_object *objs, int32_t *n_objs)
{
  const TrackEgo ego = track_ego(motion);
  for (int32_t s = 0; s < kTrackSlots; ++s)
    if (st.live[s]) {
      if (ego.on) track_move(ego, st.t[s]);
      track_predict(p, dt, st.t[s]);
    }
  bool valid[kTrackSlots];
  int32_t n_invalid = 0;
  for (int32_t d = 0; d < n; ++d) {
    valid[d] = track_det_valid(dets[d]);
    n_invalid += valid[d] ? 0 : 1;
  }
  struct Cand {
    double d2;
    int32_t s, d;
  };
  std::vector<Cand> cand;
  for (int32_t s = 0; s < kTrackSlots; ++s)
    if (st.live[s])
      for (int32_t d = 0; d < n; ++d)
        if (valid[d]) {
          const double d2 = track_d2(st.t[s].x, st.t[s].y, dets[d].px, dets[d].py);
          if (d2 <= p.gate2) cand.push_back({d2, s, d});
        }
  std::sort(cand.begin(), cand.end(), [](const Cand &a, const Cand &b) {
    return a.d2 < b.d2 || (a.d2 == b.d2 && (a.s < b.s || (a.s == b.s && a.d < b.d)));
  });
  int32_t of_slot[kTrackSlots], of_det[kTrackSlots];
  for (int32_t i = 0; i < kTrackSlots; ++i) of_slot[i] = of_det[i] = -1;
  int32_t n_matched = 0, n_deleted = 0, n_born = 0, n_dropped = 0;
  for (const Cand &c : cand)
    if (of_slot[c.s] < 0 && of_det[c.d] < 0) {
      of_slot[c.s] = c.d;
      of_det[c.d] = c.s;
      ++n_matched;
    }
  for (int32_t s = 0; s < kTrackSlots; ++s)
    if (st.live[s]) {
      if (of_slot[s] >= 0) track_match(p, dets[of_slot[s]], of_slot[s], st.t[s]);
      else if (track_miss(p, st.t[s])) {
        st.live[s] = 0;
        ++n_deleted;
      }
    }
  int32_t free_from = 0;
  for (int32_t d = 0; d < n; ++d)
    if (valid[d] && of_det[d] < 0) {
      while (free_from < kTrackSlots && st.live[free_from]) ++free_from;
      if (free_from == kTrackSlots) {
        ++n_dropped;
        continue;
      }
      st.t[free_from] = track_birth(p, dets[d], d, st.next_id++, free_from);
      st.live[free_from] = 1;
      ++n_born;
    }
  int32_t n_tracks = 0, n_confirmed = 0, n_exported = 0;
  for (int32_t s = 0; s < kTrackSlots; ++s)
    if (st.live[s]) {
      ++n_tracks;
      n_confirmed += track_confirmed(p, st.t[s]) ? 1 : 0;
      if (track_exported(p, st.t[s])) {
        if (objs) objs[n_exported] = track_export(p, st.t[s]);
        ++n_exported;
      }
    }
  if (n_objs) *n_objs = n_exported;
  if (info) {
    info->n_tracks = n_tracks; info->n_confirmed = n_confirmed; info->n_exported = n_exported;
    info->n_matched = n_matched; info->n_born = n_born; info->n_deleted = n_deleted;
    info->n_dropped = n_dropped; info->n_invalid = n_invalid;
    info->next_id = st.next_id; info->reserved = 0u;
  }
}

}  // namespace gv
