// gv_motion.hpp -- [EXTENSION] X10 the arithmetic of the controller loop, compiled for the host (gv_rollout_poses,
// gv_control_select) and for the device (gv_rollout.hip) from this one text, like gv_line.hpp:
//   motion_yaw, motion_increment   the yaw chain and the increments of a pose: the pieces of one step of the motion
//                    model (include/gridvision_hip.h has the definition) that k_rollout hands to different lanes;
//   motion_step      the whole step made of them, for the host twin;
//   control_total    combine and reject of one trajectory's two records (three with [EXTENSION] X13's dyn record).
// Every operation is one fp64 operation in the header's order; the build never contracts (-ffp-contract=off).
#pragma once

#include <math.h>
#include <stdint.h>

#include "gv_types.hpp"   // the public structs, GV_HD

namespace gv {

// The motion model by value: an enqueued rollout keeps the one it was enqueued with.
struct MotionModel {
  int32_t model;   // GV_MOTION_DIFF / GV_MOTION_OMNI
  double dt;
};

GV_HD int32_t motion_controls(int32_t model) { return model == GV_MOTION_OMNI ? 3 : 2; }   // C: floats per step

// T = T + w * dt: w is the last of a step's controls in both models
GV_HD double motion_yaw(const MotionModel &m, const float *u, double T)
{
  const double w = (double)u[motion_controls(m.model) - 1];
  return T + w * m.dt;
}

// what the step adds to X and Y, given cos / sin of the yaw BEFORE the step
GV_HD void motion_increment(const MotionModel &m, const float *u, double c, double s, double &ix, double &iy)
{
  if (m.model == GV_MOTION_OMNI) {
    const double a = (double)u[0] * m.dt, b = (double)u[1] * m.dt;
    ix = a * c - b * s;
    iy = a * s + b * c;
  } else {
    const double d = (double)u[0] * m.dt;
    ix = d * c;
    iy = d * s;
  }
}

// One whole step of the state (X, Y, T), as the definition writes it.  Host only (gv_rollout_poses): k_rollout composes
// the same three pieces itself, around its own sincos, because it hands them to different lanes.
inline void motion_step(const MotionModel &m, const float *u, double &X, double &Y, double &T)
{
  double ix, iy;
  const double c = cos(T), s = sin(T);
  motion_increment(m, u, c, s, ix, iy);
  X = X + ix;
  Y = Y + iy;
  T = motion_yaw(m, u, T);
}

// ---- combine and reject
GV_HD bool critic_nav_used(const gv_critic_weights &w) { return (w.w_nav_last | w.w_nav_sum | w.w_nav_best) != 0u; }

// The largest total of an admitted trajectory: every weight 65535, P = 4096 poses of cost 255 (cost_sum, max_cost) on
// field values of 0xFFFFFFFD, the largest below the two sentinels (sum over 4096 poses, last, best):
//   65535 * (4096 * 255 + 255 + (4096 + 2) * 0xFFFFFFFD) = 1.1535e18 < 2^61 = 2.3058e18
// [EXTENSION] X13 adds the dyn record's two terms, at most 65535 * (4096 * 255 + 255) more: 1.1535e18 still.
static_assert(65535ull * (4096ull * 255ull + 255ull + (4096ull + 2ull) * 0xFFFFFFFDull) + 65535ull * (4096ull * 255ull + 255ull) <
                  (1ull << 61),
              "an admitted total stays below 2^61, far from UINT64_MAX, the mark of a rejected trajectory");

// false: the trajectory is rejected (it collides, or a nav weight is set and a pose is not good, or a dyn configuration
// is set and a pose collides with a moving object); else its total.  nav may be null when no nav weight is set, dyn is
// null when no dyn configuration is set (w_dyn_sum, w_dyn_max are not read then).  With n_bad == 0 last and best are
// field values, never a sentinel.
GV_HD bool control_total(const gv_critic_weights &w, bool nav_used, const gv_traj_score &t, const gv_nav_score *nav,
                         const gv_dyn_score *dyn, uint32_t w_dyn_sum, uint32_t w_dyn_max, uint64_t &total)
{
  if (t.first_collision >= 0) return false;
  uint64_t v = (uint64_t)w.w_cost_sum * (uint64_t)t.cost_sum + (uint64_t)w.w_max_cost * (uint64_t)(uint32_t)t.max_cost;
  if (nav_used) {
    if (nav->n_bad > 0) return false;
    v += (uint64_t)w.w_nav_last * (uint64_t)nav->last + (uint64_t)w.w_nav_sum * nav->sum + (uint64_t)w.w_nav_best * (uint64_t)nav->best;
  }
  if (dyn) {
    if (dyn->first_collision >= 0) return false;
    v += (uint64_t)w_dyn_sum * (uint64_t)dyn->cost_sum + (uint64_t)w_dyn_max * (uint64_t)(uint32_t)dyn->max_cost;
  }
  total = v;
  return true;
}

// (total, k) of an admitted trajectory against the best so far (best_k < 0: none yet): the lexicographic minimum, which
// does not depend on the order the trajectories are visited in
GV_HD void control_take(uint64_t total, int32_t k, uint64_t &best_total, int32_t &best_k)
{
  if (k >= 0 && (best_k < 0 || total < best_total || (total == best_total && k < best_k))) {
    best_total = total;
    best_k = k;
  }
}

}  // namespace gv
