// gv_mppi.hpp -- [EXTENSION] X11 the arithmetic of an MPPI iteration's two ends, compiled for the host (gv_mppi_words,
// gv_mppi_sample_controls, gv_mppi_average) and for the device (gv_mppi.hip) from this one text, like gv_motion.hpp:
//   philox4x32_10    the Random123 counter function: four random words of (counter, key), no state;
//   mppi_sample      one pose's controls: the words of (k, p, iteration | seed), Box-Muller, the nominal step, the clamp;
//   mppi_weight      one trajectory's softmax weight from its total and the best total;
//   mppi_chunk_rows, mppi_tile_cols   the fixed shape of the device's two-stage average, a function of (K, P * C) alone;
//   [EXTENSION] X12: mppi_chain, mppi_constrain_step   the rate and turning-radius limits on a sampled sequence (float32);
//   mppi_cost_lane, mppi_cost_x, mppi_weight_cc, mppi_min_key   the control cost and the weights with it.
// Every operation is one fp64 operation in the header's order (include/gridvision_hip.h has the definition); the build
// never contracts (-ffp-contract=off).  log, sin, cos and exp are the device library's on the device and the C library's
// on the host.
#pragma once

#include <math.h>
#include <stdint.h>

#include "gv_types.hpp"   // the public structs, GV_HD

namespace gv {

GV_HD void philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1, uint32_t r[4])
{
  for (int round = 0; round < 10; ++round) {
    const uint64_t p0 = (uint64_t)0xD2511F53u * (uint64_t)c0;
    const uint64_t p1 = (uint64_t)0xCD9E8D57u * (uint64_t)c2;
    const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0;
    const uint32_t n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
    c1 = (uint32_t)p1;
    c3 = (uint32_t)p0;
    c0 = n0;
    c2 = n2;
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
  r[0] = c0; r[1] = c1; r[2] = c2; r[3] = c3;
}

// the words of pose (k, p): counter (k, p, iteration_lo, iteration_hi), key (seed_lo, seed_hi)
GV_HD void mppi_words(uint64_t seed, uint64_t iteration, uint32_t k, uint32_t p, uint32_t r[4])
{
  philox4x32_10(k, p, (uint32_t)iteration, (uint32_t)(iteration >> 32), (uint32_t)seed, (uint32_t)(seed >> 32), r);
}

GV_HD double mppi_uniform(uint32_t r) { return ((double)r + 0.5) * 2.3283064365386963e-10; }   // 2^-32: never 0 or 1

// controls[k][p][0..C) of one pose into f.  nominal is [P][C]; trajectory 0 is the nominal itself.
GV_HD void mppi_sample(const gv_mppi_config &cfg, int32_t C, const float *nominal, int32_t P, uint64_t seed, uint64_t iteration,
                       bool shift, uint32_t k, uint32_t p, float *f)
{
  int32_t pn = (int32_t)p;
  if (shift) pn = pn + 1 < P - 1 ? pn + 1 : P - 1;
  const float *nom = nominal + (size_t)pn * (size_t)C;
  double z[3] = {0.0, 0.0, 0.0};
  if (k != 0u) {
    uint32_t r[4];
    mppi_words(seed, iteration, k, p, r);
    const double R = sqrt(-2.0 * log(mppi_uniform(r[0])));
    const double A = 6.283185307179586 * mppi_uniform(r[1]);
    z[0] = R * cos(A);
    z[1] = R * sin(A);
    if (C == 3) {
      const double R2 = sqrt(-2.0 * log(mppi_uniform(r[2])));
      const double A2 = 6.283185307179586 * mppi_uniform(r[3]);
      z[2] = R2 * cos(A2);
    }
  }
  for (int32_t c = 0; c < C; ++c) {
    const double v = k != 0u ? (double)nom[c] + cfg.sigma[c] * z[c] : (double)nom[c];
    float q = (float)v;
    q = q < cfg.u_min[c] ? cfg.u_min[c] : q;
    q = q > cfg.u_max[c] ? cfg.u_max[c] : q;
    f[c] = q;
  }
}

// e_k of an admitted trajectory (total != UINT64_MAX, best_total the smallest admitted total)
GV_HD double mppi_weight(uint64_t total, uint64_t best_total, double lambda)
{
  const double x = (double)(total - best_total);
  return exp(-(x / lambda));
}

// ---- [EXTENSION] X12: limits on the sampled controls and the control-cost term (gv_set_mppi_limits).
// What a sampling makes of a gv_mppi_limits with the model's dt, once per call on the host (MppiChain, gv_types.hpp).
GV_HD MppiChain mppi_chain(const gv_mppi_limits &lim, double dt)
{
  MppiChain L;
  for (int c = 0; c < 3; ++c) {
    L.up[c] = (float)(lim.rate_up[c] * dt);
    L.dn[c] = (float)(lim.rate_down[c] * dt);
    L.u_prev[c] = lim.u_prev[c];
  }
  L.inv_r = lim.min_turn_radius > 0.0 ? (float)(1.0 / lim.min_turn_radius) : 0.0f;
  return L;
}

// can the chain change a control of the first C channels at all?  (+inf rates both ways and no radius: it cannot)
GV_HD bool mppi_chain_active(const MppiChain &L, int32_t C)
{
  bool on = L.inv_r > 0.0f;
  for (int32_t c = 0; c < C; ++c) on = on || L.up[c] < INFINITY || L.dn[c] < INFINITY;
  return on;
}

// One step of the chain: q holds f[p][0..C) and leaves as controls[k][p][0..C); s is the step before it (u_prev in
// front of step 0; NaN: that channel is free) and leaves as q.  Every operation one float32 operation, no library call.
GV_HD void mppi_constrain_step(const MppiChain &L, int32_t C, float *s, float *q)
{
  for (int32_t c = 0; c < 3; ++c) {   // a constant trip count: s and q stay in registers on the device
    if (c < C) {
      // "if s[c] is not NaN" needs no branch: from a NaN s both bounds are NaN, both compares false, q stays
      const float lo = s[c] - L.dn[c];
      const float hi = s[c] + L.up[c];
      q[c] = q[c] < lo ? lo : q[c];
      q[c] = q[c] > hi ? hi : q[c];
    }
  }
  if (L.inv_r > 0.0f) {
    const float b = fabsf(q[0]) * L.inv_r;
    q[1] = q[1] < -b ? -b : q[1];
    q[1] = q[1] > b ? b : q[1];
  }
  for (int32_t c = 0; c < 3; ++c)
    if (c < C) s[c] = q[c];
}

// The control cost g_k is a sum of J = P * C terms in a fixed order: 64 partial sums a_l over j = l, l + 64, ..
// (ascending), then the tree a_l += a_(l + w), w = 32 .. 1.  On the device lane l of a wavefront holds a_l.
constexpr int kMppiCostLanes = 64;

// q_c of the definition: gamma / sigma^2, 0 for a channel without noise
GV_HD double mppi_cost_scale(double gamma, double sigma) { return sigma > 0.0 ? gamma / (sigma * sigma) : 0.0; }

// term_j of trajectory row u ([P][C]) around the nominal the sampling read
GV_HD double mppi_cost_term(const double qc[3], int32_t C, const float *nominal, int32_t P, bool shift, const float *u, int32_t j)
{
  const int32_t p = j / C, c = j - p * C;
  int32_t pn = p;
  if (shift) pn = pn + 1 < P - 1 ? pn + 1 : P - 1;
  const double n = (double)nominal[(size_t)pn * (size_t)C + (size_t)c];
  const double q = c == 0 ? qc[0] : c == 1 ? qc[1] : qc[2];
  return q * (n * ((double)u[j] - n));
}

// a_l of the definition
GV_HD double mppi_cost_lane(const double qc[3], int32_t C, const float *nominal, int32_t P, bool shift, const float *u, int32_t l)
{
  const int32_t J = P * C;
  double a = 0.0;
  for (int32_t j = l; j < J; j += kMppiCostLanes) a = a + mppi_cost_term(qc, C, nominal, P, shift, u, j);
  return a;
}

// e_k with the control cost: x_k = (double)(total_k - best_total) + g_k, m the smallest x of the admitted
GV_HD double mppi_cost_x(uint64_t total, uint64_t best_total, double g) { return (double)(total - best_total) + g; }
GV_HD double mppi_weight_cc(double x, double m, double lambda) { return exp(-((x - m) / lambda)); }

// An order-preserving 64-bit key of a double (no NaN): a < b as doubles implies key(a) < key(b) as unsigned integers
// (-0 sorts below +0), so an integer minimum over keys is the minimum over the doubles, in any order.
GV_HD uint64_t mppi_min_key(double x)
{
  union { double d; uint64_t u; } v;
  v.d = x;
  return (v.u >> 63) ? ~v.u : v.u | 0x8000000000000000ull;
}
GV_HD double mppi_min_unkey(uint64_t key)
{
  union { double d; uint64_t u; } v;
  v.u = (key >> 63) ? key & 0x7FFFFFFFFFFFFFFFull : ~key;
  return v.d;
}

// ---- the shape of the device's average (k_mppi_partial / k_mppi_finish), fixed by (K, J = P * C) alone.
// A workgroup of kMppiThreads owns mppi_chunk_rows trajectories and mppi_tile_cols columns: its threads are
// kMppiThreads / tile row groups of `tile` columns, row group s adds rows s, s + groups, .. of the chunk in that order,
// and the groups' sums are added in group order.  k_mppi_finish adds the chunks' partials in chunk order.
constexpr int kMppiThreads = 256;
constexpr int kMppiChunkMax = 64;

GV_HD int32_t mppi_tile_cols(int64_t J)
{
  int32_t t = 16;
  while (t < kMppiThreads && (int64_t)t < J) t *= 2;
  return t;
}

// the largest of 64, 32, 16, 8 rows (not below the row groups of a workgroup) that still gives 256 workgroups, else
// the smallest: K = 2000, J = 112 -> 8 rows, 250 workgroups; K = 250, J = 40 -> 8 rows, 32 workgroups
GV_HD int32_t mppi_chunk_rows(int32_t K, int64_t J)
{
  const int32_t tile = mppi_tile_cols(J);
  const int32_t groups = kMppiThreads / tile;
  const int64_t tiles = (J + tile - 1) / tile;
  const int32_t lo = groups > 8 ? groups : 8;
  int32_t rows = kMppiChunkMax;
  while (rows > lo && (((int64_t)K + rows - 1) / rows) * tiles < 256) rows /= 2;
  return rows;
}

}  // namespace gv
