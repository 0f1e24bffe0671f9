// gv_api_shortcut_host.hip -- [EXTENSION] X21: gvx3_shortcut_host, the host twin of gvx3_shortcut
// (include/gridvision_hip_shortcut.h): gv_shortcut.hpp's text in sequential loops, what the GPU tests hold the device call
// to.  No handle, nothing enqueued; plain C++17 without a HIP header, so a host compiler alone builds it too.
#include <algorithm>
#include <cstdlib>

#include "gv_shortcut.hpp"
#include "gv_host_math.hpp"

using namespace gv;

extern "C" {

// The definition in sequential loops, path by path: per anchor the candidates from the far end of the window down, each
// through shortcut_visible_chunk until it fails or ends, the first that passes taken; then the segment's sums, its cost
// maximum over line_cell's cells and its waypoints by shortcut_waypoint.
int gvx3_shortcut_host(uint8_t grid_x, uint8_t grid_y, double resolution, const uint8_t *cost, const gvx3_shortcut_config *cfg,
                       const int32_t *src_entries, const int32_t *src_n, int32_t S, int32_t cap, int32_t wcap, uint32_t flags,
                       gvx3_shortcut_info *info, int32_t *entries, int32_t *index, float *xy)
{
  if (!cost || !cfg || !src_entries || !src_n || !info || !shortcut_config_valid(*cfg) || !path_call_ok(S, cap, 0u) ||
      !shortcut_call_ok(wcap, flags) || !shortcut_room_ok(S, wcap))
    return GV_ERR_BAD_ARG;
  GridParams g{};
  if (!host::grid_params(grid_x, grid_y, resolution, g)) return GV_ERR_BAD_ARG;
  const int32_t nx = g.nx;
  for (int32_t s = 0; s < S; ++s) {
    if (src_n[s] < 0 || src_n[s] > cap) return GV_ERR_BAD_ARG;
    for (int32_t i = 0; i < src_n[s]; ++i) {
      const int32_t e = src_entries[(size_t)s * (size_t)cap + (size_t)i];
      if (e < 0 || e >= g.G) return GV_ERR_BAD_ARG;
    }
  }
  const ShortcutRule rule = shortcut_rule(*cfg, flags);
  const auto cost_at = [&](int32_t x, int32_t y) { return (uint32_t)cost[(size_t)y * (size_t)nx + (size_t)x]; };
  for (int32_t s = 0; s < S; ++s) {
    const int32_t n = src_n[s];
    gvx3_shortcut_info rec = shortcut_info_empty();
    if (n > 0) {
      const int32_t *c = src_entries + (size_t)s * (size_t)cap;
      const size_t first = (size_t)s * (size_t)wcap;
      const auto store = [&](int32_t slot, int32_t x, int32_t y, int32_t idx) {
        if (entries) entries[first + (size_t)slot] = y * nx + x;
        if (index) index[first + (size_t)slot] = idx;
        if (xy) {
          xy[2 * (first + (size_t)slot)] = path_centre(g.pos_x, g.off_x, g.res, g.nx, x);
          xy[2 * (first + (size_t)slot) + 1] = path_centre(g.pos_y, g.off_y, g.res, g.ny, y);
        }
      };
      int32_t count = 0, n_anchors = 0, n_steps = 0, n_diag = 0, end_entry = -1;
      uint32_t max_cost = 0u;
      int32_t ia = 0, pe = c[0];
      while (ia < n - 1 && count < wcap) {
        const int32_t py = pe / nx, px = pe - py * nx;
        int32_t ib = ia + 1;
        const int32_t hi = std::min(ia + rule.window, n - 1);
        if (hi >= ia + 2 && (int32_t)cost[pe] <= rule.max_cost) {
          for (int32_t j = hi; j >= ia + 2; --j) {
            const int32_t qe = c[j], qy = qe / nx, qx = qe - qy * nx;
            LineWalk w = line_walk(px, py, qx, qy);
            bool ok = true;
            bool more = w.major > 0;
            while (more) more = shortcut_visible_chunk(cost_at, rule, w, ok);
            if (ok) {
              ib = j;
              break;
            }
          }
        }
        const int32_t qe = c[ib], qy = qe / nx, qx = qe - qy * nx;
        const int32_t ddx = std::abs(qx - px), ddy = std::abs(qy - py);
        const int32_t m = std::max(ddx, ddy);
        n_steps += m;
        n_diag += std::min(ddx, ddy);
        for (int32_t i = 0; i <= m; ++i) {
          int32_t x, y;
          line_cell(px, py, qx, qy, (uint32_t)i, x, y);
          max_cost = std::max(max_cost, cost_at(x, y));
        }
        const int32_t emit = std::min(shortcut_segment_waypoints(m, rule.spacing), wcap - count);
        int32_t x = px, y = py;
        for (int32_t t = 0; t < emit; ++t) {
          shortcut_waypoint(px, py, qx, qy, rule.spacing, t, x, y);
          store(count + t, x, y, t == 0 ? ia : -1);
        }
        end_entry = y * nx + x;
        count += emit;
        n_anchors += 1;
        ia = ib;
        pe = qe;
      }
      rec.status = GVX3_SHORTCUT_TRUNCATED;
      if (ia == n - 1 && count < wcap) {
        store(count, pe % nx, pe / nx, ia);
        max_cost = std::max(max_cost, (uint32_t)cost[pe]);
        end_entry = pe;
        count += 1;
        n_anchors += 1;
        rec.status = GVX3_SHORTCUT_OK;
      }
      rec.n_waypoints = count;
      rec.n_anchors = n_anchors;
      rec.n_src = n;
      rec.n_steps = n_steps;
      rec.n_diag_steps = n_diag;
      rec.max_cost_seen = (int32_t)max_cost;
      rec.end_entry = end_entry;
    }
    info[s] = rec;
  }
  return GV_OK;
}

}  // extern "C"
