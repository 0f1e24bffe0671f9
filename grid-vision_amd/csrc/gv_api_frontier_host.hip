// gv_api_frontier_host.hip -- [EXTENSION] X19: gvx_frontier_host, the host twin of gvx_frontier
// (include/gridvision_hip_frontier.h): gv_frontier.hpp's text in sequential loops, what the GPU tests hold the device
// call to.  No handle, nothing enqueued; plain C++17 without a HIP header, so a host compiler alone builds it too.
#include <algorithm>
#include <vector>

#include "gv_frontier.hpp"
#include "gv_host_math.hpp"

using namespace gv;

extern "C" {

// The definition in sequential loops: the frontier cells by the class test of a cell and of its four neighbours; the
// components by a flood from every frontier cell not yet labelled, in entry order, so that a component's first cell is
// its smallest entry; the records of the first `cap` clusters by plain integer arithmetic; then `best`.
int gvx_frontier_host(uint8_t grid_x, uint8_t grid_y, double resolution, const int8_t *occ_i8, const uint8_t *cost,
                      const uint32_t *field, const gvx_frontier_config *cfg, int32_t cap, uint32_t flags, gvx_frontier_info *info,
                      gvx_frontier_record *out, uint32_t *labels)
{
  if (!occ_i8 || !cfg || !info || !frontier_config_valid(*cfg) || !frontier_call_ok(cap, flags)) return GV_ERR_BAD_ARG;
  const bool use_field = (flags & GVX_FRONTIER_USE_FIELD) != 0u;
  const FrontierRule rule = frontier_rule(*cfg);
  if ((rule.max_cost < 256 && !cost) || (use_field && !field)) return GV_ERR_BAD_ARG;
  GridParams g{};
  if (!host::grid_params(grid_x, grid_y, resolution, g) || !frontier_grid_ok(g.nx, g.ny)) return GV_ERR_BAD_ARG;
  try {
    const int32_t nx = g.nx, ny = g.ny;
    const size_t G = (size_t)g.G;
    const auto unknown = [&](int32_t x, int32_t y) {
      return x >= 0 && x < nx && y >= 0 && y < ny && frontier_class(rule, occ_i8[(size_t)y * (size_t)nx + (size_t)x]) == kFrontierUnknown;
    };
    std::vector<uint32_t> lab(G, kFrontierNone);
    std::vector<uint8_t> is_frontier(G, 0);
    int32_t n_frontier = 0;
    for (int32_t y = 0; y < ny; ++y)
      for (int32_t x = 0; x < nx; ++x) {
        const size_t e = (size_t)y * (size_t)nx + (size_t)x;
        if (frontier_class(rule, occ_i8[e]) != kFrontierFree) continue;
        if (!(unknown(x - 1, y) || unknown(x + 1, y) || unknown(x, y - 1) || unknown(x, y + 1))) continue;
        if (!frontier_cost_ok(rule, cost, e)) continue;
        is_frontier[e] = 1;
        ++n_frontier;
      }

    gvx_frontier_info I{};
    I.n_frontier_cells = n_frontier;
    I.flags = flags;
    std::vector<gvx_frontier_record> recs;
    std::vector<int32_t> stack, cells;
    for (size_t e0 = 0; e0 < G; ++e0) {
      if (!is_frontier[e0] || lab[e0] != kFrontierNone) continue;
      cells.clear();
      stack.assign(1, (int32_t)e0);
      lab[e0] = (uint32_t)e0;
      while (!stack.empty()) {
        const int32_t e = stack.back();
        stack.pop_back();
        cells.push_back(e);
        const int32_t y = e / nx, x = e - y * nx;
        for (int32_t dy = -1; dy <= 1; ++dy)
          for (int32_t dx = -1; dx <= 1; ++dx) {
            const int32_t qx = x + dx, qy = y + dy;
            if (qx < 0 || qx >= nx || qy < 0 || qy >= ny) continue;
            const size_t q = (size_t)qy * (size_t)nx + (size_t)qx;
            if (!is_frontier[q] || lab[q] != kFrontierNone) continue;
            lab[q] = (uint32_t)e0;
            stack.push_back((int32_t)q);
          }
      }
      const int32_t n = (int32_t)cells.size();
      ++I.n_components;
      I.largest = std::max(I.largest, n);
      if (n < rule.min_cells) continue;
      ++I.n_clusters;
      if ((int32_t)recs.size() >= cap) continue;
      gvx_frontier_record r = frontier_record_begin((int32_t)e0, n);
      uint64_t fkey = kFrontierNoKey;
      for (const int32_t e : cells) {
        const int32_t y = e / nx, x = e - y * nx;
        r.min_x = std::min(r.min_x, x); r.max_x = std::max(r.max_x, x);
        r.min_y = std::min(r.min_y, y); r.max_y = std::max(r.max_y, y);
        r.sum_x += (uint64_t)x; r.sum_y += (uint64_t)y;
        if (use_field && field[e] < GV_NAV_UNREACHABLE) fkey = std::min(fkey, frontier_field_key(field[e], e));
      }
      const int64_t cx = (int64_t)(r.sum_x / (uint64_t)n), cy = (int64_t)(r.sum_y / (uint64_t)n);
      uint64_t ckey = kFrontierNoKey;
      for (const int32_t e : cells) {
        const int32_t y = e / nx, x = e - y * nx;
        ckey = std::min(ckey, frontier_centre_key(x, y, cx, cy, e));
      }
      frontier_record_finish(g, ckey, fkey, r);
      recs.push_back(r);
    }
    I.n_written = (int32_t)recs.size();
    uint64_t best = kFrontierNoKey;
    for (int32_t i = 0; i < I.n_written; ++i) best = std::min(best, frontier_best_key(recs[(size_t)i], i, use_field));
    I.best = frontier_best_index(best);
    *info = I;
    if (out)
      for (int32_t i = 0; i < cap; ++i) out[i] = i < I.n_written ? recs[(size_t)i] : frontier_record_zero();
    if (labels) std::copy(lab.begin(), lab.end(), labels);
    return GV_OK;
  } catch (...) {
    return GV_ERR_HIP;
  }
}

}  // extern "C"
