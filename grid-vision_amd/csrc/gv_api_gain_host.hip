// gv_api_gain_host.hip -- [EXTENSION] X20: gvx2_gain_host, the host twin of gvx2_gain (include/gridvision_hip_gain.h):
// gv_gain.hpp's text in sequential loops, what the GPU tests hold the device call to.  No handle, nothing enqueued; plain
// C++17 without a HIP header, so a host compiler alone builds it too.
#include <algorithm>
#include <vector>

#include "gv_gain.hpp"
#include "gv_host_math.hpp"

using namespace gv;

extern "C" {

// The definition in sequential loops: per candidate the 8R rays in order through gain_walk, the classes read straight from
// the layer, the seen cells in a byte window of (2R + 1)^2 that is cleared cell by cell afterwards; then `best`.
int gvx2_gain_host(uint8_t grid_x, uint8_t grid_y, double resolution, const int8_t *occ_i8, const uint32_t *field,
                   const gvx2_gain_config *cfg, int32_t n, const int32_t *entries, uint32_t flags, gvx2_gain_info *info,
                   gvx2_gain_record *out)
{
  if (!occ_i8 || !cfg || !entries || !info || !out || !gain_config_valid(*cfg) || !gain_call_ok(n, flags, GVX2_GAIN_USE_FIELD))
    return GV_ERR_BAD_ARG;
  const bool use_field = (flags & GVX2_GAIN_USE_FIELD) != 0u;
  if (use_field && !field) return GV_ERR_BAD_ARG;
  GridParams g{};
  if (!host::grid_params(grid_x, grid_y, resolution, g) || !frontier_grid_ok(g.nx, g.ny)) return GV_ERR_BAD_ARG;
  try {
    const GainRule rule = gain_rule(*cfg);
    const int32_t nx = g.nx, ny = g.ny, R = rule.radius, side = 2 * R + 1;
    std::vector<uint8_t> seen((size_t)side * (size_t)side, 0);
    std::vector<int32_t> marked;
    uint64_t best = kGainNoKey;
    int32_t n_ranked = 0;
    for (int32_t k = 0; k < n; ++k) {
      const int32_t entry = entries[k];
      if (!gain_entry_valid(entry, g.G)) {
        out[k] = gain_record_invalid(entry);
        continue;
      }
      const int32_t cy = entry / nx, cx = entry - cy * nx;
      const auto cls = [&](int32_t x, int32_t y) { return frontier_class(rule.cls, occ_i8[(size_t)y * (size_t)nx + (size_t)x]); };
      GainCounts c{};
      c.nearest_opaque_d2 = kGainNoOpaque;
      marked.clear();
      for (int32_t r = 0; r < 8 * R; ++r) {
        uint32_t d2 = kGainNoOpaque;
        const int32_t end = gain_walk(
            nx, ny, cx, cy, R, r, [&](int32_t x, int32_t y) { return cls(x, y) == kFrontierNeither; },
            [&](int32_t x, int32_t y) {
              const int32_t w = (y - cy + R) * side + (x - cx + R);
              if (seen[(size_t)w]) return;
              seen[(size_t)w] = 1;
              marked.push_back(w);
              const int32_t v = cls(x, y);
              ++(v == kFrontierUnknown ? c.n_unknown : v == kFrontierFree ? c.n_free : c.n_opaque);
            },
            d2);
        ++c.rays[end];
        c.nearest_opaque_d2 = std::min(c.nearest_opaque_d2, d2);
      }
      for (const int32_t w : marked) seen[(size_t)w] = 0;
      out[k] = gain_record(rule, entry, c, use_field, use_field ? field[entry] : 0u);
      best = std::max(best, gain_best_key(out[k], k));
      n_ranked += out[k].status == 0u ? 1 : 0;
    }
    *info = gain_info(n, n_ranked, best, out, flags, R);
    return GV_OK;
  } catch (...) {
    return GV_ERR_HIP;
  }
}

}  // extern "C"
