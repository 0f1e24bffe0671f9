// gv_shortcut.hip -- [EXTENSION] X21 line-of-sight shortcuts and waypoints of the resident paths (gvx3_*) and the seeds of
// gvx3_nav_field_from_shortcut.  The definition is include/gridvision_hip_shortcut.h's, the arithmetic gv_shortcut.hpp's
// (shared with the host twin).
//
// k_shortcut: one wavefront (a workgroup of 64) per resident path.  The anchor chain is sequential -- the next anchor is
// known only once this one's candidates have been tested -- and its state (the anchor, the output offset, the record's
// sums) is wave-uniform, as the walk's is in k_nav_path.
//   The search.  From anchor a the candidates a+2 .. min(a+W, n-1) are taken FAR TO NEAR in batches of 64, lane l of a
//     batch the candidate top - l.  Every lane walks its own line from c[a] by the iterator's stepping loop in registers
//     (LineWalk) against the costmap in global memory, kShortcutChunk cells per round: the round's cost bytes (three per
//     cell with GVX3_SHORTCUT_NO_CORNER) are loaded before any is looked at, so they are in flight together.  A ballot
//     after each round lets the batch leave once every lane has failed or reached its end.  The lowest passing lane of
//     the first batch with a passing lane is the largest visible j; no batch with one: a+1.  The anchor's own cell is
//     tested once, uniformly: an anchor that is not CLEAR sees nothing.
//   The segment.  Once (a, b) is known its cost maximum is taken a lane per cell of the line (line_cell's closed form),
//     64 per round and one wave_reduce at the end: for accepted segments only, no failed candidate's cells are in it.
//     Its waypoints are emitted a lane per waypoint by the closed form, 64 per round, at the wave-uniform running
//     offset: entry, index and centre (path_centre's fp64 expression, as k_nav_path's flush) as coalesced stores into
//     the resident buffers and, when the caller's way_xy is pinned, into that as well.
// k_shortcut has no atomics, no LDS and no scratch; no kernel waits for another workgroup; every store is a plain vector
// store from VGPRs.
// Not written, so no A/B exists: the 256-thread workgroup that tests four batches at once and combines them through LDS,
// and the variant that stages the CLEAR bits of a window around the anchor in LDS by wavefront ballots (X20's staging).
//
// k_nav_seeds_shortcut: k_nav_seeds_path's shape over the waypoints of a resident shortcut, the count read from its
// record on the device; launched for `wcap` threads.
// gfx950, wave64.
#include "gv_launch_shortcut.hpp"
#include "gv_device.hpp"
#include "gv_wave.hpp"

namespace gv {

namespace {
__device__ __forceinline__ int32_t uniform(int32_t v) { return __builtin_amdgcn_readfirstlane(v); }

// the cost byte of a cell on the map, per lane
struct GlobalCost {
  const uint8_t *c;
  int32_t nx;
  __device__ __forceinline__ uint32_t operator()(int32_t x, int32_t y) const { return c[(size_t)y * (size_t)nx + (size_t)x]; }
};

// where the waypoints of one path go
struct WayOut {
  int32_t *ent, *idx;
  float2 *xy, *xy_out;
};
__device__ __forceinline__ void store_waypoint(const GridParams &g, const WayOut &o, int32_t slot, int32_t x, int32_t y, int32_t index)
{
  const float2 c = make_float2(path_centre(g.pos_x, g.off_x, g.res, g.nx, x), path_centre(g.pos_y, g.off_y, g.res, g.ny, y));
  o.ent[slot] = y * g.nx + x;
  o.idx[slot] = index;
  o.xy[slot] = c;
  if (o.xy_out) o.xy_out[slot] = c;
}
}  // namespace

__global__ void __launch_bounds__(64) k_shortcut(ShortcutArgs a)
{
  const int lane = (int)threadIdx.x;
  const int32_t s = (int32_t)blockIdx.x;
  if (s >= a.S) return;
  const int32_t nx = a.g.nx, G = a.g.G;
  const int32_t n = min(max(uniform(a.src_info[s].n_cells), 0), a.cap);
  gvx3_shortcut_info rec = shortcut_info_empty();
  if (n > 0) {
    const int32_t *c = a.src_entries + (size_t)s * (size_t)a.cap;
    const size_t first = (size_t)s * (size_t)a.wcap;
    const WayOut out{a.entries + first, a.index + first, reinterpret_cast<float2 *>(a.xy) + first,
                     a.xy_out ? reinterpret_cast<float2 *>(a.xy_out) + first : nullptr};
    const GlobalCost cost{a.cost, nx};
    const int32_t W = a.rule.window, wcap = a.wcap, spacing = a.rule.spacing;
    int32_t count = 0, n_anchors = 0, n_steps = 0, n_diag = 0, end_entry = -1;
    uint32_t max_cost = 0u;
    int32_t ia = 0;                                          // the anchor, an index of the path ...
    int32_t pe = min(max(uniform(c[0]), 0), G - 1);          // ... and its entry
    while (ia < n - 1 && count < wcap) {
      const int32_t py = pe / nx, px = pe - py * nx;
      // ---- the next anchor
      int32_t ib = ia + 1;
      const int32_t hi = min(ia + W, n - 1);
      if (hi >= ia + 2 && (int32_t)a.cost[pe] <= a.rule.max_cost) {
#pragma unroll 1
        for (int32_t top = hi; top >= ia + 2; top -= 64) {
          const int32_t j = top - lane;
          const bool cand = j >= ia + 2;
          const int32_t qe = min(max(c[cand ? j : ia], 0), G - 1);   // no candidate: the anchor itself, a line of one cell
          const int32_t qy = qe / nx, qx = qe - qy * nx;
          LineWalk w = line_walk(px, py, qx, qy);
          bool ok = cand;
          bool more = ok && w.major > 0;
          while (__ballot(more) != 0ull) more = shortcut_visible_chunk(cost, a.rule, w, ok);
          const unsigned long long pass = __ballot(ok);
          if (pass != 0ull) {
            ib = top - (int32_t)__builtin_ctzll(pass);
            break;
          }
        }
      }
      // ---- the segment (ia, ib) is entered: its sums and its cost maximum
      const int32_t qe = min(max(uniform(c[ib]), 0), G - 1);
      const int32_t qy = qe / nx, qx = qe - qy * nx;
      const int32_t ddx = abs(qx - px), ddy = abs(qy - py);
      const int32_t m = max(ddx, ddy);
      n_steps += m;
      n_diag += min(ddx, ddy);
      uint32_t mc = 0u;
#pragma unroll 1
      for (int32_t i0 = 0; i0 <= m; i0 += 64) {
        const int32_t i = i0 + lane;
        if (i <= m) {
          int32_t x, y;
          line_cell(px, py, qx, qy, (uint32_t)i, x, y);
          mc = max(mc, cost(x, y));
        }
      }
      max_cost = max(max_cost, wave_reduce<OpMax>(mc));
      // ---- its waypoints, as many as there is room for
      const int32_t emit = min(shortcut_segment_waypoints(m, spacing), wcap - count);
#pragma unroll 1
      for (int32_t t0 = 0; t0 < emit; t0 += 64) {
        const int32_t t = t0 + lane;
        if (t < emit) {
          int32_t x, y;
          shortcut_waypoint(px, py, qx, qy, spacing, t, x, y);
          store_waypoint(a.g, out, count + t, x, y, t == 0 ? ia : -1);
        }
      }
      {
        int32_t x, y;
        shortcut_waypoint(px, py, qx, qy, spacing, emit - 1, x, y);
        end_entry = uniform(y * nx + x);
      }
      count += emit;
      n_anchors += 1;
      ia = ib;
      pe = qe;
    }
    rec.status = GVX3_SHORTCUT_TRUNCATED;
    if (ia == n - 1 && count < wcap) {                        // the last waypoint, c[n-1]
      if (lane == 0) store_waypoint(a.g, out, count, pe - (pe / nx) * nx, pe / nx, ia);
      max_cost = max(max_cost, (uint32_t)a.cost[pe]);
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
  if (lane == 0) {
    a.info[s] = rec;
    if (a.info_out) a.info_out[s] = rec;
  }
}

__global__ void __launch_bounds__(256) k_nav_seeds_shortcut(NavArgs a, const gvx3_shortcut_info *rec)
{
  const int i = (int)blockIdx.x * 256 + (int)threadIdx.x;
  if (i >= a.n_seeds || i >= rec->n_waypoints) return;
  const int c = a.seeds[i];
  if ((unsigned)c >= (unsigned)a.G || a.field[c] == GV_NAV_BLOCKED) return;   // (another seed's 0 is not GV_NAV_BLOCKED)
  a.field[c] = 0u;
  const int y = c / a.nx, x = c - y * a.nx;
  a.flags_out[(y / kNavTile) * a.tiles_x + x / kNavTile] = 1u;
  atomicAdd(a.counter, 1u);
}

void launch_shortcut(const ShortcutArgs &a, hipStream_t s)
{
  hipLaunchKernelGGL(k_shortcut, dim3((uint32_t)a.S), dim3(64), 0, s, a);
}

void launch_nav_seeds_shortcut(const NavArgs &a, const gvx3_shortcut_info *rec, int32_t wcap, hipStream_t s)
{
  NavArgs b = a;
  b.n_seeds = wcap;
  hipLaunchKernelGGL(k_nav_seeds_shortcut, dim3((uint32_t)((wcap + 255) / 256)), dim3(256), 0, s, b, rec);
}

}  // namespace gv
