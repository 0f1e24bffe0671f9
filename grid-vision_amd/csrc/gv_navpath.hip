// gv_navpath.hip -- [EXTENSION] X17 path extraction from the distance field of X9 (gv_nav_path*) and the seeds of
// gv_nav_field_from_path.  The definition is include/gridvision_hip_path.h's, the arithmetic gv_navpath.hpp's (shared
// with the host twin).
//
// k_nav_path: one wavefront (a workgroup of 64) per start.  A descent is a chain of dependent reads: the next cell is
// known only once the neighbours of this one have been compared.  The walk's state -- the cell, its value, the last
// move -- is wave-uniform.  A step reads its eight neighbours first, all in flight together, and decides by compares
// and selects (path_next).  Measured, a wavefront that takes ONE such step per round is bound by instruction issue
// (some 150 instructions of a single wavefront), not by the reads: 420 to 530 ns a step whether they came from an LDS
// window or from global memory (profiles/x17/nav_path_time.txt, "one step per round").  So the 64 lanes take up to 64
// steps per round: lane i evaluates path_next, the same text, at the cell i moves ahead in the direction of the last
// move.  A distance field's paths are runs of equal moves; the leading lanes that all repeat the last move ARE the
// walk's next cells (lane i's cell is on the path iff lanes 0 .. i - 1 repeat the move), a ballot counts them, and the
// round advances that far.  A round whose lane 0 does not repeat the move takes lane 0's step alone and turns: every
// round advances at least one cell, and the result is the sequential walk's, cell for cell.
// Path cells collect in a 128-entry LDS buffer that all lanes flush 64 at a time, a lane per cell: the entry and its
// centre (the fp64 expression of the header, evaluated in the flush) as coalesced stores into the resident buffers and,
// when the caller's paths_xy is pinned, into that as well.  A start that walks nowhere (off the map, blocked,
// unreachable) writes its record and nothing else.  No kernel waits for another workgroup; k_nav_path has no atomics
// and no scratch; every store is a plain vector store from VGPRs.
//
// Where the reads come from.  The shipped form reads the field straight from global memory: a round's 9 loads per
// lane are in flight together, so a round costs one round trip to L2 or HBM for up to 64 cells.  The other form
// (-DGV_PATH_WINDOW, built by tools/nav_path_time.py alone) first loads a kPathWindow x kPathWindow square of the field
// into LDS -- every lane four cells of a row per vector load, 16 loads a lane all issued before the first is waited
// for, the square placed AHEAD of the walk (one cell behind the current one and 62 ahead on an axis the walk has moved
// along since the last window), shifted onto the map and clipped where the map is smaller -- and walks inside it,
// loading a new one when the 3 x 3 neighbourhood of the current cell would leave it.  It was the design this kernel
// started from, when a step per round made the chain of reads look like the cost.  With 64 steps per round it loses
// by a factor of two (70 against 31 us on the empty 2000^2 map, 158 against 64 us through the gap, 334 against 167 us
// down the serpentine): a window is a round trip to memory of its own in front of every run of at most 62 cells, and
// the direct round needs only the one it has anyway.  kPathWindow = 64: at 32 a window buys 30 cells, at 128 its 64 KB
// are 64 loads a lane.
//
// k_nav_seeds_path: k_nav_seeds of gv_navfield.hip over the cells of a resident path, the count read from its record on
// the device; launched for `cap` threads.
// gfx950, wave64.
#include "gv_launch_planner.hpp"
#include "gv_device.hpp"

namespace gv {

namespace {
constexpr int kPathWindow = 64;   // side of the LDS window, in cells
constexpr int kW = kPathWindow;
constexpr int kFlush = 64;        // cells per flush: a lane per cell
constexpr uint32_t kBlocked = GV_NAV_BLOCKED;
static_assert(kW % 16 == 0 && (kW / 4) * 4 == kW && 64 % (kW / 4) == 0, "a lane loads four cells, whole rows per round");

struct __attribute__((packed, aligned(4))) Cells4 {
  uint32_t v[4];
};

__device__ __forceinline__ uint32_t uniform(uint32_t v) { return (uint32_t)__builtin_amdgcn_readfirstlane((int)v); }

// The field at a cell of the window (the -DGV_PATH_WINDOW build), per lane.  path_next also asks for cells one step off the map, which lie outside
// a window that ends at the map's edge, and lanes whose cell takes no part ask for anything: the address is clamped
// into the window and what is read there is not looked at.
struct WindowField {
  const uint32_t *w;
  int32_t x0, y0;
  __device__ __forceinline__ uint32_t operator()(int32_t x, int32_t y) const
  {
    return w[min(max(y - y0, 0), kW - 1) * kW + min(max(x - x0, 0), kW - 1)];
  }
};
// ... and straight from global memory (the shipped form), clamped into the map likewise
struct GlobalField {
  const uint32_t *f;
  int32_t nx, ny;
  __device__ __forceinline__ uint32_t operator()(int32_t x, int32_t y) const
  {
    return f[min(max(y, 0), ny - 1) * nx + min(max(x, 0), nx - 1)];
  }
};

// Where a new window begins on one axis of n cells, for the current cell c that came from `from` since the last window
// was loaded: a walk that moved up the axis keeps one cell behind it and kW - 2 ahead, one that moved down the
// reverse, one that did not move (and the first window) sits in the middle; then shifted onto the map.
__device__ __forceinline__ int32_t window_origin(int32_t c, int32_t from, int32_t n)
{
  const int32_t behind = c > from ? 1 : (c < from ? kW - 2 : kW / 2);
  return min(max(c - behind, 0), max(n - kW, 0));
}

// the kW x kW cells from (x0, y0) into win; off the map: blocked.  Every address read is a map cell's.
__device__ __forceinline__ void load_window(const uint32_t *field, int32_t nx, int32_t ny, int32_t x0, int32_t y0, uint32_t *win, int lane)
{
  constexpr int kPerRow = kW / 4, kRows = 64 / kPerRow, kBatch = 16;   // the whole window in one round of loads
  static_assert((kW / kRows) % kBatch == 0, "whole batches");
  const int col = 4 * (lane % kPerRow), gx = x0 + col;
  const bool whole = gx + 3 < nx;
#pragma unroll 1
  for (int r0 = 0; r0 < kW; r0 += kRows * kBatch) {
    uint4 q[kBatch];
#pragma unroll
    for (int j = 0; j < kBatch; ++j) {
      const int gy = y0 + r0 + j * kRows + lane / kPerRow;
      const bool row_ok = gy < ny;
      const uint32_t *p = field + (size_t)gy * (size_t)nx + (size_t)gx;
      if (row_ok && whole) {
        const Cells4 c = *reinterpret_cast<const Cells4 *>(p);
        q[j] = make_uint4(c.v[0], c.v[1], c.v[2], c.v[3]);
      } else {
        q[j].x = row_ok && gx + 0 < nx ? p[0] : kBlocked;
        q[j].y = row_ok && gx + 1 < nx ? p[1] : kBlocked;
        q[j].z = row_ok && gx + 2 < nx ? p[2] : kBlocked;
        q[j].w = row_ok && gx + 3 < nx ? p[3] : kBlocked;
      }
    }
#pragma unroll
    for (int j = 0; j < kBatch; ++j)
      *reinterpret_cast<uint4 *>(&win[(r0 + j * kRows + lane / kPerRow) * kW + col]) = q[j];
  }
}

__device__ __forceinline__ int32_t lane_value(int32_t v, int32_t from) { return __builtin_amdgcn_readlane(v, from); }

// The first min(pending, 64) collected cells become cells base .. of the path, a lane per cell; what was collected
// beyond them moves to the front of the buffer.  Returns how many cells left the buffer.
__device__ __forceinline__ int32_t flush(const PathArgs &a, int32_t *cells, int32_t *ent, float2 *xy, float2 *xy_out, int32_t base,
                                         int32_t pending, int lane)
{
  const int32_t count = min(pending, kFlush), rest = pending - count;
  __syncthreads();
  const int32_t e = cells[lane], tail = cells[kFlush + lane];
  __syncthreads();
  if (lane < rest) cells[lane] = tail;
  if (lane < count) {
    const int32_t cy = e / a.g.nx, cx = e - cy * a.g.nx;
    const float2 c = make_float2(path_centre(a.g.pos_x, a.g.off_x, a.g.res, a.g.nx, cx),
                                 path_centre(a.g.pos_y, a.g.off_y, a.g.res, a.g.ny, cy));
    ent[base + lane] = e;
    xy[base + lane] = c;
    if (xy_out) xy_out[base + lane] = c;
  }
  __syncthreads();
  return count;
}
}  // namespace

__global__ void __launch_bounds__(64) k_nav_path(PathArgs a)
{
#ifdef GV_PATH_WINDOW
  __shared__ uint32_t win_s[kW * kW];
#endif
  __shared__ int32_t cells_s[2 * kFlush];   // collected cells not yet flushed: fewer than 64 before a round, at most 127 after it
  const int lane = (int)threadIdx.x;
  const int32_t s = (int32_t)blockIdx.x;
  if (s >= a.S) return;
  const int32_t nx = a.g.nx, ny = a.g.ny, cap = a.cap;
  const bool diagonal = a.diagonal != 0u;

  int32_t e0 = (int32_t)uniform((uint32_t)a.starts[s]);
  if ((uint32_t)e0 >= (uint32_t)a.g.G) e0 = -1;
  uint32_t v = e0 >= 0 ? uniform(a.field[e0]) : kBlocked;
  gv_nav_path_info rec = path_record_begin(e0, v);
  if (rec.status == GV_PATH_REACHED) {   // a start that walks
    int32_t y = e0 / nx, x = e0 - y * nx;
    const size_t first = (size_t)s * (size_t)cap;
    int32_t *ent = a.entries + first;
    float2 *xy = reinterpret_cast<float2 *>(a.xy) + first;
    float2 *xy_out = a.xy_out ? reinterpret_cast<float2 *>(a.xy_out) + first : nullptr;
    int32_t n = 1, n_diag = 0, pending = 1;   // cells of the path so far; those of them still in cells_s
    int32_t dx = 0, dy = 0;                   // the last move: the direction the lanes look ahead in
    if (lane == 0) cells_s[0] = e0;
#ifdef GV_PATH_WINDOW
    int32_t wx0 = 0, wy0 = 0, from_x = x, from_y = y;   // the window, and the cell it was loaded at
    bool have_window = false;
#endif
    for (;;) {
      if (v == 0u) break;                                   // rec.status is GV_PATH_REACHED
      if (n == cap) { rec.status = GV_PATH_TRUNCATED; break; }
      // lane i looks at the cell i moves ahead; it takes part when that cell and its neighbours are where they can be read
      const int32_t lx = x + lane * dx, ly = y + lane * dy;
      bool ok = lx >= 0 && lx < nx && ly >= 0 && ly < ny && (lane == 0 || (dx | dy) != 0);
#ifdef GV_PATH_WINDOW
      const bool inside = have_window && (x - 1 >= wx0 || x == 0) && (x + 1 < wx0 + kW || x + 1 >= nx) &&
                          (y - 1 >= wy0 || y == 0) && (y + 1 < wy0 + kW || y + 1 >= ny);
      if (!inside) {
        wx0 = window_origin(x, from_x, nx);
        wy0 = window_origin(y, from_y, ny);
        from_x = x;
        from_y = y;
        __syncthreads();   // the window's last readers
        load_window(a.field, nx, ny, wx0, wy0, win_s, lane);
        __syncthreads();
        have_window = true;
      }
      ok = ok && (lx - 1 >= wx0 || lx == 0) && (lx + 1 < wx0 + kW || lx + 1 >= nx) && (ly - 1 >= wy0 || ly == 0) &&
           (ly + 1 < wy0 + kW || ly + 1 >= ny);
      const WindowField f{win_s, wx0, wy0};
#else
      const GlobalField f{a.field, nx, ny};
#endif
      // every lane takes the step of its own cell: one text, the header's, for the cell the walk stands on and for those
      // it would reach by repeating its last move
      int32_t mx = lx, my = ly;
      uint32_t mv = f(lx, ly);
      bool md = false;
      const bool moved = path_next(f, nx, ny, diagonal, mx, my, mv, md);
      // Lane i's cell is the walk's cell i moves from here iff lanes 0 .. i - 1 all repeat the last move; the step each
      // of those lanes took is then a step of the walk.  `run`: how many leading lanes repeat it.
      const bool repeats = ok && moved && (dx | dy) != 0 && mx - lx == dx && my - ly == dy;
      const unsigned long long not_repeating = ~__ballot(repeats);
      const int32_t run = not_repeating == 0ull ? 64 : (int32_t)__builtin_ctzll(not_repeating);
      int32_t k = min(run, cap - n);             // steps taken this round: lanes 0 .. k - 1 each contribute the cell they move to
      if (run == 0) {                            // the walk turns (or begins, or ends): lane 0's own step alone
        if (uniform((uint32_t)moved) == 0u) { rec.status = GV_PATH_STUCK; break; }
        k = 1;
        dx = (int32_t)uniform((uint32_t)mx) - x;
        dy = (int32_t)uniform((uint32_t)my) - y;
      }
      if (lane < k) cells_s[pending + lane] = my * nx + mx;
      n_diag += (int32_t)__popcll(__ballot(md && lane < k));
      x = lane_value(mx, k - 1);
      y = lane_value(my, k - 1);
      v = (uint32_t)lane_value((int32_t)mv, k - 1);
      n += k;
      pending += k;
      if (pending >= kFlush) pending -= flush(a, cells_s, ent, xy, xy_out, n - pending, pending, lane);
    }
    if (pending > 0) flush(a, cells_s, ent, xy, xy_out, n - pending, pending, lane);
    rec.n_cells = n;
    rec.end_value = v;
    rec.end_entry = y * nx + x;
    rec.n_diagonal = n_diag;
  }
  if (lane == 0) {
    a.info[s] = rec;
    if (a.info_out) a.info_out[s] = rec;
  }
}

__global__ void __launch_bounds__(256) k_nav_seeds_path(NavArgs a, const gv_nav_path_info *rec)
{
  const int i = (int)blockIdx.x * 256 + (int)threadIdx.x;
  if (i >= a.n_seeds || i >= rec->n_cells) return;
  const int c = a.seeds[i];
  if ((unsigned)c >= (unsigned)a.G || a.field[c] == kBlocked) return;   // (another seed's 0 is not kBlocked)
  a.field[c] = 0u;
  const int y = c / a.nx, x = c - y * a.nx;
  a.flags_out[(y / kNavTile) * a.tiles_x + x / kNavTile] = 1u;
  atomicAdd(a.counter, 1u);
}

void launch_nav_path(const PathArgs &a, hipStream_t s)
{
  hipLaunchKernelGGL(k_nav_path, dim3((uint32_t)a.S), dim3(64), 0, s, a);
}

void launch_nav_seeds_path(const NavArgs &a, const gv_nav_path_info *rec, int32_t cap, hipStream_t s)
{
  NavArgs b = a;
  b.n_seeds = cap;
  hipLaunchKernelGGL(k_nav_seeds_path, dim3((uint32_t)((cap + 255) / 256)), dim3(256), 0, s, b, rec);
}

}  // namespace gv
