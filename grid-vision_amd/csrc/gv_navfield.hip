// gv_navfield.hip -- [EXTENSION] X9 goal / path distance field (gv_nav_field) and its sampler (gv_score_nav):
// the geodesic distance from seed cells over the resident costmap of gv_inflate, 4-connected, with per-cell step costs
// (include/gridvision_hip.h has the definition), and the field read along K trajectories of P poses.
//
// The solver is a tiled relaxation in ROUNDS; a round is one launch of k_nav_relax.  No kernel waits for another
// workgroup: no grid-wide barrier, no cooperative launch, no spin on memory another workgroup writes.  Ordering between
// rounds is the stream's.
//   k_nav_init   every cell: GV_NAV_BLOCKED where step[cost] == 0, else GV_NAV_UNREACHABLE.
//   k_nav_seeds  a thread per seed: 0 at a seed cell that is not blocked, its tile marked active, one more seed used.
//   k_nav_relax  one wavefront (a workgroup of 64) per 64 x 64 tile.  An inactive tile leaves at once.  An active one
//                clears its flag, loads its cells and a one-cell halo into LDS (the neighbours' border cells; off the
//                map: blocked) and its step values, and relaxes the tile to its local fixpoint by directional scans,
//                d[x] = min(d[x], d[x-1] + step[x]): left to right and right to left with a lane per row, then down
//                and up with a lane per column.  The running value lives in a register, so a value crosses the whole
//                tile in one scan; a serpentine corridor inside a tile costs a pass per turn, not a pass per cell.
//                A cell has ONE owner in each phase (the lane of its row, then the lane of its column) and a barrier
//                separates the phases: no cell is ever read-modify-written by two lanes, so no update is lost and "a
//                full pass changed nothing" does prove the local fixpoint.  Halo cells are never written.
//                The local loop carries a hard pass cap (NavArgs::pass_cap, kNavPassCap = 40 by default).  A pass moves
//                a value along one more straight run in each of the four directions; the longest in-tile fixture of
//                tests/nav_cases.py, a period-2 serpentine of 30 corridors confined to one tile, needs 31 passes
//                (tests/test_nav_host.py counts them in its simulation of this kernel), and 40 leaves a margin.  A
//                tile that hits the cap marks ITSELF active for the next round and goes on there: the result stays
//                exact, and no input makes the kernel loop without bound.
//                Then the tile compares its cells with what memory holds (only this tile writes them) and stores the
//                ones that differ with plain vector stores; it marks active, for the next round, each neighbour whose
//                adjacent border row or column changed, and adds one to the round's changed-tile counter (a vector
//                atomic).  The host stops after the first round whose counter is 0.
// Exactness under any schedule.  Every value ever stored is the length of a real path from a seed: a seed's 0, or a
// neighbour's stored value plus the step of the cell entered.  Stored values only decrease.  A halo value read while
// the neighbour is storing is an aligned 32-bit load -- it does not tear -- so it is a value the neighbour did store:
// stale at worst, still a real path length, never too small.  And staleness is caught: a tile whose border changed in
// round r marks its neighbour active for round r + 1, which starts after round r has finished, so every tile's last
// look at its halo comes after that halo's last change.  When a round changes nothing, no flag is set, every tile is at
// its local fixpoint against final halos, and the whole field is a fixpoint of d[c] = min over neighbours n of
// d[n] + step[c] with 0 at the seeds.  A fixpoint is <= the true distance (induction along a shortest path), real path
// lengths are >= it: the field is the exact distance, the same integers whatever the hardware did first.
// A stored value belongs to a simple path (a relaxation that came back to a cell would offer more than the cell
// already holds), so it is at most (G - 1) * the largest step, which gv_set_nav_config keeps under GV_NAV_UNREACHABLE;
// the candidate of a relaxation may exceed 32 bits and saturates.
// A round that changes something gives its final value to at least one more cell of every unfinished shortest path, so
// rounds <= G + 2; the host loop stops there.
//
// k_score_nav: a wavefront per trajectory (four to a workgroup), a lane per pose in chunks of 64: get_index on the
// centre, one guarded field read, and the record reduced by ballots and cross-lane shuffles.
// LDS: the values in a 66 x 67 array (odd stride: the lanes of a row scan hit 32 different banks), the steps as uint16
// (1 + 255 * 254 < 2^16) with a stride of 66 halfwords = 33 dwords, 26 KB in all.
// gfx950, wave64; every store below is a plain vector store from VGPRs.
#include "gv_launch_planner.hpp"
#include "gv_device.hpp"

namespace gv {

namespace {
constexpr int kT = kNavTile;      // tile side = lanes of the wavefront
constexpr int kDS = kT + 3;       // row stride of the value array: kT + 2 columns, padded to an odd number
constexpr int kSS = kT + 2;       // row stride of the step array, in halfwords
constexpr uint32_t kBlocked = GV_NAV_BLOCKED, kUnreachable = GV_NAV_UNREACHABLE;
static_assert(kT == 64, "a lane per row / column of the tile");

// One directional scan of one row or column: d points at the halo cell in front of it, st at the step of its first
// cell; DS / SS are the strides along the scan.  The cells' values and steps are loaded eight at a time ahead of the
// chain, which runs in registers.  true: this lane lowered a value.
template <int DS, int SS>
__device__ __forceinline__ bool scan(uint32_t *d, const uint16_t *st)
{
  bool changed = false;
  uint32_t prev = d[0];
#pragma unroll 1
  for (int k0 = 0; k0 < kT; k0 += 8) {
    uint32_t cur[8], s[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      cur[j] = d[(k0 + j + 1) * DS];
      s[j] = st[(k0 + j) * SS];
    }
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      uint32_t cand = prev + s[j];
      cand = cand < prev ? kBlocked : cand;   // past 32 bits: never below a cell's value
      if (s[j] != 0 && prev < kUnreachable && cand < cur[j]) {
        cur[j] = cand;
        d[(k0 + j + 1) * DS] = cand;
        changed = true;
      }
      prev = cur[j];
    }
  }
  return changed;
}
}  // namespace

__global__ void __launch_bounds__(256) k_nav_init(NavArgs a)
{
  const int i = ((int)blockIdx.x * 256 + (int)threadIdx.x) * 4;
  if (i >= a.G) return;
  const uchar4 c = *reinterpret_cast<const uchar4 *>(a.cost + i);   // the costmap buffer has 16 bytes of slack
  uint4 v;
  v.x = nav_step(a.step, c.x) ? kUnreachable : kBlocked;
  v.y = nav_step(a.step, c.y) ? kUnreachable : kBlocked;
  v.z = nav_step(a.step, c.z) ? kUnreachable : kBlocked;
  v.w = nav_step(a.step, c.w) ? kUnreachable : kBlocked;
  *reinterpret_cast<uint4 *>(a.field + i) = v;                       // the field buffer is a multiple of 4 long
}

__global__ void __launch_bounds__(256) k_nav_seeds(NavArgs a)
{
  const int i = (int)blockIdx.x * 256 + (int)threadIdx.x;
  if (i >= a.n_seeds) return;
  const int c = a.seeds[i];
  if ((unsigned)c >= (unsigned)a.G || a.field[c] == kBlocked) return;   // (another seed's 0 is not kBlocked)
  a.field[c] = 0u;
  const int y = c / a.nx, x = c - y * a.nx;
  a.flags_out[(y / kT) * a.tiles_x + x / kT] = 1u;
  atomicAdd(a.counter, 1u);
}

__global__ void __launch_bounds__(64) k_nav_relax(NavArgs a)
{
  __shared__ uint32_t d_s[(kT + 2) * kDS];   // [row 0 .. kT+1][column 0 .. kT+1]: the tile inside a one-cell halo
  __shared__ uint16_t st_s[kT * kSS];        // [row][column]: the step of the tile's cells, 0 blocked or off the map
  const int lane = (int)threadIdx.x;
  const int tile = (int)blockIdx.x;
  if (tile >= a.tiles_x * a.tiles_y || a.flags_in[tile] == 0u) return;
  if (lane == 0) a.flags_in[tile] = 0u;      // consumed: only this tile touches its flag of this round
  const int ty = tile / a.tiles_x, tx = tile - ty * a.tiles_x;
  const int x0 = tx * kT, y0 = ty * kT, nx = a.nx, ny = a.ny;
  const int gx = x0 + lane;
  const bool col_ok = gx < nx;

  // ---- load: lane = column; lanes 0 and 1 also take the two halo columns.  Every address is clamped into the map, so
  // the loads of a batch are unconditional and issued back to back; what lies off the map is replaced afterwards.
  const int hx = lane == 0 ? x0 - 1 : x0 + kT;               // the halo column of lanes 0 / 1
  const bool hcol_ok = lane < 2 && hx >= 0 && hx < nx;
  const int gxc = min(gx, nx - 1), hxc = min(max(hx, 0), nx - 1);
  constexpr int kLoadBatch = 11;                              // kT + 2 = 6 * 11 rows
  static_assert((kT + 2) % kLoadBatch == 0, "whole batches");
#pragma unroll 1
  for (int r0 = 0; r0 < kT + 2; r0 += kLoadBatch) {
    uint32_t v[kLoadBatch], hv[kLoadBatch];
#pragma unroll
    for (int j = 0; j < kLoadBatch; ++j) {
      const int row = min(max(y0 - 1 + r0 + j, 0), ny - 1) * nx;
      v[j] = a.field[row + gxc];
      hv[j] = a.field[row + hxc];
    }
#pragma unroll
    for (int j = 0; j < kLoadBatch; ++j) {
      const int r = r0 + j, gy = y0 - 1 + r;
      const bool row_ok = gy >= 0 && gy < ny;
      d_s[r * kDS + 1 + lane] = row_ok && col_ok ? v[j] : kBlocked;
      if (lane < 2) {
        const bool corner = r == 0 || r == kT + 1;
        d_s[r * kDS + (lane == 0 ? 0 : kT + 1)] = row_ok && hcol_ok && !corner ? hv[j] : kBlocked;
      }
    }
  }
#pragma unroll 1
  for (int r0 = 0; r0 < kT; r0 += 16) {
    uint32_t c[16];
#pragma unroll
    for (int j = 0; j < 16; ++j) c[j] = a.cost[min(y0 + r0 + j, ny - 1) * nx + gxc];
#pragma unroll
    for (int j = 0; j < 16; ++j)
      st_s[(r0 + j) * kSS + lane] = y0 + r0 + j < ny && col_ok ? (uint16_t)nav_step(a.step, c[j]) : (uint16_t)0;
  }
  __syncthreads();

  // ---- relax to the local fixpoint (or the cap)
  bool capped = false;
  for (int pass = 1;; ++pass) {
    // lane = row
    bool ch = scan<1, 1>(&d_s[(lane + 1) * kDS], &st_s[lane * kSS]);
    ch |= scan<-1, -1>(&d_s[(lane + 1) * kDS + kT + 1], &st_s[lane * kSS + kT - 1]);
    __syncthreads();
    // lane = column
    ch |= scan<kDS, kSS>(&d_s[lane + 1], &st_s[lane]);
    ch |= scan<-kDS, -kSS>(&d_s[(kT + 1) * kDS + lane + 1], &st_s[(kT - 1) * kSS + lane]);
    __syncthreads();
    if (__ballot(ch) == 0ull) break;
    if (pass >= a.pass_cap) { capped = true; break; }
  }

  // ---- store what differs from memory: lane = column
  bool any = false, up = false, down = false, side = false;
#pragma unroll 1
  for (int r0 = 0; r0 < kT; r0 += 16) {
    uint32_t old[16];
#pragma unroll
    for (int j = 0; j < 16; ++j) old[j] = a.field[min(y0 + r0 + j, ny - 1) * nx + gxc];
#pragma unroll
    for (int j = 0; j < 16; ++j) {
      const int r = r0 + j, gy = y0 + r;
      const uint32_t v = d_s[(r + 1) * kDS + 1 + lane];
      if (gy < ny && col_ok && old[j] != v) {
        a.field[gy * nx + gx] = v;
        any = true;
        up |= r == 0;
        down |= r == kT - 1;
        side = true;
      }
    }
  }
  const unsigned long long b_any = __ballot(any), b_up = __ballot(up), b_down = __ballot(down), b_side = __ballot(side);
  if (lane == 0) {
    if (b_any != 0ull || capped) atomicAdd(a.counter, 1u);
    if (capped) a.flags_out[tile] = 1u;
    if (b_up != 0ull && ty > 0) a.flags_out[tile - a.tiles_x] = 1u;
    if (b_down != 0ull && ty + 1 < a.tiles_y) a.flags_out[tile + a.tiles_x] = 1u;
    if ((b_side & 1ull) != 0ull && tx > 0) a.flags_out[tile - 1] = 1u;                       // column 0 changed
    if ((b_side >> (kT - 1)) != 0ull && tx + 1 < a.tiles_x) a.flags_out[tile + 1] = 1u;      // column kT - 1 changed
  }
}

__global__ void __launch_bounds__(256) k_score_nav(NavScoreArgs a)
{
  const int lane = (int)threadIdx.x & 63;
  const int k = (int)blockIdx.x * 4 + ((int)threadIdx.x >> 6);
  if (k >= a.K) return;
  const int P = a.P, G = a.g.G;
  const float *traj = a.poses + (size_t)k * (size_t)P * 3u;
  unsigned long long sum = 0ull;        // per lane
  unsigned long long key = ~0ull;       // per lane: (value << 32) | pose of the smallest good value this lane saw
  int n_bad = 0;                        // wave-uniform
  uint32_t last = kBlocked;             // wave-uniform
  for (int p0 = 0; p0 < P; p0 += 64) {
    const int p = p0 + lane;
    const bool in = p < P;
    uint32_t v = kBlocked;
    if (in) {
      const float *q = traj + (size_t)p * 3u;
      int ix = 0, iy = 0;
      if (get_index(a.g, (double)q[0], (double)q[1], ix, iy)) {
        const int c = data_entry(a.g, ix, iy);
        if ((unsigned)c < (unsigned)G) v = a.field[c];
      }
    }
    const bool good = in && v < kUnreachable;
    if (good) {
      sum += v;
      const unsigned long long cand = ((unsigned long long)v << 32) | (unsigned)p;
      key = cand < key ? cand : key;
    }
    n_bad += __popcll(__ballot(in && !good));
    if (p0 + 64 >= P) last = (uint32_t)__shfl((int)v, P - 1 - p0, 64);
  }
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) {
    sum += __shfl_xor(sum, o, 64);
    const unsigned long long other = __shfl_xor(key, o, 64);
    key = other < key ? other : key;
  }
  if (lane == 0) {
    const bool none = key == ~0ull;
    gv_nav_score r;
    r.sum = sum;
    r.last = last;
    r.best = none ? kUnreachable : (uint32_t)(key >> 32);
    r.best_pose = none ? -1 : (int32_t)(uint32_t)key;
    r.n_bad = n_bad;
    a.scores[k] = r;
  }
}

void launch_nav_init(const NavArgs &a, hipStream_t s)
{
  hipLaunchKernelGGL(k_nav_init, dim3((uint32_t)((a.G + 1023) / 1024)), dim3(256), 0, s, a);
}

void launch_nav_seeds(const NavArgs &a, hipStream_t s)
{
  if (a.n_seeds > 0) hipLaunchKernelGGL(k_nav_seeds, dim3((uint32_t)((a.n_seeds + 255) / 256)), dim3(256), 0, s, a);
}

void launch_nav_relax(const NavArgs &a, hipStream_t s)
{
  hipLaunchKernelGGL(k_nav_relax, dim3((uint32_t)(a.tiles_x * a.tiles_y)), dim3(kT), 0, s, a);
}

void launch_score_nav(const NavScoreArgs &a, hipStream_t s)
{
  hipLaunchKernelGGL(k_score_nav, dim3((uint32_t)((a.K + 3) / 4)), dim3(256), 0, s, a);
}

}  // namespace gv
