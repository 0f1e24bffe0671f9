// gv_frontier.hip -- [EXTENSION] X19 frontier clusters (gvx_frontier*): frontier cells of the packed layer, their
// 8-connected components labelled across workgroups and XCDs, and the records of the first `cap` clusters
// (include/gridvision_hip_frontier.h has the definition; the arithmetic is gv_frontier.hpp's, the twin's text).
//
// Geometry of every kernel but the two single-workgroup ones: a wavefront is one 64-bit word of one row of the frontier
// bitmap, lane = bit = x % 64; a workgroup is four consecutive words of a row, so the workgroups' linear order is entry
// order.  A wavefront whose word holds no frontier bit leaves at once (k_frontier_cells makes the words; it alone reads
// the whole layer).  No kernel waits for another workgroup; ordering between kernels is the stream's.
//   k_frontier_cells   class of the lane's cell and of the cells above and below it, the row's UNKNOWN word by a ballot
//                      and its two carry bits by two more loads; frontier = FREE and an UNKNOWN 4-neighbour and the
//                      costmap gate.  The word goes to the bitmap; parent[e] = the first cell of the lane's run of
//                      frontier bits inside the word (a forest already: runs are united before any atomic), NONE off
//                      the frontier; labels[e] = NONE.
//   k_frontier_merge   lock-free union-find over `parent`: a frontier cell unites with E only across a word boundary
//                      (the run start did the rest), with S, and with SW and SE only where S is no frontier cell (where
//                      it is, row y + 1 joins them to S itself).  find follows parents to a root; unite hangs the larger
//                      root under the smaller by atomicMin and goes on from what it displaced.  EVERY access to `parent`
//                      in this kernel is a relaxed agent-scope atomic, served where all XCDs agree.  Parents only ever
//                      decrease and always name a cell of the same component, so the final root of a component is its
//                      smallest entry whatever the schedule was.
//   k_frontier_flatten labels[e] = find(parent, e): reads `parent`, which nobody writes any more, writes `labels`.
//   k_frontier_count   parent[root] += 1 per cell of the component (a root holds itself until then, so n_cells is
//                      parent[root] - root afterwards): one integer atomic per wavefront where its cells share a root.
//   k_frontier_roots   per workgroup the number of roots with n_cells >= min_cells; frontier cells, components, largest.
//   k_frontier_scan    one workgroup: exclusive scan of those numbers, in place; their total is n_clusters.
//   k_frontier_ranks   a cluster's rank = its workgroup's scan value + the clusters in front of it in the workgroup (by
//                      ballots: an ORDERED compaction in entry order).  parent[root] = rank below cap, else NONE; the
//                      root begins the record of a written cluster and sets its two keys to "none".
//   k_frontier_sums    pass A: sums, bounding box and field key of the written clusters by integer atomics, one set
//                      per wavefront where its cells share a cluster.
//   k_frontier_centre  pass B, the sums being complete: the centre key.
//   k_frontier_finish  one workgroup: the last step of every record, zeros behind the written ones, `best`, info; and
//                      the copies into pinned destinations.
//   k_nav_seeds_frontier  k_nav_seeds of gv_navfield.hip over the cells of the written clusters.
// All atomics are integer; every store is a plain vector store from VGPRs.  gfx950, wave64.
#include "gv_launch_frontier.hpp"
#include "gv_wave.hpp"

namespace gv {

namespace {
constexpr uint32_t kNone = kFrontierNone;

// the wavefront's place: row y, bitmap word w of it (w >= words: nothing to do), the lane's cell
struct Place {
  int lane, wave, y, w, x;
  bool valid, in;   // the word exists (uniform); the cell is on the map
  size_t e;
};
__device__ __forceinline__ Place place(const FrontierArgs &a)
{
  Place p;
  p.lane = (int)(threadIdx.x & 63u);
  p.wave = (int)(threadIdx.x >> 6);
  p.y = (int)blockIdx.y;
  p.w = (int)blockIdx.x * 4 + p.wave;
  p.valid = p.w < a.row_words - 2;
  p.x = p.w * 64 + p.lane;
  p.in = p.valid && p.x < a.g.nx;
  p.e = (size_t)p.y * (size_t)a.g.nx + (size_t)p.x;
  return p;
}
__device__ __forceinline__ unsigned long long word_of(const unsigned long long *bits, int row_words, int y, int w)
{
  const unsigned long long v = bits[(size_t)y * (size_t)row_words + (size_t)(w + 1)];   // w = -1 and w = words are the zero guards
  const uint32_t lo = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)v);      // one word per wavefront: say so
  const uint32_t hi = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(v >> 32));
  return ((unsigned long long)hi << 32) | (unsigned long long)lo;
}

__device__ __forceinline__ uint32_t load_parent(const uint32_t *p, uint32_t i)
{
  return __hip_atomic_load(p + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ uint32_t find_root(const uint32_t *p, uint32_t i)
{
  for (uint32_t q = load_parent(p, i); q != i; q = load_parent(p, i)) i = q;
  return i;
}
// find_root that halves the path it walks: a cell's parent becomes its grandparent, by atomicMin, so the word still only
// decreases and still names a cell further up its own tree
__device__ __forceinline__ uint32_t find_halving(uint32_t *p, uint32_t i)
{
  for (;;) {
    const uint32_t q = load_parent(p, i);
    if (q == i) return i;
    const uint32_t g = load_parent(p, q);
    if (g == q) return q;
    __hip_atomic_fetch_min(p + i, g, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    i = g;
  }
}
__device__ __forceinline__ void unite(uint32_t *p, uint32_t a, uint32_t b)
{
  for (;;) {
    a = find_halving(p, a);
    b = find_halving(p, b);
    if (a == b) return;
    if (a < b) { const uint32_t t = a; a = b; b = t; }   // a: the larger root goes under the smaller
    const uint32_t old = __hip_atomic_fetch_min(p + a, b, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (old == a) return;
    a = old;   // a was no root any more: unite what it hangs under with b
  }
}

// An atomic minimum or maximum only where it can still change the word.  The look is a relaxed agent-scope load; what it
// sees is the word's value now or an older one, and the word only ever moves one way, so a candidate that does not beat
// an older value does not beat the current one either: no update is skipped that would have counted.
__device__ __forceinline__ void min_i32(int32_t *p, int32_t v)
{
  if (v < __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMin(p, v);
}
__device__ __forceinline__ void max_i32(int32_t *p, int32_t v)
{
  if (v > __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMax(p, v);
}
__device__ __forceinline__ void min_u64(unsigned long long *p, unsigned long long v)
{
  if (v < __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMin(p, v);
}

// true when every frontier lane of the wavefront holds the same v (frontier lanes: the bits of F, not 0); `first`: that v
__device__ __forceinline__ bool wave_same(unsigned long long F, bool mine, uint32_t v, uint32_t &first)
{
  first = (uint32_t)__builtin_amdgcn_readlane((int)v, __ffsll((long long)F) - 1);
  return __ballot(mine && v != first) == 0ull;
}
}  // namespace

__global__ void __launch_bounds__(256) k_frontier_cells(FrontierArgs a)
{
  const Place p = place(a);
  if (!p.valid) return;
  const int nx = a.g.nx, ny = a.g.ny;
  const int8_t *row = a.i8 + (size_t)p.y * (size_t)nx;
  const int32_t c = p.in ? frontier_class(a.rule, row[p.x]) : kFrontierNeither;
  const bool up = p.in && p.y > 0 && frontier_class(a.rule, row[p.x - nx]) == kFrontierUnknown;
  const bool dn = p.in && p.y + 1 < ny && frontier_class(a.rule, row[p.x + nx]) == kFrontierUnknown;
  const unsigned long long U = __ballot(c == kFrontierUnknown);
  const int x0 = p.w * 64;
  const unsigned long long cl = (x0 > 0 && frontier_class(a.rule, row[x0 - 1]) == kFrontierUnknown) ? 1ull : 0ull;
  const unsigned long long cr = (x0 + 64 < nx && frontier_class(a.rule, row[x0 + 64]) == kFrontierUnknown) ? 1ull : 0ull;
  const unsigned long long beside = ((U << 1) | cl) | ((U >> 1) | (cr << 63));
  bool f = c == kFrontierFree && ((((beside >> p.lane) & 1ull) != 0ull) || up || dn);
  if (f) f = frontier_cost_ok(a.rule, a.cost, p.e);
  const unsigned long long F = __ballot(f);
  if (p.lane == 0) a.bits[(size_t)p.y * (size_t)a.row_words + (size_t)(p.w + 1)] = F;
  if (!p.in) return;
  const unsigned long long gaps = ~F & ((1ull << p.lane) - 1ull);        // the cells in front of the lane that are no frontier
  const int start = gaps ? 64 - __clzll((long long)gaps) : 0;            // the first cell of the lane's run
  a.parent[p.e] = f ? (uint32_t)(p.y * nx + x0 + start) : kNone;
  a.labels[p.e] = kNone;
}

__global__ void __launch_bounds__(256) k_frontier_merge(FrontierArgs a)
{
  const Place p = place(a);
  if (!p.valid) return;
  const unsigned long long F = word_of(a.bits, a.row_words, p.y, p.w);
  if (F == 0ull) return;
  const unsigned long long E = word_of(a.bits, a.row_words, p.y, p.w + 1);
  unsigned long long B0 = 0ull, B1 = 0ull, B2 = 0ull;
  if (p.y + 1 < a.g.ny) {
    B0 = word_of(a.bits, a.row_words, p.y + 1, p.w - 1);
    B1 = word_of(a.bits, a.row_words, p.y + 1, p.w);
    B2 = word_of(a.bits, a.row_words, p.y + 1, p.w + 1);
  }
  if (!((F >> p.lane) & 1ull)) return;
  const unsigned long long SW = (B1 << 1) | (B0 >> 63), SE = (B1 >> 1) | (B2 << 63);
  const uint32_t e = (uint32_t)p.e, nx = (uint32_t)a.g.nx;
  if (p.lane == 63 && (E & 1ull)) unite(a.parent, e, e + 1u);
  if ((B1 >> p.lane) & 1ull) {
    unite(a.parent, e, e + nx);
  } else {
    if ((SW >> p.lane) & 1ull) unite(a.parent, e, e + nx - 1u);
    if ((SE >> p.lane) & 1ull) unite(a.parent, e, e + nx + 1u);
  }
}

__global__ void __launch_bounds__(256) k_frontier_flatten(FrontierArgs a)
{
  const Place p = place(a);
  if (!p.valid) return;
  const unsigned long long F = word_of(a.bits, a.row_words, p.y, p.w);
  if (!((F >> p.lane) & 1ull)) return;
  a.labels[p.e] = find_root(a.parent, (uint32_t)p.e);
}

__global__ void __launch_bounds__(256) k_frontier_count(FrontierArgs a)
{
  const Place p = place(a);
  if (!p.valid) return;
  const unsigned long long F = word_of(a.bits, a.row_words, p.y, p.w);
  if (F == 0ull) return;
  const bool mine = ((F >> p.lane) & 1ull) != 0ull;
  const uint32_t root = mine ? a.labels[p.e] : kNone;
  uint32_t first;
  if (wave_same(F, mine, root, first)) {
    if (p.lane == 0) atomicAdd(a.parent + first, (uint32_t)__popcll(F));
  } else if (mine) {
    atomicAdd(a.parent + root, 1u);
  }
}

__global__ void __launch_bounds__(256) k_frontier_roots(FrontierArgs a)
{
  const Place p = place(a);
  if (!p.valid) return;
  const unsigned long long F = word_of(a.bits, a.row_words, p.y, p.w);
  if (F == 0ull) return;
  const bool root = ((F >> p.lane) & 1ull) && a.labels[p.e] == (uint32_t)p.e;
  const uint32_t n = root ? a.parent[p.e] - (uint32_t)p.e : 0u;
  const unsigned long long R = __ballot(root), Q = __ballot(root && n >= (uint32_t)a.rule.min_cells);
  const uint32_t largest = wave_reduce<OpMax>(n), cells = wave_reduce<OpAdd>(n);
  if (p.lane == 0 && R) {
    atomicAdd(a.head + 0, cells);   // every frontier cell is counted at its root
    atomicAdd(a.head + 1, (uint32_t)__popcll(R));
    atomicMax(a.head + 3, largest);
    if (Q) atomicAdd(a.head + kFrontierHead + (size_t)blockIdx.y * (size_t)a.blocks_x + (size_t)blockIdx.x, (uint32_t)__popcll(Q));
  }
}

__global__ void __launch_bounds__(1024) k_frontier_scan(FrontierArgs a)
{
  __shared__ uint32_t wave_total[16];
  __shared__ uint32_t carry_s;
  const int t = (int)threadIdx.x, lane = t & 63, wave = t >> 6;
  uint32_t *count = a.head + kFrontierHead;
  if (t == 0) carry_s = 0u;
  __syncthreads();
  for (int base = 0; base < a.n_blocks; base += 1024) {
    const int i = base + t;
    const uint32_t v = i < a.n_blocks ? count[i] : 0u;
    const uint32_t incl = wave_scan<OpAdd>(v);
    if (lane == 63) wave_total[wave] = incl;
    __syncthreads();
    uint32_t before = carry_s, total = 0u;
#pragma unroll
    for (int k = 0; k < 16; ++k) {
      before += k < wave ? wave_total[k] : 0u;
      total += wave_total[k];
    }
    if (i < a.n_blocks) count[i] = before + incl - v;
    __syncthreads();
    if (t == 0) carry_s += total;
    __syncthreads();
  }
  if (t == 0) a.head[2] = carry_s;
}

__global__ void __launch_bounds__(256) k_frontier_ranks(FrontierArgs a)
{
  __shared__ uint32_t wave_n[4];
  const Place p = place(a);
  const unsigned long long F = p.valid ? word_of(a.bits, a.row_words, p.y, p.w) : 0ull;
  const bool root = ((F >> p.lane) & 1ull) && a.labels[p.e] == (uint32_t)p.e;
  const uint32_t n = root ? a.parent[p.e] - (uint32_t)p.e : 0u;
  const bool q = root && n >= (uint32_t)a.rule.min_cells;
  const unsigned long long Q = __ballot(q);
  if (p.lane == 0) wave_n[p.wave] = (uint32_t)__popcll(Q);
  __syncthreads();
  if (!root) return;
  uint32_t rank = kNone;
  if (q) {
    rank = a.head[kFrontierHead + (size_t)blockIdx.y * (size_t)a.blocks_x + (size_t)blockIdx.x] + wave_rank(Q, p.lane);
    for (int k = 0; k < p.wave; ++k) rank += wave_n[k];
    if (rank < (uint32_t)a.cap) {
      a.rec[rank] = frontier_record_begin((int32_t)p.e, (int32_t)n);
      a.keys[2 * rank] = kFrontierNoKey;
      a.keys[2 * rank + 1] = kFrontierNoKey;
    } else {
      rank = kNone;
    }
  }
  a.parent[p.e] = rank;
}

__global__ void __launch_bounds__(256) k_frontier_sums(FrontierArgs a)
{
  const Place p = place(a);
  if (!p.valid) return;
  const unsigned long long F = word_of(a.bits, a.row_words, p.y, p.w);
  if (F == 0ull) return;
  const bool mine = ((F >> p.lane) & 1ull) != 0ull;
  const uint32_t rank = mine ? a.parent[a.labels[p.e]] : kNone;
  const bool use_field = (a.flags & GVX_FRONTIER_USE_FIELD) != 0u;
  uint64_t fkey = kFrontierNoKey;
  if (use_field && rank != kNone) {
    const uint32_t v = a.field[p.e];
    if (v < GV_NAV_UNREACHABLE) fkey = frontier_field_key(v, (int32_t)p.e);
  }
  uint32_t first;
  if (wave_same(F, mine, rank, first)) {   // one cluster (or none written) in the whole word
    const uint32_t sx = wave_sum<uint32_t>(mine ? (uint32_t)p.x : 0u);
    const uint64_t fmin = wave_min_key(fkey);
    if (p.lane != 0 || first == kNone) return;
    gvx_frontier_record *r = a.rec + first;
    const int x0 = p.w * 64, n = __popcll(F);
    atomicAdd(reinterpret_cast<unsigned long long *>(&r->sum_x), (unsigned long long)sx);
    atomicAdd(reinterpret_cast<unsigned long long *>(&r->sum_y), (unsigned long long)n * (unsigned long long)p.y);
    min_i32(&r->min_x, x0 + __ffsll((long long)F) - 1);
    max_i32(&r->max_x, x0 + 63 - __clzll((long long)F));
    min_i32(&r->min_y, p.y);
    max_i32(&r->max_y, p.y);
    if (fmin != kFrontierNoKey) min_u64(a.keys + 2 * first + 1, (unsigned long long)fmin);
  } else if (rank != kNone) {
    gvx_frontier_record *r = a.rec + rank;
    atomicAdd(reinterpret_cast<unsigned long long *>(&r->sum_x), (unsigned long long)p.x);
    atomicAdd(reinterpret_cast<unsigned long long *>(&r->sum_y), (unsigned long long)p.y);
    min_i32(&r->min_x, p.x);
    max_i32(&r->max_x, p.x);
    min_i32(&r->min_y, p.y);
    max_i32(&r->max_y, p.y);
    if (fkey != kFrontierNoKey) min_u64(a.keys + 2 * rank + 1, (unsigned long long)fkey);
  }
}

__global__ void __launch_bounds__(256) k_frontier_centre(FrontierArgs a)
{
  const Place p = place(a);
  if (!p.valid) return;
  const unsigned long long F = word_of(a.bits, a.row_words, p.y, p.w);
  if (F == 0ull) return;
  const bool mine = ((F >> p.lane) & 1ull) != 0ull;
  const uint32_t rank = mine ? a.parent[a.labels[p.e]] : kNone;
  uint64_t key = kFrontierNoKey;
  if (rank != kNone) {
    const gvx_frontier_record *r = a.rec + rank;
    const uint64_t n = (uint64_t)(uint32_t)r->n_cells;
    key = frontier_centre_key(p.x, p.y, (int64_t)(r->sum_x / n), (int64_t)(r->sum_y / n), (int32_t)p.e);
  }
  uint32_t first;
  if (wave_same(F, mine, rank, first)) {
    const uint64_t kmin = wave_min_key(key);
    if (p.lane == 0 && first != kNone) min_u64(a.keys + 2 * first, (unsigned long long)kmin);
  } else if (rank != kNone) {
    min_u64(a.keys + 2 * rank, (unsigned long long)key);
  }
}

__global__ void __launch_bounds__(256) k_frontier_finish(FrontierArgs a)
{
  __shared__ unsigned long long wave_best[4];
  const int t = (int)threadIdx.x;
  const int32_t n_clusters = (int32_t)a.head[2];
  const int32_t n_written = n_clusters < a.cap ? n_clusters : a.cap;
  const bool use_field = (a.flags & GVX_FRONTIER_USE_FIELD) != 0u;
  uint64_t best = kFrontierNoKey;
  for (int32_t i = t; i < a.cap; i += 256) {
    gvx_frontier_record r = frontier_record_zero();
    if (i < n_written) {
      r = a.rec[i];
      frontier_record_finish(a.g, a.keys[2 * i], a.keys[2 * i + 1], r);
      const uint64_t key = frontier_best_key(r, i, use_field);
      best = key < best ? key : best;
    }
    a.rec[i] = r;
    if (a.rec_out) a.rec_out[i] = r;
  }
  best = wave_min_key(best);
  if ((t & 63) == 0) wave_best[t >> 6] = best;
  __syncthreads();
  if (t != 0) return;
  for (int k = 1; k < 4; ++k) best = wave_best[k] < best ? wave_best[k] : best;
  gvx_frontier_info I;
  I.n_frontier_cells = (int32_t)a.head[0];
  I.n_components = (int32_t)a.head[1];
  I.n_clusters = n_clusters;
  I.n_written = n_written;
  I.best = frontier_best_index(best);
  I.largest = (int32_t)a.head[3];
  I.flags = a.flags;
  I.reserved = 0u;
  *a.info = I;
  if (a.info_out) *a.info_out = I;
}

__global__ void __launch_bounds__(256) k_nav_seeds_frontier(NavArgs a, FrontierSeedArgs f)
{
  const int lane = (int)(threadIdx.x & 63u), wave = (int)(threadIdx.x >> 6);
  const int y = (int)blockIdx.y, w = (int)blockIdx.x * 4 + wave;
  if (w >= f.row_words - 2) return;
  const unsigned long long F = word_of(f.bits, f.row_words, y, w);
  if (F == 0ull) return;
  const int x = w * 64 + lane;
  const int c = y * a.nx + x;
  bool seed = ((F >> lane) & 1ull) != 0ull;
  if (seed) {
    const uint32_t rank = f.rank[f.labels[c]];
    seed = rank != kNone && (f.k < 0 || rank == (uint32_t)f.k) && a.field[c] != GV_NAV_BLOCKED;   // as k_nav_seeds: a blocked cell is no seed
  }
  const unsigned long long S = __ballot(seed);
  if (S == 0ull) return;
  if (seed) a.field[c] = 0u;
  if (lane == 0) {
    a.flags_out[(y / kNavTile) * a.tiles_x + x / kNavTile] = 1u;   // a word lies in one tile
    atomicAdd(a.counter, (uint32_t)__popcll(S));
  }
}

void launch_frontier(const FrontierArgs &a, hipStream_t s)
{
  const dim3 grid((uint32_t)a.blocks_x, (uint32_t)a.g.ny), block(256);
  hipLaunchKernelGGL(k_frontier_cells, grid, block, 0, s, a);
  hipLaunchKernelGGL(k_frontier_merge, grid, block, 0, s, a);
  hipLaunchKernelGGL(k_frontier_flatten, grid, block, 0, s, a);
  hipLaunchKernelGGL(k_frontier_count, grid, block, 0, s, a);
  hipLaunchKernelGGL(k_frontier_roots, grid, block, 0, s, a);
  hipLaunchKernelGGL(k_frontier_scan, dim3(1), dim3(1024), 0, s, a);
  hipLaunchKernelGGL(k_frontier_ranks, grid, block, 0, s, a);
  hipLaunchKernelGGL(k_frontier_sums, grid, block, 0, s, a);
  hipLaunchKernelGGL(k_frontier_centre, grid, block, 0, s, a);
  hipLaunchKernelGGL(k_frontier_finish, dim3(1), dim3(256), 0, s, a);
}

void launch_nav_seeds_frontier(const NavArgs &a, const FrontierSeedArgs &f, hipStream_t s)
{
  const int32_t words = f.row_words - 2;
  hipLaunchKernelGGL(k_nav_seeds_frontier, dim3((uint32_t)((words + 3) / 4), (uint32_t)a.ny), dim3(256), 0, s, a, f);
}

}  // namespace gv
