// gv_gain.hip -- [EXTENSION] X20 information gain of exploration goals (gvx2_*): the rays of every candidate over the packed
// layer, their counts, the records and `best` (include/gridvision_hip_gain.h has the definition; the arithmetic is
// gv_gain.hpp's, the twin's text).
//   k_gain_rays       one workgroup per record slot, a lane per ray (gain_threads: whole wavefronts, 1024 lanes at the most;
//                     beyond R = 128 a lane takes a second ray).  A slot without a candidate (a frontier call, behind
//                     n_written, which the kernel reads where the frontier call left it) writes a zero record, an entry off
//                     the map its INVALID record; both leave at once, the whole workgroup together.
//                     1. The window.  The (2R + 1)^2 cells around the candidate become two bitmaps in LDS, UNKNOWN and
//                        OPAQUE (gain_row_words: rows of whole 32-bit words); a wavefront takes 64 cells of a window row per
//                        step, a byte load per lane and a ballot per class, and lanes 0 and 1 store the two words.  Cells
//                        off the map are in neither.  The third bitmap, SEEN, is zeroed by the same stores.
//                     2. The rays.  gain_walk (gv_gain.hpp) with every cell test answered from LDS; a seen cell is an LDS
//                        atomic OR, issued only where a relaxed look finds the bit still clear (bits are only ever set, so
//                        an old value can only cause an OR too many).  A lane walks its ray cell by cell: a ray stops at
//                        its first opaque cell, most of them early where there are walls, and a lane that has stopped is
//                        idle only until the longest ray of its wavefront ends.
//                     3. The counts.  The three ray counters and the minimum go through wave_reduce (gv_wave.hpp) and one
//                        LDS slot per wavefront; n_unknown, n_opaque and the seen total are popcounts of SEEN and a class,
//                        reduced the same way.  Lane 0 of the workgroup finishes the record (gain_record) and stores it,
//                        into the pinned destination as well when there is one.
//                     No variant that reads the classes from global memory was written: there is no A/B of that choice.
//   k_gain_finish     one workgroup: n_ranked and `best` over the candidates' records (gain_best_key, the largest wins),
//                     the info record, and its copy into a pinned destination.
//   k_nav_seeds_gain  k_nav_seeds of gv_navfield.hip over the cell of one resident record, the index read here.
// No kernel waits for another workgroup; ordering between kernels is the stream's.  All atomics are integer; every store to
// global memory is a plain vector store from VGPRs.  gfx950, wave64.
#include "gv_launch_gain.hpp"
#include "gv_wave.hpp"

namespace gv {

namespace {
constexpr int kGainMaxWaves = 16;
enum { kPartRay = 0, kPartMin = 3, kPartUnknown = 4, kPartOpaque = 5, kPartSeen = 6, kPartWords = 7 };
}  // namespace

__global__ void __launch_bounds__(1024) k_gain_rays(GainArgs a)
{
  extern __shared__ uint32_t bitmaps_s[];                 // UNKNOWN, OPAQUE, SEEN: gain_bitmap_words(R) words each
  __shared__ uint32_t part_s[kGainMaxWaves][kPartWords];   // what a wavefront adds to the workgroup's counts
  const int t = (int)threadIdx.x, lane = t & 63, wave = t >> 6;
  const int nt = (int)blockDim.x, waves = nt >> 6;
  const int b = (int)blockIdx.x;

  bool live = true;
  int32_t entry;
  if (a.frec) {
    live = b < a.finfo->n_written;
    entry = live ? a.frec[b].goal_entry : 0;
  } else {
    entry = a.entries[b];
  }
  if (!live || !gain_entry_valid(entry, a.g.G)) {          // the same for every lane of the workgroup
    if (t == 0) {
      const gvx2_gain_record r = live ? gain_record_invalid(entry) : gain_record_zero();
      a.rec[b] = r;
      if (a.rec_out) a.rec_out[b] = r;
    }
    return;
  }

  const int R = a.rule.radius, side = 2 * R + 1, W = gain_row_words(R), words = side * W;
  uint32_t *unk = bitmaps_s, *opq = bitmaps_s + words, *seen = bitmaps_s + 2 * words;
  const int nx = a.g.nx, ny = a.g.ny;
  const int cy = entry / nx, cx = entry - cy * nx;
  const int x0 = cx - R, y0 = cy - R;

  // ---- 1. the window: job = (row, chunk of 64 cells), dealt to the wavefronts in turn (a wavefront's lanes stay together)
  const int chunks = (side + 63) / 64;
  for (int job = wave; job < side * chunks; job += waves) {
    const int wy = job / chunks, k = job - wy * chunks;
    const int wx = k * 64 + lane, x = x0 + wx, y = y0 + wy;
    const bool in = wx < side && x >= 0 && x < nx && y >= 0 && y < ny;
    const int32_t c = in ? frontier_class(a.rule.cls, a.i8[(size_t)y * (size_t)nx + (size_t)x]) : -1;
    const unsigned long long U = __ballot(c == kFrontierUnknown), O = __ballot(c == kFrontierNeither);
    const int w = 2 * k + lane;                            // lanes 0 and 1: the chunk's two words
    if (lane < 2 && w < W) {
      unk[wy * W + w] = (uint32_t)(U >> (32 * lane));
      opq[wy * W + w] = (uint32_t)(O >> (32 * lane));
      seen[wy * W + w] = 0u;
    }
  }
  __syncthreads();

  // ---- 2. the rays
  uint32_t n_opaque = 0u, n_off = 0u, n_range = 0u, d2_min = kGainNoOpaque;
  for (int r = t; r < 8 * R; r += nt) {
    uint32_t d2 = kGainNoOpaque;
    const int32_t end = gain_walk(
        nx, ny, cx, cy, R, r,
        [&](int32_t x, int32_t y) {
          const int wx = x - x0, wy = y - y0;
          return ((opq[wy * W + (wx >> 5)] >> (wx & 31)) & 1u) != 0u;
        },
        [&](int32_t x, int32_t y) {
          const int wx = x - x0, wy = y - y0;
          uint32_t *p = seen + wy * W + (wx >> 5);
          const uint32_t bit = 1u << (wx & 31);
          if ((__hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP) & bit) == 0u) atomicOr(p, bit);
        },
        d2);
    n_opaque += end == kGainRayOpaque ? 1u : 0u;
    n_off += end == kGainRayOffMap ? 1u : 0u;
    n_range += end == kGainRayRange ? 1u : 0u;
    d2_min = d2 < d2_min ? d2 : d2_min;
  }
  n_opaque = wave_reduce<OpAdd>(n_opaque);
  n_off = wave_reduce<OpAdd>(n_off);
  n_range = wave_reduce<OpAdd>(n_range);
  d2_min = wave_reduce<OpMin>(d2_min);
  if (lane == 0) {
    part_s[wave][kPartRay + kGainRayOpaque] = n_opaque;
    part_s[wave][kPartRay + kGainRayOffMap] = n_off;
    part_s[wave][kPartRay + kGainRayRange] = n_range;
    part_s[wave][kPartMin] = d2_min;
  }
  __syncthreads();   // every ray has ended: SEEN is complete

  // ---- 3. the counts
  uint32_t n_u = 0u, n_o = 0u, n_s = 0u;
  for (int i = t; i < words; i += nt) {
    const uint32_t s = seen[i];
    n_u += (uint32_t)__popc(s & unk[i]);
    n_o += (uint32_t)__popc(s & opq[i]);
    n_s += (uint32_t)__popc(s);
  }
  n_u = wave_reduce<OpAdd>(n_u);
  n_o = wave_reduce<OpAdd>(n_o);
  n_s = wave_reduce<OpAdd>(n_s);
  if (lane == 0) {
    part_s[wave][kPartUnknown] = n_u;
    part_s[wave][kPartOpaque] = n_o;
    part_s[wave][kPartSeen] = n_s;
  }
  __syncthreads();
  if (t != 0) return;
  uint32_t sum[kPartWords] = {0u, 0u, 0u, kGainNoOpaque, 0u, 0u, 0u};
  for (int k = 0; k < waves; ++k) {
#pragma unroll
    for (int j = 0; j < kPartWords; ++j) {
      const uint32_t v = part_s[k][j];
      sum[j] = j == kPartMin ? (v < sum[j] ? v : sum[j]) : sum[j] + v;
    }
  }
  GainCounts c;
  c.n_unknown = (int32_t)sum[kPartUnknown];
  c.n_opaque = (int32_t)sum[kPartOpaque];
  c.n_free = (int32_t)(sum[kPartSeen] - sum[kPartUnknown] - sum[kPartOpaque]);   // the three classes part the seen cells
  c.rays[kGainRayOpaque] = (int32_t)sum[kPartRay + kGainRayOpaque];
  c.rays[kGainRayOffMap] = (int32_t)sum[kPartRay + kGainRayOffMap];
  c.rays[kGainRayRange] = (int32_t)sum[kPartRay + kGainRayRange];
  c.nearest_opaque_d2 = sum[kPartMin];
  const bool use_field = (a.flags & GVX2_GAIN_USE_FIELD) != 0u;
  const gvx2_gain_record r = gain_record(a.rule, entry, c, use_field, use_field ? a.field[entry] : 0u);
  a.rec[b] = r;
  if (a.rec_out) a.rec_out[b] = r;
}

__global__ void __launch_bounds__(256) k_gain_finish(GainArgs a)
{
  __shared__ unsigned long long wave_best[4];
  __shared__ uint32_t wave_ranked[4];
  const int t = (int)threadIdx.x;
  int32_t n_cand = a.n;
  if (a.frec) {
    const int32_t w = a.finfo->n_written;
    n_cand = w < a.n ? w : a.n;
  }
  uint64_t best = kGainNoKey;
  uint32_t ranked = 0u;
  for (int32_t i = t; i < n_cand; i += 256) {
    const gvx2_gain_record r = a.rec[i];
    const uint64_t key = gain_best_key(r, i);
    best = key > best ? key : best;
    ranked += r.status == 0u ? 1u : 0u;
  }
  best = wave_max64(best);
  ranked = wave_reduce<OpAdd>(ranked);
  if ((t & 63) == 0) {
    wave_best[t >> 6] = best;
    wave_ranked[t >> 6] = ranked;
  }
  __syncthreads();
  if (t != 0) return;
  for (int k = 1; k < 4; ++k) {
    best = wave_best[k] > best ? wave_best[k] : best;
    ranked += wave_ranked[k];
  }
  const gvx2_gain_info I = gain_info(n_cand, (int32_t)ranked, best, a.rec, a.flags, a.rule.radius);
  *a.info = I;
  if (a.info_out) *a.info_out = I;
}

__global__ void __launch_bounds__(64) k_nav_seeds_gain(NavArgs a, GainSeedArgs f)
{
  if (threadIdx.x != 0u) return;
  const int32_t k = f.k < 0 ? f.info->best : f.k;
  if (k < 0 || k >= f.info->n_candidates) return;          // no best, or a slot behind the candidates: no usable seed
  const gvx2_gain_record r = f.rec[k];
  if (r.status & GVX2_GAIN_INVALID) return;
  const int c = r.entry;
  if ((unsigned)c >= (unsigned)a.G || a.field[c] == GV_NAV_BLOCKED) return;   // as k_nav_seeds: a blocked cell is no seed
  a.field[c] = 0u;
  const int y = c / a.nx, x = c - y * a.nx;
  a.flags_out[(y / kNavTile) * a.tiles_x + x / kNavTile] = 1u;
  atomicAdd(a.counter, 1u);
}

// More than 64 KB of dynamic LDS (R of 208 and above) has to be announced for the kernel: raised to the largest window's size,
// on the device of the call.
bool launch_gain(const GainArgs &a, hipStream_t s)
{
  const size_t lds = gain_lds_bytes(a.rule.radius);
  if (lds > 64u * 1024u &&
      hipFuncSetAttribute(reinterpret_cast<const void *>(&k_gain_rays), hipFuncAttributeMaxDynamicSharedMemorySize,
                          (int)gain_lds_bytes(kGainMaxRadius)) != hipSuccess)
    return false;
  hipLaunchKernelGGL(k_gain_rays, dim3((uint32_t)a.n), dim3((uint32_t)gain_threads(a.rule.radius)), (uint32_t)lds, s, a);
  hipLaunchKernelGGL(k_gain_finish, dim3(1), dim3(256), 0, s, a);
  return true;
}

void launch_nav_seeds_gain(const NavArgs &a, const GainSeedArgs &f, hipStream_t s)
{
  hipLaunchKernelGGL(k_nav_seeds_gain, dim3(1), dim3(64), 0, s, a, f);
}

}  // namespace gv
