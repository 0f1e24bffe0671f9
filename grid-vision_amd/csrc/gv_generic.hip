// gv_generic.hip -- gfx950 (CDNA4, wave64) kernels of the generic frame path: the points pass with its LDS hit cache
// and the literal ray march (compact + march); its grid pass, cell by cell, is in gv_gridpass.hip.  Any grid shape
// takes this path, and so does GV_RAY_IMPL=simple; the production frame on a tile-aligned grid goes through
// gv_binning.hip and gv_raysector.hip instead.
//
// Built with -ffp-contract=off: the reference arithmetic keeps separate
// multiply/add roundings (PCL's SSE transform, grid_map's getIndex), and cell
// indices must be bit-exact, so no FMA contraction anywhere in this file.
// fp64 and fp32 divisions are the compiler's correctly rounded sequences.
//
// Reference lines are cited as file:line relative to the reference root.
#include "gv_launch_frame.hpp"
#include "gv_device.hpp"

#include <algorithm>
#include <cstdlib>

namespace gv {

// ------------------------------------------------------------ points pass --
// Generic points pass (any grid shape; also the bbox-only calls of the reference surface).
// The tile path of the production frame bins through gv_binning.hip instead.
// One pass over the resident SoA cloud (12 B/point read):
//   X1  base<-lidar transform, getIndex, hits[cell] += 1
//   X2  ray end of out-of-map points (clip_end[cell] = 1)
//   A1+A5 camera<-lidar transform, pinhole projection, first-match bbox id
//       (src/cloud_detections.cpp:250-298)
// Hit counting: points of one workgroup that fall into the same cell (the cells next to the
// sensor collect hundreds of hits per frame) are combined in an LDS direct-mapped cache
// (cell -> count) and flushed with ONE global atomicAdd per cached cell; a cell that loses its
// slot to another cell goes straight to the global atomic.  Integer adds: the grid is the same
// whatever the interleaving.
constexpr int kHitSlots = 4096;
constexpr unsigned kHitEmpty = 0xFFFFFFFFu;

template <bool BIN, bool RAY, bool BBOX, bool KEEPCELL>
__global__ void __launch_bounds__(BIN ? 1024 : 256) k_points(PointsArgs a)
{
  __shared__ unsigned s_key[BIN ? kHitSlots : 1];
  __shared__ unsigned s_cnt[BIN ? kHitSlots : 1];
  if (BIN) {
    for (int k = threadIdx.x; k < kHitSlots; k += blockDim.x) { s_key[k] = kHitEmpty; s_cnt[k] = 0; }
    __syncthreads();
  }
  // Out-of-map points (a minority) need the fp64 slab clip, ~10x the work of an in-map point: they
  // are compacted through LDS so that the clip runs on dense lanes of as few wavefronts as
  // possible instead of on a few lanes of every wavefront.
  constexpr bool CLIP = BIN && RAY;
  constexpr int kMaxThreads = BIN ? 1024 : 256;
  __shared__ float2 s_out[CLIP ? kMaxThreads : 1];
  __shared__ unsigned s_nout;
  const BBoxTest bt = a.bt;
  const uint32_t stride = gridDim.x * blockDim.x;
  for (uint32_t base = blockIdx.x * blockDim.x; base < a.n; base += stride) {   // uniform per workgroup
    const uint32_t i = base + threadIdx.x;
    const bool live = i < a.n;
    if (CLIP) {
      if (threadIdx.x == 0) s_nout = 0;
      __syncthreads();
    }
    float px = 0.f, py = 0.f, pz = 0.f;
    if (live) { px = a.x[i]; py = a.y[i]; pz = a.z[i]; }
    if (BIN) {
      float bx, by, bz;
      xform34(a.m_base, px, py, pz, bx, by, bz);
      int cell = -1;
      bool outside = false;
      if (live && isfinite(bx) && isfinite(by) && isfinite(bz)) {
        // X4 height band (gv_binning.hip, k_bin_partition): obstacles are hits, clearing ground returns ray ends
        const bool obs = !(bz < a.band.z_ground) && !(bz > a.band.z_max);
        const bool gnd = RAY && a.org.valid && bz < a.band.z_ground && a.band.clears;
        int ix, iy;
        if (get_index_fast(a.g, (double)bx, (double)by, ix, iy)) {
          cell = iy * a.g.nx + ix;
          if (obs) {
            const unsigned slot = ((unsigned)cell * 2654435761u) >> 20;   // 12 bits
            const unsigned old = atomicCAS(&s_key[slot], kHitEmpty, (unsigned)cell);
            if (old == kHitEmpty || old == (unsigned)cell) atomicAdd(&s_cnt[slot], 1u);
            else atomicAdd(&a.hits[cell], 1);   // no-return global_atomic_add
          } else if (gnd) {
            a.clip_end[cell] = 1;   // ray end at its own cell, own cell included (idempotent byte store)
          }
        } else if (RAY && a.org.valid && (obs || gnd)) {
          outside = true;
        }
      }
      if (CLIP) {
        const unsigned long long bm = __ballot(outside);
        if (bm) {
          const int lane = threadIdx.x & 63;
          const unsigned wbase = wave_append_all(&s_nout, bm, lane);
          if (outside) s_out[wbase + wave_rank(bm, lane)] = make_float2(bx, by);
        }
      }
      if (KEEPCELL && live) a.cell_idx[i] = cell;
    }
    if (BBOX) {
      float cx, cy, cz;
      xform34(a.m_cam, px, py, pz, cx, cy, cz);
      if (live) a.bbox_id[i] = (int16_t)first_bbox(a.cam, bt, cx, cy, cz);
    }
    if (CLIP) {
      __syncthreads();
      const unsigned nout = s_nout;
      for (unsigned k = threadIdx.x; k < nout; k += blockDim.x) {
        const float2 p = s_out[k];
        int ex, ey;
        clip_ray_end(a.g, a.org, (double)p.x, (double)p.y, ex, ey);
        a.clip_end[ey * a.g.nx + ex] = 1;   // idempotent byte store
      }
      __syncthreads();   // the list is reused by the next chunk
    }
  }
  if (BIN) {
    __syncthreads();
    for (int k = threadIdx.x; k < kHitSlots; k += blockDim.x) {
      const unsigned key = s_key[k];
      if (key != kHitEmpty) atomicAdd(&a.hits[key], (int)s_cnt[k]);
    }
  }
}

void launch_points(const PointsArgs &a, hipStream_t s)
{
  if (a.n == 0) return;
  // counting: 8192 points per 1024-thread workgroup (measured best of 2k..16k) so that the LDS hit cache
  // sees the duplicates of the hot cells; bbox-only: plain streaming configuration
  const uint32_t threads = a.do_bin ? 1024u : 256u;
  const uint32_t blocks = a.do_bin ? (uint32_t)std::min<uint64_t>(((uint64_t)a.n + 8191) / 8192, (uint64_t)2048)
                                   : (uint32_t)std::min<uint64_t>(((uint64_t)a.n + 255) / 256, (uint64_t)1 << 20);
  const bool keep = a.cell_idx != nullptr;
#define GV_LP(B, R, X, K) hipLaunchKernelGGL((k_points<B, R, X, K>), dim3(blocks), dim3(threads), 0, s, a)
  if (a.do_bin && a.do_ray && a.do_bbox && keep) GV_LP(true, true, true, true);
  else if (a.do_bin && a.do_ray && a.do_bbox) GV_LP(true, true, true, false);
  else if (a.do_bin && a.do_ray && keep) GV_LP(true, true, false, true);
  else if (a.do_bin && a.do_ray) GV_LP(true, true, false, false);
  else if (a.do_bin && a.do_bbox && keep) GV_LP(true, false, true, true);
  else if (a.do_bin && a.do_bbox) GV_LP(true, false, true, false);
  else if (a.do_bin && keep) GV_LP(true, false, false, true);
  else if (a.do_bin) GV_LP(true, false, false, false);
  else if (a.do_bbox) GV_LP(false, false, true, false);
#undef GV_LP
}

// --------------------------------------------------------- ray march (X2) --
// Pass 1: compact the ray ends.  A cell is an end if it has hits (end exclusive)
// and/or a clipped out-of-map ray ends there (end inclusive); both at once is the
// inclusive ray (same path).  entry = cell | include_end << 31.
__global__ void __launch_bounds__(256) k_ray_compact(const int32_t *__restrict__ hits,
                                                     const uint8_t *__restrict__ clip_end, int32_t G,
                                                     uint32_t *__restrict__ list, uint32_t *__restrict__ count)
{
  const int lane = threadIdx.x & 63;
  const int32_t stride = gridDim.x * blockDim.x;
  for (int32_t base = blockIdx.x * blockDim.x; base < G; base += stride) {
    const int32_t c = base + threadIdx.x;
    bool is_end = false;
    uint32_t e = 0;
    if (c < G) {
      const int h = hits[c];
      const uint8_t k = clip_end[c];
      is_end = (h > 0) || k;
      e = (uint32_t)c | (k ? 0x80000000u : 0u);
    }
    const unsigned long long m = __ballot(is_end);
    if (m) {
      uint32_t b = 0;
      if (lane == 0) b = atomicAdd(count, (uint32_t)__popcll(m));
      b = wave_bcast(b, 0);   // (through the permute network, not wave_append_all's scalar register: as measured here)
      if (is_end) list[b + wave_rank(m, lane)] = e;
    }
  }
}

void launch_ray_compact(const RayCompactArgs &a, hipStream_t s)
{
  const uint32_t blocks = (uint32_t)std::min<int64_t>(((int64_t)a.g.G + 255) / 256, (int64_t)256 * 8);
  hipLaunchKernelGGL(k_ray_compact, dim3(blocks), dim3(256), 0, s, a.hits, a.clip_end, a.g.G, a.list, a.count);
}

// Pass 2: one wavefront per ray, lanes over the steps.  grid_map::LineIterator
// stepping in closed form: after i steps along the major axis the minor offset is
// (major/2 + i*minor) / major (integer division).
__global__ void __launch_bounds__(256) k_ray_march(const uint32_t *__restrict__ list,
                                                   const uint32_t *__restrict__ count, GridParams g,
                                                   RayOrigin o, uint8_t *__restrict__ miss,
                                                   unsigned long long *__restrict__ stats)
{
  const int lane = threadIdx.x & 63;
  const uint32_t wave = (blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  const uint32_t nwaves = (gridDim.x * blockDim.x) >> 6;
  const uint32_t n = *count;
  unsigned long long visits = 0;
  for (uint32_t r = wave; r < n; r += nwaves) {
    const uint32_t e = list[r];
    const int inc = (int)(e >> 31);
    const int cell = (int)(e & 0x7fffffffu);
    const int ey = cell / g.nx, ex = cell - ey * g.nx;
    const int dx = ex - o.cx, dy = ey - o.cy;
    const int adx = abs(dx), ady = abs(dy);
    const int sx = (dx >= 0) ? 1 : -1, sy = (dy >= 0) ? 1 : -1;
    const bool xmaj = adx >= ady;
    const int major = xmaj ? adx : ady, minor = xmaj ? ady : adx;
    const int half = major / 2;
    const int nmark = inc ? major + 1 : major;
    const double rcp = major ? 1.0 / (double)major : 0.0;
    for (int i = lane; i < nmark; i += 64) {
      const int num = half + i * minor;
      int q = (int)((double)num * rcp);
      const int rem = num - q * major;        // exact integer quotient after one correction
      if (major == 0) q = 0;                  // a clipped end in the origin cell itself: the line is that one cell
      else if (rem >= major) ++q;
      else if (rem < 0) --q;
      const int cx = o.cx + sx * (xmaj ? i : q);
      const int cy = o.cy + sy * (xmaj ? q : i);
      miss[(size_t)cy * g.nx + cx] = 1;
    }
    visits += (unsigned long long)nmark;
  }
  if (lane == 0 && stats) {
    if (visits) atomicAdd(&stats[1], visits);
    if (wave == 0) atomicAdd(&stats[0], (unsigned long long)n);
  }
}

void launch_ray_march(const RayMarchArgs &a, hipStream_t s)
{
  if (!a.org.valid) return;
  hipLaunchKernelGGL(k_ray_march, dim3(256 * 8), dim3(256), 0, s, a.list, a.count, a.g, a.org, a.miss, a.stats);
}

}  // namespace gv
