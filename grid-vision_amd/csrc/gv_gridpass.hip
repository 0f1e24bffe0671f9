// gv_gridpass.hip -- the grid pass: the map update rule, one text of it, and the three kernels that apply it to the
// cells.  gfx950, wave64.
//   k_finalize_tiles<COUNTS>   the production frame on a tile-aligned grid: 64-cell-wide tiles, hit and free-space
//                              flags from the bitmaps of the binning and ray stages (gv_binning.hip, gv_raysector.hip)
//   k_finalize_vec4<COUNTS>    any grid with nx % 4 == 0: four cells per thread, per-cell hit / miss counts
//   k_finalize_scalar<COUNTS>  any grid shape, cell by cell (both: the generic path of gv_generic.hip, GV_RAY_IMPL=simple)
// and k_miss_to_i32, the free-cell bitmaps read back as one int32 per cell.
//
// Built with -ffp-contract=off: the rule keeps the reference's separate roundings (no FMA contraction).
//
// Reference lines are cited as file:line relative to the reference root.
#include "gv_launch_frame.hpp"

#include <hip/hip_ext.h>

#include <algorithm>

namespace gv {

// --------------------------------------------------------------- cell rule --
// One pass over the cells (A7/A8/A9/A18 + the X2 rule):
//   l += decay (:19/:69); l += 0.85f per covering rectangle, in object order (:175-182);
//   hits>0 -> l += 1.2f, else miss>0 -> l += -0.4f  [EXTENSION];
//   clamp (:21-22); occupancy = 1/(1+exp(-l)) (:25-30); int8 = (int8)(clamp01(p)*100)
//   stored at data[G-1-cell] (toOccupancyGrid).
__device__ __forceinline__ float sigmoid_ref(float l)
{
  // exp in fp64 rounded once: the correctly rounded expf (on the host it agrees on all fp32 inputs in [-3.6, 2];
  // glibc's expf, which the oracle calls, is one ulp off on 118,468 of them, tests/test_gpu_grid_pass.py).
  // An fp32 expf measured +2 % on the frame, round 3.
  const float e = (float)exp((double)(-l));
  return 1.0f / (1.0f + e);
}

// the int8 of p as the low byte of a word (the callers pack four of them, or narrow the one they store)
__device__ __forceinline__ unsigned pack_i8(float p)
{
  float v = (p - 0.0f) / (1.0f - 0.0f);
  if (isnan(v)) v = -1.0f;
  else {
    float c = v < 0.0f ? 0.0f : v;
    c = c > 1.0f ? 1.0f : c;
    v = 0.0f + c * 100.0f;
  }
  return (unsigned)(unsigned char)(signed char)v;
}

__device__ __forceinline__ float cell_update(float l, int k, bool counts, bool hit, bool miss)
{
  l = l + kLogOddsDecay;
  for (int r = 0; r < k; ++r) l = l + kRectIncrement;
  if (counts) {
    if (hit) l = l + kLogOddsOccupied;
    else if (miss) l = l + kLogOddsFree;
  }
  l = (l < kMinLogOdds) ? kMinLogOdds : l;
  l = (l > kMaxLogOdds) ? kMaxLogOdds : l;
  return l;
}

// ------------------------------------------------------- tile grid pass -----
// One 64x64 tile per workgroup.  Requires nx % 4 == 0.  Per cell: 4 B log-odds in, 4 + 4 + 1 B out (nothing out
// for a tile row that did not change, unless a.dense); hit and free-space flags come from the bitmaps (N: one word per 32 cells of a row; T: bits run
// along y, a thread's four cells are four consecutive words = one 16-byte load).  Nothing is cleared
// here: the binning tile pass rewrites / zeroes every bitmap word of the set it is about to use.
#ifndef GV_FIN_ROWS
#define GV_FIN_ROWS 64
#endif
template <bool COUNTS>
__global__ void __launch_bounds__(256) k_finalize_tiles(FinalizeTileArgs a)
{
  __shared__ Rect s_rects[64];
  __shared__ int s_nr;
  constexpr int kRows = GV_FIN_ROWS;   // rows of the grid per workgroup (64 cells wide): 16 per pass
  const int x0 = blockIdx.x * 64, y0 = a.y_begin + blockIdx.y * kRows;
  const int tid = threadIdx.x;
  GV_TL_BEGIN(a.tl);
  if (tid == 0) s_nr = 0;
  __syncthreads();
  // rectangles that touch this tile (object order must be kept only for equal cells:
  // all adds are the same constant, so the count is what matters)
  for (int r = tid; r < a.n_rects; r += 256) {
    const Rect R = a.rects[r];
    if (R.valid && R.y1 >= y0 && R.y0 <= y0 + kRows - 1 && R.x1 >= x0 && R.x0 <= x0 + 63) {
      const int k = atomicAdd(&s_nr, 1);
      if (k < 64) s_rects[k] = R;
    }
  }
  __syncthreads();
  const int nr = min(s_nr, 64);
  const bool overflow = s_nr > 64;
  const int xq = tid & 15;        // which float4 of the row
  const int x = x0 + xq * 4;
#pragma unroll
  for (int pass = 0; pass < kRows / 16; ++pass) {
    const int yl = pass * 16 + (tid >> 4);
    const int y = y0 + yl;
    if (x >= a.g.nx || y >= a.y_end) continue;
    const size_t c = (size_t)y * a.g.nx + x;
    float4 l4 = *reinterpret_cast<const float4 *>(a.log_odds + c);
    unsigned hb = 0, fb = 0;
    if (COUNTS) {
      const size_t wn = (size_t)(x >> 5) * a.ny_pad + y;
      hb = (a.hitN[wn] >> (x & 31)) & 0xFu;
      fb = (a.freeN[wn] >> (x & 31)) & 0xFu;
      const uint4 ft = *reinterpret_cast<const uint4 *>(a.freeT + (size_t)(y >> 5) * a.nx_pad + x);
      const int by = y & 31;
      fb |= ((ft.x >> by) & 1u) | (((ft.y >> by) & 1u) << 1) | (((ft.z >> by) & 1u) << 2) | (((ft.w >> by) & 1u) << 3);
    }
    // (the 4-wide count stands three times, twice here and once in k_finalize_vec4, on purpose: behind one
    // __forceinline__ helper the compiler scheduled this kernel differently, ~1,600 assembly lines of each instantiation)
    int k0 = 0, k1 = 0, k2 = 0, k3 = 0;
    if (!overflow) {
      for (int r = 0; r < nr; ++r) {
        const Rect R = s_rects[r];
        if (y >= R.y0 && y <= R.y1) {
          k0 += (x >= R.x0 && x <= R.x1);
          k1 += (x + 1 >= R.x0 && x + 1 <= R.x1);
          k2 += (x + 2 >= R.x0 && x + 2 <= R.x1);
          k3 += (x + 3 >= R.x0 && x + 3 <= R.x1);
        }
      }
    } else {
      for (int r = 0; r < a.n_rects; ++r) {
        const Rect R = a.rects[r];
        if (R.valid && y >= R.y0 && y <= R.y1) {
          k0 += (x >= R.x0 && x <= R.x1);
          k1 += (x + 1 >= R.x0 && x + 1 <= R.x1);
          k2 += (x + 2 >= R.x0 && x + 2 <= R.x1);
          k3 += (x + 3 >= R.x0 && x + 3 <= R.x1);
        }
      }
    }
    const unsigned o0 = __float_as_uint(l4.x), o1 = __float_as_uint(l4.y), o2 = __float_as_uint(l4.z), o3 = __float_as_uint(l4.w);
    l4.x = cell_update(l4.x, k0, COUNTS, hb & 1u, fb & 1u);
    l4.y = cell_update(l4.y, k1, COUNTS, hb & 2u, fb & 2u);
    l4.z = cell_update(l4.z, k2, COUNTS, hb & 4u, fb & 4u);
    l4.w = cell_update(l4.w, k3, COUNTS, hb & 8u, fb & 8u);
    // A tile row (16 lanes, 64 cells: 256 B of each float layer, 64 B of the packed one) whose log-odds all came
    // back with the bits they had is left alone: with the layers in step (gv_context::layers_in_step) occupancy and
    // the packed grid already hold what would be stored.  Bits, not ==: a NaN equals itself, -0.0 is not 0.0.
    // A row with any changed cell is written whole, so every store stays a full 64-byte piece or more.
    if (!a.dense) {
      const bool changed = ((__float_as_uint(l4.x) ^ o0) | (__float_as_uint(l4.y) ^ o1) | (__float_as_uint(l4.z) ^ o2) |
                            (__float_as_uint(l4.w) ^ o3)) != 0u;
      const unsigned long long rows = __ballot(changed);   // lanes outside the grid are inactive here: no bit
      if (((rows >> (tid & 48)) & 0xFFFFull) == 0ull) continue;
    }
    float4 p4;
    p4.x = sigmoid_ref(l4.x); p4.y = sigmoid_ref(l4.y); p4.z = sigmoid_ref(l4.z); p4.w = sigmoid_ref(l4.w);
    *reinterpret_cast<float4 *>(a.log_odds + c) = l4;   // read again by the next frame
    // occupancy and the packed grid are outputs nobody reads on the device: streaming stores
    typedef float v4f __attribute__((ext_vector_type(4)));
    v4f np4; np4.x = p4.x; np4.y = p4.y; np4.z = p4.z; np4.w = p4.w;
    __builtin_nontemporal_store(np4, reinterpret_cast<v4f *>(a.occupancy + c));
    const unsigned packed = pack_i8(p4.w) | (pack_i8(p4.z) << 8) | (pack_i8(p4.y) << 16) | (pack_i8(p4.x) << 24);
    __builtin_nontemporal_store(packed, reinterpret_cast<unsigned *>(a.occ_i8 + ((size_t)a.g.G - 4 - c)));
  }
  GV_TL_END(a.tl);
}

// `done` (optional) completes with the kernel, on its own dispatch packet (see launch_ray_sectors);
// false: nothing launched
bool launch_finalize_tiles(const FinalizeTileArgs &a, hipStream_t s, hipEvent_t done, hipEvent_t t0)
{
  const int rows = a.y_end - a.y_begin;
  if (rows <= 0) return false;
  const dim3 grid((a.g.nx + 63) / 64, (rows + GV_FIN_ROWS - 1) / GV_FIN_ROWS);
  if (a.counts) hipExtLaunchKernelGGL(k_finalize_tiles<true>, grid, dim3(256), 0, s, t0, done, 0, a);
  else hipExtLaunchKernelGGL(k_finalize_tiles<false>, grid, dim3(256), 0, s, t0, done, 0, a);
  return true;
}

// ---------------------------------------------------- generic grid pass -----
// The same rule with per-cell counts (hits int32, miss bytes of the literal march) in place of the bitmaps.
template <bool COUNTS>
__global__ void __launch_bounds__(256) k_finalize_vec4(FinalizeArgs a)
{
  // requires nx % 4 == 0 and band edges % 4 == 0: the 4 cells of a thread share a row
  const int64_t q0 = a.cell_begin >> 2, q1 = a.cell_end >> 2;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t q = q0 + blockIdx.x * (int64_t)blockDim.x + threadIdx.x; q < q1; q += stride) {
    const int64_t c = q << 2;
    const int iy = (int)(c / a.g.nx), ix = (int)(c - (int64_t)iy * a.g.nx);
    float4 l4 = *reinterpret_cast<const float4 *>(a.log_odds + c);
    int4 h4 = make_int4(0, 0, 0, 0);
    uint32_t m4 = 0;
    if (COUNTS) {
      h4 = *reinterpret_cast<const int4 *>(a.hits + c);
      m4 = *reinterpret_cast<const uint32_t *>(a.miss + c);
    }
    int k0 = 0, k1 = 0, k2 = 0, k3 = 0;
    for (int r = 0; r < a.n_rects; ++r) {
      const Rect R = a.rects[r];
      if (R.valid && iy >= R.y0 && iy <= R.y1 && ix + 3 >= R.x0 && ix <= R.x1) {
        k0 += (ix >= R.x0 && ix <= R.x1);
        k1 += (ix + 1 >= R.x0 && ix + 1 <= R.x1);
        k2 += (ix + 2 >= R.x0 && ix + 2 <= R.x1);
        k3 += (ix + 3 >= R.x0 && ix + 3 <= R.x1);
      }
    }
    l4.x = cell_update(l4.x, k0, COUNTS, h4.x > 0, (m4 & 0xffu) > 0);
    l4.y = cell_update(l4.y, k1, COUNTS, h4.y > 0, ((m4 >> 8) & 0xffu) > 0);
    l4.z = cell_update(l4.z, k2, COUNTS, h4.z > 0, ((m4 >> 16) & 0xffu) > 0);
    l4.w = cell_update(l4.w, k3, COUNTS, h4.w > 0, (m4 >> 24) > 0);
    float4 p4;
    p4.x = sigmoid_ref(l4.x); p4.y = sigmoid_ref(l4.y); p4.z = sigmoid_ref(l4.z); p4.w = sigmoid_ref(l4.w);
    *reinterpret_cast<float4 *>(a.log_odds + c) = l4;
    *reinterpret_cast<float4 *>(a.occupancy + c) = p4;
    // data[G-1-cell] (data_entry, gv_types.hpp, of the linear cell): cells c..c+3 land at G-4-c .. G-1-c in reverse order
    const uint32_t packed = pack_i8(p4.w) | (pack_i8(p4.z) << 8) | (pack_i8(p4.y) << 16) | (pack_i8(p4.x) << 24);
    *reinterpret_cast<uint32_t *>(a.occ_i8 + ((int64_t)a.g.G - 4 - c)) = packed;
    if (COUNTS && a.zero_counts) {
      *reinterpret_cast<int4 *>(a.hits + c) = make_int4(0, 0, 0, 0);
      *reinterpret_cast<uint32_t *>(a.miss + c) = 0u;
      *reinterpret_cast<uint32_t *>(a.clip_end + c) = 0u;
    }
  }
}

template <bool COUNTS>
__global__ void __launch_bounds__(256) k_finalize_scalar(FinalizeArgs a)
{
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t c = a.cell_begin + blockIdx.x * (int64_t)blockDim.x + threadIdx.x; c < a.cell_end; c += stride) {
    const int iy = (int)(c / a.g.nx), ix = (int)(c - (int64_t)iy * a.g.nx);
    int k = 0;
    for (int r = 0; r < a.n_rects; ++r) {
      const Rect R = a.rects[r];
      k += (R.valid && iy >= R.y0 && iy <= R.y1 && ix >= R.x0 && ix <= R.x1);
    }
    const int h = COUNTS ? a.hits[c] : 0;
    const int m = COUNTS ? (int)a.miss[c] : 0;
    const float l = cell_update(a.log_odds[c], k, COUNTS, h > 0, m > 0);
    const float p = sigmoid_ref(l);
    a.log_odds[c] = l;
    a.occupancy[c] = p;
    a.occ_i8[(int64_t)a.g.G - 1 - c] = (int8_t)pack_i8(p);
    if (COUNTS && a.zero_counts) {
      a.hits[c] = 0;
      a.miss[c] = 0;
      a.clip_end[c] = 0;
    }
  }
}

void launch_finalize(const FinalizeArgs &a, hipStream_t s)
{
  const int64_t ncell = a.cell_end - a.cell_begin;
  if (ncell <= 0) return;
  const bool vec = (a.g.nx % 4 == 0) && (a.cell_begin % 4 == 0) && (a.cell_end % 4 == 0);
  const bool counts = a.hits != nullptr;
  if (vec) {
    const uint32_t blocks = (uint32_t)std::min<int64_t>((ncell / 4 + 255) / 256, (int64_t)256 * 16);
    if (counts) hipLaunchKernelGGL(k_finalize_vec4<true>, dim3(blocks), dim3(256), 0, s, a);
    else hipLaunchKernelGGL(k_finalize_vec4<false>, dim3(blocks), dim3(256), 0, s, a);
  } else {
    const uint32_t blocks = (uint32_t)std::min<int64_t>((ncell + 255) / 256, (int64_t)256 * 16);
    if (counts) hipLaunchKernelGGL(k_finalize_scalar<true>, dim3(blocks), dim3(256), 0, s, a);
    else hipLaunchKernelGGL(k_finalize_scalar<false>, dim3(blocks), dim3(256), 0, s, a);
  }
}

// ------------------------------------------------------- miss read-back -----
// free-cell bitmaps N | T as int32 0/1 per cell
__global__ void __launch_bounds__(256) k_miss_to_i32(const unsigned *__restrict__ fN, const unsigned *__restrict__ fT,
                                                     int nx, int ny, int nx_pad, int ny_pad,
                                                     int32_t *__restrict__ out)
{
  const size_t G = (size_t)nx * ny;
  const size_t stride = (size_t)gridDim.x * blockDim.x;
  for (size_t c = blockIdx.x * (size_t)blockDim.x + threadIdx.x; c < G; c += stride) {
    const int y = (int)(c / nx), x = (int)(c - (size_t)y * nx);
    const unsigned n = fN[(size_t)(x >> 5) * ny_pad + y] >> (x & 31);
    const unsigned t = fT[(size_t)(y >> 5) * nx_pad + x] >> (y & 31);
    out[c] = (int32_t)((n | t) & 1u);
  }
}

void launch_miss_to_i32(const MissToI32Args &a, hipStream_t s)
{
  hipLaunchKernelGGL(k_miss_to_i32, dim3(2048), dim3(256), 0, s, a.freeN, a.freeT, a.nx, a.ny, a.nx_pad, a.ny_pad, a.out);
}

}  // namespace gv
