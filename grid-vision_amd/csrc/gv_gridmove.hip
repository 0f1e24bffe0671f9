// gv_gridmove.hip -- [EXTENSION] X3 ego-motion compensation (gv_grid_move): nearest-cell resample of the three grid
// layers under a planar rigid transform S, grid_map's GridMap::move() for a grid registered to the base frame.
//
// New cell (ix, iy) takes the values of the old cell containing S applied to its centre:
//   centre  c = (pos + off) - (i + 0.5) * res                       (fp64, per axis)
//   source  (c0*cx - s0*cy) + tx,  (s0*cx + c0*cy) + ty             (no FMA: -ffp-contract=off)
//   cell    grid_map getIndex of the source (get_index_fast: the exact division decides near a cell border)
// Off-map sources take the constructor state (0.0f, 0.5f, 50).  Values are copied, never recomputed, so all three
// layers stay bit for bit what the oracle's update sequence produces.  The gather writes a scratch copy of the
// layers and one copy kernel moves it back: the resident layer pointers (gv_device_layers) never change.
// gfx950, wave64; every store below is a plain vector store from VGPRs.
#include "gv_launch_frame.hpp"
#include "gv_device.hpp"

#include <algorithm>

namespace gv {

__device__ __forceinline__ int move_source(const GridMoveArgs &a, double hx, double hy, int ix, int iy)
{
  const double cx = hx - ((double)ix + 0.5) * a.g.res;
  const double cy = hy - ((double)iy + 0.5) * a.g.res;
  const double sx = (a.c * cx - a.s * cy) + a.tx;
  const double sy = (a.s * cx + a.c * cy) + a.ty;
  int jx, jy;
  return get_index_fast(a.g, sx, sy, jx, jy) ? jy * a.g.nx + jx : -1;
}

// nx % 4 == 0: a lane resamples 4 consecutive cells of one row and writes them as one float4 per float layer and one
// dword of the packed layer (data[G-1-c] order: cells c..c+3 are the bytes G-4-c .. G-1-c, reversed).  A workgroup
// covers 256 x 4 destination cells (G - 1 - c: data_entry, gv_types.hpp, of the linear cell c); for small yaw their sources are a compact, nearly aligned patch.
__global__ void __launch_bounds__(256) k_grid_move4(GridMoveArgs a)
{
  const int ix0 = (int)(blockIdx.x * 64u + threadIdx.x) * 4;
  const int iy = (int)(blockIdx.y * 4u + threadIdx.y);
  if (ix0 >= a.g.nx || iy >= a.g.ny) return;
  const double hx = a.g.pos_x + a.g.off_x, hy = a.g.pos_y + a.g.off_y;
  const int G = a.g.G;
  float lo[4], oc[4];
  uint32_t packed = 0;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int src = move_source(a, hx, hy, ix0 + k, iy);
    uint32_t b = 50u;
    lo[k] = kLogOddsPrior;
    oc[k] = kInitProbability;
    if (src >= 0) {
      lo[k] = a.lo[src];
      oc[k] = a.occ[src];
      b = (uint32_t)(uint8_t)a.i8[G - 1 - src];
    }
    packed |= b << (8 * (3 - k));
  }
  const int c = iy * a.g.nx + ix0;
  *reinterpret_cast<float4 *>(a.lo_out + c) = make_float4(lo[0], lo[1], lo[2], lo[3]);
  *reinterpret_cast<float4 *>(a.occ_out + c) = make_float4(oc[0], oc[1], oc[2], oc[3]);
  *reinterpret_cast<uint32_t *>(a.i8_out + (G - 4 - c)) = packed;
}

// any nx: one cell per lane, 64 x 4 cells per workgroup
__global__ void __launch_bounds__(256) k_grid_move1(GridMoveArgs a)
{
  const int ix = (int)(blockIdx.x * 64u + threadIdx.x);
  const int iy = (int)(blockIdx.y * 4u + threadIdx.y);
  if (ix >= a.g.nx || iy >= a.g.ny) return;
  const int src = move_source(a, a.g.pos_x + a.g.off_x, a.g.pos_y + a.g.off_y, ix, iy);
  const int G = a.g.G, c = iy * a.g.nx + ix;
  float lo = kLogOddsPrior, oc = kInitProbability;
  int8_t b = 50;
  if (src >= 0) {
    lo = a.lo[src];
    oc = a.occ[src];
    b = a.i8[G - 1 - src];
  }
  a.lo_out[c] = lo;
  a.occ_out[c] = oc;
  a.i8_out[G - 1 - c] = b;
}

void launch_grid_move(const GridMoveArgs &a, hipStream_t s)
{
  const dim3 block(64, 4);
  const uint32_t gy = (uint32_t)(a.g.ny + 3) / 4;
  if (a.g.nx % 4 == 0)
    hipLaunchKernelGGL(k_grid_move4, dim3((uint32_t)(a.g.nx / 4 + 63) / 64, gy), block, 0, s, a);
  else
    hipLaunchKernelGGL(k_grid_move1, dim3((uint32_t)(a.g.nx + 63) / 64, gy), block, 0, s, a);
}

// The copy back: segment blockIdx.y of up to three, 16 bytes per lane (both sides 16-byte aligned), the tail bytes by
// the first workgroup of the segment.
struct CopySegments {
  const uint8_t *src[3];
  uint8_t *dst[3];
  size_t bytes[3];
};

__global__ void __launch_bounds__(256) k_copy_segments(CopySegments a)
{
  const uint8_t *src = a.src[blockIdx.y];
  uint8_t *dst = a.dst[blockIdx.y];
  const size_t bytes = a.bytes[blockIdx.y], n16 = bytes / 16;
  const size_t stride = (size_t)gridDim.x * 256u;
  for (size_t i = blockIdx.x * (size_t)256u + threadIdx.x; i < n16; i += stride)
    reinterpret_cast<uint4 *>(dst)[i] = reinterpret_cast<const uint4 *>(src)[i];
  if (blockIdx.x == 0 && n16 * 16 + threadIdx.x < bytes) dst[n16 * 16 + threadIdx.x] = src[n16 * 16 + threadIdx.x];
}

void launch_grid_move_copy_back(const GridMoveArgs &a, hipStream_t s)
{
  const size_t G = (size_t)a.g.G;
  CopySegments c{{reinterpret_cast<const uint8_t *>(a.lo_out), reinterpret_cast<const uint8_t *>(a.occ_out),
                  reinterpret_cast<const uint8_t *>(a.i8_out)},
                 {reinterpret_cast<uint8_t *>(a.lo), reinterpret_cast<uint8_t *>(a.occ), reinterpret_cast<uint8_t *>(a.i8)},
                 {G * sizeof(float), G * sizeof(float), G}};
  const uint32_t blocks = (uint32_t)std::min<size_t>(std::max<size_t>((G * sizeof(float) / 16 + 255) / 256, 1), 1024);
  hipLaunchKernelGGL(k_copy_segments, dim3(blocks, 3), dim3(256), 0, s, c);
}

}  // namespace gv
