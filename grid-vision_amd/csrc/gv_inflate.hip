// gv_inflate.hip -- [EXTENSION] X6 inflated costmap layer (gv_inflate): the exact squared Euclidean distance of every
// cell to the nearest lethal cell, bounded by d2max, and the cost the host-built table gives for it
// (include/gridvision_hip.h has the definition).
//
// Everything works in OccupancyGrid.data order, the order of the packed int8 layer: byte y * nx + x is "row" y,
// "column" x.  That is the cell order turned by 180 degrees, and distances do not care, so nothing is reversed.
//   k_lethal_bits    packed layer -> bitmap, one bit per cell along x (one ballot per 64 cells), rows padded to whole
//                    64-bit words with a zero guard word on either side;
//   k_inflate_tiles  a 64 x 64 tile per workgroup.  The window -- the tile's rows and rc halo rows above and below, the
//                    tile's bitmap word and its two neighbours -- is loaded once, a row per thread, into LDS.  A tile
//                    whose whole window holds no lethal bit writes zeros and leaves (most tiles of a real map).
//                    Phase A: lane x finds g = the distance along a row to its nearest lethal bit within +-rc (shifts,
//                    count leading / trailing zeros), one byte per cell in LDS.  Phase B: a lane owns a column and 16
//                    rows, d2 = min over the rows dy of dy^2 + g^2 in integers, then cost = table[d2] from LDS.  Rows
//                    more than rc away cannot matter: (rc + 1)^2 > d2max.  The results are staged in LDS and stored
//                    4 cells per lane where nx % 4 == 0, a cell per lane otherwise: the one difference between sizes.
// Any nx, ny: cells past the map are computed and not stored; rows off the map hold no obstacle.
// gfx950, wave64; every store below is a plain vector store from VGPRs.
#include "gv_launch_planner.hpp"
#include "gv_device.hpp"

namespace gv {

namespace {
constexpr int kTile = 64;                         // cells per tile side = bits per bitmap word = lanes per wavefront
constexpr int kMaxRc = 63;                        // a row's window is the tile's word and its two neighbours
constexpr int kNoG = 255;                         // LDS byte: no lethal bit of this row within rc
constexpr int kRowsPerLane = kTile / 4;           // phase B: four wavefronts share the tile's rows
constexpr int kTableMax = (kMaxRc + 1) * (kMaxRc + 1);   // d2max + 1 <= 4096
}  // namespace

// Wavefront w of a workgroup: row blockIdx.y * 4 + w, bitmap words blockIdx.x * 4 .. + 3 of it.
__global__ void __launch_bounds__(256) k_lethal_bits(InflateArgs a)
{
  const int lane = (int)(threadIdx.x & 63u), wave = (int)(threadIdx.x >> 6);
  const int y = (int)blockIdx.y * 4 + wave;
  if (y >= a.ny) return;
  const int words = a.row_words - 2;
  const int8_t *row = a.i8 + (size_t)y * (size_t)a.nx;
  unsigned long long *out = a.bits + (size_t)y * (size_t)a.row_words + 1;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int w = (int)blockIdx.x * 4 + k;
    if (w >= words) break;
    const int x = w * 64 + lane;
    const bool lethal = x < a.nx && (int)row[x] >= a.thr;
    const unsigned long long m = __ballot(lethal);
    if (lane == 0) out[w] = m;
  }
}

// The tile's 64 x 64 results to the layers, V cells per store (4 where nx % 4 == 0: a tile starts on a multiple of 64
// cells, so every group of 4 cells of a row is 4-byte aligned in the cost layer and 8-byte aligned in dist2, and lies
// wholly inside or outside the map).  kEmpty: no staged values, every cell is cost 0 / no distance.
template <int V, bool kEmpty>
__device__ __forceinline__ void store_tile(const InflateArgs &a, int x0, int y0, int tid, const uint8_t *cost, const uint16_t *dist2)
{
  constexpr int kPerRow = kTile / V, kUnits = kTile * kPerRow;
#pragma unroll
  for (int k = 0; k < kUnits / 256; ++k) {
    const int u = k * 256 + tid;
    const int row = u / kPerRow, col = (u % kPerRow) * V;
    const int x = x0 + col, y = y0 + row;
    if (y >= a.ny || x >= a.nx) continue;
    const size_t c = (size_t)y * (size_t)a.nx + (size_t)x;
    if constexpr (V == 4) {
      *reinterpret_cast<uint32_t *>(a.cost + c) = kEmpty ? 0u : *reinterpret_cast<const uint32_t *>(cost + row * kTile + col);
      if (a.dist2)
        *reinterpret_cast<uint2 *>(a.dist2 + c) =
            kEmpty ? make_uint2(0xFFFFFFFFu, 0xFFFFFFFFu) : *reinterpret_cast<const uint2 *>(dist2 + row * kTile + col);
    } else {
      a.cost[c] = kEmpty ? (uint8_t)0 : cost[row * kTile + col];
      if (a.dist2) a.dist2[c] = kEmpty ? (uint16_t)65535 : dist2[row * kTile + col];
    }
  }
}

template <int V>
__global__ void __launch_bounds__(256) k_inflate_tiles(InflateArgs a)
{
  constexpr int kRowsMax = kTile + 2 * kMaxRc;
  __shared__ unsigned long long win[kRowsMax * 3];             // the window's three words per row, masked to +-rc of the tile
  __shared__ __attribute__((aligned(16))) uint8_t g[3 * kTile * kTile];   // phase A / B: kRowsMax rows of g; then the staged results
  __shared__ uint8_t table[kTableMax];
  static_assert(kRowsMax * kTile <= 3 * kTile * kTile, "g holds the halo rows");
  const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int x0 = (int)blockIdx.x * kTile, y0 = (int)blockIdx.y * kTile;
  const int rc = a.rc, rows = kTile + 2 * rc;

  // one row of the window per thread (rows <= 190): the tile's own word, the top rc bits of the word to its left and the
  // low rc bits of the word to its right (guard words at the row's ends); rows off the map hold no obstacle
  int any = 0;
  if (tid < rows) {
    const int y = y0 - rc + tid;
    unsigned long long lo = 0ull, mid = 0ull, hi = 0ull;
    if (y >= 0 && y < a.ny) {
      const unsigned long long *p = a.bits + (size_t)y * (size_t)a.row_words + 1 + blockIdx.x;
      lo = rc ? p[-1] & (~0ull << (64 - rc)) : 0ull;
      mid = p[0];
      hi = rc ? p[1] & (~0ull >> (64 - rc)) : 0ull;
    }
    win[tid * 3 + 0] = lo;
    win[tid * 3 + 1] = mid;
    win[tid * 3 + 2] = hi;
    any = (lo | mid | hi) != 0ull;
  }
  if (!__syncthreads_or(any)) {   // empty window: a workgroup-uniform branch
    store_tile<V, true>(a, x0, y0, tid, nullptr, nullptr);
    return;
  }

  for (int i = tid; i <= a.d2max; i += 256) table[i] = a.table[i];

  // phase A: g of the window's rows, a row per wavefront at a time
  for (int r = wave; r < rows; r += 4) {
    const unsigned long long lo = win[r * 3 + 0], mid = win[r * 3 + 1], hi = win[r * 3 + 2];
    int gv = kNoG;
    if ((lo | mid | hi) != 0ull) {
      // up: bit k = the cell k to the right of this lane's (bit 0 its own); down: bit 63 - k = the cell k to the left
      const unsigned long long up = (mid >> lane) | (lane ? hi << (64 - lane) : 0ull);
      const unsigned long long down = (mid << (63 - lane)) | (lane < 63 ? lo >> (lane + 1) : 0ull);
      const int dr = up ? __builtin_ctzll(up) : 64;
      const int dl = down ? __builtin_clzll(down) : 64;
      const int d = dr < dl ? dr : dl;
      if (d <= rc) gv = d;
    }
    g[r * kTile + lane] = (uint8_t)gv;
  }
  __syncthreads();

  // phase B: tile rows i0 .. i0 + 15 of column `lane`; window row i0 + s is dy = s - rc - i away from tile row i0 + i.
  // Two window rows per step; per row c = g^2 + dy^2 is carried from i to i + 1 by c += (2 i + 1) - 2 (s - rc)
  // (one three-operand add), and the two candidates and the running minimum are one three-operand minimum.
  // kNoG^2 = 65025 is above every d2max, so a row without a bit drops out by itself; a pair of rows without one for
  // the whole wavefront is skipped.
  const int i0 = wave * kRowsPerLane;
  unsigned acc[kRowsPerLane];
#pragma unroll
  for (int i = 0; i < kRowsPerLane; ++i) acc[i] = 0xFFFFFFu;
  const int n_src = kRowsPerLane + 2 * rc;   // even
  for (int s = 0; s < n_src; s += 2) {
    const unsigned ga = g[(i0 + s) * kTile + lane], gb = g[(i0 + s + 1) * kTile + lane];
    if (__ballot((ga & gb) != (unsigned)kNoG) == 0ull) continue;
    const int base = s - rc;
    unsigned ca = ga * ga + (unsigned)(base * base), cb = gb * gb + (unsigned)((base + 1) * (base + 1));
    const unsigned da = (unsigned)(-2 * base), db = da - 2u;
#pragma unroll
    for (int i = 0; i < kRowsPerLane; ++i) {
      const unsigned m = ca < cb ? ca : cb;
      acc[i] = m < acc[i] ? m : acc[i];
      ca += da + (unsigned)(2 * i + 1);
      cb += db + (unsigned)(2 * i + 1);
    }
  }
  __syncthreads();   // every wavefront has read its rows of g: the block now stages the results

  uint8_t *const cost_s = g;                                               // [64][64]
  uint16_t *const dist2_s = reinterpret_cast<uint16_t *>(g + kTile * kTile);   // [64][64]
#pragma unroll
  for (int i = 0; i < kRowsPerLane; ++i) {
    const bool has = acc[i] <= (unsigned)a.d2max;
    cost_s[(i0 + i) * kTile + lane] = has ? table[acc[i]] : (uint8_t)0;
    if (a.dist2) dist2_s[(i0 + i) * kTile + lane] = has ? (uint16_t)acc[i] : (uint16_t)65535;
  }
  __syncthreads();
  store_tile<V, false>(a, x0, y0, tid, cost_s, dist2_s);
}

void launch_lethal_bits(const InflateArgs &a, hipStream_t s)
{
  const uint32_t words = (uint32_t)(a.row_words - 2);
  hipLaunchKernelGGL(k_lethal_bits, dim3((words + 3) / 4, (uint32_t)(a.ny + 3) / 4), dim3(256), 0, s, a);
}

void launch_inflate_tiles(const InflateArgs &a, hipStream_t s)
{
  const dim3 grid((uint32_t)(a.nx + kTile - 1) / kTile, (uint32_t)(a.ny + kTile - 1) / kTile);
  if (a.nx % 4 == 0)
    hipLaunchKernelGGL(k_inflate_tiles<4>, grid, dim3(256), 0, s, a);
  else
    hipLaunchKernelGGL(k_inflate_tiles<1>, grid, dim3(256), 0, s, a);
}

}  // namespace gv
