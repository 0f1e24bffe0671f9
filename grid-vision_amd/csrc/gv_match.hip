// gv_match.hip -- [EXTENSION] X16 scan-to-costmap matching (gv_match_scan*): the kernels.  The definition is in
// include/gridvision_hip_match.h, the arithmetic in gv_match.hpp (shared with the host twin).
//
// Three kernels on the public stream, behind one memset of the call's block (the counter of used points and the
// score volume):
//   k_match_points  a lane per selected point: the map update's fp32 transform, the finite test and the height band;
//                   the used points' (bx, by) go to a compact list, a wavefront taking its places with one atomic add
//                   (ballot + popcount).  The list's order depends on scheduling; every later use is a sum over it.
//   k_match_score   the hot one: a workgroup per (chunk of kMatchChunk points, yaw candidate t).  The 256 lanes first
//                   rotate and bin the chunk's points under (c_t, s_t) -- two fp64 divisions a point -- into LDS,
//                   each cell with its kind: the whole window on the map, the window across the border, or nothing
//                   to add.  Then lanes own window candidates, candidate = lane + 256 k, consecutive lanes on
//                   consecutive i: their cost bytes are adjacent in memory (descending, the data order), so one
//                   wavefront load touches one or two 64-byte lines.  A lane keeps its up to 17 sums (65 x 65
//                   candidates over 256 lanes; the kernel is instantiated per count, so they stay in registers) and
//                   walks the chunk's points, which every lane reads from LDS at the same address (a broadcast).  A
//                   point of the first kind adds cost[base - off_k] with off_k = j_k * nx + i_k precomputed: no
//                   compare, no multiply; the second kind tests every candidate's cell.  The kind is wave-uniform, so
//                   the branch is a scalar one.  At the end every lane adds its sums into the volume with uint32
//                   atomic adds: integer sums in any order give the same bytes.
//   k_match_select  one workgroup over the volume: the maximum of the 64-bit key of match_key (score, Chebyshev
//                   distance, linear index) per lane, by shuffles per wavefront, through LDS per workgroup; the volume
//                   goes to a pinned destination on the way; one thread writes the 64-byte record.
// No kernel waits for another workgroup; no float atomics.  Every store is a plain vector store from VGPRs.
// Memory: a point rereads its window of up to 65 x 65 bytes for every yaw candidate; the costmap (4 MB at 2000 x 2000)
// stays in L2 / Infinity Cache, neighbouring points of a scan share their windows' lines in the L1.
// gfx950, wave64.
#include "gv_launch_match.hpp"
#include "gv_device.hpp"

namespace gv {

namespace {
constexpr int kThreads = 256;
constexpr int kSelThreads = 1024;
}  // namespace

__global__ void __launch_bounds__(kThreads) k_match_points(MatchPointsArgs a)
{
  const uint32_t sel = blockIdx.x * (uint32_t)kThreads + threadIdx.x;
  const int lane = (int)threadIdx.x & 63;
  bool used = false;
  float bx = 0.0f, by = 0.0f, bz = 0.0f;
  if (sel < a.n_sel) {
    const size_t i = (size_t)sel * (size_t)a.stride;   // (n_sel - 1) * stride < n
    match_base_point(a.m_base, a.x[i], a.y[i], a.z[i], bx, by, bz);
    used = match_used(bx, by, bz, a.use_band, a.band);
  }
  const unsigned long long m = __ballot(used);
  if (m == 0ull) return;
  const uint32_t base = wave_append(a.used, m, lane);
  if (used) a.pts[base + wave_rank(m, lane)] = make_float2(bx, by);   // < n_used <= n_sel
}

template <int KACC>
__global__ void __launch_bounds__(kThreads) k_match_score(MatchArgs a)
{
  __shared__ int2 cell_s[kMatchChunk];
  __shared__ uint8_t kind_s[kMatchChunk];   // 0: adds nothing, 1: the whole window on the map, 2: across the border
  const int tid = (int)threadIdx.x;
  const int t = (int)blockIdx.y;            // < NT
  const uint32_t n_used = a.head[0];
  const uint32_t p0 = blockIdx.x * (uint32_t)kMatchChunk;
  if (p0 >= n_used) return;
  const int cnt = (int)min((uint32_t)kMatchChunk, n_used - p0);
  const int wx = a.p.wx, wy = a.p.wy, nx = a.g.nx, ny = a.g.ny;
  const int NX = 2 * wx + 1, ncand = NX * (2 * wy + 1);
  const float2 cs = make_float2(load_karg<float>(offsetof(MatchArgs, rot) + (size_t)t * 8u),
                                load_karg<float>(offsetof(MatchArgs, rot) + (size_t)t * 8u + 4u));

  for (int q = tid; q < cnt; q += kThreads) {
    const float2 b = a.pts[p0 + (uint32_t)q];
    int32_t ux = 0, uy = 0;
    uint8_t kind = 0;
    if (match_cell(a.g, a.p, cs.x, cs.y, b.x, b.y, ux, uy)) {   // |ux|, |uy| < 2^30: the sums below stay in int32
      const int x0 = ux - wx, x1 = ux + wx, y0 = uy - wy, y1 = uy + wy;
      if (x1 < 0 || y1 < 0 || x0 >= nx || y0 >= ny) kind = 0;
      else kind = (x0 >= 0 && y0 >= 0 && x1 < nx && y1 < ny) ? 1 : 2;
    }
    cell_s[q] = make_int2(ux, uy);
    kind_s[q] = kind;
  }
  __syncthreads();

  // this lane's candidates; a lane past the window's end takes the centre (always in the window) and writes nothing
  uint32_t acc[KACC];
  int off[KACC], ci[KACC], cj[KACC];
#pragma unroll
  for (int k = 0; k < KACC; ++k) {
    const int cand = tid + kThreads * k;
    const bool own = cand < ncand;
    cj[k] = own ? cand / NX - wy : 0;
    ci[k] = own ? cand % NX - wx : 0;
    off[k] = cj[k] * nx + ci[k];
    acc[k] = 0u;
  }

  const int last = a.g.G - 1;   // last - (iy * nx + ix) is data_entry (gv_types.hpp)
  const uint8_t *cost = a.cost;
  for (int q = 0; q < cnt; ++q) {
    const int kind = __builtin_amdgcn_readfirstlane((int)kind_s[q]);
    if (kind == 0) continue;
    const int2 u = cell_s[q];
    if (kind == 1) {
      const uint8_t *base = cost + (last - (u.y * nx + u.x));
#pragma unroll
      for (int k = 0; k < KACC; ++k) acc[k] += (uint32_t)base[-off[k]];
    } else {
#pragma unroll
      for (int k = 0; k < KACC; ++k) {
        const int ix = u.x + ci[k], iy = u.y + cj[k];
        if ((unsigned)ix < (unsigned)nx && (unsigned)iy < (unsigned)ny) acc[k] += (uint32_t)cost[last - (iy * nx + ix)];
      }
    }
  }

  uint32_t *vol = a.head + kMatchHeadWords + (size_t)t * (size_t)ncand;
#pragma unroll
  for (int k = 0; k < KACC; ++k) {
    const int cand = tid + kThreads * k;
    if (cand < ncand && acc[k] != 0u) atomicAdd(&vol[cand], acc[k]);
  }
}

__global__ void __launch_bounds__(kSelThreads) k_match_select(MatchArgs a)
{
  __shared__ uint64_t best_s[kSelThreads / 64];
  const int tid = (int)threadIdx.x;
  const int NX = match_nx(a.p), NY = match_ny(a.p), NT = match_nt(a.p);
  const uint32_t ncand = (uint32_t)(NX * NY), total = ncand * (uint32_t)NT;
  const uint32_t *vol = a.head + kMatchHeadWords;
  uint64_t best = 0ull;   // every key is above it
  for (uint32_t lin = (uint32_t)tid; lin < total; lin += (uint32_t)kSelThreads) {
    const uint32_t v = vol[lin];
    if (a.scores_out) a.scores_out[lin] = v;
    const int t = (int)(lin / ncand), r = (int)(lin % ncand);
    const uint64_t key = match_key(v, t - a.p.wt, r / NX - a.p.wy, r % NX - a.p.wx, lin);
    best = key > best ? key : best;
  }
  best = wave_max64(best);
  if ((tid & 63) == 0) best_s[tid >> 6] = best;
  __syncthreads();
  if (tid == 0) {
    for (int w = 1; w < kSelThreads / 64; ++w) best = best_s[w] > best ? best_s[w] : best;
    const uint32_t centre = ((uint32_t)a.p.wt * (uint32_t)NY + (uint32_t)a.p.wy) * (uint32_t)NX + (uint32_t)a.p.wx;
    *a.result = match_record(a.g, a.p, match_key_lin(best), match_key_score(best), vol[centre], a.head[0]);
  }
}

void launch_match_points(const MatchPointsArgs &a, hipStream_t s)
{
  hipLaunchKernelGGL(k_match_points, dim3((a.n_sel + kThreads - 1) / kThreads), dim3(kThreads), 0, s, a);
}

// the instantiation with room for ceil(NY * NX / 256) sums a lane
void launch_match_score(const MatchArgs &a, hipStream_t s)
{
  const int per_lane = (match_nx(a.p) * match_ny(a.p) + kThreads - 1) / kThreads;
  const dim3 grid((a.n_sel + (uint32_t)kMatchChunk - 1) / (uint32_t)kMatchChunk, (uint32_t)match_nt(a.p));
  if (per_lane <= 1) hipLaunchKernelGGL(k_match_score<1>, grid, dim3(kThreads), 0, s, a);
  else if (per_lane <= 2) hipLaunchKernelGGL(k_match_score<2>, grid, dim3(kThreads), 0, s, a);
  else if (per_lane <= 4) hipLaunchKernelGGL(k_match_score<4>, grid, dim3(kThreads), 0, s, a);
  else if (per_lane <= 7) hipLaunchKernelGGL(k_match_score<7>, grid, dim3(kThreads), 0, s, a);
  else if (per_lane <= 12) hipLaunchKernelGGL(k_match_score<12>, grid, dim3(kThreads), 0, s, a);
  else hipLaunchKernelGGL(k_match_score<17>, grid, dim3(kThreads), 0, s, a);
}

void launch_match_select(const MatchArgs &a, hipStream_t s)
{
  hipLaunchKernelGGL(k_match_select, dim3(1), dim3(kSelThreads), 0, s, a);
}

}  // namespace gv
