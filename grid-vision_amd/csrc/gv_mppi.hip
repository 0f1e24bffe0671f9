// gv_mppi.hip -- [EXTENSION] X11 the two ends of an MPPI iteration (include/gridvision_hip.h has the definitions; the
// arithmetic is gv_mppi.hpp's, shared with the host twins gv_mppi_sample_controls and gv_mppi_average).
//
// k_mppi_sample: nominal -> controls[K][P][C].  One pose per lane: one Philox call, Box-Muller in fp64 (one log, one
// cos and one sin; a second log and cos for the third channel), the nominal step, the clamp.  No state is carried, so
// lane i simply takes pose i of the K * P; it stores C floats at controls + i * C, and consecutive lanes write one
// contiguous run.  Bounds: pose i is touched only when i < K * P <= 2^24; the nominal row is pn <= P - 1.
//
// The average, two launches, no atomics, no ticket: the order of every sum is fixed by (K, P * C) (gv_mppi.hpp).
// k_mppi_partial: workgroup (chunk, tile) owns `rows` trajectories and `tile` columns of the J = P * C.  Its first
//   `rows` threads compute the chunk's weights once into LDS (-1 marks a rejected trajectory); then thread (s, jj) --
//   row group s, column jj of the tile -- walks rows s, s + groups, .. of the chunk.  For a fixed trajectory the J floats
//   are contiguous, so a row group reads one contiguous run.  The row groups' sums meet in LDS and are added in group
//   order; one fp64 partial per column and chunk, and one partial weight sum per chunk (the column tile 0 writes it).
// k_mppi_finish: a workgroup owns 64 columns; its wavefront g adds the partials and the weight sums of chunks g, g + 4, ..
//   in that order (a quarter of the serial chain each, eight loads in flight), the four sums meet in LDS and are added
//   in wavefront order; then divide, round and store to the resident nominal and to nominal_out.  Thread 0 forwards the
//   16-byte result.  With no trajectory admitted the nominal is left as it is (and still copied out).
// LDS: k_mppi_partial 64 + 256 doubles, 2.5 KB; k_mppi_finish 512 doubles, 4 KB.
// gfx950, wave64; every store below is a plain vector store from VGPRs.
#include "gv_device.hpp"
#include "gv_mppi.hpp"

namespace gv {

namespace {
constexpr int kFinishCols = 64;                            // columns of a k_mppi_finish workgroup: one per lane of a wavefront
constexpr int kFinishGroups = kMppiThreads / kFinishCols;  // its wavefronts: wavefront g adds chunks g, g + 4, ..
}  // namespace

__global__ void __launch_bounds__(kMppiThreads) k_mppi_sample(MppiSampleArgs a)
{
  const uint32_t i = blockIdx.x * (uint32_t)kMppiThreads + threadIdx.x;
  if (i >= (uint32_t)a.K * (uint32_t)a.P) return;
  const uint32_t k = i / (uint32_t)a.P, p = i - k * (uint32_t)a.P;
  float f[3];
  mppi_sample(a.cfg, a.C, a.nominal, a.P, a.seed, a.iteration, a.shift, k, p, f);
  float *dst = a.controls + (size_t)i * (size_t)a.C;
  if (a.C == 3) {
    dst[0] = f[0]; dst[1] = f[1]; dst[2] = f[2];
  } else {
    *reinterpret_cast<float2 *>(dst) = make_float2(f[0], f[1]);   // i * 8 bytes into a hipMalloc block
  }
}

void launch_mppi_sample(const MppiSampleArgs &a, hipStream_t s)
{
  const uint32_t n = (uint32_t)a.K * (uint32_t)a.P;
  hipLaunchKernelGGL(k_mppi_sample, dim3((n + kMppiThreads - 1) / kMppiThreads), dim3(kMppiThreads), 0, s, a);
}

__global__ void __launch_bounds__(kMppiThreads) k_mppi_partial(MppiAverageArgs a)
{
  __shared__ double e_s[kMppiChunkMax];
  __shared__ double acc_s[kMppiThreads];
  const int tid = (int)threadIdx.x;
  const int groups = kMppiThreads / a.tile, s = tid / a.tile, jj = tid - s * a.tile;
  const int chunk = (int)blockIdx.x, k0 = chunk * a.rows;
  const int nr = min(a.rows, a.K - k0);
  const int j = (int)blockIdx.y * a.tile + jj;
  if (tid < nr) {
    const uint64_t t = a.totals[k0 + tid];
    if (a.totals_out && blockIdx.y == 0) a.totals_out[k0 + tid] = t;
    e_s[tid] = t != UINT64_MAX ? mppi_weight(t, a.result->best_total, a.lambda) : -1.0;
  }
  __syncthreads();
  double acc = 0.0;
  if (j < a.J) {
    const float *u = a.controls + (size_t)k0 * (size_t)a.J + (size_t)j;
#pragma unroll 4
    for (int r = s; r < nr; r += groups) {
      const double e = e_s[r], v = (double)u[(size_t)r * (size_t)a.J];   // the load does not wait for the weight
      if (e >= 0.0) acc = acc + e * v;
    }
  }
  acc_s[tid] = acc;
  __syncthreads();
  if (s == 0 && j < a.J) {
    for (int g = 1; g < groups; ++g) acc = acc + acc_s[g * a.tile + jj];
    a.partial[(size_t)chunk * (size_t)a.J + (size_t)j] = acc;
  }
  if (tid == 0 && blockIdx.y == 0) {
    double S = 0.0;
    for (int r = 0; r < nr; ++r) {
      const double e = e_s[r];
      if (e >= 0.0) S = S + e;
    }
    a.partial[(size_t)gridDim.x * (size_t)a.J + (size_t)chunk] = S;
  }
}

__global__ void __launch_bounds__(kMppiThreads) k_mppi_finish(MppiAverageArgs a)
{
  __shared__ double n_s[kMppiThreads], s_s[kMppiThreads];
  const int tid = (int)threadIdx.x, jj = tid & (kFinishCols - 1), g = tid / kFinishCols;
  const int j = (int)blockIdx.x * kFinishCols + jj;
  const gv_control_result res = *a.result;
  if (blockIdx.x == 0 && tid == 0 && a.result_out)
    *reinterpret_cast<uint4 *>(a.result_out) =
        make_uint4((uint32_t)res.best, (uint32_t)res.n_valid, (uint32_t)res.best_total, (uint32_t)(res.best_total >> 32));
  double N = 0.0, S = 0.0;
  if (res.n_valid > 0 && j < a.J) {
    const int chunks = (a.K + a.rows - 1) / a.rows;
    const double *pn = a.partial + j, *ps = a.partial + (size_t)chunks * (size_t)a.J;
#pragma unroll 8
    for (int c = g; c < chunks; c += kFinishGroups) {
      N = N + pn[(size_t)c * (size_t)a.J];
      S = S + ps[c];
    }
  }
  n_s[tid] = N;
  s_s[tid] = S;
  __syncthreads();
  if (g != 0 || j >= a.J) return;
  float v = a.nominal[j];
  if (res.n_valid > 0) {
    for (int q = 1; q < kFinishGroups; ++q) {
      N = N + n_s[q * kFinishCols + jj];
      S = S + s_s[q * kFinishCols + jj];
    }
    v = (float)(N / S);
    a.nominal[j] = v;
  }
  if (a.nominal_out) a.nominal_out[j] = v;
}

void launch_mppi_average(const MppiAverageArgs &a, hipStream_t s)
{
  const uint32_t chunks = (uint32_t)((a.K + a.rows - 1) / a.rows), tiles = (uint32_t)((a.J + a.tile - 1) / a.tile);
  hipLaunchKernelGGL(k_mppi_partial, dim3(chunks, tiles), dim3(kMppiThreads), 0, s, a);
  hipLaunchKernelGGL(k_mppi_finish, dim3((uint32_t)((a.J + kFinishCols - 1) / kFinishCols)), dim3(kMppiThreads), 0, s, a);
}

}  // namespace gv
