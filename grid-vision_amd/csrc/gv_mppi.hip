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
//
// [EXTENSION] X12, launched only when limits are set (gv_set_mppi_limits); k_mppi_sample is as it was.
// k_mppi_constrain: the chain of rate and turning-radius limits over controls[K][P][C], in place, behind k_mppi_sample.
//   The chain is serial along p and independent across k, and a step is a handful of float32 compares: there is no
//   per-pose part worth spreading, so -- unlike k_rollout's 8 -- a workgroup of four wavefronts owns kChainTraj = 64
//   trajectories and walks P in chunks of kChainSteps = 32 steps, three phases a chunk:
//     load    32 threads per trajectory copy the chunk's cnt * C contiguous floats of a trajectory into its LDS row,
//             128 bytes per 32 threads; a thread takes eight rows and issues their loads before the first is used --
//             the kernel is a few round trips to memory and little else;
//     chain   lane t of the first wavefront -- every lane of it a chain -- runs mppi_constrain_step over row t, in
//             place, eight steps read from LDS at a time, the step before it carried in registers from chunk to
//             chunk;
//     store   as the load, LDS to global memory.
//   LDS: 64 rows of 32 * 3 + 1 = 97 floats, 24.3 KB.  A 4-byte LDS access is served in two groups of 32 lanes over 32
//   banks; 97 = 1 mod 32, so the chain lanes of a group, one row apart each, land on 32 different banks.
//   Bounds: trajectory k0 + t is touched only below K, step p0 + p only below P; rows hold C <= 3 floats a step.
// k_mppi_control_cost: g_k, a wavefront per trajectory (lane l holds a_l of gv_mppi.hpp, then the shuffle tree), four
//   trajectories per wavefront one after the other, sixteen per workgroup.  Lane 0 then has x_k of an admitted
//   trajectory; the minimum m of x goes to one 64-bit word by an integer atomicMin on mppi_min_key -- a minimum does
//   not depend on the order, so no sum sees an atomic -- once per workgroup, after the wavefronts' minima met in LDS.
//   The word is cleared to all ones by a memset enqueued in front.  k_mppi_partial then reads x_k and m instead of the
//   totals' difference (both arguments null without gamma: X11's text).
// gfx950, wave64; every store below is a plain vector store from VGPRs.
#include "gv_launch_planner.hpp"
#include "gv_device.hpp"
#include "gv_mppi.hpp"

namespace gv {

namespace {
constexpr int kFinishCols = 64;                            // columns of a k_mppi_finish workgroup: one per lane of a wavefront
constexpr int kFinishGroups = kMppiThreads / kFinishCols;  // its wavefronts: wavefront g adds chunks g, g + 4, ..
constexpr int kChainTraj = 64;                             // trajectories of a k_mppi_constrain workgroup: one per lane of a wavefront
constexpr int kChainSteps = 32;                            // steps per chunk
constexpr int kChainRow = kChainSteps * 3 + 1;             // floats of an LDS row: 1 mod 32, so rows one apart differ in bank
constexpr int kChainPer = 32;                              // threads per trajectory in the load and the store
constexpr int kChainBatch = kChainTraj / (kMppiThreads / kChainPer);   // rows a thread takes, their loads in flight together
constexpr int kChainSub = 8;                               // steps a chain lane reads from LDS at a time
constexpr int kCostWaves = kMppiThreads / kMppiCostLanes;  // wavefronts of a k_mppi_control_cost workgroup
constexpr int kCostPerWave = 4;                            // trajectories a wavefront takes, one after the other
static_assert(kMppiCostLanes == 64 && kChainTraj == 64, "a lane per partial sum, a lane per chain");
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
    if (a.x)
      e_s[tid] = t != UINT64_MAX ? mppi_weight_cc(a.x[k0 + tid], mppi_min_unkey(*a.x_min_key), a.lambda) : -1.0;
    else
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

// ---- [EXTENSION] X12
// C, the floats per step, is a template argument: with it constant a step of the chain is straight-line code
template <int C>
__global__ void __launch_bounds__(kMppiThreads) k_mppi_constrain(MppiConstrainArgs a)
{
  __shared__ float row_s[kChainTraj * kChainRow];
  const int tid = (int)threadIdx.x, g = tid / kChainPer, l = tid % kChainPer;
  const int k0 = (int)blockIdx.x * kChainTraj;
  const int nt = min(kChainTraj, a.K - k0);   // trajectories of this workgroup
  const int P = a.P;
  const size_t row_len = (size_t)P * (size_t)C;   // floats from one trajectory to the next
  const bool chain = tid < nt;
  float s[3] = {a.chain.u_prev[0], a.chain.u_prev[1], a.chain.u_prev[2]};   // the chain lanes' state

  for (int p0 = 0; p0 < P; p0 += kChainSteps) {
    const int cnt = min(kChainSteps, P - p0), n = cnt * C;   // steps and floats of a trajectory in this chunk
    float *chunk = a.controls + ((size_t)k0 * (size_t)P + (size_t)p0) * (size_t)C;   // row t, float r: chunk[t * row_len + r]
    // 32 threads per trajectory: thread (g, l) takes floats l, l + 32, .. of rows g, g + 8, .., g + 56, the eight rows'
    // loads issued before the first is used.
    auto copy = [&](bool to_lds) {
      for (int r = l; r < n; r += kChainPer) {
        float v[kChainBatch];
#pragma unroll
        for (int i = 0; i < kChainBatch; ++i) {
          const int t = g + i * (kMppiThreads / kChainPer);
          v[i] = 0.0f;
          if (t < nt) v[i] = to_lds ? chunk[(size_t)t * row_len + (size_t)r] : row_s[t * kChainRow + r];
        }
#pragma unroll
        for (int i = 0; i < kChainBatch; ++i) {
          const int t = g + i * (kMppiThreads / kChainPer);
          if (t >= nt) continue;
          if (to_lds) row_s[t * kChainRow + r] = v[i];
          else chunk[(size_t)t * row_len + (size_t)r] = v[i];
        }
      }
    };
    copy(true);
    __syncthreads();
    // ---- chain: lane = trajectory, kChainSub steps read from LDS at a time
    if (chain) {
      float *u = row_s + tid * kChainRow;
      int b = 0;
      for (; b + kChainSub <= cnt; b += kChainSub) {   // whole groups of kChainSub steps
        float f[kChainSub][3];
#pragma unroll
        for (int i = 0; i < kChainSub; ++i) {
          const int r = (b + i) * C;
          f[i][0] = u[r];
          f[i][1] = u[r + 1];
          f[i][2] = C == 3 ? u[r + 2] : 0.0f;
        }
#pragma unroll
        for (int i = 0; i < kChainSub; ++i) {
          const int r = (b + i) * C;
          mppi_constrain_step(a.chain, C, s, f[i]);
          u[r] = f[i][0];
          u[r + 1] = f[i][1];
          if (C == 3) u[r + 2] = f[i][2];
        }
      }
      for (; b < cnt; ++b) {                           // the last cnt % kChainSub steps
        const int r = b * C;
        float q[3] = {u[r], u[r + 1], C == 3 ? u[r + 2] : 0.0f};
        mppi_constrain_step(a.chain, C, s, q);
        u[r] = q[0];
        u[r + 1] = q[1];
        if (C == 3) u[r + 2] = q[2];
      }
    }
    __syncthreads();
    copy(false);
    __syncthreads();   // the rows are free for the next chunk
  }
}

void launch_mppi_constrain(const MppiConstrainArgs &a, hipStream_t s)
{
  const dim3 grid((uint32_t)((a.K + kChainTraj - 1) / kChainTraj));
  if (a.C == 3) hipLaunchKernelGGL(k_mppi_constrain<3>, grid, dim3(kMppiThreads), 0, s, a);
  else hipLaunchKernelGGL(k_mppi_constrain<2>, grid, dim3(kMppiThreads), 0, s, a);
}

__global__ void __launch_bounds__(kMppiThreads) k_mppi_control_cost(MppiCostArgs a)
{
  __shared__ uint64_t key_s[kCostWaves];
  const int tid = (int)threadIdx.x, lane = tid & (kMppiCostLanes - 1), wave = tid / kMppiCostLanes;
  const int kb = ((int)blockIdx.x * kCostWaves + wave) * kCostPerWave;
  const uint64_t best_total = a.result->best_total;
  const size_t J = (size_t)a.P * (size_t)a.C;
  uint64_t key = UINT64_MAX;   // lane 0: the smallest key of this wavefront's admitted trajectories
  for (int i = 0; i < kCostPerWave; ++i) {
    const int k = kb + i;
    if (k >= a.K) break;       // the same for every lane of the wavefront
    double v = mppi_cost_lane(a.qc, a.C, a.nominal, a.P, a.shift, a.controls + (size_t)k * J, lane);
    v = wave_tree_sum_shfl(v);   // lane 0: the 64 values in the fixed tree's order
    if (lane == 0) {
      a.g[k] = v;
      const uint64_t t = a.totals[k];
      if (t != UINT64_MAX) {
        const double x = mppi_cost_x(t, best_total, v);
        a.x[k] = x;
        const uint64_t kx = mppi_min_key(x);
        key = kx < key ? kx : key;
      }
    }
  }
  if (lane == 0) key_s[wave] = key;
  __syncthreads();
  if (tid == 0) {
    for (int w = 1; w < kCostWaves; ++w) key = key_s[w] < key ? key_s[w] : key;
    if (key != UINT64_MAX) atomicMin(reinterpret_cast<unsigned long long *>(a.x_min_key), (unsigned long long)key);
  }
}

void launch_mppi_control_cost(const MppiCostArgs &a, hipStream_t s)
{
  constexpr int per = kCostWaves * kCostPerWave;
  hipLaunchKernelGGL(k_mppi_control_cost, dim3((uint32_t)((a.K + per - 1) / per)), dim3(kMppiThreads), 0, s, a);
}

}  // namespace gv
