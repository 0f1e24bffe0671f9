// gv_dynscore.hip -- [EXTENSION] X13 scoring against predicted moving objects (gv_score_dynamic): K trajectories of P
// poses against at most 128 oriented rectangles that move at constant velocity, each pose at its own time
// (include/gridvision_hip.h has the definition; the arithmetic is gv_dyn.hpp's, shared with gv_dyn_score_poses).
//
// One workgroup of four wavefronts owns one whole trajectory, as in gv_trajscore.hip; it walks the poses in chunks of 64.
//   tables   the object table (n rows of 8 doubles, at most 8 KB) and the cost table (at most 3970 bytes) are copied
//            into LDS once per workgroup.
//   tests    lane = pose of the chunk, wavefront w = objects w, w + 4, ..: every lane of a wavefront reads the same
//            row, a broadcast read of four 16-byte words, and runs the fp64 text of one (pose, object) pair for every
//            circle.  All four wavefronts take the same 64 poses, so a 56-pose trajectory still fills 224 lanes; each
//            recomputes the pose's sincos (needed only when a circle is off the centre), which costs what waiting
//            for one wavefront to do it would.  A wavefront leaves the lexicographic minimum of (d2, j) over its
//            objects in LDS.
//   poses    the first wavefront combines the four minima of its lane's pose (a minimum: the order does not show),
//            reads the cost from the table and accumulates the record of the lane's poses in registers; the pose cost
//            goes out a byte per lane.
//   record   after the last chunk: integer maximum, sum and minimum and the (d2, j) minimum across the wavefront by
//            shuffles, one 24-byte record per trajectory from one lane.  No atomics, no order shows.
// Bounds: pose p0 + lane is read only below P, trajectory k only below K (the grid is K workgroups), objects only
// below n_obj <= 128 = the LDS rows (a count read from the device, X14's fed set, is clamped to 0..128 first), table
// entries only at (uint32_t)u with u < T <= the LDS bytes.
// gfx950, wave64; every store below is a plain vector store from VGPRs.
#include "gv_launch_planner.hpp"
#include "gv_device.hpp"
#include "gv_dyn.hpp"

namespace gv {

namespace {
constexpr int kChunk = 64;      // poses per chunk = lanes per wavefront
constexpr int kWaves = 4;       // wavefronts per workgroup: they share the objects
constexpr int kTableMax = 4096; // (63 + 1)^2: more than any table with Rc <= 63 holds
}  // namespace

// kFed: the set was written on the device by a fed gv_track_update (X14) and its count is read from there; the other
// instantiation is the kernel as it was, n_obj from the arguments.
template <bool kFed>
__global__ void __launch_bounds__(kChunk *kWaves) k_score_dynamic(DynArgs a)
{
  __shared__ __attribute__((aligned(16))) DynObject obj_s[kDynMaxObjects];
  __shared__ __attribute__((aligned(16))) uint8_t table_s[kTableMax];
  __shared__ double d2_s[kWaves * kChunk];
  __shared__ int32_t j_s[kWaves * kChunk];
  const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int k = (int)blockIdx.x;
  if (k >= a.K) return;
  const int P = a.P;
  // a fed set has its count on the device: one uniform read per workgroup, clamped to the rows
  const int n_obj = kFed ? max(0, min(*a.n_obj_dev, kDynMaxObjects)) : min(a.n_obj, kDynMaxObjects);
  const int T = min(a.p.T, kTableMax);
  const float *traj = a.poses + (size_t)k * (size_t)P * 3u;

  {
    const double *src = reinterpret_cast<const double *>(a.objs);
    double *dst = reinterpret_cast<double *>(obj_s);
    for (int i = tid; i < n_obj * 8; i += kChunk * kWaves) dst[i] = src[i];
    for (int i = tid; i < T; i += kChunk * kWaves) table_s[i] = a.table[i];
  }
  __syncthreads();

  DynAccum acc;   // the first wavefront's lanes: over the poses lane, lane + 64, ..
  for (int p0 = 0; p0 < P; p0 += kChunk) {
    const int p = p0 + lane;
    double best = INFINITY;
    int32_t best_j = -1;
    if (p < P) dyn_pose_min(a.p, obj_s, n_obj, wave, kWaves, traj + (size_t)p * 3u, p, best, best_j);
    d2_s[wave * kChunk + lane] = best;
    j_s[wave * kChunk + lane] = best_j;
    __syncthreads();
    if (wave == 0 && p < P) {
#pragma unroll
      for (int w = 1; w < kWaves; ++w) dyn_take(d2_s[w * kChunk + lane], j_s[w * kChunk + lane], best, best_j);
      const int32_t cost = dyn_cost(a.p, table_s, best);
      dyn_accumulate(a.p, p, cost, best, best_j, acc);
      if (a.pose_cost) a.pose_cost[(size_t)k * (size_t)P + (size_t)p] = (uint8_t)cost;
    }
    __syncthreads();   // the first wavefront is done with the chunk's minima
  }

  if (wave == 0) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
      DynAccum q;
      q.max_cost = __shfl_xor(acc.max_cost, o, 64);
      q.first = __shfl_xor(acc.first, o, 64);
      q.sum = (uint32_t)__shfl_xor((int)acc.sum, o, 64);
      q.best = __shfl_xor(acc.best, o, 64);
      q.best_j = __shfl_xor(acc.best_j, o, 64);
      acc.max_cost = max(acc.max_cost, q.max_cost);
      if (q.first >= 0 && (acc.first < 0 || q.first < acc.first)) acc.first = q.first;
      acc.sum += q.sum;
      dyn_take(q.best, q.best_j, acc.best, acc.best_j);
    }
    if (lane == 0) a.scores[k] = dyn_record(acc);
  }
}

void launch_score_dynamic(const DynArgs &a, hipStream_t s)
{
  if (a.n_obj_dev) hipLaunchKernelGGL(k_score_dynamic<true>, dim3((uint32_t)a.K), dim3(kChunk * kWaves), 0, s, a);
  else hipLaunchKernelGGL(k_score_dynamic<false>, dim3((uint32_t)a.K), dim3(kChunk * kWaves), 0, s, a);
}

}  // namespace gv
