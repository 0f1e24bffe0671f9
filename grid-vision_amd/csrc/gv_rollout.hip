// gv_rollout.hip -- [EXTENSION] X10 the two ends of a sampling controller's loop (include/gridvision_hip.h has the
// definitions; the arithmetic is gv_motion.hpp's, shared with the host twins gv_rollout_poses and gv_control_select).
//
// k_rollout: controls -> poses[K][P][3].  A trajectory is three chains of fp64 adds (T, then X and Y) around one
// sincos per pose, and the sincos is the expensive part and independent per pose once the yaw chain has run.  So a
// trajectory is NOT a lane's loop (2000 trajectories would be 32 wavefronts of serial fp64 trig).  A workgroup of four
// wavefronts takes kTraj = 8 trajectories and walks P in chunks of 64 steps, four phases a chunk:
//   yaw chain   lane t < 8 runs T = T + w * dt of trajectory t over the chunk, the yaw before every step into LDS
//               (and the yaw after the last one);
//   per pose    32 threads per trajectory, thread l takes steps l and l + 32: sincos of the step's yaw and the two
//               increments of motion_increment into LDS.  All 256 threads work here: 512 poses a chunk;
//   x/y chain   lane t < 8 runs X = X + ix, Y = Y + iy (two independent chains a lane) and rounds the pose to float32
//               into LDS;
//   store       32 threads per trajectory copy the chunk's 12 bytes per pose, contiguous per trajectory, to global
//               memory, 128 bytes per 32 threads at a time, and fetch the next chunk's controls the same way.
// The chains carry X, Y, T in registers from chunk to chunk.  Every value is computed by the operations of the
// sequential definition in its order, on the same inputs: only which lane does an independent piece is chosen here, so
// the poses equal the sequential loop's bit for bit given the device's own sincos.
// LDS: 8 rows of 65 doubles (yaw), 65 double pairs (increments), 193 floats (controls) and 193 floats (poses): 24.3 KB.
// The odd rows keep the eight chain lanes, one row apart, on different banks.
// Bounds: trajectory k0 + t is touched only when it is below K, step p0 + p only below P; the buffers hold K * P * C
// controls (K * C when constant) and K * P * 3 pose floats.
//
// k_control_select: one workgroup of 1024 threads strides over the K record pairs (1024 strides at K = 2^20, two at
// K = 2000): control_total per trajectory, the optional totals[k], and the lexicographic minimum of (total, k) over the
// admitted -- in registers, then across the wavefront by shuffles, then across the sixteen wavefronts through LDS.  A
// minimum and a count: no order shows.  One 16-byte store of the result.  No ticket, no second kernel, no wait for
// another workgroup.
// gfx950, wave64; every store below is a plain vector store from VGPRs.
#include "gv_launch_planner.hpp"
#include "gv_device.hpp"
#include "gv_motion.hpp"

namespace gv {

namespace {
constexpr int kTraj = 8;                     // trajectories per workgroup
constexpr int kPer = 32;                     // threads per trajectory in the per-pose and store phases
constexpr int kChunk = 64;                   // steps per chunk
constexpr int kThreads = kTraj * kPer;
constexpr int kYawRow = kChunk + 1;          // the yaw before each step and after the last
constexpr int kFloatRow = kChunk * 3 + 1;    // a chunk's controls (C <= 3 floats a step) or poses of one trajectory
constexpr int kSelectThreads = 1024;
static_assert(kThreads == 256 && kTraj <= 64, "the chain lanes are the first lanes of the first wavefront");
}  // namespace

__global__ void __launch_bounds__(kThreads) k_rollout(RolloutArgs a)
{
  __shared__ double yaw_s[kTraj * kYawRow];
  __shared__ double2 inc_s[kTraj * kYawRow];
  __shared__ float ctrl_s[kTraj * kFloatRow];
  __shared__ float out_s[kTraj * kFloatRow];
  const int tid = (int)threadIdx.x, j = tid / kPer, l = tid % kPer;
  const int k0 = (int)blockIdx.x * kTraj;
  const int nt = min(kTraj, a.K - k0);      // trajectories of this workgroup
  const int P = a.P;
  const MotionModel m{a.model, a.dt};
  const int C = motion_controls(a.model);
  const bool chain = tid < nt, mine = j < nt;

  // the controls of steps [p0, p0 + cnt) of trajectory k0 + j: cnt * C contiguous floats
  auto fetch_controls = [&](int p0, int cnt) {
    if (!mine) return;
    const float *src = a.controls + ((size_t)(k0 + j) * (size_t)P + (size_t)p0) * (size_t)C;
    for (int r = l; r < cnt * C; r += kPer) ctrl_s[j * kFloatRow + r] = src[r];
  };
  if (a.constant) {
    if (mine && l < C) ctrl_s[j * kFloatRow + l] = a.controls[(size_t)(k0 + j) * (size_t)C + (size_t)l];
  } else {
    fetch_controls(0, min(kChunk, P));
  }
  const int ustep = a.constant ? 0 : C;     // floats from one step's controls to the next's

  double X = a.start[0], Y = a.start[1], T = a.start[2];   // the chain lanes' state

  for (int p0 = 0; p0 < P; p0 += kChunk) {
    const int cnt = min(kChunk, P - p0);
    __syncthreads();   // the chunk's controls are in LDS; the chunk before it has left yaw_s and inc_s

    // ---- yaw chain: lane = trajectory
    if (chain) {
      double *yaw = yaw_s + tid * kYawRow;
      const float *u = ctrl_s + tid * kFloatRow;
      for (int p = 0; p < cnt; ++p) {
        yaw[p] = T;
        T = motion_yaw(m, u + p * ustep, T);
      }
      yaw[cnt] = T;
    }
    __syncthreads();

    // ---- per pose: 32 threads per trajectory
    if (mine) {
      for (int p = l; p < cnt; p += kPer) {
        double s, c, ix, iy;
        sincos(yaw_s[j * kYawRow + p], &s, &c);
        motion_increment(m, ctrl_s + j * kFloatRow + p * ustep, c, s, ix, iy);
        inc_s[j * kYawRow + p] = make_double2(ix, iy);
      }
    }
    __syncthreads();

    // ---- x / y chains: lane = trajectory
    if (chain) {
      const double *yaw = yaw_s + tid * kYawRow;
      const double2 *inc = inc_s + tid * kYawRow;
      float *out = out_s + tid * kFloatRow;
      for (int p = 0; p < cnt; ++p) {
        const double2 d = inc[p];
        X = X + d.x;
        Y = Y + d.y;
        out[p * 3 + 0] = (float)X;
        out[p * 3 + 1] = (float)Y;
        out[p * 3 + 2] = (float)yaw[p + 1];
      }
    }
    __syncthreads();

    // ---- store the chunk's poses, fetch the next chunk's controls
    if (mine) {
      float *dst = a.poses + ((size_t)(k0 + j) * (size_t)P + (size_t)p0) * 3u;
      for (int r = l; r < cnt * 3; r += kPer) dst[r] = out_s[j * kFloatRow + r];
    }
    if (!a.constant && p0 + kChunk < P) fetch_controls(p0 + kChunk, min(kChunk, P - p0 - kChunk));
  }
}

void launch_rollout(const RolloutArgs &a, hipStream_t s)
{
  hipLaunchKernelGGL(k_rollout, dim3((uint32_t)((a.K + kTraj - 1) / kTraj)), dim3(kThreads), 0, s, a);
}

__global__ void __launch_bounds__(kSelectThreads) k_control_select(ControlSelectArgs a)
{
  __shared__ uint64_t total_s[kSelectThreads / 64];
  __shared__ int32_t k_s[kSelectThreads / 64], n_s[kSelectThreads / 64];
  const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const bool nav_used = critic_nav_used(a.w);
  uint64_t best_total = UINT64_MAX;
  int32_t best_k = -1, n = 0;
  for (int32_t k = tid; k < a.K; k += kSelectThreads) {
    uint64_t total = UINT64_MAX;
    const bool ok = control_total(a.w, nav_used, a.traj[k], nav_used ? a.nav + k : nullptr, a.dyn ? a.dyn + k : nullptr,
                                  a.w_dyn_sum, a.w_dyn_max, total);
    if (!ok) total = UINT64_MAX;
    if (a.totals) a.totals[k] = total;
    if (ok) {
      ++n;
      control_take(total, k, best_total, best_k);
    }
  }
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) {
    const uint64_t t = (uint64_t)__shfl_xor((unsigned long long)best_total, o, 64);
    const int32_t k = __shfl_xor(best_k, o, 64);
    control_take(t, k, best_total, best_k);
    n += __shfl_xor(n, o, 64);
  }
  if (lane == 0) {
    total_s[wave] = best_total;
    k_s[wave] = best_k;
    n_s[wave] = n;
  }
  __syncthreads();
  if (tid == 0) {
    for (int w = 1; w < kSelectThreads / 64; ++w) {
      control_take(total_s[w], k_s[w], best_total, best_k);
      n += n_s[w];
    }
    if (best_k < 0) best_total = UINT64_MAX;
    *reinterpret_cast<uint4 *>(a.result) =
        make_uint4((uint32_t)best_k, (uint32_t)n, (uint32_t)best_total, (uint32_t)(best_total >> 32));
  }
}

void launch_control_select(const ControlSelectArgs &a, hipStream_t s)
{
  hipLaunchKernelGGL(k_control_select, dim3(1), dim3(kSelectThreads), 0, s, a);
}

}  // namespace gv
