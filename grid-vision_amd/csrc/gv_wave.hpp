// gv_wave.hpp -- how the 64 lanes of a wavefront cooperate in the gfx950 kernels: scans, reductions, appends.  wave64 only;
// nothing of the project is included.  Which family, when:
//   DPP      (dpp .. wave_min_key, wave_butterfly's row steps)  The cross-lane step is a modifier of a VALU op (gfx9: row_shr /
//            row_shl / row_ror, quad_perm, wave_shl:1, row_bcast:15/31): VALU issue slots, no LDS traffic; a 64-lane scan is
//            six dependent VALU ops (tens of cycles).  For loops short of LDS bandwidth, and for groups inside a row of 16.
//   shuffles (shfl_xor64 .. wave_sum64, wave_tree_sum_shfl)  Every step is a ds_bpermute, a trip through the permute network of
//            the LDS crossbar: six dependent LDS latencies (hundreds of cycles), one instruction per 32 bits whatever the
//            lane pattern.  For the one reduction behind a long loop.
//   ballots  (wave_rank .. wave_append_all)  One atomic add per wavefront, not per lane.
// Where the result lands: the xor butterflies, wave_reduce, group_sum and wave_min_key leave it in EVERY lane; wave_scan
// leaves the reduction in lane 63 only; the fixed-order trees in lane 0 only (the other lanes hold partial sums).  The DPP
// and the shuffle form of one step are different machine code: a kernel's choice was measured at that kernel.
// Who must be active at the call ("ACTIVE:" at each family): a cross-lane read of a lane that EXEC has switched off is not
// defined here -- a lane that returned early, sits in the other arm of a divergent branch, or left a loop with a
// lane-dependent trip count.  A ragged tail is therefore predicated (`v = i < n ? x[i] : identity`) above these helpers,
// never `if (i >= n) return;`.  Every contract below is held lane by lane by tests/test_gpu_wave.py, through the probe
// kernel of gv_test_wave.hip; that test refuses a partial wavefront for every helper marked "all 64", and runs the others
// under the partial masks their line allows.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace gv {

// ---- DPP: src of the lane the control word CTRL names; a lane the row / bank masks leave out keeps `old`, a lane whose
// source does not exist reads `old` too, or 0 with BOUND_CTRL
// ACTIVE: the lane and its source lane; the helpers built on them say what that means for each
template <int CTRL, int ROW_MASK = 0xF, int BANK_MASK = 0xF, bool BOUND_CTRL = false>
__device__ __forceinline__ unsigned dpp(unsigned old, unsigned src)
{
  return (unsigned)__builtin_amdgcn_update_dpp((int)old, (int)src, CTRL, ROW_MASK, BANK_MASK, BOUND_CTRL);
}
template <int CTRL, bool BOUND_CTRL = false>
__device__ __forceinline__ unsigned long long dpp64(unsigned long long v)   // both halves, old = 0
{
  const unsigned lo = dpp<CTRL, 0xF, 0xF, BOUND_CTRL>(0u, (unsigned)(v & 0xffffffffull));
  const unsigned hi = dpp<CTRL, 0xF, 0xF, BOUND_CTRL>(0u, (unsigned)(v >> 32));
  return ((unsigned long long)hi << 32) | (unsigned long long)lo;
}
template <int CTRL>
__device__ __forceinline__ double dpp_f64(double v)   // a lane whose source falls outside its row reads 0.0
{
  return __longlong_as_double((long long)dpp64<CTRL, true>((unsigned long long)__double_as_longlong(v)));
}
struct OpAdd { static constexpr unsigned id = 0u; __device__ static unsigned f(unsigned a, unsigned b) { return a + b; } };
struct OpMax { static constexpr unsigned id = 0u; __device__ static unsigned f(unsigned a, unsigned b) { return a > b ? a : b; } };
struct OpMin { static constexpr unsigned id = 0xFFFFFFFFu; __device__ static unsigned f(unsigned a, unsigned b) { return a < b ? a : b; } };
// inclusive scan over the 64 lanes (lane 63 ends up with the reduction); wave_reduce: that reduction, in every lane
// ACTIVE: all 64 (wave_scan, wave_reduce, wave_shift_down, wave_min_key)
template <class Op>
__device__ __forceinline__ unsigned wave_scan(unsigned v)
{
  v = Op::f(v, dpp<0x111>(Op::id, v));        // row_shr:1
  v = Op::f(v, dpp<0x112>(Op::id, v));        // row_shr:2
  v = Op::f(v, dpp<0x114>(Op::id, v));        // row_shr:4
  v = Op::f(v, dpp<0x118>(Op::id, v));        // row_shr:8
  v = Op::f(v, dpp<0x142, 0xA>(Op::id, v));   // row_bcast:15 -> rows 1, 3
  v = Op::f(v, dpp<0x143, 0xC>(Op::id, v));   // row_bcast:31 -> rows 2, 3
  return v;
}
template <class Op>
__device__ __forceinline__ unsigned wave_reduce(unsigned v) { return (unsigned)__builtin_amdgcn_readlane((int)wave_scan<Op>(v), 63); }
// value of lane + H (H = 1, 2, 4, 8) or `fill` past lane 63: H single-lane wave shifts
template <int H>
__device__ __forceinline__ unsigned wave_shift_down(unsigned v, unsigned fill)
{
#pragma unroll
  for (int k = 0; k < H; ++k) v = dpp<0x130>(fill, v);   // wave_shl:1
  return v;
}
// every lane of a group of LANES consecutive lanes (8 or 16, aligned) ends with the group's sum
// ACTIVE: all LANES lanes of the group together; other groups of the wavefront may be off (k_radius_sorted: a point's
// lanes leave its candidate loop together, the points of a wavefront at different times)
template <int LANES>
__device__ __forceinline__ int group_sum(int v)
{
  if constexpr (LANES == 16) {
    v += (int)dpp<0x128>(0u, (unsigned)v);   // row_ror:8
    v += (int)dpp<0x124>(0u, (unsigned)v);   // row_ror:4
    v += (int)dpp<0x122>(0u, (unsigned)v);   // row_ror:2
    v += (int)dpp<0x121>(0u, (unsigned)v);   // row_ror:1
  } else {
    v += (int)dpp<0x141>(0u, (unsigned)v);   // row_half_mirror: lane i <-> 7 - i of its half row
    v += (int)dpp<0xB1>(0u, (unsigned)v);    // quad_perm [1,0,3,2]
    v += (int)dpp<0x4E>(0u, (unsigned)v);    // quad_perm [2,3,0,1]
  }
  return v;
}
// 64-bit minimum, in every lane: rotations inside the rows of 16, then the two cross-row steps through the permute network
__device__ __forceinline__ unsigned long long wave_min_key(unsigned long long v)
{
  unsigned long long o;
  o = dpp64<0x128>(v); v = o < v ? o : v;   // row_ror:8
  o = dpp64<0x124>(v); v = o < v ? o : v;   // row_ror:4
  o = dpp64<0x122>(v); v = o < v ? o : v;   // row_ror:2
  o = dpp64<0x121>(v); v = o < v ? o : v;   // row_ror:1
  o = __shfl_xor(v, 16); v = o < v ? o : v;
  o = __shfl_xor(v, 32); v = o < v ? o : v;
  return v;
}

// ---- xor butterflies: v op= (v of lane ^ o), o = 32 .. 1, by shuffles; the result in every lane.  Integer sums and maxima
// only: the order of the operands differs from lane to lane.  (The arg-reductions and the loops that carry two reductions
// at once are this butterfly written out at their kernels: behind a shared loop they compiled otherwise)
// ACTIVE: all 64 (every lane is some lane's partner at every step)
template <class T>
__device__ __forceinline__ T wave_sum(T v)   // int or unsigned
{
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
template <class T>
__device__ __forceinline__ T wave_max(T v)   // int or unsigned
{
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) v = max(v, __shfl_xor(v, o, 64));
  return v;
}
__device__ __forceinline__ uint64_t shfl_xor64(uint64_t v, int o)
{
  const uint32_t lo = (uint32_t)__shfl_xor((int)(uint32_t)v, o, 64);
  const uint32_t hi = (uint32_t)__shfl_xor((int)(uint32_t)(v >> 32), o, 64);
  return ((uint64_t)hi << 32) | lo;
}
__device__ __forceinline__ uint64_t wave_max64(uint64_t v)
{
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) { const uint64_t other = shfl_xor64(v, o); v = other > v ? other : v; }
  return v;
}
__device__ __forceinline__ uint64_t wave_sum64(uint64_t v)
{
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) v += shfl_xor64(v, o);
  return v;
}

// ---- fixed-order trees: v[i] += v[i + off], off = 32 .. 1.  Lane 0 ends with the sum of the 64 values in ONE order of
// additions, the oracle's (tree_sum64, oracle/ransac.c).  Two forms of one tree: lane 0 of both holds the same value in the
// same rounding order; which one a kernel uses was decided by measurement at that kernel.  DPP form: only lanes below `off`
// matter at each step, so the four in-row steps are DPP shifts (no LDS traffic); the other two go through the permute network.
// ACTIVE: all 64 (a lane without a value contributes +0.0, as the oracle's tree pads)
__device__ __forceinline__ double wave_butterfly(double v)
{
  v = v + __shfl_down(v, 32);
  v = v + __shfl_down(v, 16);
  v = v + dpp_f64<0x108>(v);   // row_shl:8
  v = v + dpp_f64<0x104>(v);   // row_shl:4
  v = v + dpp_f64<0x102>(v);   // row_shl:2
  v = v + dpp_f64<0x101>(v);   // row_shl:1
  return v;
}
__device__ __forceinline__ double wave_tree_sum_shfl(double v)   // shuffle form: lanes l < w hold a_l + a_(l + w)
{
#pragma unroll
  for (int w = 32; w >= 1; w >>= 1) v = v + __shfl_down(v, w, 64);
  return v;
}

// ---- wave-aggregated append: mask = __ballot(this lane appends), not 0.  rank: the lane's place among the appending lanes;
// leader: the first of them; bcast: lane `lane`'s v, in every lane.
// ACTIVE: any subset of the lanes, the same at the __ballot and at the call; wave_bcast's source lane is one of them
__device__ __forceinline__ unsigned wave_rank(unsigned long long m, int lane) { return (unsigned)__popcll(m & ((1ull << lane) - 1ull)); }
__device__ __forceinline__ int wave_leader(unsigned long long mask) { return __ffsll((long long)mask) - 1; }
template <class T> __device__ __forceinline__ T wave_bcast(T v, int lane) { return __shfl(v, lane, 64); }
// One atomic add of the popcount: the first of the wavefront's places, in every lane; lane l's is that + wave_rank(mask, l).
// Any subset of the lanes may be active: the leader is an appending lane.
__device__ __forceinline__ uint32_t wave_append(uint32_t *counter, unsigned long long mask, int lane)
{
  const int leader = wave_leader(mask);
  uint32_t base = 0u;
  if (lane == leader) base = atomicAdd(counter, (uint32_t)__popcll(mask));
  return (uint32_t)wave_bcast((int)base, leader);
}
// The same where lane 0 is known to be active: lane 0 adds, the base comes back by readfirstlane, not the permute network.
// ACTIVE: any subset that holds lane 0 (with lane 0 off nobody adds, and the first active lane's zero comes back)
__device__ __forceinline__ unsigned wave_append_all(unsigned *counter, unsigned long long mask, int lane)
{
  unsigned base = 0;
  if (lane == 0) base = atomicAdd(counter, (unsigned)__popcll(mask));
  return (unsigned)__builtin_amdgcn_readfirstlane((int)base);
}

}  // namespace gv
