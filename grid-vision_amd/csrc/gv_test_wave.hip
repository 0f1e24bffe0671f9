// gv_test_wave.hip -- the probe kernel of gv_wave.hpp and its test hook (gv_test_hooks.h: gv_test_wave).  k_test_wave is
// the one kernel of the library that exists for a test: it runs ONE helper of gv_wave.hpp, in the instantiation `op`
// names, on 64 values a wavefront, and stores every lane's result.  No product code calls it; tests/test_gpu_wave.py
// compares what it stores bit for bit with the plain references of tests/wave_ref.py.
#include "gv_context.hpp"
#include "gv_wave.hpp"

namespace gv {

namespace {

__device__ __forceinline__ uint64_t f64_bits(double v) { return (uint64_t)__double_as_longlong(v); }
// high word: the wavefront's base (or leader), low word: the lane's place (or rank)
__device__ __forceinline__ uint64_t pack_words(uint32_t hi, uint32_t lo) { return ((uint64_t)hi << 32) | (uint64_t)lo; }

}  // namespace

// One wavefront per 64 inputs: blockDim.x is a multiple of 64, so a wavefront is in range as a whole or leaves as a whole.
// `op` and `arg` are uniform.  A result goes to out[] and nowhere else: a wrong helper gives a wrong number, never a wild
// address (the append ops' only address is `counter`).
__global__ void k_test_wave(int32_t op, int32_t arg, const uint64_t *__restrict__ in, const uint64_t *__restrict__ active,
                            int64_t n_waves, uint64_t *__restrict__ out, uint32_t *counter)
{
  const int64_t t = (int64_t)blockIdx.x * (int64_t)blockDim.x + (int64_t)threadIdx.x;
  const int64_t w = t >> 6;
  if (w >= n_waves) return;
  const int lane = (int)(threadIdx.x & 63u);
  const uint64_t v = in[t];
  uint64_t r = GV_TEST_WAVE_INACTIVE;
  if ((active[w] >> lane) & 1ull) {
    const unsigned lo = (unsigned)v;
    const double d = __longlong_as_double((long long)v);
    switch (op) {
      case GV_TEST_WAVE_SCAN_ADD: r = wave_scan<OpAdd>(lo); break;
      case GV_TEST_WAVE_SCAN_MAX: r = wave_scan<OpMax>(lo); break;
      case GV_TEST_WAVE_SCAN_MIN: r = wave_scan<OpMin>(lo); break;
      case GV_TEST_WAVE_REDUCE_ADD: r = wave_reduce<OpAdd>(lo); break;
      case GV_TEST_WAVE_REDUCE_MAX: r = wave_reduce<OpMax>(lo); break;
      case GV_TEST_WAVE_REDUCE_MIN: r = wave_reduce<OpMin>(lo); break;
      case GV_TEST_WAVE_SHIFT_DOWN_1: r = wave_shift_down<1>(lo, (unsigned)arg); break;
      case GV_TEST_WAVE_SHIFT_DOWN_2: r = wave_shift_down<2>(lo, (unsigned)arg); break;
      case GV_TEST_WAVE_SHIFT_DOWN_4: r = wave_shift_down<4>(lo, (unsigned)arg); break;
      case GV_TEST_WAVE_SHIFT_DOWN_8: r = wave_shift_down<8>(lo, (unsigned)arg); break;
      case GV_TEST_WAVE_GROUP_SUM_8: r = (unsigned)group_sum<8>((int)lo); break;
      case GV_TEST_WAVE_GROUP_SUM_16: r = (unsigned)group_sum<16>((int)lo); break;
      case GV_TEST_WAVE_MIN_KEY: r = wave_min_key((unsigned long long)v); break;
      case GV_TEST_WAVE_SUM_I32: r = (unsigned)wave_sum<int>((int)lo); break;
      case GV_TEST_WAVE_SUM_U32: r = wave_sum<unsigned>(lo); break;
      case GV_TEST_WAVE_MAX_I32: r = (unsigned)wave_max<int>((int)lo); break;
      case GV_TEST_WAVE_MAX_U32: r = wave_max<unsigned>(lo); break;
      case GV_TEST_WAVE_MAX64: r = wave_max64(v); break;
      case GV_TEST_WAVE_SUM64: r = wave_sum64(v); break;
      case GV_TEST_WAVE_SHFL_XOR64: r = shfl_xor64(v, arg); break;
      case GV_TEST_WAVE_BUTTERFLY: r = f64_bits(wave_butterfly(d)); break;
      case GV_TEST_WAVE_TREE_SHFL: r = f64_bits(wave_tree_sum_shfl(d)); break;
      case GV_TEST_WAVE_DPP_F64_SHL_1: r = f64_bits(dpp_f64<0x101>(d)); break;
      case GV_TEST_WAVE_DPP_F64_SHL_2: r = f64_bits(dpp_f64<0x102>(d)); break;
      case GV_TEST_WAVE_DPP_F64_SHL_4: r = f64_bits(dpp_f64<0x104>(d)); break;
      case GV_TEST_WAVE_DPP_F64_SHL_8: r = f64_bits(dpp_f64<0x108>(d)); break;
      case GV_TEST_WAVE_RANK_LEADER: {
        const unsigned long long m = __ballot((int)(lo & 1u));
        r = m ? pack_words((uint32_t)wave_leader(m), wave_rank(m, lane)) : GV_TEST_WAVE_SKIPPED;
        break;
      }
      case GV_TEST_WAVE_BCAST_U64: r = wave_bcast<unsigned long long>((unsigned long long)v, arg); break;
      case GV_TEST_WAVE_BCAST_I32: r = (unsigned)wave_bcast<int>((int)lo, arg); break;
      case GV_TEST_WAVE_BCAST_F64: r = f64_bits(wave_bcast<double>(d, arg)); break;
      case GV_TEST_WAVE_APPEND: {
        const unsigned long long m = __ballot((int)(lo & 1u));
        if (m) {
          const uint32_t base = wave_append(counter, m, lane);
          r = pack_words(base, base + wave_rank(m, lane));
        } else {
          r = GV_TEST_WAVE_SKIPPED;
        }
        break;
      }
      case GV_TEST_WAVE_APPEND_ALL: {
        const unsigned long long m = __ballot((int)(lo & 1u));
        if (m) {
          const unsigned base = wave_append_all(counter, m, lane);
          r = pack_words(base, base + wave_rank(m, lane));
        } else {
          r = GV_TEST_WAVE_SKIPPED;
        }
        break;
      }
      default: break;
    }
  }
  out[t] = r;
}

}  // namespace gv

namespace {

bool partial_mask_ok(int32_t op)
{
  switch (op) {
    case GV_TEST_WAVE_RANK_LEADER:
    case GV_TEST_WAVE_BCAST_U64:
    case GV_TEST_WAVE_BCAST_I32:
    case GV_TEST_WAVE_BCAST_F64:
    case GV_TEST_WAVE_APPEND:
    case GV_TEST_WAVE_APPEND_ALL: return true;
    default: return false;
  }
}

// group_sum<LANES>: a group of LANES aligned lanes is active as a whole or not at all
bool whole_groups(uint64_t a, int lanes)
{
  const uint64_t g = lanes == 16 ? 0xFFFFull : 0xFFull;
  for (int s = 0; s < 64; s += lanes) {
    const uint64_t b = (a >> s) & g;
    if (b != 0 && b != g) return false;
  }
  return true;
}

bool is_bcast(int32_t op) { return op == GV_TEST_WAVE_BCAST_U64 || op == GV_TEST_WAVE_BCAST_I32 || op == GV_TEST_WAVE_BCAST_F64; }

// gv_test_wave's argument rules (gv_test_hooks.h), before anything touches the device
bool wave_args_ok(int32_t op, int32_t arg, int32_t threads, const uint64_t *active, int64_t n_waves)
{
  if (n_waves < 1 || n_waves > 4096) return false;
  if (threads != 64 && threads != 256 && threads != 1024) return false;
  if (op < 0 || op >= GV_TEST_WAVE_OPS) return false;
  if (op == GV_TEST_WAVE_SHFL_XOR64 && (arg < 1 || arg > 63)) return false;
  if (is_bcast(op) && (arg < 0 || arg > 63)) return false;
  for (int64_t w = 0; w < n_waves; ++w) {
    const uint64_t a = active[w];
    if (op == GV_TEST_WAVE_GROUP_SUM_8 || op == GV_TEST_WAVE_GROUP_SUM_16) {
      if (!whole_groups(a, op == GV_TEST_WAVE_GROUP_SUM_8 ? 8 : 16)) return false;
    } else if (!partial_mask_ok(op) && a != ~0ull) {
      return false;
    }
    if (is_bcast(op) && !((a >> arg) & 1ull)) return false;
    if (op == GV_TEST_WAVE_APPEND_ALL && !(a & 1ull)) return false;
  }
  return true;
}

}  // namespace

int gv_test_wave(gv_handle h, int32_t op, int32_t arg, int32_t threads, const uint64_t *in, const uint64_t *active,
                 int64_t n_waves, uint64_t *out, uint32_t *counter_out)
{
  if (!h || !in || !active || !out || !counter_out) return GV_ERR_BAD_ARG;
  if (!wave_args_ok(op, arg, threads, active, n_waves)) return GV_ERR_BAD_ARG;
  GV_TRY
  int rc = use_device(h);
  if (rc) return rc;
  const size_t n = (size_t)n_waves * 64;
  DevBuf<uint64_t> d_in, d_active, d_out;   // the call's own: released when it returns, whichever way
  DevBuf<uint32_t> d_counter;
  if ((rc = d_in.reserve(h, n)) || (rc = d_active.reserve(h, (size_t)n_waves)) || (rc = d_out.reserve(h, n)) ||
      (rc = d_counter.reserve(h, 1)))
    return rc;
  GV_HIP(hipMemcpyAsync(d_in, in, n * sizeof(uint64_t), hipMemcpyHostToDevice, h->stream));
  GV_HIP(hipMemcpyAsync(d_active, active, (size_t)n_waves * sizeof(uint64_t), hipMemcpyHostToDevice, h->stream));
  GV_HIP(hipMemsetAsync(d_counter, 0, sizeof(uint32_t), h->stream));
  const unsigned blocks = (unsigned)((n + (size_t)threads - 1) / (size_t)threads);
  hipLaunchKernelGGL(gv::k_test_wave, dim3(blocks), dim3((unsigned)threads), 0, h->stream, op, arg,
                     (const uint64_t *)d_in, (const uint64_t *)d_active, n_waves, (uint64_t *)d_out, (uint32_t *)d_counter);
  GV_HIP(hipGetLastError());
  GV_HIP(hipMemcpyAsync(out, d_out, n * sizeof(uint64_t), hipMemcpyDeviceToHost, h->stream));
  GV_HIP(hipMemcpyAsync(counter_out, d_counter, sizeof(uint32_t), hipMemcpyDeviceToHost, h->stream));
  GV_HIP(hipStreamSynchronize(h->stream));
  return GV_OK;
  GV_CATCH
}
