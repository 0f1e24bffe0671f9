// gv_ransac.hip -- the device-resident RANSAC ground plane of the "next tier" cloud_detections calls (SURVEY 8(f)-2:
// segmentGroundPlane, src/cloud_detections.cpp:105-138).  Nothing here moves O(N) bytes to the host.  The per-bbox
// cloud path that uses the plane is gv_cloudops.hip's; the two share the sweep geometry (kCo*, gv_launch_pose.hpp) and
// the inlier test (plane_inlier_dev, gv_device.hpp).
//
// Round 3: every step is one sweep of the cloud or less -- all hypotheses are counted in ONE pass (planes in LDS, one
// transform per point); the refinement is ONE pass of fp64 raw moments whose fixed 64-ary tree is finished by the
// last workgroup to arrive (no tree-level launches).
// gfx950, wave64, built with -ffp-contract=off (gv_device.hpp says why).
#include "gv_launch_pose.hpp"
#include "gv_device.hpp"

#include <algorithm>

namespace gv {

// ------------------------------------------------------------------ RANSAC --
__device__ __forceinline__ unsigned long long splitmix64_dev(unsigned long long z)
{
  z += 0x9E3779B97F4A7C15ull;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

// hypothesis t: three draws of the counter-based stream seed + 3t + {0,1,2} (mod n), plane through the
// three camera-frame points as PCL's SampleConsensusModelPlane (isSampleGood + computeModelCoefficients,
// fp32).  An unusable sample gets a NaN plane: it can never collect an inlier.  Every workgroup of the counting
// pass makes the planes itself (150 loads: cheaper than a launch of its own and the 4 us of a one-wavefront kernel).
__device__ __forceinline__ float4 ransac_hypothesis(const float *__restrict__ x, const float *__restrict__ y,
                                                    const float *__restrict__ z, uint32_t n, const Mat34f &m,
                                                    unsigned long long seed, int t)
{
  float p[3][3];
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const uint32_t id = (uint32_t)(splitmix64_dev(seed + 3ull * (unsigned long long)t + (unsigned long long)k) % (unsigned long long)n);
    xform34(m, x[id], y[id], z[id], p[k][0], p[k][1], p[k][2]);
  }
  const float qnan = __uint_as_float(0x7fc00000u);
  float4 out = make_float4(qnan, qnan, qnan, qnan);
  bool ok = true;
#pragma unroll
  for (int k = 0; k < 3; ++k) ok = ok && isfinite(p[0][k]) && isfinite(p[1][k]) && isfinite(p[2][k]);
  if (ok) {
    const float a[3] = {p[1][0] - p[0][0], p[1][1] - p[0][1], p[1][2] - p[0][2]};
    const float b[3] = {p[2][0] - p[0][0], p[2][1] - p[0][1], p[2][2] - p[0][2]};
    const float r0 = a[0] / b[0], r1 = a[1] / b[1], r2 = a[2] / b[2];
    if ((r0 != r1) || (r2 != r1)) {
      float nn[3] = {a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]};
      const float len = sqrtf((nn[0] * nn[0] + nn[1] * nn[1]) + nn[2] * nn[2]);
      if (len > 0.0f && isfinite(len)) {
        nn[0] /= len; nn[1] /= len; nn[2] /= len;
        out = make_float4(nn[0], nn[1], nn[2], -1.0f * (((nn[0] * p[0][0]) + nn[1] * p[0][1]) + nn[2] * p[0][2]));
      }
    }
  }
  return out;
}

// counts[h] += inliers of hypothesis h, ALL hypotheses in one pass over the cloud: a workgroup transforms its
// 4096 points once (4 per thread, in registers) and walks the planes, which sit in LDS; per plane and
// wavefront the four ballots are counted on the scalar unit and one lane adds them to the plane's LDS counter.
__global__ void __launch_bounds__(kCoThreads) k_ransac_count_all(const float *__restrict__ x, const float *__restrict__ y,
                                                                 const float *__restrict__ z, uint32_t n, Mat34f m,
                                                                 unsigned long long seed, int h0, int iters, float thr_f,
                                                                 unsigned *__restrict__ counts, int stride)
{
  extern __shared__ float4 s_pl[];   // iters planes, then iters counters
  unsigned *s_cnt = reinterpret_cast<unsigned *>(s_pl + iters);
  const int tid = threadIdx.x;
  for (int t = tid; t < iters; t += kCoThreads) { s_pl[t] = ransac_hypothesis(x, y, z, n, m, seed, h0 + t); s_cnt[t] = 0u; }
  const float qnan = __uint_as_float(0x7fc00000u);
  float px[kCoPts], py[kCoPts], pz[kCoPts];
  const size_t base = (size_t)blockIdx.x * kCoBlock;
#pragma unroll
  for (int j = 0; j < kCoPts; ++j) {
    const size_t i = base + (size_t)j * kCoThreads + tid;
    px[j] = py[j] = pz[j] = qnan;   // a NaN point is nobody's inlier
    if (i < n) xform34(m, x[i], y[i], z[i], px[j], py[j], pz[j]);
  }
  __syncthreads();
  // two points per packed-fp32 instruction (v_pk_mul_f32 / v_pk_add_f32: the same separately rounded products and
  // sums as plane_inlier_dev, at twice the rate)
  typedef float v2f __attribute__((ext_vector_type(2)));
  const v2f ax = {px[0], px[1]}, ay = {py[0], py[1]}, az = {pz[0], pz[1]};
  const v2f bx = {px[2], px[3]}, by = {py[2], py[3]}, bz = {pz[2], pz[3]};
  static_assert(kCoPts == 4, "two packed pairs per thread");
  for (int h = 0; h < iters; ++h) {
    const float4 pl = s_pl[h];
    const v2f nx = {pl.x, pl.x}, ny = {pl.y, pl.y}, nz = {pl.z, pl.z}, nw = {pl.w, pl.w};
    const v2f da = ((nx * ax + ny * ay) + nz * az) + nw;
    const v2f db = ((nx * bx + ny * by) + nz * bz) + nw;
    unsigned c = (unsigned)__popcll(__ballot(fabsf(da.x) < thr_f)) + (unsigned)__popcll(__ballot(fabsf(da.y) < thr_f)) +
                 (unsigned)__popcll(__ballot(fabsf(db.x) < thr_f)) + (unsigned)__popcll(__ballot(fabsf(db.y) < thr_f));
    if ((tid & 63) == 0 && c) atomicAdd(&s_cnt[h], c);
  }
  __syncthreads();
  for (int t = tid; t < iters; t += kCoThreads)
    if (s_cnt[t]) atomicAdd(&counts[(size_t)(blockIdx.x % kRansacCountSlices) * stride + t], s_cnt[t]);   // sliced: see gv_launch_pose.hpp
}

// unit eigenvector of the smallest eigenvalue of a symmetric 3x3 (fp64): oracle/ransac.c, operation for operation -- the
// closed form of pcl::eigen33 (scaled matrix, trigonometric roots, largest cross product of rows of A - lambda I).
// Rounds 2-3 ran a cyclic Jacobi here: ninety dependent fp64 divisions and square roots on one lane, 14 us of the
// kernel's 27.  (atan2 / cos / sin may differ from glibc's in the last bit: 1e-16 on lambda, far below the fp32 the
// plane is stored in; the tests accept a last-bit difference of the coefficients and say so.)
__device__ __forceinline__ void smallest_eigenvector3_dev(const double cov[6], double v[3])
{
  double a00 = cov[0], a01 = cov[1], a02 = cov[2], a11 = cov[3], a12 = cov[4], a22 = cov[5];
  double scale = fmax(fmax(fmax(fabs(a00), fabs(a01)), fmax(fabs(a02), fabs(a11))), fmax(fabs(a12), fabs(a22)));
  if (!(scale > 2.2250738585072014e-308)) scale = 1.0;
  a00 = a00 / scale; a01 = a01 / scale; a02 = a02 / scale; a11 = a11 / scale; a12 = a12 / scale; a22 = a22 / scale;
  const double c0 = (((a00 * a11) * a22 + (2.0 * a01) * a02 * a12) - (a00 * a12) * a12 - (a11 * a02) * a02) - (a22 * a01) * a01;
  const double c1 = ((((a00 * a11 - a01 * a01) + a00 * a22) - a02 * a02) + a11 * a22) - a12 * a12;
  const double c2 = (a00 + a11) + a22;
  const double c2_over_3 = c2 * (1.0 / 3.0);
  double a_over_3 = (c2 * c2_over_3 - c1) * (1.0 / 3.0);
  if (a_over_3 < 0.0) a_over_3 = 0.0;
  const double half_b = 0.5 * (c0 + c2_over_3 * (2.0 * c2_over_3 * c2_over_3 - c1));
  double q = a_over_3 * a_over_3 * a_over_3 - half_b * half_b;
  if (q < 0.0) q = 0.0;
  const double rho = sqrt(a_over_3);
  const double theta = atan2(sqrt(q), half_b) * (1.0 / 3.0);
  const double cos_theta = cos(theta), sin_theta = sin(theta);
  const double r0 = c2_over_3 + 2.0 * rho * cos_theta;
  const double r1 = c2_over_3 - rho * (cos_theta + 1.7320508075688772 * sin_theta);
  const double r2 = c2_over_3 - rho * (cos_theta - 1.7320508075688772 * sin_theta);
  double lam = r0;
  if (r1 < lam) lam = r1;
  if (r2 < lam) lam = r2;
  if (lam <= 0.0) lam = 0.0;
  a00 -= lam; a11 -= lam; a22 -= lam;
  const double v1[3] = {a01 * a12 - a02 * a11, a02 * a01 - a00 * a12, a00 * a11 - a01 * a01};
  const double v2[3] = {a01 * a22 - a02 * a12, a02 * a02 - a00 * a22, a00 * a12 - a01 * a02};
  const double v3[3] = {a11 * a22 - a12 * a12, a12 * a02 - a01 * a22, a01 * a12 - a11 * a02};
  const double l1 = (v1[0] * v1[0] + v1[1] * v1[1]) + v1[2] * v1[2];
  const double l2 = (v2[0] * v2[0] + v2[1] * v2[1]) + v2[2] * v2[2];
  const double l3 = (v3[0] * v3[0] + v3[1] * v3[1]) + v3[2] * v3[2];
  const bool p1 = l1 >= l2 && l1 >= l3, p2 = !p1 && l2 >= l1 && l2 >= l3;
  double nn[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) nn[k] = p1 ? v1[k] : (p2 ? v2[k] : v3[k]);
  const double len = sqrt(p1 ? l1 : (p2 ? l2 : l3));
  // sign: the component of largest magnitude (the first of equals) is made positive
  double big = nn[0];
  if (fabs(nn[1]) > fabs(big)) big = nn[1];
  if (fabs(nn[2]) > fabs(big)) big = nn[2];
  const double sg = (big < 0) ? -1.0 / len : 1.0 / len;
  v[0] = nn[0] * sg; v[1] = nn[1] * sg; v[2] = nn[2] * sg;
}

constexpr int kMom = 10;   // Sx Sy Sz Qxx Qxy Qxz Qyy Qyz Qzz + the inlier count (as a double: exact)

// Selection + refinement (optimizeModelCoefficients) in one pass.  Every workgroup finds the best hypothesis
// (most inliers, first wins ties) from the counts, then accumulates the fp64 raw moments of that plane's
// inliers by the fixed 64-ary tree of oracle/ransac.c: level 0 = 64 consecutive points reduced by the
// wavefront butterfly v[i] += v[i + off], off = 32 .. 1 (non-inliers and padding contribute +0.0); a
// workgroup holds 64 level-0 groups, so its level-1 sum is one more butterfly out of LDS.  The workgroup
// whose ticket comes last runs the remaining levels and solves for the plane.  Same tree on both sides:
// the device rounds exactly as the oracle does, whatever the number of workgroups.
__global__ void __launch_bounds__(kCoThreads) k_ransac_moments(const float *__restrict__ x, const float *__restrict__ y,
                                                               const float *__restrict__ z, uint32_t n, Mat34f m,
                                                               unsigned long long seed, unsigned *__restrict__ counts,
                                                               int iters, float thr_f, double *__restrict__ part_a,
                                                               double *__restrict__ part_b, RansacState *__restrict__ st)
{
  __shared__ double s_l0[64][kMom];
  __shared__ unsigned s_bestc, s_last;
  __shared__ int s_best;
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  if (tid < 64) {
    unsigned bc = 0;
    int bi = 0x7fffffff;
    for (int t = tid; t < iters; t += 64) {
      unsigned c = 0;
#pragma unroll
      for (int sl = 0; sl < kRansacCountSlices; ++sl) c += counts[(size_t)sl * iters + t];
      if (c > bc) { bc = c; bi = t; }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
      const unsigned oc = __shfl_xor(bc, off);
      const int oi = __shfl_xor(bi, off);
      if (oc > bc || (oc == bc && oi < bi)) { bc = oc; bi = oi; }
    }
    if (tid == 0) { s_bestc = bc; s_best = bc ? bi : 0; }
  }
  __syncthreads();
  const unsigned bestc = s_bestc;
  const float4 pl = bestc ? ransac_hypothesis(x, y, z, n, m, seed, s_best) : make_float4(0.f, 0.f, 0.f, 0.f);
  // A wavefront owns four level-0 groups (256 consecutive points).  Row q of 16 lanes takes group 4 w + q, and
  // lane r of the row the group's points r, r + 16, r + 32, r + 48: the butterfly's steps 32 and 16 are then adds
  // between the lane's own four values, and steps 8 .. 1 are DPP shifts inside the row -- for the four groups at
  // once, nothing through the permute network.  Same pairs, same order of additions as tree_sum64.
  {
    const int q = lane >> 4, r = lane & 15;
    const int g = w * kCoPts + q;   // level-0 group of this workgroup: points [64 g, 64 g + 64) of its 4096
    const size_t i0 = (size_t)blockIdx.x * kCoBlock + (size_t)g * 64 + r;
    float px[4], py[4], pz[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      const size_t i = i0 + 16 * t;
      const bool in = i < n && bestc;
      px[t] = in ? x[i] : 0.f;
      py[t] = in ? y[i] : 0.f;
      pz[t] = in ? z[i] : 0.f;
    }
    auto moments = [&](int t, double *v) {
#pragma unroll
      for (int k = 0; k < kMom; ++k) v[k] = 0.0;
      float cx, cy, cz;
      xform34(m, px[t], py[t], pz[t], cx, cy, cz);
      if (i0 + 16 * t < n && bestc && plane_inlier_dev(pl, cx, cy, cz, thr_f)) {
        const double dx = (double)cx, dy = (double)cy, dz = (double)cz;
        v[0] = dx; v[1] = dy; v[2] = dz;
        v[3] = dx * dx; v[4] = dx * dy; v[5] = dx * dz; v[6] = dy * dy; v[7] = dy * dz; v[8] = dz * dz;
        v[9] = 1.0;
      }
    };
    double a[kMom], b[kMom], c[kMom];
    moments(0, a);
    moments(2, c);
#pragma unroll
    for (int k = 0; k < kMom; ++k) a[k] = a[k] + c[k];   // step 32: v[r] += v[r + 32]
    moments(1, b);
    moments(3, c);
#pragma unroll
    for (int k = 0; k < kMom; ++k) b[k] = b[k] + c[k];   //          v[r + 16] += v[r + 48]
#pragma unroll
    for (int k = 0; k < kMom; ++k) {
      double v = a[k] + b[k];        // step 16
      v = v + dpp_f64<0x108>(v);     // row_shl:8
      v = v + dpp_f64<0x104>(v);     // row_shl:4
      v = v + dpp_f64<0x102>(v);     // row_shl:2
      v = v + dpp_f64<0x101>(v);     // row_shl:1
      if (r == 0) s_l0[g][k] = v;
    }
  }
  __syncthreads();
  if (w < kMom) {   // level 1: one wavefront per quantity
    const double t = wave_butterfly(s_l0[lane][w]);
    // (agent-scope atomic store: written through to the device's coherence point, where the last workgroup's atomic
    //  loads read it -- see the note at the ticket)
    if (lane == 0) __hip_atomic_store(&part_a[(size_t)blockIdx.x * kMom + w], t, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  // The ticket.  What the last workgroup reads -- the partial sums -- was written by agent-scope atomic stores and is
  // read by agent-scope atomic loads; the ticket itself only has to come after this workgroup's stores have been
  // acknowledged (vmcnt, then the barrier).  A release FENCE instead (rounds 2-3) is a write-back of the whole L2 of the
  // XCD by every workgroup (buffer_wbl2): 10 us of this kernel, 15 us of k_pca_extent (profiles/r04/ticket_fence_ab.txt).
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  if (tid == 0) s_last = take_last_ticket(&st->ticket) ? 1u : 0u;
  __syncthreads();
  if (!s_last) return;
  // levels 2..: groups of 64 partial sums per wavefront.
  size_t cnt = gridDim.x;
  __shared__ double s_tot[kMom];
  const bool short_tree = cnt > 1 && cnt <= 4096;   // up to 16.7 M points: levels 2 and 3 without a trip through memory
  if (short_tree) {
    // ONE round of loads (every wavefront its groups, all ten quantities in flight), level-2 sums into LDS, the
    // level-3 butterfly out of LDS: the tail used to be store -> wait -> barrier -> load per level (10 us of
    // dependent round trips for 245 partial sums)
    const int groups = (int)((cnt + 63) / 64);
    for (int g = w; g < groups; g += kCoThreads / 64) {
      const size_t i = (size_t)g * 64 + lane;
      double v[kMom];
#pragma unroll
      for (int k = 0; k < kMom; ++k)
        v[k] = (i < cnt) ? __hip_atomic_load(&part_a[i * kMom + k], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0.0;
#pragma unroll
      for (int k = 0; k < kMom; ++k) v[k] = wave_butterfly(v[k]);
      if (lane == 0) {
#pragma unroll
        for (int k = 0; k < kMom; ++k) s_l0[g][k] = v[k];
      }
    }
    __syncthreads();
    if (groups > 1) {   // level 3: the group sums and zeros, as the oracle's tree pads them
      if (w < kMom) {
        const double t = wave_butterfly(lane < groups ? s_l0[lane][w] : 0.0);
        if (lane == 0) s_tot[w] = t;
      }
    } else if (tid < kMom) {
      s_tot[tid] = s_l0[0][tid];
    }
    __syncthreads();
  } else {
    // the general tree: ping-pong between the two scratch arrays (agent-scope accesses: other wavefronts of this
    // workgroup wrote them)
    const double *src = part_a;
    double *dst = part_b;
    while (cnt > 1) {
      const size_t groups = (cnt + 63) / 64;
      for (size_t g = (size_t)w; g < groups; g += kCoThreads / 64) {
        const size_t i = g * 64 + lane;
        double v[kMom];
#pragma unroll
        for (int k = 0; k < kMom; ++k)
          v[k] = (i < cnt) ? __hip_atomic_load(&src[i * kMom + k], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0.0;
#pragma unroll
        for (int k = 0; k < kMom; ++k) v[k] = wave_butterfly(v[k]);
        if (lane == 0) {
#pragma unroll
          for (int k = 0; k < kMom; ++k) __hip_atomic_store(&dst[g * kMom + k], v[k], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
      }
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      __syncthreads();
      const double *t = src;
      src = dst;
      dst = const_cast<double *>(t);
      cnt = groups;
    }
    // one workgroup: its level-1 sums ARE the totals only if the tree had a single level-1 group; the oracle's
    // tree always takes at least one level per 64 values, which the loop above reproduces for cnt > 1 and which
    // is the identity (sum of one value and 63 zeros) for cnt == 1
    if (tid < kMom) s_tot[tid] = __hip_atomic_load(&src[tid], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __syncthreads();
  }
  // every workgroup has read the counts: cleared here for the next call (no memset launch; nobody waits for these)
  for (int t = tid; t < iters * kRansacCountSlices; t += kCoThreads) counts[t] = 0u;
  if (tid == 0) {
    double mom[kMom];
    for (int k = 0; k < kMom; ++k) mom[k] = s_tot[k];
    const unsigned long long mi = (unsigned long long)mom[9];
    float4 refined = pl;
    if (bestc && mi >= 3) {
      const double dm = (double)mi;
      const double cx = mom[0] / dm, cy = mom[1] / dm, cz = mom[2] / dm;
      const double cov[6] = {mom[3] / dm - cx * cx, mom[4] / dm - cx * cy, mom[5] / dm - cx * cz,
                             mom[6] / dm - cy * cy, mom[7] / dm - cy * cz, mom[8] / dm - cz * cz};
      double nv[3];
      smallest_eigenvector3_dev(cov, nv);
      refined = make_float4((float)nv[0], (float)nv[1], (float)nv[2], (float)(-((nv[0] * cx + nv[1] * cy) + nv[2] * cz)));
    }
    st->best_count = bestc;
    st->plane = pl;
    st->refined = refined;
    st->m = bestc ? mi : 0ull;
    st->n_inliers = 0ull;   // counted by the mask / classify pass that follows
  }
}

// inliers of the refined plane: mask[i] (device resident) and their number
__global__ void __launch_bounds__(kCoThreads) k_ransac_mask(const float *__restrict__ x, const float *__restrict__ y,
                                                            const float *__restrict__ z, uint32_t n, Mat34f m, float thr_f,
                                                            RansacState *__restrict__ st, uint8_t *__restrict__ mask,
                                                            RansacState *__restrict__ st_copy, CallDone done)
{
  __shared__ unsigned s_n;
  const float4 pl = st->refined;
  const bool have = st->best_count != 0;
  if (threadIdx.x == 0) s_n = 0u;
  __syncthreads();
  unsigned c = 0;
#pragma unroll
  for (int j = 0; j < kCoPts; ++j) {
    const size_t i = (size_t)blockIdx.x * kCoBlock + (size_t)j * kCoThreads + threadIdx.x;
    bool in = false;
    if (i < n) {
      float cx, cy, cz;
      xform34(m, x[i], y[i], z[i], cx, cy, cz);
      in = have && plane_inlier_dev(pl, cx, cy, cz, thr_f);
      mask[i] = in ? 1 : 0;
    }
    c += (unsigned)__popcll(__ballot(in));
  }
  if ((threadIdx.x & 63) == 0 && c) atomicAdd(&s_n, c);
  __syncthreads();
  if (threadIdx.x == 0) {
    if (s_n) atomicAdd(&st->n_inliers, (unsigned long long)s_n);
    if (st_copy) {   // the workgroup that finishes last hands the final state out (the count is an agent-scope atomic:
      // no fence, only this thread's atomic acknowledged before its ticket)
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      if (take_last_ticket(&st->ticket)) {
        RansacState o = *st;
        o.n_inliers = __hip_atomic_load(&st->n_inliers, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        o.ticket = 0u;
        *st_copy = o;
        call_done(done, 1u);
      }
    }
  }
}

size_t ransac_scratch_doubles(size_t n)
{
  const size_t nblk = (n + kCoBlock - 1) / kCoBlock;
  return (size_t)kMom * (nblk + (nblk + 63) / 64 + 2) + 64;
}

void launch_ransac_plane(const RansacArgs &a, hipStream_t s)
{
  const uint32_t nblk = (uint32_t)(((size_t)a.n + kCoBlock - 1) / kCoBlock);
  for (int h0 = 0; h0 < a.iters; h0 += 2048) {   // planes + counters of one launch sit in LDS (20 bytes per hypothesis)
    const int hn = std::min(2048, a.iters - h0);
    hipLaunchKernelGGL(k_ransac_count_all, dim3(nblk), dim3(kCoThreads), (size_t)hn * (sizeof(float4) + sizeof(unsigned)), s, a.x, a.y,
                       a.z, a.n, a.m_cam, a.seed, h0, hn, a.thr_f, a.counts + h0, a.iters);
  }
  double *part_a = a.scratch, *part_b = a.scratch + (size_t)kMom * (nblk + 1);
  hipLaunchKernelGGL(k_ransac_moments, dim3(nblk), dim3(kCoThreads), 0, s, a.x, a.y, a.z, a.n, a.m_cam, a.seed, a.counts, a.iters,
                     a.thr_f, part_a, part_b, a.st);
}

void launch_ransac_mask(const RansacArgs &a, const CallDone &done, hipStream_t s)
{
  const uint32_t nblk = (uint32_t)(((size_t)a.n + kCoBlock - 1) / kCoBlock);
  hipLaunchKernelGGL(k_ransac_mask, dim3(nblk), dim3(kCoThreads), 0, s, a.x, a.y, a.z, a.n, a.m_cam, a.thr_f, a.st, a.mask, a.st_copy,
                     done);
}


}  // namespace gv
