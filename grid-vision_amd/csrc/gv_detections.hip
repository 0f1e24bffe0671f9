// gv_detections.hip -- gfx950 (CDNA4, wave64) kernels over a frame's detections: the bbox-test tables, the two
// rectangle kernels and the vision-orientation solver.
//
// Built with -ffp-contract=off: the reference arithmetic keeps separate
// multiply/add roundings (PCL's SSE transform, grid_map's getIndex), and cell
// indices must be bit-exact, so no FMA contraction anywhere in this file.
// fp64 and fp32 divisions are the compiler's correctly rounded sequences.
//
// Reference lines are cited as file:line relative to the reference root.
#include "gv_launch_frame.hpp"   // the tables and the rectangles
#include "gv_launch_pose.hpp"    // VisionArgs: the solver is the pose calls' as much as the frame's
#include "gv_device.hpp"

#include <algorithm>
#include <cstdlib>

namespace gv {

// Exact fp32 form of the first-match bbox test, built on the device from the uploaded gv_bbox
// array: (double)u >= x_min <=> u >= (smallest float >= x_min), (double)u <= x_max <=> u <= (largest
// float <= x_max) for every float u (NaN bounds stay NaN: always false), and per 16x16-pixel tile the
// mask of boxes whose float range can contain a pixel of that tile (a superset is enough: the mask
// only prunes).  One thread per (tile, 64-box word); every workgroup first converts the boxes of its
// words once into LDS (the first workgroup also stores them), so a thread's loop reads LDS only.
constexpr int kPrepBoxes = 256;   // boxes staged per round
__global__ void __launch_bounds__(256) k_bbox_prepare(const gv_bbox *__restrict__ bb, int32_t nb, int32_t tiles_x,
                                                      int32_t tiles_y, int32_t mask_words, float4 *__restrict__ bbox_f,
                                                      unsigned long long *__restrict__ tile_mask,
                                                      const uint4 *__restrict__ copy_src, uint4 *__restrict__ copy_dst,
                                                      uint32_t copy_words)
{
  __shared__ int4 s_r[kPrepBoxes];   // tile range {tx0, ty0, tx1, ty1} of a box (empty range: tx0 > tx1)
  const int gid = blockIdx.x * blockDim.x + threadIdx.x;
  // optional rider (gv_tick): the detection block goes from its pinned staging to the device in this kernel instead of
  // a copy command in front of it (`bb` then points INTO the staging: the boxes are read over PCIe by every workgroup)
  for (uint32_t i = (uint32_t)gid; i < copy_words; i += gridDim.x * blockDim.x) copy_dst[i] = copy_src[i];
  const int nwords = tiles_x * tiles_y * mask_words;
  const int wd = (gid < nwords) ? gid % mask_words : 0, tile = (gid < nwords) ? gid / mask_words : 0;
  const int tx = tile % tiles_x, ty = tile / tiles_x;
  unsigned long long m = 0ull;
  for (int b0 = 0; b0 < nb; b0 += kPrepBoxes) {
    __syncthreads();
    const int i = b0 + (int)threadIdx.x;
    if (i < nb) {
      const gv_bbox b = bb[i];
      const float4 f = make_float4(__double2float_ru(b.x_min), __double2float_ru(b.y_min), __double2float_rd(b.x_max),
                                   __double2float_rd(b.y_max));
      if (blockIdx.x == 0) bbox_f[i] = f;
      // the box's tile range, once per workgroup (every thread used to redo this for every box): tiles whose
      // pixel range [16t, 16t+16) can contain a u in [f.x, f.z]
      int4 r = make_int4(1, 1, 0, 0);   // empty or NaN box never matches
      if (f.x <= f.z && f.y <= f.w) {
        int tx0 = (int)floorf(fmaxf(f.x, 0.0f) / 16.0f), tx1 = (int)floorf(fminf(f.z, 16.0f * tiles_x - 1.0f) / 16.0f);
        int ty0 = (int)floorf(fmaxf(f.y, 0.0f) / 16.0f), ty1 = (int)floorf(fminf(f.w, 16.0f * tiles_y - 1.0f) / 16.0f);
        r = make_int4(max(tx0, 0), max(ty0, 0), min(tx1, tiles_x - 1), min(ty1, tiles_y - 1));
      }
      s_r[threadIdx.x] = r;
    }
    __syncthreads();
    const int lo = max(b0, 64 * wd), hi = min(min(nb, b0 + kPrepBoxes), 64 * wd + 64);
    for (int q0 = lo; q0 < hi; q0 += 8) {   // eight LDS reads in flight, predicated (no rolled remainder loop)
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        const int q = q0 + u;
        const int4 r = s_r[min(q, hi - 1) - b0];
        if (q < hi && tx >= r.x && tx <= r.z && ty >= r.y && ty <= r.w) m |= 1ull << (q & 63);
      }
    }
  }
  if (gid < nwords) tile_mask[gid] = m;
}

void launch_bbox_prepare(const BBoxPrepareArgs &a, hipStream_t s)
{
  const int n = std::max(a.tiles_x * a.tiles_y * a.mask_words, 1);   // (>= 1 workgroup: it also stores the thresholds)
  hipLaunchKernelGGL(k_bbox_prepare, dim3((n + 255) / 256), dim3(256), 0, s, a.bboxes, a.nb, a.tiles_x, a.tiles_y, a.mask_words,
                     a.bbox_f, a.tile_mask, static_cast<const uint4 *>(a.copy_src), static_cast<uint4 *>(a.copy_dst),
                     (uint32_t)((a.copy_bytes + 15) / 16));
}

// ------------------------------------------------------------- rectangles --
__global__ void k_rects_from_poses(const gv_lshape_pose *__restrict__ poses, int32_t n, GridParams g,
                                   bool from_cam, Xform64 bc, Rect *__restrict__ rects)
{
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  gv_lshape_pose p = poses[i];
  if (from_cam) {
    // tf2::doTransform(Pose): position = basis * v + origin  (grid_vision_node.cpp:370-374)
    const double vx = p.px, vy = p.py, vz = p.pz;
    p.px = ((bc.b[0] * vx + bc.b[1] * vy) + bc.b[2] * vz) + bc.o[0];
    p.py = ((bc.b[3] * vx + bc.b[4] * vy) + bc.b[5] * vz) + bc.o[1];
  }
  rects[i] = rect_from_pose(g, p);
}

void launch_rects_from_poses(const RectsFromPosesArgs &a, hipStream_t s)
{
  if (a.n <= 0) return;
  hipLaunchKernelGGL(k_rects_from_poses, dim3((a.n + 63) / 64), dim3(64), 0, s, a.poses, a.n, a.g, a.from_cam, a.bc, a.rects);
}

// getEstimatedDepth  src/occupancy_grid.cpp:185-196
__device__ __forceinline__ float estimated_depth(int label)
{
  switch (label) {
  case 9: return 3.5f;   // VEHICLE
  case 2: return 0.6f;   // PERSON
  case 0: return 2.5f;   // BIKE
  case 1: return 2.5f;   // MOTORBIKE
  default: return -1.0f;
  }
}

// computeBoundingBox3D  src/occupancy_grid.cpp:107-138 (dead code in the reference)
__global__ void k_rects_from_points(const double *__restrict__ pts, const gv_bbox *__restrict__ bb, int32_t n,
                                    GridParams g, Rect *__restrict__ rects)
{
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const float d = estimated_depth(bb[i].label);
  const double x = pts[3 * i], y = pts[3 * i + 1];
  const double c[8] = {x + d, y + (d / 2), x + d, y - (d / 2), x, y - (d / 2), x, y + (d / 2)};
  rects[i] = rect_from_corners(g, c);
}

void launch_rects_from_points(const RectsFromPointsArgs &a, hipStream_t s)
{
  if (a.n <= 0) return;
  hipLaunchKernelGGL(k_rects_from_points, dim3((a.n + 63) / 64), dim3(64), 0, s, a.pts_xyz, a.bboxes, a.n, a.g, a.rects);
}

// ------------------------------------------------- vision orientation (A13/A14) --
// Eigen::ColPivHouseholderQR<Matrix<float,4,3>>::solve, restated; one lane each.
__device__ void qr_solve_4x3(const float Ain[12], const float bin[4], float x[3])
{
  float a[4][3], c[4], hc[3], ncu[3], ncd[3];
  int transp[3];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
#pragma unroll
    for (int j = 0; j < 3; ++j) a[i][j] = Ain[i * 3 + j];
    c[i] = bin[i];
  }
  float maxn = 0.0f;
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    float s = 0.0f;
#pragma unroll
    for (int i = 0; i < 4; ++i) s += a[i][j] * a[i][j];
    ncu[j] = ncd[j] = sqrtf(s);
    if (ncu[j] > maxn) maxn = ncu[j];
  }
  const float eps = FLT_EPSILON;
  const float th = maxn * eps / 4.0f;
  const float threshold_helper = th * th;
  const float downdate_thr = sqrtf(eps);
  int nonzero = 3;
  float maxpivot = 0.0f;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    int big = k;
    float bigv = ncu[k];
#pragma unroll
    for (int j = k + 1; j < 3; ++j)
      if (ncu[j] > bigv) { bigv = ncu[j]; big = j; }
    const float big_sq = bigv * bigv;
    if (nonzero == 3 && big_sq < threshold_helper * (float)(4 - k)) nonzero = k;
    transp[k] = big;
    if (big != k) {
#pragma unroll
      for (int j = k + 1; j < 3; ++j) {
        if (j == big) {
#pragma unroll
          for (int i = 0; i < 4; ++i) { const float t = a[i][k]; a[i][k] = a[i][j]; a[i][j] = t; }
          float t = ncu[k]; ncu[k] = ncu[j]; ncu[j] = t;
          t = ncd[k]; ncd[k] = ncd[j]; ncd[j] = t;
        }
      }
    }
    float tail = 0.0f;
#pragma unroll
    for (int i = k + 1; i < 4; ++i) tail += a[i][k] * a[i][k];
    const float c0 = a[k][k];
    float tau, beta;
    if (tail <= FLT_MIN) {
      tau = 0.0f;
      beta = c0;
#pragma unroll
      for (int i = k + 1; i < 4; ++i) a[i][k] = 0.0f;
    } else {
      beta = sqrtf(c0 * c0 + tail);
      if (c0 >= 0.0f) beta = -beta;
#pragma unroll
      for (int i = k + 1; i < 4; ++i) a[i][k] = a[i][k] / (c0 - beta);
      tau = (beta - c0) / beta;
    }
    hc[k] = tau;
    a[k][k] = beta;
    if (fabsf(beta) > maxpivot) maxpivot = fabsf(beta);
    if (tau != 0.0f) {
#pragma unroll
      for (int j = k + 1; j < 3; ++j) {
        float tmp = 0.0f;
#pragma unroll
        for (int i = k + 1; i < 4; ++i) tmp += a[i][k] * a[i][j];
        tmp += a[k][j];
        a[k][j] -= tau * tmp;
#pragma unroll
        for (int i = k + 1; i < 4; ++i) a[i][j] -= tau * a[i][k] * tmp;
      }
    }
#pragma unroll
    for (int j = k + 1; j < 3; ++j) {
      if (ncu[j] != 0.0f) {
        float t = fabsf(a[k][j]) / ncu[j];
        t = (1.0f + t) * (1.0f - t);
        t = t < 0.0f ? 0.0f : t;
        const float r = ncu[j] / ncd[j];
        const float t2 = t * r * r;
        if (t2 <= downdate_thr) {
          float s = 0.0f;
#pragma unroll
          for (int i = k + 1; i < 4; ++i) s += a[i][j] * a[i][j];
          ncd[j] = sqrtf(s);
          ncu[j] = ncd[j];
        } else
          ncu[j] *= sqrtf(t);
      }
    }
  }
  int perm[3] = {0, 1, 2};
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    // perm[k] <-> perm[transp[k]] with register-resident selects
    const int tk = transp[k];
    const int pk = perm[k];
    const int pt = (tk == 0) ? perm[0] : (tk == 1) ? perm[1] : perm[2];
    perm[k] = pt;
    if (tk == 0) perm[0] = (k == 0) ? pt : pk;
    if (tk == 1) perm[1] = (k == 1) ? pt : pk;
    if (tk == 2) perm[2] = (k == 2) ? pt : pk;
  }
  const float prethr = fabsf(maxpivot) * (eps * 3.0f);
  int rank = 0;
#pragma unroll
  for (int i = 0; i < 3; ++i)
    if (i < nonzero && fabsf(a[i][i]) > prethr) ++rank;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    if (hc[k] != 0.0f) {
      float tmp = 0.0f;
#pragma unroll
      for (int i = k + 1; i < 4; ++i) tmp += a[i][k] * c[i];
      tmp += c[k];
      c[k] -= hc[k] * tmp;
#pragma unroll
      for (int i = k + 1; i < 4; ++i) c[i] -= hc[k] * a[i][k] * tmp;
    }
  }
  float y[3] = {0.0f, 0.0f, 0.0f};
#pragma unroll
  for (int i = 2; i >= 0; --i) {
    if (i < rank) {
      float s = c[i];
#pragma unroll
      for (int j = i + 1; j < 3; ++j)
        if (j < rank) s -= a[i][j] * y[j];
      y[i] = s / a[i][i];
    }
  }
  x[0] = x[1] = x[2] = 0.0f;
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    if (i < rank) {
      const int p = perm[i];
      if (p == 0) x[0] = y[i];
      if (p == 1) x[1] = y[i];
      if (p == 2) x[2] = y[i];
    }
  }
}

// One wavefront per bbox: the 2 x 4 x 2 x 4 = 64 constraint combinations of
// calcLocation (src/vision_orientation.cpp:359-374) are exactly the 64 lanes.
__global__ void __launch_bounds__(64) k_vision(const float *__restrict__ orient, const float *__restrict__ conf,
                                               const float *__restrict__ dims, const gv_bbox *__restrict__ bboxes,
                                               int32_t nb, gv_cam_params cam, VisionOut *__restrict__ out,
                                               gv_lshape_pose *__restrict__ poses_cam, float *__restrict__ sets,
                                               VisionOut *__restrict__ out_dev)
{
  const int bi = blockIdx.x;
  if (bi >= nb) return;
  const int lane = threadIdx.x;
  const gv_bbox bb = bboxes[bi];
  const float *cs = conf + bi * 2, *os = orient + bi * 4, *ds = dims + bi * 3;
  // postProcessOutputs :466-470
  const int argmax = (cs[1] > cs[0]) ? 1 : 0;
  // generateBins(2) :241-258
  const float interval = (float)(2.0f * 3.14159265358979323846 / 2);
  const float bin = (argmax ? interval : 0.0f) + interval / 2.0f;
  // computeAlpha :260-275
  // The device's contract: each of the six trig values is evaluated in fp64 and rounded once to fp32, everything
  // else runs in the reference's fp32 operation order, and the lowest set index wins on equal residuals
  // (tests/vision_ref.py restates it; tests/test_gpu_vision.py holds all 64 sets to it bit for bit).  That is
  // NOT what the host's float libm returns: glibc 2.35's atan2f differs from the rounded fp64 value for about
  // one argument in six, atanf for 7 %, tanf for 4 %, sinf and cosf for over 1 % (DESIGN, Tolerances), so alpha can
  // sit one ulp from the oracle's, and next to a threshold that is another corner branch.
  float alpha = (float)atan2((double)os[argmax * 2 + 1], (double)os[argmax * 2 + 0]);
  alpha += bin;
  alpha -= (float)3.14159265358979323846;
  // computeThetaRay :277-292
  const float fovx = 2.0f * (float)atan((double)(cam.orig_w / (2.0f * cam.fx)));
  const float box_center_x = (float)((bb.x_min + bb.x_max) / 2.0f);
  float ddx = box_center_x - (cam.orig_w / 2.0f);
  const float sign = (ddx < 0) ? -1.0f : 1.0f;
  ddx = fabsf(ddx);
  float theta_ray = (float)atan((double)((2.0f * ddx * (float)tan((double)(fovx / 2.0f))) / cam.orig_w));
  theta_ray *= sign;
  // class averages  include/grid_vision/vision_orientation.hpp:58-69, dims :472-495
  float al = 0, aw = 0, ah = 0;
  int valid = 1;
  switch (bb.label) {
  case 9: al = 3.884f; aw = 1.629f; ah = 1.526f; break;
  case 0: al = 1.763f; aw = 0.597f; ah = 1.737f; break;
  case 1: al = 2.2f; aw = 0.8f; ah = 1.5f; break;
  case 2: al = 0.842f; aw = 0.660f; ah = 1.761f; break;
  default: valid = 0; break;
  }
  const float len = ds[2] + al, wid = ds[0] + aw, hgt = ds[1] + ah;
  // calcLocation :294-447
  const float orient_f = alpha + theta_ray;
  const float c = (float)cos((double)orient_f), s = (float)sin((double)orient_f);
  const float Rm[9] = {c, 0, s, 0, 1, 0, -s, 0, c};
  const float box[4] = {(float)bb.x_min, (float)bb.y_min, (float)bb.x_max, (float)bb.y_max};
  const float hx = (float)((double)len / 2.0f);
  const float hy = (float)((double)wid / 2.0f);
  const float hz = (float)((double)hgt / 2.0f);
  int left_mult = 1, right_mult = -1;
  const float deg88 = (float)(88 * 3.14159265358979323846 / 180.0f);
  const float deg90 = (float)(90 * 3.14159265358979323846 / 180.0f);
  const float deg92 = (float)(92 * 3.14159265358979323846 / 180.0f);
  if (alpha < deg92 && alpha > deg88) { left_mult = 1; right_mult = 1; }
  else if (alpha < -deg88 && alpha > -deg92) { left_mult = -1; right_mult = -1; }
  else if (alpha < deg90 && alpha > -deg90) { left_mult = -1; right_mult = 1; }
  const int switch_mult = (alpha > 0) ? 1 : -1;
  // lane -> (left, top, right, bottom) in the reference's loop order :363-374
  const int l = lane >> 5, t = (lane >> 3) & 3, r = (lane >> 2) & 1, b = lane & 3;
  const float li = l ? 1.0f : -1.0f, ri = r ? 1.0f : -1.0f;
  const float ti = (t >> 1) ? 1.0f : -1.0f, tj = (t & 1) ? 1.0f : -1.0f;
  const float bi_ = (b >> 1) ? 1.0f : -1.0f, bj = (b & 1) ? 1.0f : -1.0f;
  const float X[4][3] = {{left_mult * hx, li * hy, -switch_mult * hz},
                         {ti * hx, -hy, tj * hz},
                         {right_mult * hx, ri * hy, switch_mult * hz},
                         {bi_ * hx, hy, bj * hz}};
  const float P[3][4] = {{cam.fx, 0.0f, cam.cx, 0.0f}, {0.0f, cam.fy, cam.cy, 0.0f}, {0.0f, 0.0f, 1.0f, 0.0f}};
  float A[12], bv[4];
#pragma unroll
  for (int row = 0; row < 4; ++row) {
    float RX[3];
#pragma unroll
    for (int q = 0; q < 3; ++q) RX[q] = (Rm[q * 3] * X[row][0] + Rm[q * 3 + 1] * X[row][1]) + Rm[q * 3 + 2] * X[row][2];
    float pM3[3];
#pragma unroll
    for (int q = 0; q < 3; ++q) pM3[q] = ((P[q][0] * RX[0] + P[q][1] * RX[1]) + P[q][2] * RX[2]) + P[q][3] * 1.0f;
    const int idx = row & 1;   // indices = {0,1,0,1} :379
    const float v = box[row];
#pragma unroll
    for (int cc = 0; cc < 3; ++cc) A[row * 3 + cc] = P[idx][cc] - v * P[2][cc];   // :412 (pM(:, :3) == P(:, :3))
    bv[row] = v * pM3[2] - pM3[idx];                                             // :415
  }
  float loc[3];
  qr_solve_4x3(A, bv, loc);
  float err = 0.0f;
#pragma unroll
  for (int row = 0; row < 4; ++row) {
    const float rr = ((A[row * 3] * loc[0] + A[row * 3 + 1] * loc[1]) + A[row * 3 + 2] * loc[2]) - bv[row];
    err += rr * rr;
  }
  // sequential "if (error < best_error)" from FLT_MAX (:382,:424) == min with lowest index on ties
  float best = (err < FLT_MAX) ? err : FLT_MAX;
  int who = (err < FLT_MAX) ? lane : 64;
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const float ob = __shfl_xor(best, off);
    const int ow = __shfl_xor(who, off);
    if (ob < best || (ob == best && ow < who)) { best = ob; who = ow; }
  }
  if (sets) {   // gv_test_vision_sets only: every lane's (loc, err), then the winner (64 = none) behind all nb * 64 sets
    float *o = sets + ((size_t)bi * 64 + lane) * 4;
    o[0] = loc[0]; o[1] = loc[1]; o[2] = loc[2]; o[3] = err;
    if (lane == 0) reinterpret_cast<int32_t *>(sets + (size_t)nb * 256)[bi] = who;
  }
  const int src = (who < 64) ? who : 0;
  const float l0 = __shfl(loc[0], src), l1 = __shfl(loc[1], src), l2 = __shfl(loc[2], src);
  if (lane == 0) {
    VisionOut o;
    o.loc[0] = (who < 64) ? l0 : 0.0f;
    o.loc[1] = (who < 64) ? l1 : 0.0f;
    o.loc[2] = (who < 64) ? l2 : 0.0f;
    o.orient = orient_f;
    o.err = best;
    o.dims[0] = len; o.dims[1] = wid; o.dims[2] = hgt;
    o.valid = valid;
    out[bi] = o;
    if (out_dev) out_dev[bi] = o;   // a GV_TICK_KEEP_DETS tick only: the record once more, in device memory (k_tick_dets reads it)
    gv_lshape_pose p;
    p.px = o.loc[0]; p.py = o.loc[1]; p.pz = o.loc[2];
    p.qx = 0; p.qy = 0; p.qz = 0; p.qw = 1;
    p.length = valid ? (double)len : __builtin_nan("");   // NaN marks "no pose": its corners fail getIndex
    p.width = wid;
    p.height = hgt;
    poses_cam[bi] = p;
  }
}

void launch_vision(const VisionArgs &a, hipStream_t s)
{
  if (a.nb <= 0) return;
  hipLaunchKernelGGL(k_vision, dim3(a.nb), dim3(64), 0, s, a.orient, a.conf, a.dims, a.bboxes, a.nb, a.cam, a.out, a.poses_cam,
                     a.sets, a.out_dev);
}

}  // namespace gv
