// gv_cloudio.hip -- gfx950 (CDNA4, wave64) kernels that move a cloud or a layer from one form to another: the
// camera-frame copy, the PointCloud2 de-interleave, the packed grid to pinned memory, and the fill / hold / convert
// helpers of the host side.
//
// Built with -ffp-contract=off: the reference arithmetic keeps separate
// multiply/add roundings (PCL's SSE transform, grid_map's getIndex), and cell
// indices must be bit-exact, so no FMA contraction anywhere in this file.
// fp64 and fp32 divisions are the compiler's correctly rounded sequences.
//
// Reference lines are cited as file:line relative to the reference root.
#include "gv_launch_frame.hpp"
#include "gv_device.hpp"

#include <algorithm>
#include <cstdlib>

namespace gv {

// The packed grid to pinned host memory by a kernel of its own (gv_publish_grid_async): 16-byte stores of consecutive
// lanes, i.e. posted PCIe writes of whole lines, from a few workgroups -- the copy engines stay with the cloud uploads.
__global__ void __launch_bounds__(256) k_publish_grid(const uint4 *__restrict__ src, uint4 *__restrict__ dst, uint32_t n16)
{
  for (uint32_t i = blockIdx.x * 256u + threadIdx.x; i < n16; i += gridDim.x * 256u) dst[i] = src[i];
}

void launch_publish_grid(const int8_t *src, int8_t *dst_host, size_t bytes, int blocks, hipStream_t s)
{
  const uint32_t n16 = (uint32_t)(bytes / 16);
  if (n16) hipLaunchKernelGGL(k_publish_grid, dim3(blocks), dim3(256), 0, s, reinterpret_cast<const uint4 *>(src),
                              reinterpret_cast<uint4 *>(dst_host), n16);
}

// A1 standalone: camera-frame copy of the cloud (transformLidarToCamera)
__global__ void __launch_bounds__(256) k_transform(const float *__restrict__ x, const float *__restrict__ y,
                                                   const float *__restrict__ z, uint32_t n, Mat34f m,
                                                   float *__restrict__ ox, float *__restrict__ oy,
                                                   float *__restrict__ oz)
{
  const uint32_t stride = gridDim.x * blockDim.x;
  for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
    float a, b, c;
    xform34(m, x[i], y[i], z[i], a, b, c);
    ox[i] = a;
    oy[i] = b;
    oz[i] = c;
  }
}

void launch_transform_cloud(const TransformCloudArgs &a, hipStream_t s)
{
  if (!a.n) return;
  const uint32_t blocks = (uint32_t)std::min<uint64_t>(((uint64_t)a.n + 255) / 256, (uint64_t)4096);
  hipLaunchKernelGGL(k_transform, dim3(blocks), dim3(256), 0, s, a.x, a.y, a.z, a.n, a.m, a.ox, a.oy, a.oz);
}

// PointCloud2 bytes -> SoA (pcl::fromROSMsg, src/grid_vision_node.cpp:105).  One
// thread per point; fields may be unaligned inside point_step, so assemble from bytes
// when the offsets are not 4-byte aligned.
__global__ void __launch_bounds__(256) k_deinterleave(const uint8_t *__restrict__ d, uint32_t n,
                                                      uint32_t step, uint32_t offx, uint32_t offy,
                                                      uint32_t offz, float *__restrict__ x,
                                                      float *__restrict__ y, float *__restrict__ z,
                                                      bool aligned)
{
  const uint32_t stride = gridDim.x * blockDim.x;
  for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
    const uint8_t *p = d + (size_t)i * step;
    if (aligned) {
      x[i] = *reinterpret_cast<const float *>(p + offx);
      y[i] = *reinterpret_cast<const float *>(p + offy);
      z[i] = *reinterpret_cast<const float *>(p + offz);
    } else {
      uint32_t w[3];
      const uint32_t off[3] = {offx, offy, offz};
      for (int k = 0; k < 3; ++k)
        w[k] = (uint32_t)p[off[k]] | ((uint32_t)p[off[k] + 1] << 8) | ((uint32_t)p[off[k] + 2] << 16)
               | ((uint32_t)p[off[k] + 3] << 24);
      x[i] = __uint_as_float(w[0]);
      y[i] = __uint_as_float(w[1]);
      z[i] = __uint_as_float(w[2]);
    }
  }
}

void launch_deinterleave(const DeinterleaveArgs &a, hipStream_t s)
{
  if (!a.n) return;
  const bool aligned = ((a.point_step | a.off_x | a.off_y | a.off_z) & 3u) == 0 && (((uintptr_t)a.data) & 3u) == 0;
  const uint32_t blocks = (uint32_t)std::min<uint64_t>(((uint64_t)a.n + 255) / 256, (uint64_t)4096);
  hipLaunchKernelGGL(k_deinterleave, dim3(blocks), dim3(256), 0, s, a.data, a.n, a.point_step, a.off_x, a.off_y,
                     a.off_z, a.x, a.y, a.z, aligned);
}

// ------------------------------------------------------------------ misc --
__global__ void k_fill_f32(float *p, float v, size_t n)
{
  const size_t stride = (size_t)gridDim.x * blockDim.x;
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n; i += stride) p[i] = v;
}

void launch_fill_f32(float *p, float v, size_t n, hipStream_t s)
{
  if (!n) return;
  const uint32_t blocks = (uint32_t)std::min<size_t>((n + 255) / 256, (size_t)4096);
  hipLaunchKernelGGL(k_fill_f32, dim3(blocks), dim3(256), 0, s, p, v, n);
}

// one wavefront that stays on the device for `ticks` of the constant-rate clock (100 MHz): the queue probe of
// gv_create (is the upload stream's hardware queue shared with a busy stream?)
__global__ void k_hold(unsigned long long ticks, unsigned *sink)
{
  const unsigned long long t0 = __builtin_amdgcn_s_memrealtime();
  unsigned n = 0;
  while ((unsigned long long)__builtin_amdgcn_s_memrealtime() - t0 < ticks) {
    __builtin_amdgcn_s_sleep(32);
    ++n;
  }
  if (sink && n == 0xFFFFFFFFu) *sink = n;
}

void launch_hold(unsigned long long ticks, hipStream_t s)
{
  hipLaunchKernelGGL(k_hold, dim3(1), dim3(64), 0, s, ticks, (unsigned *)nullptr);
}

__global__ void k_i16_to_i32(const int16_t *in, int32_t *out, size_t n)
{
  const size_t stride = (size_t)gridDim.x * blockDim.x;
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n; i += stride) out[i] = (int32_t)in[i];
}

void launch_i16_to_i32(const int16_t *in, int32_t *out, size_t n, hipStream_t s)
{
  if (!n) return;
  const uint32_t blocks = (uint32_t)std::min<size_t>((n + 255) / 256, (size_t)4096);
  hipLaunchKernelGGL(k_i16_to_i32, dim3(blocks), dim3(256), 0, s, in, out, n);
}

__global__ void k_u8_to_i32(const uint8_t *in, int32_t *out, size_t n)
{
  const size_t stride = (size_t)gridDim.x * blockDim.x;
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n; i += stride) out[i] = in[i] ? 1 : 0;
}

void launch_u8_to_i32(const uint8_t *in, int32_t *out, size_t n, hipStream_t s)
{
  if (!n) return;
  const uint32_t blocks = (uint32_t)std::min<size_t>((n + 255) / 256, (size_t)4096);
  hipLaunchKernelGGL(k_u8_to_i32, dim3(blocks), dim3(256), 0, s, in, out, n);
}

}  // namespace gv
