// dev_filter.h — what the image-space units (denoise.hip, variance.hip,
// firefly.hip, temporal.hip) share on the device: the guide word's classes, the
// finiteness tests, the filter kernels' weights, the direct kernels' pixel
// mapping and the same-surface terms.  Every float expression keeps the shape
// the definitions give it, parentheses included — the units are compiled with
// contraction on, and the shape decides which products fuse.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace mrt {
namespace {

// The guide word (kern_stage.h guide_kernel): the material index, bit 31 set on
// a light; a miss is all ones.  A pixel is filterable iff word < kNotFilterable.
constexpr uint32_t kNotFilterable = 0x80000000u;
constexpr uint32_t kMissWord = 0xFFFFFFFFu;
// a light pixel: not filterable and not a miss
__device__ __forceinline__ bool is_light(uint32_t word) { return word - kNotFilterable < kMissWord - kNotFilterable; }

__device__ __forceinline__ bool finite1(float x) { return (__float_as_uint(x) & 0x7F800000u) != 0x7F800000u; }
__device__ __forceinline__ bool finite3(float x, float y, float z) { return finite1(x) && finite1(y) && finite1(z); }
__device__ __forceinline__ float lum(float r, float g, float b) { return (0.2126f * r + 0.7152f * g) + 0.0722f * b; }

__device__ __forceinline__ float kern(int d) {   // (1/16, 1/4, 3/8, 1/4, 1/16)[d + 2]
  return d == 0 ? 0.375f : ((d == 1 || d == -1) ? 0.25f : 0.0625f);
}
__device__ __forceinline__ float hat(int d) { return d == 0 ? 0.5f : 0.25f; }   // (1/4, 1/2, 1/4)[d + 1]
__device__ __forceinline__ float normal_weight(float D, uint32_t e) {          // max(0, D)^(2^e)
  D = fmaxf(0.0f, D);
  for (uint32_t j = 0; j < e; ++j) D *= D;
  return D;
}

// One pixel per lane over the whole image: a block of 256 threads is 64 x 4
// pixels, a wave one row of 64 — a tap row outside the image is skipped by the
// whole wave, a tap column by its lanes, and a pixel's 16-B records are
// coalesced.  False for a lane outside the image.
__device__ __forceinline__ bool pixel_64x4(uint32_t width, uint32_t height, int& x, int& y, size_t& i) {
  x = (int)(blockIdx.x * 64u + (threadIdx.x & 63u));
  y = (int)(blockIdx.y * 4u + (threadIdx.x >> 6));
  i = (size_t)y * width + (uint32_t)x;
  return x < (int)width && y < (int)height;
}
inline dim3 grid_64x4(uint32_t width, uint32_t height) { return dim3((width + 63) / 64, (height + 3) / 4); }

// The same-surface terms of a centre p (normal n, position x, distance t) and a
// tap q: n_p.n_q, |n_p.(x_q - x_p)| and 1 / (sigma_plane t_p).
// (Scalars, not float3: handed a vector built from parts of two staged 16-B
// records, the compiler splits each record's LDS read in two.)
__device__ __forceinline__ float normal_dot(float nx, float ny, float nz, float qnx, float qny, float qnz) {
  return (nx * qnx + ny * qny) + nz * qnz;
}
__device__ __forceinline__ float plane_distance(float nx, float ny, float nz, float px, float py, float pz, float qpx,
                                                float qpy, float qpz) {
  return fabsf((nx * (qpx - px) + ny * (qpy - py)) + nz * (qpz - pz));
}
__device__ __forceinline__ float inv_plane(float sigma_plane, float t) { return 1.0f / (sigma_plane * t); }

}  // namespace
}  // namespace mrt
