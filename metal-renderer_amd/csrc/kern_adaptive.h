// kern_adaptive.h — adaptive sampling (include/mrt.h "adaptive sampling",
// DESIGN.md §2.1q): the counted accumulate of a refine draw, the merge of two
// counted images, the per-tile priority from the variance plane and the
// selection of the highest-priority tiles.  The render kernels read the tile
// list through slot_pixel_l (dev_shade.h).
#pragma once
#include "kern_stage.h"

namespace mrt { namespace MRT_NS {
#if MRT_EMIT_MAIN   // (not in the stream unit)
namespace {

// slot_pixel of a listed tile: pixel p (8x8-block order) of tile t
__device__ __forceinline__ void tile_pixel(uint32_t t, uint32_t p, uint32_t tiles_x, uint32_t& x, uint32_t& y) {
  const uint32_t ty = t / tiles_x, tx = t - ty * tiles_x;
  const uint32_t blk = p >> 6, q = p & 63u;
  x = tx * kTile + (blk & 7u) * 8u + (q & 7u);
  y = ty * kTile + (blk >> 3) * 8u + (q >> 3);
}

// accumulate_frame_kernel for the extra samples of a refine draw: the tiles
// are those of a.tile_list and every pixel carries its own sample count, since
// the tiles of one draw have been refined a different number of times.  With
// n = (uint32_t)E[p].w: E[p].rgb = accumulate_value(E[p].rgb, c, n),
// E[p].w = n + 1, frame by frame in order (n == 0 overwrites), and EM[p] the
// same over (l, l*l, 0).  E is a.image, EM a.moments; both are counted images
// and hold the same count.  As the MOMENTS accumulate: two frames' loads in
// flight, at most 32 VGPRs and no scratch, so that it runs beside a rendering
// batch.
__global__ __launch_bounds__(kBlock) __attribute__((amdgpu_num_vgpr(32))) void accumulate_counted_kernel(AccumArgs a) {
  fold_draw_counters(a);
  for (uint32_t idx = blockIdx.x * kBlock + threadIdx.x; idx < a.num_slots; idx += gridDim.x * kBlock) {
    uint32_t x, y;
    tile_pixel(a.tile_list[idx >> 12], idx & 4095u, a.tiles_x, x, y);
    if (x >= a.width || y >= a.height) continue;
    const uint32_t pix = y * a.width + x;
    const float4* rad = a.radiance + idx;
    float4 cur = a.image[pix];
    const float4 m = a.moments[pix];
    const uint32_t n = (uint32_t)cur.w;
    float m1 = m.x, m2 = m.y;
    constexpr uint32_t kLoads = kAccLoads / 2;
    uint32_t j = 0;
    for (; j + kLoads <= a.batch; j += kLoads) {
      float4 c[kLoads];
#pragma unroll
      for (uint32_t k = 0; k < kLoads; ++k) {
        typedef float v4f __attribute__((ext_vector_type(4)));
        const v4f v = __builtin_nontemporal_load(reinterpret_cast<const v4f*>(rad + (size_t)(j + k) * a.num_slots));
        c[k] = make_float4(v.x, v.y, v.z, v.w);
      }
#pragma unroll
      for (uint32_t k = 0; k < kLoads; ++k) {
        cur = accumulate_value(cur, mk(c[k]), n + j + k);
        accumulate_moments(m1, m2, mk(c[k]), n + j + k);
      }
    }
    for (; j < a.batch; ++j) {
      const V3 c = mk(rad[(size_t)j * a.num_slots]);
      cur = accumulate_value(cur, c, n + j);
      accumulate_moments(m1, m2, c, n + j);
    }
    const float count = float(n + a.batch);
    a.image[pix] = make_float4(cur.x, cur.y, cur.z, count);
    a.moments[pix] = make_float4(m1, m2, 0.0f, count);
  }
}

__device__ __forceinline__ bool finite_rgb(const float4& c) {
  const uint32_t m = 0x7F800000u;
  return (fbits(c.x) & m) != m && (fbits(c.y) & m) != m && (fbits(c.z) & m) != m;
}

// mrt_counted_merge: one load-load-store pass; the three branches that copy
// are bitwise moves
__global__ __launch_bounds__(kBlock) void counted_merge_kernel(MergeArgs a) {
  const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
  if (i >= a.count) return;
  const float4 A = a.a[i], B = a.b[i];
  const float ha = A.w, hb = B.w;
  float4 o;
  if (hb == 0.0f || !finite_rgb(B)) {
    o = A;
  } else if (ha == 0.0f || !finite_rgb(A)) {
    o = B;
  } else {
    const float t = ha + hb;
    o = make_float4(m_div(ha * A.x + hb * B.x, t), m_div(ha * A.y + hb * B.y, t), m_div(ha * A.z + hb * B.z, t), t);
  }
  a.out[i] = o;
}

// mrt_tile_priority: one block per tile, a wave per row of 64 pixels (16 rows
// each); the lanes' partial sums are reduced through the wave (DPP shuffles),
// the four waves' through LDS.  Rows and columns outside the image are skipped.
__global__ __launch_bounds__(kBlock) void tile_priority_kernel(PriorityArgs a) {
  __shared__ float s_part[kBlock / 64];
  const uint32_t t = blockIdx.x;
  const uint32_t ty = t / a.tiles_x, tx = t - ty * a.tiles_x;
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  const uint32_t x = tx * kTile + lane;
  float sum = 0.0f;
  if (x < a.width) {
    for (uint32_t r = wave; r < kTile; r += kBlock / 64) {
      const uint32_t y = ty * kTile + r;
      if (y >= a.height) break;
      const size_t i = (size_t)y * a.width + x;
      if (fbits(a.guide_n[i].w) >= 0x80000000u) continue;
      const float4 c = a.image[i];
      if (!finite_rgb(c)) continue;
      const float l = luminance(mk(c));
      sum += m_div(a.variance[i], l * l + a.eps2);
    }
  }
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) sum += __shfl_xor(sum, o);
  if (lane == 0) s_part[wave] = sum;
  __syncthreads();
  if (threadIdx.x == 0) a.priority[t] = (s_part[0] + s_part[1]) + (s_part[2] + s_part[3]);
}

// mrt_tile_select: rank by counting.  Tile t's rank is the number of tiles
// that beat it under (priority descending, tile index ascending); a priority
// that is not finite or is negative counts as 0.  Every block stages the whole
// priority array through LDS in chunks of one block, so any tile count up to
// kMaxSelectTiles is served by ceil(tiles / 256) blocks; ranks are a
// permutation, so list[r] has exactly one writer.
__device__ __forceinline__ float select_key(float p) {
  return ((fbits(p) & 0x7F800000u) != 0x7F800000u && p > 0.0f) ? p : 0.0f;
}
__global__ __launch_bounds__(kBlock) void tile_select_kernel(const float* priority, uint32_t tiles, uint32_t count,
                                                             uint32_t* list) {
  __shared__ float s_key[kBlock];
  const uint32_t t = blockIdx.x * kBlock + threadIdx.x;
  const float mine = t < tiles ? select_key(priority[t]) : 0.0f;
  uint32_t rank = 0;
  for (uint32_t base = 0; base < tiles; base += kBlock) {
    const uint32_t u = base + threadIdx.x;
    __syncthreads();
    s_key[threadIdx.x] = u < tiles ? select_key(priority[u]) : 0.0f;
    __syncthreads();
    const uint32_t n = min((uint32_t)kBlock, tiles - base);
    for (uint32_t k = 0; k < n; ++k) {
      const float other = s_key[k];   // the same address in every lane: an LDS broadcast
      rank += (other > mine || (other == mine && base + k < t)) ? 1u : 0u;
    }
  }
  if (t < tiles && rank < count) list[rank] = t;
}

}  // namespace
#endif  // MRT_EMIT_MAIN

}}  // namespace mrt::MRT_NS
