// kern_adaptive.h — adaptive sampling (include/mrt.h "adaptive sampling",
// DESIGN.md §2.1q): the counted accumulate of a refine draw, the merge of two
// counted images, the per-tile priority from the variance plane, the
// selection of the highest-priority tiles, and the error estimate of a stop
// rule (§2.1r): the per-tile mean relative error and the tiles above a threshold.  The render kernels read the tile
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

// a / b correctly rounded in both builds (the fast build's own division is not):
// the double quotient of two floats rounds to the float quotient (53 >= 2 * 24 + 2)
__device__ __forceinline__ float ieee_div(float a, float b) { return (float)((double)a / (double)b); }

// mrt_tile_priority and mrt_tile_error: one block per tile, a wave per row of
// 64 pixels (16 rows each); the lanes' partial sums are reduced through the
// wave (DPP shuffles), the four waves' through LDS.  Rows and columns outside
// the image are skipped.
// MRT_TILE_LANE_TERMS is the part the two kernels share: a lane's walk down its
// column of tile blockIdx.x, with ADD executed on the `term` of every pixel that
// counts.  A macro and not a function: behind a function boundary, however
// inlined, the compiler splits the pixel's rgb load in two and allocates
// registers anew, and tile_priority_kernel's code is to stay what it was, to the
// instruction.
#define MRT_TILE_LANE_TERMS(a, ADD)                                     \
  const uint32_t t = blockIdx.x;                                        \
  const uint32_t ty = t / a.tiles_x, tx = t - ty * a.tiles_x;           \
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;     \
  const uint32_t x = tx * kTile + lane;                                 \
  if (x < a.width) {                                                    \
    for (uint32_t r = wave; r < kTile; r += kBlock / 64) {              \
      const uint32_t y = ty * kTile + r;                                \
      if (y >= a.height) break;                                         \
      const size_t i = (size_t)y * a.width + x;                         \
      if (fbits(a.guide_n[i].w) >= kNotFilterable) continue;            \
      const float4 c = a.image[i];                                      \
      if (!finite_rgb(c)) continue;                                     \
      const float l = luminance(mk(c));                                 \
      const float term = m_div(a.variance[i], l * l + a.eps2);          \
      ADD;                                                              \
    }                                                                   \
  }

__global__ __launch_bounds__(kBlock) void tile_priority_kernel(PriorityArgs a) {
  __shared__ float s_part[kBlock / 64];
  float sum = 0.0f;
  MRT_TILE_LANE_TERMS(a, sum += term)
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) sum += __shfl_xor(sum, o);
  if (lane == 0) s_part[wave] = sum;
  __syncthreads();
  if (threadIdx.x == 0) a.priority[t] = (s_part[0] + s_part[1]) + (s_part[2] + s_part[3]);
}

// mrt_tile_error: the same terms, counted, and summed in double (the order is
// free, so no order is left to matter: up to 4096 float terms add up exactly
// enough that the mean, args.p.priority[t], is the float nearest to that of the
// terms; the double adds of a lane hide behind its loads)
__global__ __launch_bounds__(kBlock) void tile_error_kernel(ErrorArgs args) {
  __shared__ double s_part[kBlock / 64];
  __shared__ uint32_t s_count[kBlock / 64];
  const PriorityArgs& a = args.p;
  double sum = 0.0;
  uint32_t counted = 0;
  MRT_TILE_LANE_TERMS(a, (sum += (double)term, counted += 1u))
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) {
    sum += __shfl_xor(sum, o);
    counted += __shfl_xor(counted, o);
  }
  if (lane == 0) {
    s_part[wave] = sum;
    s_count[wave] = counted;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    const double total = (s_part[0] + s_part[1]) + (s_part[2] + s_part[3]);
    const uint32_t n = (s_count[0] + s_count[1]) + (s_count[2] + s_count[3]);
    a.priority[t] = n ? (float)(total / (double)n) : 0.0f;
    args.pixels[t] = n;
  }
}
#undef MRT_TILE_LANE_TERMS

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

// mrt_tile_threshold: tile_select_kernel's ranking over key(t) = the mean error
// of a tile with counted pixels, where only a tile above the threshold is
// listed: every such tile outranks every other, so the above tiles hold the
// ranks 0 .. A-1 and list[r] still has one writer.  Block 0, which stages every
// tile like the others, also sums the summary from what it stages (a thread
// the tiles u = threadIdx.x mod 256, then wave and LDS as above) and writes it
// from thread 0 with ordinary stores.
__device__ __forceinline__ float threshold_key(float e, uint32_t pixels) { return pixels ? select_key(e) : 0.0f; }
__global__ __launch_bounds__(kBlock) void tile_threshold_kernel(ThresholdArgs a) {
  __shared__ float s_key[kBlock];
  __shared__ float s_f[2][kBlock / 64];
  __shared__ uint32_t s_u[3][kBlock / 64];
  const uint32_t t = blockIdx.x * kBlock + threadIdx.x;
  const float mine = t < a.tiles ? threshold_key(a.mean_error[t], a.pixels[t]) : 0.0f;
  const bool first = blockIdx.x == 0;
  uint32_t rank = 0;
  float weighted = 0.0f, worst = 0.0f;
  uint32_t above = 0, counted = 0, pixels = 0;
  for (uint32_t base = 0; base < a.tiles; base += kBlock) {
    const uint32_t u = base + threadIdx.x;
    const uint32_t n_u = u < a.tiles ? a.pixels[u] : 0u;
    const float k_u = u < a.tiles ? threshold_key(a.mean_error[u], n_u) : 0.0f;
    __syncthreads();
    s_key[threadIdx.x] = k_u;
    __syncthreads();
    if (first) {
      weighted += (float)((double)k_u * (double)n_u);   // the rounded product, never contracted into the sum
      worst = fmaxf(worst, k_u);
      above += k_u > a.threshold ? 1u : 0u;
      counted += n_u ? 1u : 0u;
      pixels += n_u;
    }
    const uint32_t n = min((uint32_t)kBlock, a.tiles - base);
    for (uint32_t k = 0; k < n; ++k) {
      const float other = s_key[k];   // an LDS broadcast
      rank += (other > mine || (other == mine && base + k < t)) ? 1u : 0u;
    }
  }
  if (t < a.tiles && mine > a.threshold && rank < a.max_count) a.list[rank] = t;
  if (!first) return;   // (the whole block)
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) {
    weighted += __shfl_xor(weighted, o);
    worst = fmaxf(worst, __shfl_xor(worst, o));
    above += __shfl_xor(above, o);
    counted += __shfl_xor(counted, o);
    pixels += __shfl_xor(pixels, o);
  }
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  if (lane == 0) {
    s_f[0][wave] = weighted;
    s_f[1][wave] = worst;
    s_u[0][wave] = above;
    s_u[1][wave] = counted;
    s_u[2][wave] = pixels;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    const float w = (s_f[0][0] + s_f[0][1]) + (s_f[0][2] + s_f[0][3]);
    const uint32_t A = (s_u[0][0] + s_u[0][1]) + (s_u[0][2] + s_u[0][3]);
    const uint32_t px = (s_u[2][0] + s_u[2][1]) + (s_u[2][2] + s_u[2][3]);
    ErrorSummary o;
    o.frame_error = px ? ieee_div(w, float(px)) : 0.0f;
    o.max_tile_error = fmaxf(fmaxf(s_f[1][0], s_f[1][1]), fmaxf(s_f[1][2], s_f[1][3]));
    o.tiles_above = A;
    o.tiles_listed = min(A, a.max_count);
    o.tiles_counted = (s_u[1][0] + s_u[1][1]) + (s_u[1][2] + s_u[1][3]);
    o.pixels = px;
    o.reserved[0] = o.reserved[1] = 0u;
    *a.summary = o;
  }
}

}  // namespace
#endif  // MRT_EMIT_MAIN

}}  // namespace mrt::MRT_NS
