// kern_stage.h — frame accumulation, the stage kernels over the reference's AoS records, first-hit guides,
// the display blit and the owned-tile pack / unpack
#pragma once
#include "dev_filter.h"
#include "dev_shade.h"
#include "dev_sweep.h"

namespace mrt { namespace MRT_NS { namespace {

// accumulateImage (renderer/Shaders.metal:233-249) for a batch of frames over
// the owned tiles: image = f == 0 ? c : mix(c, image, f/(f+1)).  Frames are
// accumulated strictly in order (the running mean is order-dependent): one
// thread applies the batch's frames to its pixel in frame order.
// At most 32 VGPRs (four frames' loads in flight instead of eight): the
// render kernels hold 5 waves x 96 of a SIMD's 512 VGPRs (the path kernel;
// the stream kernel since r5 5 persistent blocks x 80), so a 32-VGPR
// accumulate wave fits beside them and batch b's accumulate (main stream)
// runs while batch b + 1 renders on the other stream instead of waiting for
// its drain (the 2-stream period was launch + ~0.33 ms on C2).  One call,
// alternating: C2 10755 / 10762 -> 11024 / 11033 Mpaths/s (+2.5 %), C2 L=5
// +2.0 %, C2 1/8 share 10340 -> 10733 (+3.7 %), C4 +0.5 %.
// MOMENTS (MRT_FLAG_MOMENTS): the luminance moments image gets the same
// recurrence over (l, l*l, 0), l = lum(c), from the same read of the radiance
// rows — two more running means in registers.  With two frames' loads in
// flight instead of four it stays within the 32 VGPRs without scratch (27;
// with four the compiler takes 38) (include/mrt.h "variance-guided denoising").
constexpr uint32_t kAccLoads = 4;
__device__ __forceinline__ float luminance(V3 c) { return (0.2126f * c.x + 0.7152f * c.y) + 0.0722f * c.z; }
// accumulate_value of (l, l*l) into the two running means
__device__ __forceinline__ void accumulate_moments(float& m1, float& m2, V3 c, uint32_t f) {
  const float l = luminance(c);
  const float l2 = l * l;
  if (f > 0) {
    const float factor = m_div(float(f), float(f + 1));
    m1 = mixf(l, m1, factor);
    m2 = mixf(l2, m2, factor);
  } else {
    m1 = l;
    m2 = l2;
  }
}
// the last accumulate of a draw (a.counters set): block 0 copies the draw's
// statistics words to the host's pinned copy and zeroes the counters
__device__ __forceinline__ void fold_draw_counters(const AccumArgs& a) {
  if (a.counters && blockIdx.x == 0) {   // the draw's render launches have completed (stream order)
    for (uint32_t i = threadIdx.x; i < a.copy_words; i += kBlock) a.host_counters[i] = a.counters[i];
    for (uint32_t i = threadIdx.x; i < a.span_words; i += kBlock)
      a.host_counters[a.span_word + i] = a.counters[a.span_word + i];
    __syncthreads();
    for (uint32_t i = threadIdx.x; i < a.zero_words; i += kBlock) a.counters[i] = 0u;
    __threadfence_system();
  }
}
template <bool MOMENTS>
__global__ __launch_bounds__(kBlock) __attribute__((amdgpu_num_vgpr(32))) void accumulate_frame_kernel(AccumArgs a) {
  fold_draw_counters(a);
  for (uint32_t idx = blockIdx.x * kBlock + threadIdx.x; idx < a.num_slots; idx += gridDim.x * kBlock) {
    uint32_t x, y;
    slot_pixel(idx, a.shard_rank, a.shard_count, a.tiles_x, x, y);
    if (x >= a.width || y >= a.height) continue;
    const uint32_t pix = y * a.width + x;
    // the running mean stays in registers across the batch's frames (one
    // image read and one write per pixel); radiance rows are read once,
    // eight frames' loads in flight at a time
    const float4* rad = a.radiance + idx;
    if (!a.accumulate) {   // ACCUMULATE_IMAGE false (Shaders.metal:241): the batch's last frame alone
      const float4 c = rad[(size_t)(a.batch - 1) * a.num_slots];
      a.image[pix] = make_float4(c.x, c.y, c.z, 1.0f);
      continue;
    }
    float4 cur = a.frame_index > 0 ? a.image[pix] : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    float m1 = 0.0f, m2 = 0.0f;
    if constexpr (MOMENTS) {
      if (a.frame_index > 0) {
        const float4 m = a.moments[pix];
        m1 = m.x;
        m2 = m.y;
      }
    }
    constexpr uint32_t kLoads = MOMENTS ? kAccLoads / 2 : kAccLoads;
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
        cur = accumulate_value(cur, mk(c[k]), a.frame_index + j + k);
        if constexpr (MOMENTS) accumulate_moments(m1, m2, mk(c[k]), a.frame_index + j + k);
      }
    }
    for (; j < a.batch; ++j) {
      const V3 c = mk(rad[(size_t)j * a.num_slots]);
      cur = accumulate_value(cur, c, a.frame_index + j);
      if constexpr (MOMENTS) accumulate_moments(m1, m2, c, a.frame_index + j);
    }
    a.image[pix] = cur;
    if constexpr (MOMENTS) a.moments[pix] = make_float4(m1, m2, 0.0f, 1.0f);
  }
}

// ---------------------------------------------------------------------------
// Stage kernels over the reference AoS records (B-2 ABI, parity replay)
// ---------------------------------------------------------------------------
// (the stage kernel takes the camera by value — no device block to keep alive;
// moved = 0: the reference's camera)
__global__ __launch_bounds__(kBlock) void raygen_kernel(uint32_t W, uint32_t H, const float4* noise, RefRay* rays,
                                                        CameraBlock cam, uint32_t moved) {
  const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
  if (i >= W * H) return;
  const uint32_t x = i % W, y = i / W;
  V3 o, d;
  camera_ray<true>(x, y, W, H, noise[(x % kNoiseDim) + (y % kNoiseDim) * kNoiseDim], noise, moved ? &cam : nullptr, o, d);
  RefRay& r = rays[i];
  r.origin[0] = o.x; r.origin[1] = o.y; r.origin[2] = o.z;
  r.direction[0] = d.x; r.direction[1] = d.y; r.direction[2] = d.z;
  r.maxDistance = __builtin_inff();
  r.params[0] = 1.0f; r.params[1] = 0.0f; r.params[2] = 0.0f; r.params[3] = 1.00029f;
  for (int k = 0; k < 3; ++k) { r.throughput[k] = 1.0f; r.radiance[k] = 0.0f; }
}

template <int STACK>
__global__ __launch_bounds__(kBlock) void intersect_kernel(DeviceScene sc, const uint8_t* rays, uint32_t stride,
                                                           uint32_t count, RefIntersection* out, uint32_t* spill) {
  const LdsCtx cx = stage_lds<kGlobal>(sc, 0, spill);
  for (uint32_t i = blockIdx.x * kBlock + threadIdx.x; i < count; i += gridDim.x * kBlock) {
    const float* r = reinterpret_cast<const float*>(rays + (size_t)i * stride);
    RefIntersection res{-1.0f, 0xFFFFFFFFu, {0.0f, 0.0f}};
    const float tmax = r[7];
    if (tmax >= 0.0f) {   // maxDistance < 0 disables the ray (Shaders.metal:124,173)
      const V3 o = mk(r[0], r[1], r[2]), d = mk(r[4], r[5], r[6]);
      const Hit h = trace_nearest<STACK, kGlobal>(sc, cx, o, d, r[3], tmax);
      if (h.found) {
        res.distance = h.t;
        res.triangleIndex = h.prim;
        res.coordinates[0] = h.u;
        res.coordinates[1] = h.v;
      }
    }
    out[i] = res;
  }
}

// First-hit guide buffers of the denoiser (denoise.hip), one pixel per lane
// over the whole frame (index y * W + x, row 0 at the bottom, whatever the
// sharding).  The guide ray is the pixel's camera ray at the pixel centre
// (jitter sample (0.5, 0.5): both jitter terms are exactly 0) through a
// pinhole (the host passes the camera block with lens_radius = 0), traced with
// tmin 0 and no tmax.  gn[p] = (hn, bits(word)), gp[p] = (hv, t), with hv, hn
// and the material index as shade_hit computes them; word = the material
// index, bit 31 set on a light triangle; a miss writes (0, 0, 0, ~0u) and
// (0, 0, 0, -1).  A pixel is filterable iff word < kNotFilterable (dev_filter.h).
// (The ray, the trace, the miss record and this kernel's interpolation stand
// in both guide kernels: guide_point here, or one function for any of the
// rest, changes the kernels' code — DESIGN §2.1w.)
// the word of a hit from its primitive's first two shading records, as a float's bits
__device__ __forceinline__ float guide_word(float4 r0, float4 r1) {
  return bitsf(fbits(r0.w) | (fbits(r1.w) != 0xFFFFFFFFu ? kNotFilterable : 0u));
}
template <int STACK>
__global__ __launch_bounds__(kBlock) void guide_kernel(DeviceScene sc, uint32_t W, uint32_t H, CameraBlock cam,
                                                       uint32_t moved, float4* gn, float4* gp, uint32_t* spill) {
  const LdsCtx cx = stage_lds<kGlobal>(sc, 0, spill);
  const uint32_t count = W * H;
  for (uint32_t i = blockIdx.x * kBlock + threadIdx.x; i < count; i += gridDim.x * kBlock) {
    const uint32_t x = i % W, y = i / W;
    V3 o, d;
    camera_ray<true>(x, y, W, H, make_float4(0.5f, 0.5f, 0.5f, 0.5f), nullptr, moved ? &cam : nullptr, o, d);
    const Hit h = trace_nearest<STACK, kGlobal>(sc, cx, o, d, 0.0f, __builtin_inff());
    float4 n = make_float4(0.0f, 0.0f, 0.0f, bitsf(kMissWord)), p = make_float4(0.0f, 0.0f, 0.0f, -1.0f);
    if (h.found) {
      const float wu = h.u, wv = h.v, ww = (1.0f - h.u) - h.v;   // shade_hit's interpolation
      const float4 P0 = fetch_prim<kGlobal>(sc, cx, h.prim, 0), P1 = fetch_prim<kGlobal>(sc, cx, h.prim, 1);
      const float4 P2 = fetch_prim<kGlobal>(sc, cx, h.prim, 2);
      const float4 N0 = fetch_prim<kGlobal>(sc, cx, h.prim, 3), N1 = fetch_prim<kGlobal>(sc, cx, h.prim, 4);
      const float4 N2 = fetch_prim<kGlobal>(sc, cx, h.prim, 5);
      const V3 hv = add(add(mul(mk(P0), wu), mul(mk(P1), wv)), mul(mk(P2), ww));
      const V3 hn = normalize(add(add(mul(mk(N0), wu), mul(mk(N1), wv)), mul(mk(N2), ww)));
      n = make_float4(hn.x, hn.y, hn.z, guide_word(P0, P1));
      p = make_float4(hv.x, hv.y, hv.z, h.t);
    }
    gn[i] = n;
    gp[i] = p;
  }
}

// guide_kernel's interpolation of one scene's six shading records at (wu, wv, ww)
__device__ __forceinline__ void guide_point(const float4 (&R)[6], float wu, float wv, float ww, V3& hv, V3& hn) {
  hv = add(add(mul(mk(R[0]), wu), mul(mk(R[1]), wv)), mul(mk(R[2]), ww));
  hn = normalize(add(add(mul(mk(R[3]), wu), mul(mk(R[4]), wv)), mul(mk(R[5]), ww)));
}

// guide_kernel across a scene change (mrt_guides_motion): gn / gp exactly as
// guide_kernel writes them for `sc`, and in mn / mp the same surface point —
// primitive h.prim at the hit's barycentrics — as it lies in the previous scene,
// interpolated from `prev_prims` (that scene's shading records, 6 float4 per
// primitive, the same primitive order and count: the host checks it) with the
// same expressions: mp[p] = (previous position, t), mn[p] = (previous shading
// normal, bits(word)), word and t the current hit's.  A miss writes the miss
// record to all four planes.  The previous records are addressed only behind
// the trace (their base is a kernel argument, held in SGPRs): the traversal
// loop carries nothing for them, and the twelve loads of a hit go out together.
template <int STACK>
__global__ __launch_bounds__(kBlock) void guide_motion_kernel(DeviceScene sc, const float4* __restrict__ prev_prims,
                                                              uint32_t W, uint32_t H, CameraBlock cam, uint32_t moved,
                                                              float4* gn, float4* gp, float4* mn, float4* mp,
                                                              uint32_t* spill) {
  const LdsCtx cx = stage_lds<kGlobal>(sc, 0, spill);
  const uint32_t count = W * H;
  for (uint32_t i = blockIdx.x * kBlock + threadIdx.x; i < count; i += gridDim.x * kBlock) {
    const uint32_t x = i % W, y = i / W;
    V3 o, d;
    camera_ray<true>(x, y, W, H, make_float4(0.5f, 0.5f, 0.5f, 0.5f), nullptr, moved ? &cam : nullptr, o, d);
    const Hit h = trace_nearest<STACK, kGlobal>(sc, cx, o, d, 0.0f, __builtin_inff());
    float4 n = make_float4(0.0f, 0.0f, 0.0f, bitsf(kMissWord)), p = make_float4(0.0f, 0.0f, 0.0f, -1.0f);
    float4 qn = n, qp = p;
    if (h.found && h.prim < sc.num_triangles) {   // (always: the bound keeps a bad record inside both buffers)
      const float wu = h.u, wv = h.v, ww = (1.0f - h.u) - h.v;   // shade_hit's interpolation
      float4 C[6], Q[6];
#pragma unroll
      for (uint32_t k = 0; k < 6; ++k) C[k] = fetch_prim<kGlobal>(sc, cx, h.prim, k);
#pragma unroll
      for (uint32_t k = 0; k < 6; ++k) Q[k] = prev_prims[6 * (size_t)h.prim + k];
      const float w = guide_word(C[0], C[1]);
      V3 hv, hn;
      guide_point(C, wu, wv, ww, hv, hn);
      n = make_float4(hn.x, hn.y, hn.z, w);
      p = make_float4(hv.x, hv.y, hv.z, h.t);
      guide_point(Q, wu, wv, ww, hv, hn);
      qn = make_float4(hn.x, hn.y, hn.z, w);
      qp = make_float4(hv.x, hv.y, hv.z, h.t);
    }
    gn[i] = n;
    gp[i] = p;
    mn[i] = qn;
    mp[i] = qp;
  }
}

__global__ __launch_bounds__(kBlock) void shade_kernel(DeviceScene sc, uint32_t W, uint32_t H, uint32_t f,
                                                       uint32_t L, const float4* noise,
                                                       const RefIntersection* isect, RefRay* rays,
                                                       RefShadowRay* srays, uint32_t flags) {
  const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
  if (i >= W * H) return;
  const uint32_t x = i % W, y = i / W;
  RefShadowRay& sr = srays[i];
  RefRay& r = rays[i];
  sr.maxDistance = -1.0f;                                   // Shaders.metal:119
  const RefIntersection is = isect[i];
  if (is.distance < kDistanceEpsilon) { r.maxDistance = -1.0f; return; }   // :122-126
  PathState s;
  s.o = mk(r.origin[0], r.origin[1], r.origin[2]);
  s.d = mk(r.direction[0], r.direction[1], r.direction[2]);
  s.T = mk(r.throughput[0], r.throughput[1], r.throughput[2]);
  s.R = mk(r.radiance[0], r.radiance[1], r.radiance[2]);
  s.pdf = r.params[0];
  s.prevDiffuse = r.params[1];
  s.ior = r.params[3];
  const uint32_t bounce = (uint32_t)r.params[2];
  Hit h;
  h.t = is.distance; h.prim = is.triangleIndex; h.u = is.coordinates[0]; h.v = is.coordinates[1]; h.found = true;
  ShadowRay sh;
  const LdsCtx cx = stage_lds<kGlobal>(sc, 0);
  shade_hit<kGlobal, false>(sc, cx, h, s, noise[shade_noise_cell(x, y, bounce, f)], bounce, L, true, sh,
                     (flags & kShadeDebugMaterial) != 0);
  if (bounce + 1 < L) {
    sr.origin[0] = sh.o.x; sr.origin[1] = sh.o.y; sr.origin[2] = sh.o.z;
    sr.direction[0] = sh.d.x; sr.direction[1] = sh.d.y; sr.direction[2] = sh.d.z;
    sr.maxDistance = sh.valid ? __builtin_inff() : -1.0f;
    sr.targetIndex = sh.target;
    sr.throughput[0] = sh.L.x; sr.throughput[1] = sh.L.y; sr.throughput[2] = sh.L.z;
  }
  r.radiance[0] = s.R.x; r.radiance[1] = s.R.y; r.radiance[2] = s.R.z;
  r.direction[0] = s.d.x; r.direction[1] = s.d.y; r.direction[2] = s.d.z;
  r.origin[0] = s.o.x; r.origin[1] = s.o.y; r.origin[2] = s.o.z;
  r.maxDistance = __builtin_inff();
  r.params[0] = s.pdf; r.params[1] = s.prevDiffuse; r.params[2] = float(bounce + 1); r.params[3] = s.ior;
  r.throughput[0] = s.T.x; r.throughput[1] = s.T.y; r.throughput[2] = s.T.z;
}

// lightSamplingHandler — Shaders.metal:214-231
__global__ __launch_bounds__(kBlock) void resolve_kernel(uint32_t count, const RefIntersection* isect, RefRay* rays,
                                                         const RefShadowRay* srays) {
  const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
  if (i >= count) return;
  const RefIntersection is = isect[i];
  if (is.distance >= kDistanceEpsilon && is.triangleIndex == srays[i].targetIndex)
    for (int k = 0; k < 3; ++k) rays[i].radiance[k] += srays[i].throughput[k];
}

__global__ __launch_bounds__(kBlock) void accumulate_kernel(uint32_t W, uint32_t H, uint32_t f, const RefRay* rays,
                                                            float4* image, bool accumulate) {
  const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
  if (i >= W * H) return;
  accumulate_pixel(image, i, mk(rays[i].radiance[0], rays[i].radiance[1], rays[i].radiance[2]), accumulate ? f : 0u);
}

// mrt_moments: accumulate_kernel over (l, l*l, 0), l = lum(radiance)
__global__ __launch_bounds__(kBlock) void moments_kernel(uint32_t W, uint32_t H, uint32_t f, const RefRay* rays,
                                                         float4* moments) {
  const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
  if (i >= W * H) return;
  const float l = luminance(mk(rays[i].radiance[0], rays[i].radiance[1], rays[i].radiance[2]));
  accumulate_pixel(moments, i, mk(l, l * l, 0.0f), f);
}

}  // namespace

#if MRT_EMIT_MAIN   // (not in the stream unit)
// blitFragment — renderer/Shaders.metal:33-70 with the compile-time switches
// of Raytracing.h:11-12,25-31 as runtime flags (include/mrt.h MRT_DISPLAY_*):
// tone map 1 - exp(-c) (ENABLE_TONE_MAPPING), toSRGB on rgb (MANUAL_SRGB,
// Raytracing.h:130-135), then the COMPARISON_MODE against a reference image
// scaled by COMPARISON_SCALE.  One output pixel per image pixel (the
// reference samples the W x H texture with a nearest filter).
__device__ __forceinline__ float to_srgb(float v) {   // Raytracing.h:130-135
  if (v <= 0.0f) return 0.0f;
  if (v >= 1.0f) return 1.0f;
#if MRT_PRECISE
  return (v < 0.0031308f) ? (12.92f * v) : (1.055f * powf(v, 1.0f / 2.4f) - 0.055f);
#else
  return (v < 0.0031308f) ? (12.92f * v) : (1.055f * __powf(v, 1.0f / 2.4f) - 0.055f);
#endif
}
__device__ __forceinline__ float4 display_map(float4 c, uint32_t flags) {
  if (flags & 1u) {   // tone mapping (applies to all four channels, as color = 1 - exp(-color))
#if MRT_PRECISE
    c = make_float4(1.0f - expf(-c.x), 1.0f - expf(-c.y), 1.0f - expf(-c.z), 1.0f - expf(-c.w));
#else
    c = make_float4(1.0f - __expf(-c.x), 1.0f - __expf(-c.y), 1.0f - __expf(-c.z), 1.0f - __expf(-c.w));
#endif
  }
  if (flags & 2u) c = make_float4(to_srgb(c.x), to_srgb(c.y), to_srgb(c.z), c.w);
  return c;
}
__global__ __launch_bounds__(kBlock) void display_kernel(const float4* image, const float4* reference, float4* out,
                                                         uint32_t n, uint32_t flags, float scale) {
  const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
  if (i >= n) return;
  const float4 c = display_map(image[i], flags);
  const uint32_t mode = (flags >> 8) & 0xFFu;
  if (mode == 0u || !reference) { out[i] = c; return; }
  const float4 r = display_map(reference[i], flags);   // the reference texture goes through the same blit
  float4 o;
  if (mode == 1u) {          // COMPARE_ABSOLUTE_VALUE
    o = make_float4(fabsf(c.x - r.x), fabsf(c.y - r.y), fabsf(c.z - r.z), fabsf(c.w - r.w));
  } else if (mode == 2u) {   // COMPARE_REF_TO_COLOR
    o = make_float4(fmaxf(0.0f, r.x - c.x), fmaxf(0.0f, r.y - c.y), fmaxf(0.0f, r.z - c.z), fmaxf(0.0f, r.w - c.w));
  } else if (mode == 3u) {   // COMPARE_COLOR_TO_REF
    o = make_float4(fmaxf(0.0f, c.x - r.x), fmaxf(0.0f, c.y - r.y), fmaxf(0.0f, c.z - r.z), fmaxf(0.0f, c.w - r.w));
  } else {                   // COMPARE_LUMINANCE: red = output brighter, green = reference brighter
    const float lc = (c.x * (1.0f / 3.0f) + c.y * (1.0f / 3.0f)) + c.z * (1.0f / 3.0f);
    const float lr = (r.x * (1.0f / 3.0f) + r.y * (1.0f / 3.0f)) + r.z * (1.0f / 3.0f);
    o = make_float4(fmaxf(0.0f, lc - lr), fmaxf(0.0f, lr - lc), 0.0f, 1.0f);
  }
  out[i] = make_float4(o.x * scale, o.y * scale, o.z * scale, o.w * scale);
}

// owned-tile pack/unpack for the multi-GPU exchange (renderer.cpp
// mrt_tiles_pack / mrt_tiles_unpack): packed index = k * 4096 + ty * 64 + tx
// for the k-th owned tile (global tile rank + k * count, row-major tiles)
__global__ __launch_bounds__(kBlock) void tiles_move_kernel(const float4* src, float4* dst, uint32_t W, uint32_t H,
                                                            uint32_t rank, uint32_t count, uint32_t tiles_x,
                                                            uint32_t owned, bool pack) {
  const uint64_t n = (uint64_t)owned * kTile * kTile;
  for (uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += (uint64_t)gridDim.x * kBlock) {
    const uint32_t k = (uint32_t)(i >> 12), p = (uint32_t)(i & 4095u);
    const uint32_t t = rank + k * count;
    const uint32_t ty = t / tiles_x, tx = t - ty * tiles_x;
    const uint32_t x = tx * kTile + (p & 63u), y = ty * kTile + (p >> 6);
    const bool in = x < W && y < H;
    if (pack) dst[i] = in ? src[(size_t)y * W + x] : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    else if (in) dst[(size_t)y * W + x] = src[i];
  }
}
#endif  // MRT_EMIT_MAIN

}}  // namespace mrt::MRT_NS
