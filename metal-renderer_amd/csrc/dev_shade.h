// dev_shade.h — materials, sampling, the camera ray, slot / pixel maps, intersectionHandler's shading, accumulation
#pragma once
#include "dev_lds.h"
#include "kernels.h"

namespace mrt { namespace MRT_NS { namespace {

// ---------------------------------------------------------------------------
// Shading helpers — renderer/KernelHelpers.h, renderer/Raytracing.h
// ---------------------------------------------------------------------------
// fresnel — KernelHelpers.h:7-21
__device__ __forceinline__ float fresnel(V3 n, V3 i, float etaOut, float etaIn) {
  float result = 1.0f;
  const float etaScale = m_div(etaOut, etaIn);
  const float cosThetaI = fminf(fmaxf(dot(n, i), -1.0f), 1.0f);
  const float sinThetaTSquared = (etaScale * etaScale) * (1.0f - cosThetaI * cosThetaI);
  if (sinThetaTSquared < 1.0f) {
    const float cosThetaT = m_sqrt(1.0f - sinThetaTSquared);
    const float rS = m_div(etaIn * cosThetaI - etaOut * cosThetaT, etaIn * cosThetaI + etaOut * cosThetaT);
    const float rP = m_div(etaIn * cosThetaT - etaOut * cosThetaI, etaIn * cosThetaT + etaOut * cosThetaI);
    result = 0.5f * (rS * rS + rP * rP);
  }
  return result;
}
// triangleSamplePDF — Raytracing.h:168-171
__device__ __forceinline__ float triangleSamplePDF(float area, float cosTheta, float dist) {
  return m_div(dist * dist, area * cosTheta);
}
// balanceHeuristic (power heuristic) — Raytracing.h:173-178
__device__ __forceinline__ float balanceHeuristic(float f, float g) {
  const float f2 = f * f, g2 = g * g;
  return m_div(f2, f2 + g2);
}
// buildOrthonormalBasis — Raytracing.h:189-205
__device__ __forceinline__ void buildOrthonormalBasis(V3 n, V3& u, V3& v) {
  if (n.z < 0.0f) {
    const float a = m_rcp(1.0f - n.z);
    const float b = n.x * n.y * a;
    u = mk(1.0f - n.x * n.x * a, -b, n.x);
    v = mk(b, n.y * n.y * a - 1.0f, -n.y);
  } else {
    const float a = m_rcp(1.0f + n.z);
    const float b = -n.x * n.y * a;
    u = mk(1.0f - n.x * n.x * a, b, -n.x);
    v = mk(b, 1.0f - n.y * n.y * a, -n.y);
  }
}
// generateDiffuseBounce + alignWithNormal — Raytracing.h:207-223 (smp = noise.zw)
__device__ __forceinline__ V3 diffuseBounce(float sx, float sy, V3 n) {
  const float cosTheta = m_sqrt(sy);
  const float phi = sx * kPi * 2.0f;
  const float sinTheta = m_sqrt(1.0f - cosTheta * cosTheta);
  V3 u, v;
  buildOrthonormalBasis(n, u, v);
  const float cp = m_cos(phi), sp = m_sin(phi);
  return add(mul(add(mul(u, cp), mul(v, sp)), sinTheta), mul(n, cosTheta));
}
__device__ __forceinline__ bool isMirrorDir(V3 wI, V3 n, V3 wO) {
  return fabsf(dot(reflect(wI, n), wO) - 1.0f) < kAngleEpsilon;
}

struct Mat {
  V3 kd, le;
  float ior;
  uint32_t type;
};
template <int MODE>
__device__ __forceinline__ Mat load_material(const DeviceScene& sc, const LdsCtx& cx, uint32_t m) {
  const float4 a = fetch_mat<MODE>(sc, cx, m, 0), b = fetch_mat<MODE>(sc, cx, m, 1);
  return {mk(a), mk(b), a.w, fbits(b.w)};
}

// sampleMaterial — KernelHelpers.h:56-114
__device__ __forceinline__ void sampleMaterial(const Mat& m, V3 wI, V3 wO, V3 n, const float4& ns, float& bsdf,
                                               float& pdf) {
  const float cosTheta = dot(wO, n);
  constexpr float invPi = 1.0f / kPi;
  bool diffuse_lobe = (m.type == kDiffuse);
  bool zero_lobe = false;
  if (m.type == kPlastic || m.type == kDielectric) {
    const float fI = fresnel(n, neg(wI), 1.0f, m.ior);
    if (fI < ns.y) {
      diffuse_lobe = (m.type == kPlastic);
      zero_lobe = (m.type == kDielectric);
    }
  }
  if (zero_lobe) {
    bsdf = pdf = 0.0f;
  } else if (diffuse_lobe) {
    bsdf = pdf = invPi * cosTheta;
  } else {   // mirror lobe
    bsdf = isMirrorDir(wI, n, wO) ? cosTheta : 0.0f;
    pdf = 1.0f;
  }
}

// generateNextBounce — KernelHelpers.h:116-179
__device__ __forceinline__ V3 generateNextBounce(const Mat& m, V3 wI, float currentIoR, V3 n, const float4& ns,
                                                 float& bsdf, float& pdf, float& ior) {
  constexpr float invPi = 1.0f / kPi;
  ior = currentIoR;
  int lobe = 0;   // 0 diffuse, 1 mirror, 2 pass-through
  if (m.type == kMirror) {
    lobe = 1;
  } else if (m.type == kPlastic || m.type == kDielectric) {
    const float fI = fresnel(n, neg(wI), currentIoR, m.ior);
    lobe = (fI < ns.y) ? (m.type == kPlastic ? 0 : 2) : 1;
  }
  V3 wO;
  if (lobe == 0) {
    wO = diffuseBounce(ns.z, ns.w, n);
    bsdf = pdf = invPi * dot(wO, n);
  } else if (lobe == 1) {
    wO = reflect(wI, n);
    bsdf = dot(wO, n);
    pdf = 1.0f;
  } else {
    ior = m.ior;
    wO = wI;
    bsdf = pdf = 1.0f;
  }
  return wO;
}

// lightTriangleSamplePDF — KernelHelpers.h:181-190
__device__ __forceinline__ float lightTriangleSamplePDF(float tpdf, float area, V3 source, V3 sv, V3 sn,
                                                        V3& dirOut, float& LdotD) {
  const V3 d = sub(sv, source);
  const float dist = length(d);
  dirOut = normalize(d);
  LdotD = -dot(dirOut, sn);
  const float valid = float(dist >= kDistanceEpsilon) * float(LdotD >= kAngleEpsilon);
  return valid * tpdf * triangleSamplePDF(area, LdotD, dist);
}

// selectLightTriangle — KernelHelpers.h:49-54.  The linear scan returns the
// first index with !(cdf[index+1] <= xi) (or count); cdf is non-decreasing, so
// a binary search returns the same index.
template <int MODE>
__device__ __forceinline__ uint32_t selectLightTriangle(const DeviceScene& sc, const LdsCtx& cx, uint32_t count,
                                                        float xi) {
  uint32_t lo = 0, hi = count;
  while (lo < hi) {
    const uint32_t mid = (lo + hi) >> 1;
    if (fetch_light<MODE>(sc, cx, mid + 1, 2).w <= xi) lo = mid + 1;   // entry mid+1: (v1.n, cdf)
    else hi = mid;
  }
  return lo;
}

// ---------------------------------------------------------------------------
// Path state + the per-hit shading of intersectionHandler
// ---------------------------------------------------------------------------
struct PathState {
  V3 o, d, T, R;
  float pdf;          // Ray.params.x
  float ior;          // Ray.params.w
  float prevDiffuse;  // Ray.params.y (0 or 1)
  uint32_t mtype;     // material type of the surface the next ray leaves (set with the next ray)
};
struct ShadowRay {
  V3 o, d, L;
  uint32_t target;
  bool valid;
  bool graze;   // cosine to the light below the occluder tree's guard (shadow_root)
};

// rayGenerator — renderer/Shaders.metal:75-103 (camera fixed at t = 0),
// generalised to a movable camera (kernels.h CameraBlock; DESIGN.md "Camera").
// cam == nullptr (wave-uniform: a kernel argument) is the reference's camera
// and keeps its expression, so its bits do not depend on x * 1 + y * 0
// identities.  Otherwise, with (u, v) as in the reference and s = tan(half fov):
//   pinhole:   c = (u s, v s, -1), w = normalize(c), o = origin
//   thin lens: (xi1, xi2) = (z, w) of the frame's raygen table at cell
//              ((x + 32) % 64, (y + 32) % 64) — not the cell of the pixel's
//              own jitter and bounce-0 shading sample (shade_noise_cell) —
//              l = lens sqrt(xi1) (cos 2 pi xi2, sin 2 pi xi2),
//              w = normalize(c focus - (l, 0)), o = origin + right l.x + up l.y
//   d = (right w.x + up w.y) + forward (-w.z)
// The block is read with scalar loads (uniform address) inside this function only.
// CAM: the kernel instantiation for a moved camera.  The persistent kernels
// are compiled twice — with CAM = false camera_ray is the reference's
// expression alone, so the default camera's kernels are the code they were
// before the camera could move (compiled in one kernel, the moved branch cost
// the default camera 26 % on C2, measured: DESIGN.md 2.1f "Two instantiations").
template <bool CAM>
__device__ __forceinline__ void camera_ray(uint32_t x, uint32_t y, uint32_t W, uint32_t H, const float4& ns,
                                           const float4* table, const CameraBlock* __restrict__ cam, V3& o, V3& d) {
  const float aspect = m_div(float(H), float(W));
  const float wm1 = float(W - 1), hm1 = float(H - 1);
  const float dudvx = m_div(ns.x * 2.0f - 1.0f, wm1);
  const float dudvy = m_div(ns.y * 2.0f - 1.0f, hm1);
  const float ncx = m_div(float(2 * x), wm1) - 1.0f;
  const float ncy = m_div(float(2 * y), hm1) - 1.0f;
  if (!CAM || cam == nullptr) {
    d = normalize(mk(dudvx + ncx, dudvy + ncy * aspect, -1.0f));
    o = mk(kCameraX, kCameraY, kCameraZ);   // up - view * 2.35
    return;
  }
  // The block's address goes through an opaque move, so its (loop-invariant)
  // loads stay here instead of being hoisted out of the persistent kernels'
  // loops, where 15 more live SGPRs would spill.
  asm volatile("" : "+s"(cam));
  const float s = cam->tan_half_fov;
  const V3 right = mk(cam->right[0], cam->right[1], cam->right[2]), up = mk(cam->up[0], cam->up[1], cam->up[2]);
  const V3 fwd = mk(cam->forward[0], cam->forward[1], cam->forward[2]);
  const V3 c = mk((dudvx + ncx) * s, (dudvy + ncy * aspect) * s, -1.0f);
  o = mk(cam->origin[0], cam->origin[1], cam->origin[2]);
  V3 w;
  if (cam->lens_radius > 0.0f) {
    const float4 ls = table[((x + kNoiseDim / 2) % kNoiseDim) + ((y + kNoiseDim / 2) % kNoiseDim) * kNoiseDim];
    const float rad = cam->lens_radius * m_sqrt(ls.z), phi = ls.w * 6.28318530718f;
    const float lx = rad * m_cos(phi), ly = rad * m_sin(phi);
    const V3 p = mul(c, cam->focus_distance);
    w = normalize(mk(p.x - lx, p.y - ly, p.z));
    o = add(add(o, mul(right, lx)), mul(up, ly));
  } else {
    w = normalize(c);
  }
  d = add(add(mul(right, w.x), mul(up, w.y)), mul(fwd, -w.z));
}

// Owned slots: slot s of a frame = owned tile k = s >> 12 (global tile
// rank + k * count) and pixel p = s & 4095 inside it in 8x8-block order (a
// wave's 64 lanes cover one 8x8 block).  A ray's tag is its global slot
// g = frame_in_batch * num_slots + s — at bounce 0 simply the launch index.
__device__ __forceinline__ void slot_pixel(uint32_t s, uint32_t rank, uint32_t count, uint32_t tiles_x, uint32_t& x,
                                           uint32_t& y) {
  const uint32_t k = s >> 12, p = s & 4095u;
  const uint32_t t = rank + k * count;
  const uint32_t ty = t / tiles_x, tx = t - ty * tiles_x;
  const uint32_t blk = p >> 6, q = p & 63u;
  x = tx * kTile + (blk & 7u) * 8u + (q & 7u);
  y = ty * kTile + (blk >> 3) * 8u + (q >> 3);
}

// n / d for n < 2^31 through the launch's magic (kernels.h MagicDiv; draw_n
// checks every multiplier against its divisor d)
__device__ __forceinline__ uint32_t mdiv(uint32_t n, MagicDiv m, uint32_t d) {
  (void)d;
  return m.m ? (__umulhi(n, m.m) >> m.sh) : n;
}
// slot_pixel with the launch's magic for tiles_x
__device__ __forceinline__ void slot_pixel_a(uint32_t s, const BounceArgs& a, uint32_t& x, uint32_t& y) {
  const uint32_t k = s >> 12, p = s & 4095u;
  const uint32_t t = a.shard_rank + k * a.shard_count;
  const uint32_t ty = mdiv(t, a.div_tiles, a.tiles_x), tx = t - ty * a.tiles_x;
  const uint32_t blk = p >> 6, q = p & 63u;
  x = tx * kTile + (blk & 7u) * 8u + (q & 7u);
  y = ty * kTile + (blk >> 3) * 8u + (q >> 3);
}

// LIST: the kernel instantiation that renders the tiles of a.tile_list
// (adaptive sampling, include/mrt.h): owned tile k = s >> 12 is tile
// tile_list[k].  With LIST = false this is slot_pixel_a and the kernels are
// the code they were before a launch could carry a list (as CAM above).
// UNIFORM: the caller's lanes hold slots of one tile (a wave of camera rays:
// 64 consecutive slots from a multiple of 64), so the list entry is one scalar
// load; otherwise (a lane's own path, any tile) a load per lane of a list
// that is at most 64 KB and stays in the CU's cache.
template <bool LIST, bool UNIFORM = false>
__device__ __forceinline__ void slot_pixel_l(uint32_t s, const BounceArgs& a, uint32_t& x, uint32_t& y) {
  if constexpr (!LIST) {
    slot_pixel_a(s, a, x, y);
  } else {
    const uint32_t p = s & 4095u;
    const uint32_t k = UNIFORM ? __builtin_amdgcn_readfirstlane(s >> 12) : s >> 12;
    const uint32_t t = a.tile_list[k];
    const uint32_t ty = mdiv(t, a.div_tiles, a.tiles_x), tx = t - ty * a.tiles_x;
    const uint32_t blk = p >> 6, q = p & 63u;
    x = tx * kTile + (blk & 7u) * 8u + (q & 7u);
    y = ty * kTile + (blk >> 3) * 8u + (q >> 3);
  }
}

// The launch's dynamic work distribution (kernels.h): the length of one of the
// kGrabRanges ranges of a launch's N indices, a whole number of grabs
__device__ __forceinline__ uint32_t grab_range_len(uint32_t N) {
  return ((N + kGrabRanges - 1) / kGrabRanges + kGrab - 1) / kGrab * kGrab;
}

// noise table of frame (batch frame fj) - back, back in {0, 1, 2}
__device__ __forceinline__ const float4* noise_table(const BounceArgs& a, uint32_t fj, uint32_t back) {
  return a.noise_window + (a.noise_offset + fj - back) * (kNoiseDim * kNoiseDim);
}

__device__ __forceinline__ uint32_t shade_noise_cell(uint32_t x, uint32_t y, uint32_t bounce, uint32_t f) {
  // renderer/Shaders.metal:135-136
  return ((x + bounce + f / 3) % kNoiseDim) + ((y + bounce + f / 5) % kNoiseDim) * kNoiseDim;
}

// intersectionHandler body for a ray with a valid hit (distance >= 1e-4),
// renderer/Shaders.metal:128-211.  Emits the NEE shadow ray (when
// bounce + 1 < L), adds MIS-weighted emission, and — when `next` — samples
// the next bounce and updates the throughput.
template <int MODE, bool SKIP_ZERO = true>
__device__ __forceinline__ void shade_hit(const DeviceScene& sc, const LdsCtx& cx, const Hit& h, PathState& s,
                                          const float4& ns, uint32_t bounce, uint32_t L, bool next, ShadowRay& sh,
                                          bool debug_material) {
  // Loads are staged behind scheduling barriers: hoisting all 13 float4
  // record loads together would pin ~50 VGPRs and halve occupancy.
  // interpolate(float2) — KernelHelpers.h:23-47
  const float wu = h.u, wv = h.v, ww = (1.0f - h.u) - h.v;
  uint32_t mat_index, light_index;
  V3 hv, hn;
  {
    const float4 P0 = fetch_prim<MODE>(sc, cx, h.prim, 0), P1 = fetch_prim<MODE>(sc, cx, h.prim, 1);
    const float4 P2 = fetch_prim<MODE>(sc, cx, h.prim, 2);
    mat_index = fbits(P0.w);
    light_index = fbits(P1.w);
    hv = add(add(mul(mk(P0), wu), mul(mk(P1), wv)), mul(mk(P2), ww));
  }
  {
    const float4 N0 = fetch_prim<MODE>(sc, cx, h.prim, 3), N1 = fetch_prim<MODE>(sc, cx, h.prim, 4);
    const float4 N2 = fetch_prim<MODE>(sc, cx, h.prim, 5);
    hn = normalize(add(add(mul(mk(N0), wu), mul(mk(N1), wv)), mul(mk(N2), ww)));
  }
  const Mat m = load_material<MODE>(sc, cx, mat_index);
  const V3 wI = s.d;
  if (debug_material) {   // DEBUG_MATERIAL (Shaders.metal:7,142-147): radiance := Fresnel, emission and NEE add to it
    const float f = fresnel(hn, neg(wI), 1.0f, 1.5f);
    s.R = mk(f, f, f);
  }
  sh.valid = false;
  sh.graze = true;
  // light sampling — Shaders.metal:150-176
  if (bounce + 1 < L) {
    const uint32_t li = selectLightTriangle<MODE>(sc, cx, sc.num_lights, ns.z);
    // barycentric(noise.wx) — Raytracing.h:182-187
    const float r1 = m_sqrt(ns.w), r2 = ns.x;
    const float bu = 1.0f - r1, bv = r1 * (1.0f - r2), bw = r1 * r2;
    V3 lv, ln;
    float lpdf;
    uint32_t lindex;
    {
      const float4 LB = fetch_light<MODE>(sc, cx, li, 1), LD = fetch_light<MODE>(sc, cx, li, 3);
      const float4 LF = fetch_light<MODE>(sc, cx, li, 5);
      lv = add(add(mul(mk(LB), bu), mul(mk(LD), bv)), mul(mk(LF), bw));
      lpdf = LB.w;
      lindex = fbits(LD.w);
    }
    {
      const float4 LC = fetch_light<MODE>(sc, cx, li, 2), LE = fetch_light<MODE>(sc, cx, li, 4);
      const float4 LG = fetch_light<MODE>(sc, cx, li, 6);
      ln = normalize(add(add(mul(mk(LC), bu), mul(mk(LE), bv)), mul(mk(LG), bw)));
    }
    const float4 LA = fetch_light<MODE>(sc, cx, li, 0);
    V3 dirToLight;
    float cosL;
    const float lightPdf = lightTriangleSamplePDF(lpdf, LA.w, hv, lv, ln, dirToLight, cosL);
    sh.graze = !(cosL >= sc.occ_cos_min);
    float materialBsdf, materialPdf;
    sampleMaterial(m, wI, dirToLight, hn, ns, materialBsdf, materialPdf);
    const float weight = balanceHeuristic(lightPdf, materialPdf);
    const float scale = m_div(weight * materialBsdf, lightPdf);
    sh.L = mk(((LA.x * m.kd.x) * s.T.x) * scale, ((LA.y * m.kd.y) * s.T.y) * scale,
              ((LA.z * m.kd.z) * s.T.z) * scale);
    sh.o = add(hv, mul(hn, kDistanceEpsilon));
    sh.d = dirToLight;
    sh.target = lindex;
    // A light sample of exactly zero (a mirror, a plastic mirror lobe or a
    // dielectric pass-through: the material's BSDF is 0 toward the light)
    // changes nothing whether or not it is occluded — R + 0 == R bit for bit,
    // R never being -0 (it starts at +0 and +0 + -0 == +0) — so its shadow
    // query is not traced (except by the B-2 stage kernel, whose shadow-ray
    // records follow the reference: traced as the reference does)
    sh.valid = (lightPdf > 0.0f) && (lindex != h.prim);
    if (SKIP_ZERO) sh.valid = sh.valid && !((sh.L.x == 0.0f) & (sh.L.y == 0.0f) & (sh.L.z == 0.0f));
  }
  // emission with MIS — Shaders.metal:180-197 (the light vertex re-derived
  // there is the hit vertex itself: lights[ref.lightTriangleIndex].index == prim)
  if (light_index != 0xFFFFFFFFu) {
    const float area = fetch_light<MODE>(sc, cx, light_index, 0).w, tpdf = fetch_light<MODE>(sc, cx, light_index, 1).w;
    V3 dirToLight;
    float cosE;
    const float mPdf = s.pdf;
    const float lPdf = s.prevDiffuse * lightTriangleSamplePDF(tpdf, area, s.o, hv, hn, dirToLight, cosE);
    const float weight = balanceHeuristic(mPdf, lPdf);
    const float k = weight * mPdf;
    s.R = add(s.R, mk((m.le.x * s.T.x) * k, (m.le.y * s.T.y) * k, (m.le.z * s.T.z) * k));
  }
  // next ray — Shaders.metal:199-211
  if (next) {
    float bsdf, pdf, ior;
    const V3 wO = generateNextBounce(m, wI, s.ior, hn, ns, bsdf, pdf, ior);
    s.d = wO;
    s.o = add(hv, mul(hn, kDistanceEpsilon));
    s.pdf = pdf;
    s.prevDiffuse = float(m.type == kDiffuse);
    s.mtype = m.type;
    s.ior = ior;
    const float q = m_div(bsdf, pdf);
    s.T = mk(s.T.x * (m.kd.x * q), s.T.y * (m.kd.y * q), s.T.z * (m.kd.z * q));
  }
}

// accumulateImage — renderer/Shaders.metal:233-249: the value written for
// frame f given the stored pixel
__device__ __forceinline__ float4 accumulate_value(const float4& stored, V3 c, uint32_t f) {
  if (f > 0) {
    const float factor = m_div(float(f), float(f + 1));
    return make_float4(mixf(c.x, stored.x, factor), mixf(c.y, stored.y, factor), mixf(c.z, stored.z, factor), 1.0f);
  }
  return make_float4(c.x, c.y, c.z, 1.0f);
}
__device__ __forceinline__ void accumulate_pixel(float4* image, uint32_t pix, V3 c, uint32_t f) {
  image[pix] = accumulate_value(f > 0 ? image[pix] : make_float4(0.0f, 0.0f, 0.0f, 0.0f), c, f);
}

// Device-measured execution span of a frame batch's render launch(es): the
// earliest block start and the latest wave end on the chip's wall clock.
// With batches on two streams the next launch's blocks start while this one
// drains, so host events around a launch would time the wait as well.
__device__ __forceinline__ void span_begin(const BounceArgs& a) {
  if (a.span && threadIdx.x == 0) atomicMax(a.span, ~(unsigned long long)wall_clock64());
}
__device__ __forceinline__ void span_end(const BounceArgs& a) {
  if (a.span && (threadIdx.x & 63u) == 0) atomicMax(a.span + 1, (unsigned long long)wall_clock64());
}

}}}  // namespace mrt::MRT_NS::(anonymous)
