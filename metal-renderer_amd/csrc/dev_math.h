// dev_math.h — scalar math of the two builds, float3 helpers, the triangle tests and the BVH4 box test
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include "dev_config.h"
#include "kernels.h"
#include "tri_accept.h"

namespace mrt { namespace MRT_NS { namespace {

// ---------------------------------------------------------------------------
// scalar math (precision policy)
// ---------------------------------------------------------------------------
#if MRT_PRECISE
__device__ __forceinline__ float m_rcp(float x) { return 1.0f / x; }
__device__ __forceinline__ float m_sqrt(float x) { return sqrtf(x); }
__device__ __forceinline__ float m_rsqrt(float x) { return 1.0f / sqrtf(x); }
__device__ __forceinline__ float m_div(float a, float b) { return a / b; }
__device__ __forceinline__ float m_sin(float x) { return (float)sin((double)x); }
__device__ __forceinline__ float m_cos(float x) { return (float)cos((double)x); }
#else
__device__ __forceinline__ float m_rcp(float x) { return __builtin_amdgcn_rcpf(x); }
__device__ __forceinline__ float m_sqrt(float x) { return __builtin_sqrtf(x); }
__device__ __forceinline__ float m_rsqrt(float x) { return __builtin_amdgcn_rsqf(x); }
__device__ __forceinline__ float m_div(float a, float b) { return a * __builtin_amdgcn_rcpf(b); }
__device__ __forceinline__ float m_sin(float x) { return __sinf(x); }
__device__ __forceinline__ float m_cos(float x) { return __cosf(x); }
#endif

// ---------------------------------------------------------------------------
// float3 helpers with explicit evaluation order (MSL semantics)
// ---------------------------------------------------------------------------
struct V3 { float x, y, z; };
__device__ __forceinline__ V3 mk(float x, float y, float z) { return {x, y, z}; }
__device__ __forceinline__ V3 mk(const float4& a) { return {a.x, a.y, a.z}; }
__device__ __forceinline__ V3 add(V3 a, V3 b) { return {a.x + b.x, a.y + b.y, a.z + b.z}; }
__device__ __forceinline__ V3 sub(V3 a, V3 b) { return {a.x - b.x, a.y - b.y, a.z - b.z}; }
__device__ __forceinline__ V3 mul(V3 a, float s) { return {a.x * s, a.y * s, a.z * s}; }
__device__ __forceinline__ V3 neg(V3 a) { return {-a.x, -a.y, -a.z}; }
__device__ __forceinline__ float dot(V3 a, V3 b) { return (a.x * b.x + a.y * b.y) + a.z * b.z; }
__device__ __forceinline__ V3 cross(V3 a, V3 b) {
  return {a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x};
}
__device__ __forceinline__ float length(V3 a) { return m_sqrt(dot(a, a)); }
__device__ __forceinline__ V3 normalize(V3 a) { return mul(a, m_rsqrt(dot(a, a))); }
// MSL reflect(I, N) = I - 2 * dot(N, I) * N
__device__ __forceinline__ V3 reflect(V3 i, V3 n) { const float k = 2.0f * dot(n, i); return sub(i, mul(n, k)); }
// MSL mix(x, y, a) = x + (y - x) * a
__device__ __forceinline__ float mixf(float x, float y, float a) { return x + (y - x) * a; }

__device__ __forceinline__ float bitsf(uint32_t u) { return __uint_as_float(u); }
__device__ __forceinline__ uint32_t fbits(float f) { return __float_as_uint(f); }
// set bits of a wave mask in the lanes below this one (v_mbcnt: no per-lane
// 64-bit mask kept live — in the stream kernel that mask was spilled, r6)
__device__ __forceinline__ uint32_t lanes_below_in(uint64_t mask) {
  return __builtin_amdgcn_mbcnt_hi((uint32_t)(mask >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)mask, 0u));
}

// ---------------------------------------------------------------------------
// Geometry: MPS nearest-hit semantics (renderer/Renderer.mm:464-469)
// ---------------------------------------------------------------------------
// Moller-Trumbore, cull none; (u, v) are the weights of (V0, V1) as
// interpolate() expects (renderer/KernelHelpers.h:37-47).
// The fast build contracts the test's products and sums into FMAs (a
// no-contraction variant measured slower and was removed in r6); which
// triangle a near-tie ray reports may then differ from the IEEE answer, never
// with the visiting order (the culling slack, interior_step).
__device__ __forceinline__ float tdot(V3 a, V3 b) {
  return (a.x * b.x + a.y * b.y) + a.z * b.z;
}
__device__ __forceinline__ V3 tcross(V3 a, V3 b) {
  return {a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x};
}
__device__ __forceinline__ bool tri_test(V3 o, V3 d, V3 v0, V3 e1, V3 e2, float tmin, float tmax, float& t,
                                         float& u, float& v) {
  // early exits: most candidate triangles fail the first barycentric test,
  // and a wave whose lanes all fail skips the rest (s_cbranch_execz)
  const V3 p = tcross(d, e2);
  const float det = tdot(e1, p);
  if (det == 0.0f) return false;
  const float inv = m_rcp(det);
  const V3 s = sub(o, v0);
  const float b1 = tdot(s, p) * inv;
  if (!(b1 >= 0.0f && b1 <= 1.0f)) return false;
  const V3 q = tcross(s, e1);
  const float b2 = tdot(d, q) * inv;
  if (!(b2 >= 0.0f && b1 + b2 <= 1.0f)) return false;
  const float tt = tdot(e2, q) * inv;
  if (!(tt >= tmin && tt <= tmax)) return false;
  t = tt;
  u = (1.0f - b1) - b2;
  v = b1;
  return true;
}

// The same arithmetic as tri_test without the early exits (so the same hits,
// bit for bit), for the leaf loops: the distance range test is left to the
// caller.  Every operand is needed before the first decision, so the loads of
// a triangle are all in flight together instead of v0's being issued only
// after the determinant test passed.  SHORT: the range test without b1 <= 1,
// which the rest implies (tri_accept.h) — the sweep's and the camera lists'
// form; the walk keeps the full one, and with it the path kernel its code.
template <bool SHORT = false>
__device__ __forceinline__ bool tri_bary(V3 o, V3 d, V3 v0, V3 e1, V3 e2, float& t, float& u, float& v) {
  const V3 p = tcross(d, e2);
  const float det = tdot(e1, p);
  const float inv = m_rcp(det);
  const V3 s = sub(o, v0);
  const float b1 = tdot(s, p) * inv;
  const V3 q = tcross(s, e1);
  const float b2 = tdot(d, q) * inv;
  t = tdot(e2, q) * inv;
  u = (1.0f - b1) - b2;
  v = b1;
  if constexpr (SHORT) {
#if MRT_PRECISE
    const float sum = b1 + b2;
#else
    // the fast build forms b1 + b2 as one fma, and with which of the two
    // products depends on the code around it (with b2's in every leaf test
    // of the walk's form; with b1's once b1 <= 1 was gone: two pixels of C2
    // changed).  Written out, it is the walk's: fma(d . q, inv, b1).
    const float sum = __builtin_fmaf(tdot(d, q), inv, b1);
#endif
    return bary_inside_short(det, b1, b2, sum);
  }
  // (tri_accept.h bary_inside restates it; the text stands here because the
  // call orders the path kernel's compares differently)
  return (det != 0.0f) & (b1 >= 0.0f) & (b1 <= 1.0f) & (b2 >= 0.0f) & (b1 + b2 <= 1.0f);
}

struct Hit {
  float t, u, v;
  uint32_t prim;
  bool found;
};

// Node rows in ray order.  In the all-in-LDS mode every BVH4 node's x and y
// plane rows are staged in four copies, one per sign quadrant of (dir.x,
// dir.y), each pre-ordered (near, far) for rays of that quadrant; a ray reads
// the copy of its quadrant and its z rows in ray order by a row offset, so
// the box test pairs no planes by min/max (24 fewer VALU ops per node).
// Slab distances are monotone in the plane coordinate for a fixed direction
// (in both builds), so the quadrant's near plane is exactly the min of the
// pair and results are bit-identical.  (Eight octant copies measured -7.5 %
// on C2: the larger LDS image cost a resident block.)  The other modes (top
// nodes in LDS, the rest in global memory) read a node's plane rows in ray
// order through per-lane row offsets; their empty child slots are masked by
// their inverted box alone, global nodes are fetched with buffer loads
// (32-bit offsets from one descriptor), and LDS + spill stacks take plain LDS
// pushes / pops in steps where no lane can reach the spill area.  r4 A/B
// (C4 / C3 Mpaths/s, alternating in one call): buffer loads + spill fast
// path 2890 -> 2946 / 2686 -> 2735; the empty-box mask 3007-3033 / 2818-2823
// and plain pops 2971-2976 / 2791-2792 against 2922 / 2752 without either.
// Variants measured slower and removed in r6: unconditional three-entry
// pushes, an unsorted (slot-order) z row, a no-contraction triangle test.
constexpr uint32_t kQuadCopies = 4;                      // (x, y) sign quadrants
constexpr uint32_t kQuadCopyF4 = 7;                      // six plane rows + the refs row
constexpr uint32_t kQuadNodeF4 = kQuadCopies * kQuadCopyF4;

struct RayBox {   // precomputed slab-test terms
  V3 inv;
#if !MRT_PRECISE
  V3 oinv;
#endif
  uint32_t quad_f4;   // kQuadCopyF4 x quadrant; quadrant bit a set where direction component a (x, y) is negative
};

__device__ __forceinline__ float safe_inv(float d) {
  const float dd = fabsf(d) > 1e-20f ? d : copysignf(1e-20f, d);
  return m_rcp(dd);
}

__device__ __forceinline__ RayBox make_raybox(V3 o, V3 d) {
  RayBox r;
  r.inv = mk(safe_inv(d.x), safe_inv(d.y), safe_inv(d.z));
#if !MRT_PRECISE
  r.oinv = mk(o.x * r.inv.x, o.y * r.inv.y, o.z * r.inv.z);
#endif
  r.quad_f4 = kQuadCopyF4 * ((fbits(r.inv.x) >> 31) | ((fbits(r.inv.y) >> 31) << 1));
  return r;
}

// slab entry/exit on one axis; boxes are padded at build time so either form
// is conservative.
__device__ __forceinline__ float slab(float p, float o, float inv, float oinv) {
#if MRT_PRECISE
  (void)oinv;
  return (p - o) * inv;
#else
  (void)o;
  return fmaf(p, inv, -oinv);
#endif
}

// Box test of the four children of a BVH4 node (component-major node, see
// mrt_layout.h); returns each child's entry distance, +inf for a miss or an
// empty slot.  ORDERED: the x and y plane rows arrive as (near, far) (a
// quadrant copy of the all-in-LDS mode); otherwise as (lo, hi).
// LIVE = false (rows in ray order only): empty child slots are not masked by
// their ref but by their box — the builders store an inverted box (lo = +inf,
// hi = -inf) in every empty slot, whose near slab is +inf in every ray order
// (in the (lo, hi) order min/max would turn it into an infinite box)
template <int ORDERED, bool LIVE = true>   // 0: (lo, hi) rows; 2: x, y rows (near, far); 3: all rows (near, far)
__device__ __forceinline__ void box4(const float4* q, V3 o, const RayBox& rb, float tmin, float tmax, float tn[4]) {
#if MRT_PRECISE
  const float ox = o.x, oy = o.y, oz = o.z;
  const float oix = 0.0f, oiy = 0.0f, oiz = 0.0f;
#else
  const float ox = 0.0f, oy = 0.0f, oz = 0.0f;
  const float oix = rb.oinv.x, oiy = rb.oinv.y, oiz = rb.oinv.z;
  (void)o;
#endif
  const float* f = reinterpret_cast<const float*>(q);
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const float x0 = slab(f[k], ox, rb.inv.x, oix), x1 = slab(f[4 + k], ox, rb.inv.x, oix);
    const float y0 = slab(f[8 + k], oy, rb.inv.y, oiy), y1 = slab(f[12 + k], oy, rb.inv.y, oiy);
    const float z0 = slab(f[16 + k], oz, rb.inv.z, oiz), z1 = slab(f[20 + k], oz, rb.inv.z, oiz);
    float tnear, tfar;
    if constexpr (ORDERED == 3) {
      tnear = fmaxf(fmaxf(x0, y0), fmaxf(z0, tmin));
      tfar = fminf(fminf(x1, y1), fminf(z1, tmax));
    } else if constexpr (ORDERED == 2) {
      tnear = fmaxf(fmaxf(x0, y0), fmaxf(fminf(z0, z1), tmin));
      tfar = fminf(fminf(x1, y1), fminf(fmaxf(z0, z1), tmax));
    } else {
      tnear = fmaxf(fmaxf(fminf(x0, x1), fminf(y0, y1)), fmaxf(fminf(z0, z1), tmin));
      tfar = fminf(fminf(fmaxf(x0, x1), fmaxf(y0, y1)), fminf(fmaxf(z0, z1), tmax));
    }
    if constexpr (LIVE) {
      const bool live = (int32_t)fbits(f[24 + k]) != kEmptyChild;
      tn[k] = (live & (tnear <= tfar)) ? tnear : __builtin_inff();
    } else {
      static_assert(ORDERED == 3, "inverted empty boxes miss only with rows in ray order");
      tn[k] = (tnear <= tfar) ? tnear : __builtin_inff();
    }
  }
}

}}}  // namespace mrt::MRT_NS::(anonymous)
