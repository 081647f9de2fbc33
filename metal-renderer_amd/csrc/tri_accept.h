// tri_accept.h — the acceptance predicates of the leaf tests, in the walk's
// form and in the sweep's shorter one.  Plain C++ on values the
// caller computed, so that the kernels and the host test
// (tools/tri_accept_model.cpp, tests/test_tri_accept_host.py) compile the
// same text.  The short forms leave out what the rest implies, bit for bit,
// in both builds' arithmetic:
//   * b1 <= 1.  `sum` is fl(b1 + b2) in the precise build and the single
//     rounding fma(dq, inv, b1) with b2 = fl(dq * inv) in the fast one.
//     Rounding is monotone and b1 is a float: b2 >= 0 with an exact product
//     x = dq * inv >= 0 gives sum >= b1, so sum <= 1 needs b1 <= 1.  A product
//     x < 0 that rounds to -0 (b2 >= 0 holds) is below the smallest denormal
//     in magnitude, and b1 > 1 means b1 >= 1 + 2^-23: b1 + x rounds to b1 or
//     above, sum > 1.  A NaN b1 or b2 fails its own >= 0.
//   * !found.  Where a nearest query keeps h.prim == 0xFFFFFFFF while nothing
//     is found (the sweep and the camera rays' lists: both start there, every
//     update writes a triangle's index, below 2^31, and a recycled ray's
//     partial hit is stored and read back as (t, u, v, prim) with found derived
//     from prim), prim < h.prim holds whenever !found does.
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define MRT_ACCEPT_FN __host__ __device__ __forceinline__
#else
#define MRT_ACCEPT_FN inline
#endif

namespace mrt {

constexpr uint32_t kNoPrim = 0xFFFFFFFFu;

// tri_bary's range test: (det, b1, b2, sum) as it computes them
MRT_ACCEPT_FN bool bary_inside(float det, float b1, float b2, float sum) {
  return (det != 0.0f) & (b1 >= 0.0f) & (b1 <= 1.0f) & (b2 >= 0.0f) & (sum <= 1.0f);
}
MRT_ACCEPT_FN bool bary_inside_short(float det, float b1, float b2, float sum) {
  return (det != 0.0f) & (b1 >= 0.0f) & (b2 >= 0.0f) & (sum <= 1.0f);
}

// a nearest query takes the triangle: in range, and (t, prim) below the hit it holds
MRT_ACCEPT_FN bool nearest_accepts(bool ok, float t, float tmin, float ht, bool found, uint32_t prim, uint32_t hprim) {
  const bool hit = ok & (t >= tmin) & (t <= ht);
  return hit & (!found | (t < ht) | (prim < hprim));
}
MRT_ACCEPT_FN bool nearest_accepts_short(bool ok, float t, float tmin, float ht, uint32_t prim, uint32_t hprim) {
  const bool hit = ok & (t >= tmin) & (t <= ht);
  return hit & ((t < ht) | (prim < hprim));
}

// the occlusion rule of a shadow query towards `target` at distance tT:
// triangle prim (in range, at t) occludes iff it is another triangle with
// (t, prim) below (tT, target) and t in [tmin, tT]
MRT_ACCEPT_FN bool occlusion_accepts(bool ok, float t, float tT, uint32_t prim, uint32_t target, float tmin = 0.0f) {
  return ok & (prim != target) & (t >= tmin) & (t <= tT) & ((t < tT) | (prim < target));
}

}  // namespace mrt
