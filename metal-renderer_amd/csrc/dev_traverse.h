// dev_traverse.h — the while-while BVH walk: interior step, leaf tests, camera-ray candidate lists
#pragma once
#include "dev_diag.h"
#include "dev_lds.h"

namespace mrt { namespace MRT_NS { namespace {

// While-while traversal with postponed leaves (Aila & Laine 2009, recast for
// 64-lane waves): a lane that reaches a leaf parks it and keeps descending
// interior nodes until every lane of the wave holds a leaf, then the wave
// tests leaves together — interior and leaf work are not interleaved lane by
// lane.  The per-lane stack is in LDS (entries beyond STACK spill to global
// memory); kDone marks an empty stack.
// ANY = false: nearest hit in [tmin, h.t]; ties -> lowest primitive index.
// ANY = true:  stop at the first primitive k != target with (t_k, k) <
//              (t_target, target) in [0, t_target] (shadow occlusion).
// Both results are independent of the visiting order, so every tree (host
// SAH, device LBVH / PLOC) returns the same (brute-force) answer.
constexpr int32_t kDone = 0x7FFFFFFF;   // empty-stack marker

template <int STACK>
__device__ __forceinline__ int32_t stack_pop(const LdsCtx& cx, int& sp) {
  // LDS + spill stacks: a plain LDS pop when no active lane's top entry is
  // in the spill area (wave-uniform test)
  if (STACK < 0 && !__any(sp > (STACK < 0 ? -STACK : STACK))) {
    const int32_t n = sp > 0 ? (int32_t)lds_u32()[cx.stack_base + threadIdx.x + (sp - 1) * kBlock] : kDone;
    sp = max(sp - 1, 0);
    return n;
  }
  const int32_t n = sp > 0 ? stack_get<STACK>(cx, sp - 1) : kDone;
  sp = max(sp - 1, 0);
  return n;
}

// One interior node: returns the next node to visit (nearest hit child, or a
// popped entry, or kDone); the other hit children are pushed far-to-near.
// Culling slack: a child is culled only when its entry lies beyond the
// current h.t by more than 2^-11 of it.  Box padding (bvh.cpp) is relative to
// the box's own coordinates, but the ray-triangle test's t error is relative
// to the ray's distance and grows for tiny or slanted triangles: on the
// 1M-triangle mesh (1e-3-sized triangles near x, z = 0) a test returned t
// 1.5e-5 before the padded box's entry, so whether that triangle was found
// depended on whether a farther hit had shortened h.t first — i.e. on the
// lane's visiting order, which the slack rounds make timing-dependent (C5:
// one pixel in 8.3 M differed between identical runs).  Visiting
// the few boxes just behind h.t makes the answer the brute-force one again in
// such cases (it never changes an answer: the leaf tests' t <= h.t rule
// decides).
[[maybe_unused]] constexpr float kCullScale = 1.0f + 0x1p-11f;
template <int STACK, int MODE, bool ANY>
__device__ __forceinline__ int32_t interior_step(const DeviceScene& sc, const LdsCtx& cx, int32_t node, V3 o,
                                                 const RayBox& rb, float tmin, float tmax, int& sp) {
  {
    float t[4];
    int32_t r[4];
    {
      float4 q[7];
      fetch_node4<MODE>(sc, cx, node, rb, q);
      tmax *= kCullScale;   // +inf stays +inf
      box4<MODE == kGlobal ? 0 : 3, MODE != kTopLds>(q, o, rb, tmin, tmax, t);
      r[0] = (int32_t)fbits(q[6].x); r[1] = (int32_t)fbits(q[6].y); r[2] = (int32_t)fbits(q[6].z); r[3] = (int32_t)fbits(q[6].w);
    }
    const float inf = __builtin_inff();
    // near-to-far order for occlusion rays too: measured +2.5 % (C2, r1) and
    // +4.5 % (C4) over slot order — near children hold the likely occluders
    // 4-input sorting network on (t, ref); misses (+inf) sink to the end
#define MRT_CE(i, j)                                      \
    {                                                     \
      const bool sw_ = t[j] < t[i];                       \
      const float ti_ = sw_ ? t[j] : t[i];                \
      const int32_t ri_ = sw_ ? r[j] : r[i];              \
      t[j] = sw_ ? t[i] : t[j];                           \
      r[j] = sw_ ? r[i] : r[j];                           \
      t[i] = ti_;                                         \
      r[i] = ri_;                                         \
    }
    if (MODE != kAllLds) {
      MRT_CE(0, 1) MRT_CE(2, 3) MRT_CE(0, 2) MRT_CE(1, 3) MRT_CE(1, 2)
    } else {
      // all-in-LDS trees: only the nearest hit child is picked, the others
      // are pushed in slot order — the full sort's 10 more VALU ops per node
      // cost more than the better pop order saves in a shallow tree (C2:
      // occlusion queries +0.5 %, 9661 / 9646 vs 9587 / 9613; nearest
      // queries too, another +2.8 %, 9895 / 9898 vs 9630 / 9635).
      // Global-memory trees keep the full sort (C4 = for occlusion).
      MRT_CE(0, 1) MRT_CE(0, 2) MRT_CE(0, 3)
    }
#undef MRT_CE
    // LDS + spill stacks (deep trees): when no lane of the wave can reach
    // the spill area in this step (sp + 3 <= LDS entries, wave-uniform),
    // the pushes and the pop are plain LDS accesses — no per-entry
    // LDS-or-spill branches (their exec-mask bookkeeping was ~40 of the ~250
    // instructions of a global-tree interior step)
    if (STACK < 0 && !__any(sp + 3 > (STACK < 0 ? -STACK : STACK))) {
      constexpr int kL = STACK < 0 ? -STACK : STACK;
      uint32_t* st = lds_u32() + cx.stack_base + threadIdx.x;
      if (t[3] < inf) { st[sp * kBlock] = (uint32_t)r[3]; ++sp; }
      if (t[2] < inf) { st[sp * kBlock] = (uint32_t)r[2]; ++sp; }
      if (t[1] < inf) { st[sp * kBlock] = (uint32_t)r[1]; ++sp; }
      int32_t next = r[0];
      if (!(t[0] < inf)) {
        next = sp > 0 ? (int32_t)st[(sp - 1) * kBlock] : kDone;
        sp = max(sp - 1, 0);
      }
      (void)kL;
      return next;
    }
    {
      if (t[3] < inf) { stack_push<STACK>(cx, sp, r[3]); ++sp; }
      if (t[2] < inf) { stack_push<STACK>(cx, sp, r[2]); ++sp; }
      if (t[1] < inf) { stack_push<STACK>(cx, sp, r[1]); ++sp; }
    }
    int32_t next = r[0];
    if (!(t[0] < inf)) next = stack_pop<STACK>(cx, sp);
    return next;
  }
}

// The triangles [first, first + cnt) of a leaf in index order, two at a time
// with both triangles' loads issued before either test (one memory or LDS
// round trip per pair; C4 +8 % with the flat-load fix below, C2 +3.9 % for
// LDS-resident leaves).  Nearest (any = false): updates h (ties ->
// lowest primitive index; (u, v) to uv[0], uv[kBlock] when uv is non-null).
// Occlusion (any = true): true at the first primitive k != target with
// (t_k, k) < (h.t, target).
// Leaf-ordered triangles ka and kb (kb tested only when `pair`), both loaded
// before either test.
template <int MODE>
__device__ __forceinline__ bool tri_pair(const DeviceScene& sc, const LdsCtx& cx, V3 o, V3 d, float tmin,
                                         uint32_t ka, uint32_t kb, bool pair, Hit& h, bool any, uint32_t target,
                                         uint32_t* uv) {
  float4 a0, a1, a2, b0, b1, b2;
  fetch_tri<MODE>(sc, cx, ka, a0, a1, a2);
  fetch_tri<MODE>(sc, cx, kb, b0, b1, b2);
  float t[2], u[2], v[2];
  bool ok[2];
  ok[0] = tri_bary(o, d, mk(a0), mk(a1), mk(a2), t[0], u[0], v[0]);
  ok[1] = tri_bary(o, d, mk(b0), mk(b1), mk(b2), t[1], u[1], v[1]) & pair;
  const uint32_t prim[2] = {fbits(a0.w), fbits(b0.w)};
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    // (tri_accept.h occlusion_accepts, with tmin, and nearest_accepts restate the
    // two rules; the text stands here because either call changes every
    // kernel's code, in all three units)
    const bool hit = ok[j] & (t[j] >= tmin) & (t[j] <= h.t);
    if (any) {
      if (hit & (prim[j] != target) & ((t[j] < h.t) | (prim[j] < target))) return true;
    } else if (hit & (!h.found | (t[j] < h.t) | (prim[j] < h.prim))) {
      h.found = true;
      h.t = t[j];
      if (uv) {
        uv[0] = fbits(u[j]);
        uv[kBlock] = fbits(v[j]);
      } else {
        h.u = u[j];
        h.v = v[j];
      }
      h.prim = prim[j];
    }
  }
  return false;
}

// tri_pair for the nearest queries that keep h.prim == kNoPrim while nothing
// is found (the sweep, the camera rays' lists): the short predicates of
// tri_accept.h — no b1 <= 1, no !h.found — and h.found is not kept up; the
// caller derives it from h.prim when the query is over.
template <int MODE>
__device__ __forceinline__ void tri_pair_nearest(const DeviceScene& sc, const LdsCtx& cx, V3 o, V3 d, float tmin,
                                                 uint32_t ka, uint32_t kb, bool pair, Hit& h) {
  float4 a0, a1, a2, b0, b1, b2;
  fetch_tri<MODE>(sc, cx, ka, a0, a1, a2);
  fetch_tri<MODE>(sc, cx, kb, b0, b1, b2);
  float t[2], u[2], v[2];
  bool ok[2];
  ok[0] = tri_bary<true>(o, d, mk(a0), mk(a1), mk(a2), t[0], u[0], v[0]);
  ok[1] = tri_bary<true>(o, d, mk(b0), mk(b1), mk(b2), t[1], u[1], v[1]) & pair;
  const uint32_t prim[2] = {fbits(a0.w), fbits(b0.w)};
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    if (nearest_accepts_short(ok[j], t[j], tmin, h.t, prim[j], h.prim)) {
      h.t = t[j];
      h.u = u[j];
      h.v = v[j];
      h.prim = prim[j];
    }
  }
}

template <int MODE>
__device__ __forceinline__ bool leaf_tests(const DeviceScene& sc, const LdsCtx& cx, V3 o, V3 d, float tmin,
                                           uint32_t first, uint32_t cnt, Hit& h, bool any, uint32_t target,
                                           uint32_t* uv) {
  for (uint32_t k = 0; k < cnt; k += 2) {
    const uint32_t k1 = min(k + 1, cnt - 1);
    if (tri_pair<MODE>(sc, cx, o, d, tmin, first + k, first + k1, k1 != k, h, any, target, uv)) return true;
  }
  return false;
}

// Camera rays of one 8x8 pixel block through the block's candidate list
// (primary.h): the nearest hit over the listed triangles with the leaf test's
// arithmetic and tie rule — the traversal's answer, since the list holds
// every triangle a ray of the block can hit.  `list` / `cnt` are
// wave-uniform, and the list is read through the constant address space:
// that is what makes its reads scalar loads (through a plain global pointer
// they are vector loads of a uniform address).  LDS-resident triangles are
// broadcast reads.
typedef const __attribute__((address_space(4))) uint32_t* PrimaryWords;
template <int MODE>
__device__ __forceinline__ void primary_nearest(const DeviceScene& sc, const LdsCtx& cx, PrimaryWords list,
                                                uint32_t cnt, V3 o, V3 d, Hit& h) {
  h.t = __builtin_inff();
  h.u = h.v = 0.0f;
  h.prim = kNoPrim;
  h.found = false;
  for (uint32_t j = 0; j < cnt; j += 2) {
    const uint32_t j1 = min(j + 1, cnt - 1);
#if MRT_LANESTATS   // the pair's wait joins the header's in slot 38 (one event per header)
    const uint64_t t0_ = ls_clock();
    const uint32_t e0_ = list[j], e1_ = list[j1];
    asm volatile("s_waitcnt lgkmcnt(0)" ::"s"(e0_), "s"(e1_) : "memory");
    LS_ADD(38, (uint32_t)(ls_clock() - t0_));
#endif
    tri_pair_nearest<MODE>(sc, cx, o, d, 0.0f, list[j], list[j1], j1 != j, h);
  }
  h.found = h.prim != kNoPrim;
}

template <int STACK, int MODE, bool ANY>
__device__ __forceinline__ bool traverse(const DeviceScene& sc, const LdsCtx& cx, V3 o, V3 d, float tmin, Hit& h,
                                         uint32_t target, int32_t root) {
  const RayBox rb = make_raybox(o, d);
  int32_t node = root, leaf = 0;
  int sp = 0;
  constexpr int kLs = ANY ? 6 : 0;
  (void)kLs;
  LS_ADD(kLs + 0, ls_lanes());
  LS_ADD(kLs + 1, 1);
  if (node < 0) { leaf = node; node = kDone; }
  while (node != kDone || leaf != 0) {
    // interior nodes
    while (node != kDone && node >= 0) {
      LS_ADD(kLs + 2, 1);
      LS_ADD(kLs + 3, ls_lanes());
      node = interior_step<STACK, MODE, ANY>(sc, cx, node, o, rb, tmin, h.t, sp);
      if (node < 0 && leaf == 0) {   // park the leaf, keep descending
        leaf = node;
        node = stack_pop<STACK>(cx, sp);
      }
      if (__ballot(leaf == 0) == 0ull) break;
    }
    // leaves
    while (leaf < 0) {
      LS_ADD(kLs + 4, 1);
      LS_ADD(kLs + 5, ls_lanes());
      const uint32_t lr = ~(uint32_t)leaf;
      const uint32_t first = lr >> kLeafCountBits, cnt = (lr & (kMaxLeafSize - 1)) + 1;
      if (leaf_tests<MODE>(sc, cx, o, d, tmin, first, cnt, h, ANY, target, nullptr)) return true;
      leaf = 0;
      if (node < 0) {   // the next node is a leaf too: take it now
        leaf = node;
        node = stack_pop<STACK>(cx, sp);
      }
    }
  }
  return false;
}

}}}  // namespace mrt::MRT_NS::(anonymous)
