// dev_shadow.h — shadow queries: tree choice, light / convex-solid / own-surface shortcuts, the last bounce's light hit
#pragma once
#include "dev_traverse.h"
#include "shadow_plan.h"

namespace mrt { namespace MRT_NS { namespace {

// The tree a shadow ray from o traverses: the occluder tree when o is inside
// every culled plane by the margin (occluders.h: no triangle of those planes
// can then stand between o and a light) and the ray does not graze the
// light's plane (`graze`: cosine below occ_cos_min, where the light's own t
// error could reach a culled crossing), else the main tree.  The plane data
// is wave-uniform (kernel argument, scalar registers).  So are the two roots:
// named scalars, because a per-lane select of two kernel arguments compiles
// to a select of their addresses and one vector load from the kernel-argument
// segment, waited for at once.
__device__ __forceinline__ int32_t shadow_root(const DeviceScene& sc, V3 o, bool graze) {
  const int32_t main_root = __builtin_amdgcn_readfirstlane(sc.root);
  if (sc.occ_planes == 0) return main_root;
  const int32_t occ_root = __builtin_amdgcn_readfirstlane(sc.occ_root);
  bool inside = !graze;
  for (uint32_t k = 0; k < sc.occ_planes; ++k) {
    const float* p = sc.occ_plane[k];
    inside &= fmaf(p[0], o.x, fmaf(p[1], o.y, fmaf(p[2], o.z, -p[3]))) <= -sc.occ_margin;
  }
  return inside ? occ_root : main_root;
}
// The same with the per-lane select of the two kernel arguments: the path
// kernel's, whose register allocation is left as it is (its queries have no
// stores in flight before them).  (The plane loop stands in both: one function
// for it changes the kernels' code)
__device__ __forceinline__ int32_t shadow_root_select(const DeviceScene& sc, V3 o, bool graze) {
  if (sc.occ_planes == 0 || graze) return sc.root;
  bool inside = true;
  for (uint32_t k = 0; k < sc.occ_planes; ++k) {
    const float* p = sc.occ_plane[k];
    inside &= fmaf(p[0], o.x, fmaf(p[1], o.y, fmaf(p[2], o.z, -p[3]))) <= -sc.occ_margin;
  }
  return inside ? sc.occ_root : sc.root;
}

// Light record k as the leaf test's triangle: the record's vertices are its
// primitive's, in its order (scene flattening, Renderer.mm:394-413) — three
// independent loads, and v2 - v1, v3 - v1 are the leaf record's e1, e2 bit
// for bit.  prim = lights[k].index.
struct LightTri {
  uint32_t prim;
  V3 p0, e1, e2;
};
template <int MODE>
__device__ __forceinline__ LightTri light_triangle(const DeviceScene& sc, const LdsCtx& cx, uint32_t k) {
  const float4 LB = fetch_light<MODE>(sc, cx, k, 1), LD = fetch_light<MODE>(sc, cx, k, 3);
  const float4 LF = fetch_light<MODE>(sc, cx, k, 5);
  const V3 p0 = mk(LB);
  return LightTri{fbits(LD.w), p0, sub(mk(LD), p0), sub(mk(LF), p0)};
}

// The light triangles of an occluder tree built without them (DeviceScene::
// occ_lights): every shadow ray enters the light's own leaf box, so instead
// of a leaf visit per ray the other light triangles are tested here in one
// wave-uniform loop — the leaf test's arithmetic (light_triangle) and the
// occlusion rule (tri_accept.h occlusion_accepts), so the query's answer
// is unchanged — bit for bit in the precise build; in the fast build the
// compiler may contract this inlined tri_bary differently from the leaf
// loop's (as origin_occludes), so a near-tie can flip within the 1e-2 gate.
// `tl` = the target's light index (its shading record's p1.w): the loop runs
// num_lights - 1 times, lane by lane over every light but the target (whose
// test the occlusion rule always rejected) — r6: one test instead of two per
// C2 shadow ray.
template <int MODE>
__device__ __forceinline__ bool lights_occlude(const DeviceScene& sc, const LdsCtx& cx, V3 o, V3 d, uint32_t target,
                                               uint32_t tl, float tT) {
  bool occ = false;
  for (uint32_t j = 0; j + 1 < sc.num_lights; ++j) {   // wave-uniform trip count
    const uint32_t k = j < tl ? j : j + 1u;            // per lane: the j-th light other than the target
    const LightTri l = light_triangle<MODE>(sc, cx, k);
    float t, u, v;
    const bool ok = tri_bary(o, d, l.p0, l.e1, l.e2, t, u, v);
    occ |= occlusion_accepts(ok, t, tT, l.prim, target);
  }
  return occ;
}

// One face's triangles (conv_face_tris: two primitive ids, 0xFFFF = none)
// under the leaf test's arithmetic and occlusion rule, as lights_occlude.
template <int MODE>
__device__ __forceinline__ bool face_occludes(const DeviceScene& sc, const LdsCtx& cx, V3 o, V3 d, uint32_t pair,
                                              uint32_t target, float tT) {
  bool occ = false;
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const uint32_t prim = (pair >> (16 * j)) & 0xFFFFu;
    if (prim != 0xFFFFu) {
      const V3 p0 = mk(fetch_prim<MODE>(sc, cx, prim, 0)), p1 = mk(fetch_prim<MODE>(sc, cx, prim, 1));
      const V3 p2 = mk(fetch_prim<MODE>(sc, cx, prim, 2));
      float t, u, v;
      const bool ok = tri_bary(o, d, p0, sub(p1, p0), sub(p2, p0), t, u, v);
      occ |= occlusion_accepts(ok, t, tT, prim, target);
    }
  }
  return occ;
}

// Convex occluders (r6, occluders.h ConvexSet): the occlusion walk of the
// light samples was ~24 % of the C2 stream kernel (ablation MRT_DEBUG=32:
// 11.07 -> 8.45 ms per launch), paid per wave for its longest lane.  When
// every triangle of the occluder tree lies on a convex solid (the Cornell
// box's two blocks), a lane decides each solid in straight-line code:
//   * the segment [o, o + t_T d] against the solid's three bounding slabs
//     pushed out by delta (16x the BVH boxes' padding); an empty interval
//     means no triangle of the solid can report a hit — the padded-volume
//     argument the BVH's own culling rests on, with a wider margin;
//   * a ray from a face of a solid (the origin primitive's shading record:
//     p2.w = its face code, n0.w..n2.w = the face's outward unit normal n)
//     with d . n >= kConvexLeaveDot (1e-3) skips that solid: n's plane
//     supports the convex solid and the origin is ~1e-4 outside it (x >=
//     0.999, the flat shading normal's cosine to n, occluders.cpp), so the
//     segment moves away from the solid.  The leaf test's error is what
//     bounds the threshold: a ray grazing an adjacent face's plane near the
//     shared edge gets barycentrics off by ~u |s| |e| / (|cos| area), so over
//     3 M adversarial grazing rays from the blocks' faces (70 % within
//     1e-1 ... 1e-6 of an edge, tilted 1e-1 ... 1e-8 off the face) the largest
//     d . n of a ray that hits its own solid was 1.0e-5 (IEEE) / -4.2e-5
//     (FMA): 100x below the threshold (tests/test_convex_occluders.py).
//     (r6; before, the slab pair's axis normal with d . n >= 0.01: grazing
//     rays off a block's own face then fell through to the exhaustive test
//     of its other faces, in 15-20 % of C2's shadow waves at bounces >= 1);
//   * otherwise the face the segment enters the padded solid through (or, from
//     inside it, leaves it through) has its triangles leaf-tested with the
//     occlusion rule: a hit is the traversal's own answer ("occluded"); if
//     it does not hit, the face the segment leaves through, and then the
//     solid's other faces — the leaf test over every triangle of the solid,
//     which is what the walk would have tested.
// Returns whether a solid occludes; the occluder tree is not walked.
// convex_own_skip: the solid a ray along d from primitive `origin` leaves and
// so skips (the second rule); 0xFFFFFFFF: none.
template <int MODE>
__device__ __forceinline__ uint32_t convex_own_skip(const DeviceScene& sc, const LdsCtx& cx, V3 d, uint32_t origin) {
  const uint32_t own = fbits(fetch_prim<MODE>(sc, cx, origin, 2).w);   // c * 8 + face + 1 of the origin's solid
  const V3 own_n = mk(fetch_prim<MODE>(sc, cx, origin, 3).w, fetch_prim<MODE>(sc, cx, origin, 4).w,
                      fetch_prim<MODE>(sc, cx, origin, 5).w);   // its face's outward unit normal (0 off the solids)
  return ((own != 0u) & (dot(d, own_n) >= kConvexLeaveDot)) ? (own - 1u) >> 3 : 0xFFFFFFFFu;
}

// This form decides solid by solid, faces and all, inside the loop: the
// kernels that read the scene from global memory keep it (the path kernel's
// code is as it was); the all-in-LDS kernels take convex_occlusion below.
template <int MODE>
__device__ __forceinline__ bool convex_occlusion_loop(const DeviceScene& sc, const LdsCtx& cx, V3 o, V3 d,
                                                      uint32_t target, float tT, uint32_t origin) {
  const uint32_t own_skip = convex_own_skip<MODE>(sc, cx, d, origin);
  bool occluded = false;
  for (uint32_t c = 0; c < sc.conv_count; ++c) {   // wave-uniform; the three slabs unrolled (scalar operands)
    const float* B = sc.conv_obb[c];
    float t0 = 0.0f, t1 = tT;
    uint32_t fin = 8u, fout = 8u;   // entry / exit face (2a + side); 8 = none
#pragma unroll
    for (uint32_t a = 0; a < 3; ++a) {
      const float nd = (B[3 * a] * d.x + B[3 * a + 1] * d.y) + B[3 * a + 2] * d.z;
      const float no = (B[3 * a] * o.x + B[3 * a + 1] * o.y) + B[3 * a + 2] * o.z;
      const float inv = m_rcp(nd);
      const float tlo = (B[9 + 2 * a] - no) * inv, thi = (B[10 + 2 * a] - no) * inv;
      // along +n (the sign bit, so that nd = -0 pairs with inv = -inf): enters
      // through the lo face, leaves through the hi face; parallel rays get
      // (-inf, +inf) inside the slab, an empty interval outside, and NaN (no
      // constraint, the conservative side) exactly on a slab plane
      const bool pos = (fbits(nd) >> 31) == 0u;
      const float tn = pos ? tlo : thi, tf = pos ? thi : tlo;
      const bool in_ = tn > t0, out_ = tf < t1;
      t0 = in_ ? tn : t0;
      fin = in_ ? (pos ? 2u * a : 2u * a + 1u) : fin;
      t1 = out_ ? tf : t1;
      fout = out_ ? (pos ? 2u * a + 1u : 2u * a) : fout;
    }
    const bool leaves_own = own_skip == c;
    if ((t0 <= t1) & !leaves_own & !occluded) {
      LS_ADD_SPLIT(48, 1);
      uint32_t pin = 0xFFFFFFFFu, pout = 0xFFFFFFFFu;
#pragma unroll
      for (uint32_t k = 0; k < 6; ++k) {
        pin = fin == k ? sc.conv_face_tris[c][k] : pin;
        pout = fout == k ? sc.conv_face_tris[c][k] : pout;
      }
      bool hit = face_occludes<MODE>(sc, cx, o, d, pin != 0xFFFFFFFFu ? pin : pout, target, tT);
      if (!hit & (pin != 0xFFFFFFFFu)) hit = face_occludes<MODE>(sc, cx, o, d, pout, target, tT);
      // neither face certifies (a near miss within delta, or an entry through
      // another face near an edge): the solid's other faces, which makes the
      // lane's answer the leaf test over every triangle of the solid
      if (!hit) {
#pragma unroll
        for (uint32_t k = 0; k < 6; ++k)
          if (!hit & (k != fin) & (k != fout)) hit = face_occludes<MODE>(sc, cx, o, d, sc.conv_face_tris[c][k], target, tT);
      }
      occluded |= hit;
    }
  }
  return occluded;
}

// Solid c's three padded slabs against the segment [o, o + tT d], the
// arithmetic of convex_occlusion_loop word for word (which keeps its own text:
// calling this changes the path and per-bounce kernels' code):
// whether an interval is left, and the entry / exit face (2a + side; 8 = none).
__device__ __forceinline__ bool convex_slabs(const DeviceScene& sc, uint32_t c, V3 o, V3 d, float tT, uint32_t& fin,
                                             uint32_t& fout) {
  const float* B = sc.conv_obb[c];
  float t0 = 0.0f, t1 = tT;
  fin = 8u;
  fout = 8u;
#pragma unroll
  for (uint32_t a = 0; a < 3; ++a) {
    const float nd = (B[3 * a] * d.x + B[3 * a + 1] * d.y) + B[3 * a + 2] * d.z;
    const float no = (B[3 * a] * o.x + B[3 * a + 1] * o.y) + B[3 * a + 2] * o.z;
    const float inv = m_rcp(nd);
    const float tlo = (B[9 + 2 * a] - no) * inv, thi = (B[10 + 2 * a] - no) * inv;
    const bool pos = (fbits(nd) >> 31) == 0u;
    const float tn = pos ? tlo : thi, tf = pos ? thi : tlo;
    const bool in_ = tn > t0, out_ = tf < t1;
    t0 = in_ ? tn : t0;
    fin = in_ ? (pos ? 2u * a : 2u * a + 1u) : fin;
    t1 = out_ ? tf : t1;
    fout = out_ ? (pos ? 2u * a + 1u : 2u * a) : fout;
  }
  return t0 <= t1;
}

// The same decisions in another order (shadow_plan.h; kAllLds
// only: the face pairs are read from the LDS image by a per-lane index).
// Occlusion is an OR over solids and triangles, so a face test need not wait
// for its solid's turn: the loop over the solids keeps the slab tests and
// files what each lane crosses into its plan; then every lane tests the entry
// face of the FIRST solid it crosses, the whole wave in one pass — where the
// loop form made a divergent pass per solid, each with the few lanes that
// cross that one; and only if a lane is left neither occluded nor done (a
// ballot) does the rest run: per crossed solid the faces not yet tested, in the
// loop form's order.  Per (ray, solid) the same slabs, the same own-face
// skip and the leaf test over the same triangles until one hits: the answer
// is the loop form's.
template <int MODE>
__device__ __forceinline__ bool convex_occlusion(const DeviceScene& sc, const LdsCtx& cx, V3 o, V3 d, uint32_t target,
                                                 float tT, uint32_t origin) {
  const uint32_t own_skip = convex_own_skip<MODE>(sc, cx, d, origin);
  uint32_t plan = 0u;
  for (uint32_t c = 0; c < sc.conv_count; ++c) {   // wave-uniform; the three slabs unrolled (scalar operands)
    uint32_t fin, fout;
    const bool crosses = convex_slabs(sc, c, o, d, tT, fin, fout);
    plan = shadow_plan_add(plan, c, crosses & (own_skip != c), fin, fout);
  }
  bool occluded = false;
  if (shadow_plan_has(plan)) {   // the one face pass
    LS_ADD_SPLIT(48, 1);
    const uint32_t at = shadow_plan_pair_index(shadow_plan_solid(plan), shadow_plan_first_face(plan));
    occluded = face_occludes<MODE>(sc, cx, o, d, lds_u32()[cx.conv_base + at], target, tT);
  }
  const bool more = shadow_plan_has(plan) & !occluded;
  if (__ballot(more)) {   // the rare rest: a near miss within delta, an entry near an edge, a second solid
    const uint32_t crossed = more ? shadow_plan_crossed(plan) : 0u;
    for (uint32_t c = 0; c < sc.conv_count; ++c) {
      if (((crossed >> c) & 1u) & !occluded) {
        uint32_t fin, fout;
        convex_slabs(sc, c, o, d, tT, fin, fout);
        uint32_t todo = shadow_plan_todo(plan, c);
        bool hit = false;
        while ((todo != 0u) & !hit) {
          const uint32_t k = shadow_plan_next_face(fin, fout, todo);
          todo &= ~(1u << k);
          hit = face_occludes<MODE>(sc, cx, o, d, lds_u32()[cx.conv_base + shadow_plan_pair_index(c, k)], target, tT);
        }
        occluded |= hit;
      }
    }
  }
  return occluded;
}

template <int STACK, int MODE>
__device__ __forceinline__ bool trace_occluded(const DeviceScene& sc, const LdsCtx& cx, V3 o, V3 d, uint32_t target,
                                               uint32_t tl, float t_target, bool graze, uint32_t origin,
                                               uint32_t dbg = 0u) {
  Hit h;
  h.t = t_target;
  h.found = false;
  LS_T0();
  int32_t root = shadow_root(sc, o, graze);
#if MRT_LANESTATS
  asm volatile("" ::"v"(root));
  LS_T1(40);
#endif
  const bool via_occ = root == sc.occ_root;
  if (sc.conv_count && via_occ) {
    LS_ADD_SPLIT(49, 1);
    if (!(dbg & 512u) && (MODE == kAllLds && !MRT_CONVEX_LOOP ? convex_occlusion<MODE>(sc, cx, o, d, target, t_target, origin)
                                          : convex_occlusion_loop<MODE>(sc, cx, o, d, target, t_target, origin)))
      return true;
    root = kDone;   // no walk (the light triangles are still tested below)
  }
  if (sc.occ_lights && via_occ && !(dbg & 1024u) && lights_occlude<MODE>(sc, cx, o, d, target, tl, t_target)) return true;
  return traverse<STACK, MODE, true>(sc, cx, o, d, 0.0f, h, target, root);
}

// The shadow ray's own surface first (exact early-out, r4).  The occlusion
// query answers "occluded" as soon as ANY primitive k != target passes the
// leaf test with (t_k, k) < (t_T, target) in [0, t_T]; the triangle the ray
// leaves is such a k whenever the light lies behind that triangle's plane
// (the ray re-crosses the surface ~1e-4 from its origin: about half of a
// closed mesh's shadow rays, each of which would otherwise descend the tree
// to the origin's own leaf).  It is tested with the leaf test's arithmetic
// (tri_bary over the shading record's vertices: the leaf record's v0,
// e1 = v1 - v0, e2 = v2 - v0 are the same float operations, bvh.cpp) and its
// acceptance rule, so "occluded" here is the traversal's answer and
// "not occluded" changes nothing — bit-exactly in the precise build (no FMA
// contraction).  In the fast build (-ffp-contract=fast) the compiler may fuse
// this inlined copy of tri_bary differently from the leaf loop's, so on a
// near-tie (t within an ulp of t_T or 0) the two can disagree; the fast
// build's 1e-2 image gate covers such flips.  Scenes of >= kOriginTestTriangles only
// (DeviceScene::origin_test).
// the last bounce's occlusion query of a light hit through the occluder tree
// (shadow_root) instead of the main tree
template <int MODE>
__device__ __forceinline__ bool origin_occludes(const DeviceScene& sc, const LdsCtx& cx, V3 o, V3 d, uint32_t prim,
                                                uint32_t target, float tT) {
  if (!sc.origin_test) return false;   // wave-uniform (kernel argument)
  const V3 p0 = mk(fetch_prim<MODE>(sc, cx, prim, 0)), p1 = mk(fetch_prim<MODE>(sc, cx, prim, 1));
  const V3 p2 = mk(fetch_prim<MODE>(sc, cx, prim, 2));
  float t, u, v;
  const bool ok = tri_bary(o, d, p0, sub(p1, p0), sub(p2, p0), t, u, v);
  return occlusion_accepts(ok, t, tT, prim, target);
}

// Shadow-ray resolve under MPS nearest-hit semantics + lightSamplingHandler
// (renderer/Shaders.metal:214-231): contributes iff the nearest hit of the
// shadow ray (tmin 0, tmax inf) is the target triangle at t >= 1e-4.
// `origin` = the primitive the ray leaves (origin_occludes).
template <int STACK, int MODE>
__device__ bool shadow_reaches_target(const DeviceScene& sc, const LdsCtx& cx, V3 o, V3 d, uint32_t target,
                                      uint32_t origin, bool graze, uint32_t dbg = 0u) {
  const float4 P1 = fetch_prim<MODE>(sc, cx, target, 1);   // .w: the target's light index
  const V3 p0 = mk(fetch_prim<MODE>(sc, cx, target, 0)), p1 = mk(P1);
  const V3 p2 = mk(fetch_prim<MODE>(sc, cx, target, 2));
  float tT, u, v;
  if (!tri_test(o, d, p0, sub(p1, p0), sub(p2, p0), 0.0f, __builtin_inff(), tT, u, v)) return false;
  if (!(tT >= kDistanceEpsilon)) return false;
  if (!(dbg & 128u) && origin_occludes<MODE>(sc, cx, o, d, origin, target, tT)) return false;
  if (dbg & 32u) return true;   // ablation: no occlusion traversal
  return !trace_occluded<STACK, MODE>(sc, cx, o, d, target, fbits(P1.w), tT, graze, origin, dbg);
}

// Last bounce (bounce + 1 == MAX_PATH_LENGTH): intersectionHandler adds no
// light sample and makes no next ray there (Shaders.metal:150,199), so the
// nearest hit matters only if it is an emitter — every emitter is a light
// triangle (scene flattening) — and only through its emission.  So the
// nearest query becomes: the nearest (t, prim) over the light triangles
// alone (leaf-test arithmetic and tie rule over their shading records), then
// — if one is hit at t >= 1e-4 — the occlusion query "does any other
// triangle k beat it, (t_k, k) < (t_L, L)" (the shadow query's any-hit
// traversal).  Not beaten: the nearest hit is that light (emission follows
// as before); beaten, missed, or nearer than 1e-4: no emission, which is
// all the reference's nearest hit could add.  Exact (precise build
// bitwise); scenes with <= kLightShortcutMax light triangles
// (DeviceScene::light_shortcut), not with DEBUG_MATERIAL (which shades
// every hit).  Returns true when the occlusion query is still to run (h
// holds the light hit); false: h.found says whether there is emission.
// Measured (r4, alternating in one call): C2 (stream kernel) 9738 / 9743 ->
// 10772 / 10778 Mpaths/s (+10.6 %); the path kernel keeps the full query
// (its variant measured C4 -1.3 %, C3 -3.4 %, removed in r6).
// `graze`: the hit light's cosine to the ray is below the occluder tree's
// guard (shadow_root; |d . n| / |n| over the geometric normal n = e1 x e2,
// which occluders.cpp's cos_min covers as it covers the interpolated normal).
template <int MODE>
__device__ __forceinline__ bool last_bounce_light_hit(const DeviceScene& sc, const LdsCtx& cx, V3 o, V3 d, Hit& h,
                                                      bool& graze) {
  h.t = __builtin_inff();
  h.u = h.v = 0.0f;
  h.prim = 0xFFFFFFFFu;
  h.found = false;
  float gd = 0.0f, gn = 1.0f;   // the nearest light's (d . n)^2 and n . n
  for (uint32_t k = 0; k < sc.num_lights; ++k) {   // wave-uniform
    const LightTri l = light_triangle<MODE>(sc, cx, k);
    float t, u, v;
    const bool ok = tri_bary(o, d, l.p0, l.e1, l.e2, t, u, v);
    const bool hit = ok & (t >= 0.0f) & (t <= h.t);
    if (hit & (!h.found | (t < h.t) | (l.prim < h.prim))) {
      h.found = true;
      h.t = t;
      h.u = u;
      h.v = v;
      h.prim = l.prim;
      const V3 n = tcross(l.e1, l.e2);
      const float dn = tdot(d, n);
      gd = dn * dn;
      gn = tdot(n, n);
    }
  }
  if (h.found && h.t < kDistanceEpsilon) h.found = false;   // no emission whatever is nearer
  graze = !(gd >= sc.occ_cos_min2 * gn);
  return h.found;
}

}}}  // namespace mrt::MRT_NS::(anonymous)
