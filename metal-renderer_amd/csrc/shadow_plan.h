// shadow_plan.h — the order in which a shadow ray's lane tests the faces of the
// convex solids its segment crosses (dev_shadow.h convex_occlusion, DESIGN
// §2.1v).  Occlusion is an OR over solids and triangles, so the order is free;
// this one lets a wave test every lane's most likely face in one pass:
//   1. the entry face of the FIRST solid the lane crosses (its exit face when
//      the segment starts inside the padded solid), every lane at once;
//   2. only for lanes that pass did not certify: that solid's exit face, then
//      its other faces, then each later crossed solid's entry face, exit face
//      and other faces — each (solid, face) once, until a face hits.
// Plain C++ on values the caller computed, so that the kernels and the host
// test (tools/shadow_plan_model.cpp, tests/test_shadow_plan_host.py) compile
// the same text.
//
// A lane's plan is one register, filled by the wave-uniform loop over the
// solids:
//   bits 0-3   entry face of the first crossed solid (2 * axis + side; 8 = none)
//   bits 4-7   its exit face (8 = none)
//   bits 8-9   the first crossed solid's index
//   bit  10    the lane crosses a solid
//   bits 12-15 the later crossed solids, bit 12 + c for solid c (<= kMaxConvex = 4)
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define MRT_PLAN_FN __host__ __device__ __forceinline__
#else
#define MRT_PLAN_FN inline
#endif

namespace mrt {

constexpr uint32_t kPlanNoFace = 8u;       // convex_occlusion's "no entry / exit face"
constexpr uint32_t kPlanHas = 1u << 10;
constexpr uint32_t kPlanLaterShift = 12u;
constexpr uint32_t kPlanAllFaces = 0x3Fu;
constexpr uint32_t kPlanRow = 8u;          // pairs per solid in the staged table (6 faces, 2 x "no triangles")

// solid c's turn in the loop: `crossed` = its slabs leave the segment an
// interval and the lane does not leave that solid's own face
MRT_PLAN_FN uint32_t shadow_plan_add(uint32_t plan, uint32_t c, bool crossed, uint32_t fin, uint32_t fout) {
  const uint32_t first = fin | (fout << 4) | (c << 8) | kPlanHas;
  const uint32_t later = plan | ((1u << kPlanLaterShift) << c);
  return crossed ? ((plan & kPlanHas) ? later : first) : plan;
}

MRT_PLAN_FN bool shadow_plan_has(uint32_t plan) { return (plan & kPlanHas) != 0u; }
MRT_PLAN_FN uint32_t shadow_plan_fin(uint32_t plan) { return plan & 15u; }
MRT_PLAN_FN uint32_t shadow_plan_fout(uint32_t plan) { return (plan >> 4) & 15u; }
MRT_PLAN_FN uint32_t shadow_plan_solid(uint32_t plan) { return (plan >> 8) & 3u; }
MRT_PLAN_FN uint32_t shadow_plan_later(uint32_t plan) { return (plan >> kPlanLaterShift) & 15u; }

// the face of the one pass: the entry face, the exit face from inside, 8 when
// the segment lies inside the padded solid (no face: the rest tests all six)
MRT_PLAN_FN uint32_t shadow_plan_first_face(uint32_t plan) {
  const uint32_t fin = shadow_plan_fin(plan);
  return fin != kPlanNoFace ? fin : shadow_plan_fout(plan);
}

// where (solid, face)'s primitive pair stands in the staged table; face 8
// reads one of the row's two "no triangles" entries
MRT_PLAN_FN uint32_t shadow_plan_pair_index(uint32_t solid, uint32_t face) {
  return solid * kPlanRow + (face < kPlanRow - 1u ? face : kPlanRow - 1u);
}

// every crossed solid as a bit mask (bit c)
MRT_PLAN_FN uint32_t shadow_plan_crossed(uint32_t plan) {
  return shadow_plan_has(plan) ? (shadow_plan_later(plan) | (1u << shadow_plan_solid(plan))) : 0u;
}

// the faces of solid c still to test when the rest begins: all six, less the
// one pass's face on the first solid
MRT_PLAN_FN uint32_t shadow_plan_todo(uint32_t plan, uint32_t c) {
  const uint32_t tested = shadow_plan_solid(plan) == c ? (1u << shadow_plan_first_face(plan)) : 0u;   // 1 << 8: none
  return kPlanAllFaces & ~tested;
}

// the next face of a solid with faces `todo` (non-zero) left: entry, exit,
// then the others in index order
MRT_PLAN_FN uint32_t shadow_plan_next_face(uint32_t fin, uint32_t fout, uint32_t todo) {
  if ((todo >> fin) & 1u) return fin;     // (todo < 64: a face code of 8 finds no bit)
  if ((todo >> fout) & 1u) return fout;
  return (uint32_t)__builtin_ctz(todo);
}

}  // namespace mrt
