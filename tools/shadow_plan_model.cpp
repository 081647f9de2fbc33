// shadow_plan_model.cpp — the shadow query's face order (metal-renderer_amd/
// csrc/shadow_plan.h) against the per-solid loop it replaces, one
// lane at a time, exhaustively over what the header sees:
//   * every set of crossed solids out of 1 ... 4 (the empty set included),
//     with every own-face skip (none, or any one solid);
//   * one solid of the set takes every (entry, exit) face code, 8 = none
//     included, with every pattern of hits over its six faces, while each of
//     the others takes one of two codes, hitting some face or none — each
//     solid of the set in turn.
// The lane is driven as dev_shadow.h convex_occlusion drives it: the plan is
// filled solid by solid, the one pass tests the plan's first face, the rest
// runs per crossed solid until a face hits.  Checked per case: the sequence of
// (solid, face) tests is the loop's — each crossed, unskipped solid's faces
// entry, exit, rest, each once, stopping only at a hit — the result is the
// loop's, the table index stays inside the solid's row, and the plan's fields
// read back what was packed.
// usage: shadow_plan_model   ->  one line: cases, tests, mismatches
#include <cstdint>
#include <cstdio>
#include <vector>

#include "shadow_plan.h"

using namespace mrt;

namespace {

constexpr uint32_t kMaxConvex = 4;

struct Lane {
  uint32_t count;                 // solids of the scene
  bool cand[kMaxConvex];          // crossed and not skipped
  uint32_t fin[kMaxConvex], fout[kMaxConvex];
  uint32_t hits[kMaxConvex];      // bit k: face k's triangles occlude
};

typedef std::vector<uint32_t> Seq;   // solid * 8 + face per test

// the per-solid loop (convex_occlusion_loop): a face code of 8 has no triangles
bool loop_form(const Lane& L, Seq& seq) {
  bool occluded = false;
  for (uint32_t c = 0; c < L.count; ++c) {
    if (!L.cand[c] || occluded) continue;
    const uint32_t fin = L.fin[c], fout = L.fout[c];
    bool hit = false;
    auto test = [&](uint32_t k) {
      if (k == 8u) return;
      seq.push_back(c * 8u + k);
      hit = hit || ((L.hits[c] >> k) & 1u);
    };
    test(fin != 8u ? fin : fout);
    if (!hit && fin != 8u) test(fout);
    if (!hit)
      for (uint32_t k = 0; k < 6u; ++k)
        if (!hit && k != fin && k != fout) test(k);
    occluded = occluded || hit;
  }
  return occluded;
}

// the plan's order, as the kernel drives it; `bad` counts broken invariants
bool plan_form(const Lane& L, Seq& seq, long& bad) {
  uint32_t plan = 0u;
  for (uint32_t c = 0; c < L.count; ++c) plan = shadow_plan_add(plan, c, L.cand[c], L.fin[c], L.fout[c]);
  uint32_t first = kMaxConvex, later = 0u;
  for (uint32_t c = 0; c < L.count; ++c) {
    if (!L.cand[c]) continue;
    if (first == kMaxConvex) first = c;
    else later |= 1u << c;
  }
  if (shadow_plan_has(plan) != (first != kMaxConvex)) ++bad;
  if (first != kMaxConvex && (shadow_plan_solid(plan) != first || shadow_plan_fin(plan) != L.fin[first] ||
                              shadow_plan_fout(plan) != L.fout[first] || shadow_plan_later(plan) != later ||
                              shadow_plan_crossed(plan) != (later | (1u << first))))
    ++bad;
  if (first == kMaxConvex && shadow_plan_crossed(plan) != 0u) ++bad;
  auto test = [&](uint32_t c, uint32_t k) {
    const uint32_t at = shadow_plan_pair_index(c, k);
    if (at / kPlanRow != c || (k < 6u ? at % kPlanRow != k : at % kPlanRow < 6u)) ++bad;
    if (k >= 6u) return false;   // the row's "no triangles" entries
    seq.push_back(c * 8u + k);
    return ((L.hits[c] >> k) & 1u) != 0u;
  };
  bool occluded = false;
  if (shadow_plan_has(plan)) occluded = test(shadow_plan_solid(plan), shadow_plan_first_face(plan));
  const bool more = shadow_plan_has(plan) && !occluded;
  if (more) {
    const uint32_t crossed = shadow_plan_crossed(plan);
    for (uint32_t c = 0; c < L.count; ++c) {
      if (!((crossed >> c) & 1u) || occluded) continue;
      uint32_t todo = shadow_plan_todo(plan, c);
      bool hit = false;
      while (todo != 0u && !hit) {
        const uint32_t k = shadow_plan_next_face(L.fin[c], L.fout[c], todo);
        if (k >= 6u || !((todo >> k) & 1u)) { ++bad; break; }
        todo &= ~(1u << k);
        hit = test(c, k);
      }
      occluded = occluded || hit;
    }
  }
  return occluded;
}

}  // namespace

int main() {
  static const uint32_t codes[7] = {0, 1, 2, 3, 4, 5, 8};
  // the solids that are not being varied: (entry, exit, hits)
  static const uint32_t others[4][3] = {{0, 3, 0x00}, {8, 4, 0x10}, {5, 8, 0x02}, {8, 8, 0x24}};
  long cases = 0, tests = 0, mismatches = 0, bad = 0;
  Seq a, b;
  for (uint32_t count = 1; count <= kMaxConvex; ++count)
    for (uint32_t set = 0; set < (1u << count); ++set)
      for (uint32_t skip = 0; skip <= count; ++skip)   // count: no own-face skip
        for (uint32_t vary = 0; vary < count; ++vary) {
          if (set != 0u && !((set >> vary) & 1u)) continue;   // (the empty set: once per position, nothing to vary)
          for (uint32_t o = 0; o < (1u << (count - 1u)); ++o)   // the other solids' codes, a bit each
            for (uint32_t ci = 0; ci < 49u; ++ci)
              for (uint32_t h = 0; h < 64u; ++h) {
                if (set == 0u && (o | ci | h)) continue;
                if (ci / 7u == ci % 7u && ci / 7u != 6u) continue;   // entry == exit: the slabs never give it
                Lane L;
                L.count = count;
                for (uint32_t c = 0; c < count; ++c) {
                  const uint32_t bit = c == vary ? 0u : (o >> (c < vary ? c : c - 1u)) & 1u;
                  const uint32_t* q = others[2u * bit + (c & 1u)];
                  L.cand[c] = ((set >> c) & 1u) && c != skip;
                  L.fin[c] = c == vary ? codes[ci / 7u] : q[0];
                  L.fout[c] = c == vary ? codes[ci % 7u] : q[1];
                  L.hits[c] = c == vary ? h : q[2];
                }
                a.clear();
                b.clear();
                const bool ra = loop_form(L, a), rb = plan_form(L, b, bad);
                ++cases;
                tests += (long)a.size();
                if (ra != rb || a != b) ++mismatches;
                // on its own terms: no (solid, face) twice; without a hit every face of every crossed solid
                uint32_t seen = 0u, want = 0u;
                for (uint32_t t : b) {
                  const uint32_t m = 1u << (6u * (t >> 3) + (t & 7u));
                  if (seen & m) ++bad;
                  seen |= m;
                }
                for (uint32_t c = 0; c < count; ++c) want |= L.cand[c] ? 0x3Fu << (6u * c) : 0u;
                if ((seen & ~want) || (!rb && seen != want)) ++bad;
              }
        }
  std::printf("shadow plan: cases %ld tests %ld mismatches %ld invariants %ld\n", cases, tests, mismatches, bad);
  return (mismatches || bad) ? 1 : 0;
}
