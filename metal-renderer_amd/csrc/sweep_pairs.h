// sweep_pairs.h — the leaf-box sweep's device list (dev_sweep.h sweep_nearest,
// DESIGN §2.1l), derived from the per-leaf list mrt_scene_create builds: one
// record per group of at most two triangles, since the leaf test computes two
// triangles at a time whatever the leaf holds.
//   * a two-triangle leaf is one record;
//   * single-triangle leaves are paired greedily: repeatedly the pair whose
//     union box has the smallest surface area, provided that area is below the
//     sum of the two members' areas (ties: the lowest ids); an unpaired single
//     stays alone;
//   * a leaf of more than two triangles gives ceil(cnt / 2) records, each with
//     the leaf's box.
// A record's box is the component-wise min / max of its members' boxes, it
// stands at the position of its first member, and its lo.w names its
// triangles: ka | kb << 16, indices into the leaf-ordered triangle array,
// kb == ka for a single.  A union box is entered no later than either member's,
// so the sweep's candidates are a superset of the per-leaf list's and its cull
// removes no more: the answer stays the minimum of (t, prim) over the tested
// triangles.  Header-only: the library and tools/walk_model.cpp share it.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <vector>

#include "mrt_layout.h"

namespace mrt {

// leaves: 8 floats per leaf, (lo.xyz, bits(leaf ref), hi.xyz, 0) in list order.
// out: 8 floats per record, (lo.xyz, bits(ka | kb << 16), hi.xyz, 0); left
// empty when a triangle index does not fit 16 bits.  pair_singles = false: no
// two leaves share a record (the A/B switch MRT_SWEEP_PAIRS=0).
inline void sweep_pair_records(const std::vector<float>& leaves, bool pair_singles, std::vector<float>& out) {
  out.clear();
  const int n = (int)(leaves.size() / 8);
  auto bits = [&](int i) { uint32_t u; std::memcpy(&u, &leaves[8 * (size_t)i + 3], 4); return ~u; };
  auto first = [&](int i) { return bits(i) >> kLeafCountBits; };
  auto count = [&](int i) { return (bits(i) & (uint32_t)(kMaxLeafSize - 1)) + 1u; };
  auto area = [](const float* lo, const float* hi) {
    const double x = (double)hi[0] - lo[0], y = (double)hi[1] - lo[1], z = (double)hi[2] - lo[2];
    return x * y + y * z + z * x;
  };
  auto unite = [&](int i, int j, float* lo, float* hi) {
    for (int a = 0; a < 3; ++a) {
      lo[a] = std::min(leaves[8 * (size_t)i + a], leaves[8 * (size_t)j + a]);
      hi[a] = std::max(leaves[8 * (size_t)i + 4 + a], leaves[8 * (size_t)j + 4 + a]);
    }
  };
  for (int i = 0; i < n; ++i)
    if (first(i) + count(i) > 0x10000u) return;
  std::vector<int> mate(n, -1);
  while (pair_singles) {
    int bi = -1, bj = -1;
    double best = 0.0;
    for (int i = 0; i < n; ++i) {
      if (count(i) != 1 || mate[i] >= 0) continue;
      for (int j = i + 1; j < n; ++j) {
        if (count(j) != 1 || mate[j] >= 0) continue;
        float lo[3], hi[3];
        unite(i, j, lo, hi);
        const double a = area(lo, hi);
        if (!(a < area(&leaves[8 * (size_t)i], &leaves[8 * (size_t)i + 4]) +
                      area(&leaves[8 * (size_t)j], &leaves[8 * (size_t)j + 4])))
          continue;
        if (bi < 0 || a < best) { bi = i; bj = j; best = a; }
      }
    }
    if (bi < 0) break;
    mate[bi] = bj;
    mate[bj] = bi;
  }
  auto emit = [&](const float* lo, const float* hi, uint32_t ka, uint32_t kb) {
    const uint32_t w = ka | (kb << 16);
    float wf;
    std::memcpy(&wf, &w, 4);
    out.insert(out.end(), {lo[0], lo[1], lo[2], wf, hi[0], hi[1], hi[2], 0.0f});
  };
  for (int i = 0; i < n; ++i) {
    const float *lo = &leaves[8 * (size_t)i], *hi = lo + 4;
    const uint32_t f = first(i), cnt = count(i);
    if (mate[i] >= 0) {
      if (mate[i] < i) continue;   // in its first member's record
      float ulo[3], uhi[3];
      unite(i, mate[i], ulo, uhi);
      emit(ulo, uhi, f, first(mate[i]));
      continue;
    }
    for (uint32_t k = 0; k < cnt; k += 2) emit(lo, hi, f + k, f + std::min(k + 1, cnt - 1));
  }
}

// Phase 1's list (dev_sweep.h sweep_centre): record i of
// `pairs` as (c.xyz, bits(i), e.xyz, bits(1 << i)) — centre and half-extent
// per axis with [c - e, c + e] containing [lo, hi] in exact arithmetic.  c is
// the rounded midpoint and e the smallest float that is at least
// max(c - lo, hi - c): the double differences are checked with their exact
// rounding errors (two-sum) and e is stepped up with nextafter until it holds.
// The fast build's phase 1 reads this list; phase 2 and the precise build
// keep `pairs`.
inline void sweep_phase1_records(const std::vector<float>& pairs, std::vector<float>& out) {
  out.clear();
  // a - b > e in exact arithmetic, for values of floats: a - b = s + err exactly (two-sum)
  auto exceeds = [](double a, double b, double e) {
    const double y = -b, s = a + y, a1 = s - y, y1 = s - a1, err = (a - a1) + (y - y1);
    return s > e || (s == e && err > 0.0);
  };
  const size_t n = pairs.size() / 8;
  for (size_t i = 0; i < n; ++i) {
    const float *lo = &pairs[8 * i], *hi = lo + 4;
    float c[3], e[3];
    for (int a = 0; a < 3; ++a) {
      c[a] = (float)(0.5 * ((double)lo[a] + (double)hi[a]));
      e[a] = (float)std::max((double)c[a] - (double)lo[a], (double)hi[a] - (double)c[a]);
      auto holds = [&](float x) { return !exceeds(c[a], lo[a], x) && !exceeds(hi[a], c[a], x); };
      while (!holds(e[a])) e[a] = std::nextafter(e[a], INFINITY);
      while (e[a] > 0.0f && holds(std::nextafter(e[a], 0.0f))) e[a] = std::nextafter(e[a], 0.0f);   // (the cast rounded up)
    }
    const uint32_t id = (uint32_t)i, bit = 1u << (i & 31u);
    float idf, bitf;
    std::memcpy(&idf, &id, 4);
    std::memcpy(&bitf, &bit, 4);
    out.insert(out.end(), {c[0], c[1], c[2], idf, e[0], e[1], e[2], bitf});
  }
}

}  // namespace mrt
