// walk_model — CPU model of the stream kernel's nearest-hit queries on a small
// all-in-LDS scene (C2: the Cornell box), to count what a 64-lane wave spends
// in the while-while walk (dev_traverse.h traverse) and what other query shapes
// would spend on the same rays in the same waves.
//
// Builds the product tree (scene.cpp, bvh.cpp, the options mrt_scene_create
// uses), generates paths of L = 4 bounces — camera rays of 8x8 pixel blocks
// from the reference's camera, then cosine-distributed directions about the
// hit triangle's normal (a diffuse stand-in for the shader: the ray
// distribution is close to, not equal to, the renderer's) — and groups them
// into waves by the stream kernel's wave-local queue policy: the deepest
// bounce level holding 64 rays runs, else 64 new camera rays; the queues'
// remainders run as partial waves at the end.  Binned by octant, either a
// level holding 64 rays runs its fullest bin (its 128 slots cannot wait for
// more), or every bin waits for a whole wave (eight times the slots).  Bounce 0 (candidate lists)
// and the last bounce (light shortcut) are not walks in the product and are
// not counted; bounces 1 and 2 are.
//
// Every query is answered by a lock-step restatement of traverse() /
// interior_step() / leaf_tests() in the precise build's arithmetic, and:
//   1. with each level's queue binned by ray-direction octant;
//   2. by leaves in order of box entry, culled against the hit so far (the
//      order an ideal walk would have), and by the walk with a full child sort;
//   3. by the two-phase sweep (sweep_nearest): all leaf boxes, the two nearest
//      kept as keys and the rest as a mask, then entry-ordered leaf tests.
//   4. by the sweep with a cap on a pass's rest pops, unfinished rays going
//      back on their level's queue (recycling): caps 0-3 and
//      unbounded, on rays that are the same for every cap.
//   5. by the sweep over triangle-pair records (sweep_pairs.h):
//      A. single-triangle leaves paired, B. a culled or missing key ends the
//      lane with no pop, C. a third key — each variant on the same waves, and
//      on an adversarial set (origins inside and on the faces of the record
//      boxes, with every zero entry forced to -0).
//   6. by the sweep with phase 1 on centre / half-extent records in the fast
//      build's arithmetic, on part 5's rays and on the
//      adversarial set extended by directions with components 0, -0, +-1e-20;
//      no record holding a triangle the ray hits may be missed, and no key may
//      lie beyond that triangle's cull bound.
//   7. the leaf tests' acceptance predicates in the walk's form and in the
//      sweep's short one (tri_accept.h), in both builds'
//      arithmetic, on part 6's adversarial rays against every triangle.
// The sweep's (found, t, prim) is compared with the walk's for every ray, and
// so is every recycled ray's once it finishes; no queue may pass kStreamCap.
//
// build (in tools/): g++ -O2 -std=c++17 -ffp-contract=off -I../metal-renderer_amd/csrc walk_model.cpp
//        ../metal-renderer_amd/csrc/{scene,bvh}.cpp -o walk_model -lpthread
// usage: walk_model <scene.obj> [camera blocks = 2000]
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "bvh.h"
#include "scene.h"
#include "sweep_pairs.h"
#include "tri_accept.h"

using namespace mrt;

namespace {

constexpr int kWave = 64;
constexpr int32_t kDone = 0x7FFFFFFF;
constexpr float kCull = 1.0f + 0x1p-11f;
const float kInf = INFINITY;

uint32_t fb(float f) { uint32_t u; std::memcpy(&u, &f, 4); return u; }
float bf(uint32_t u) { float f; std::memcpy(&f, &u, 4); return f; }

struct Ray { float o[3], d[3]; };
struct Hit { bool found = false; float t = INFINITY; uint32_t prim = 0xFFFFFFFFu; };

BvhResult g_bvh;
std::vector<float> g_sweep;   // 8 floats per leaf, as mrt_scene_create builds them

float safe_inv(float d) { return 1.0f / (std::fabs(d) > 1e-20f ? d : std::copysign(1e-20f, d)); }
float tdot(const float* a, const float* b) { return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]; }
void tcross(const float* a, const float* b, float* c) {
  c[0] = a[1] * b[2] - a[2] * b[1];
  c[1] = a[2] * b[0] - a[0] * b[2];
  c[2] = a[0] * b[1] - a[1] * b[0];
}

// dev_math.h tri_bary + tri_pair's acceptance (nearest; ties -> lowest primitive)
void tri_test(const Ray& r, uint32_t k, Hit& h) {
  const float* T = &g_bvh.tris[12 * (size_t)k];
  float p[3], s[3], q[3];
  tcross(r.d, T + 8, p);
  const float det = tdot(T + 4, p), inv = 1.0f / det;
  for (int a = 0; a < 3; ++a) s[a] = r.o[a] - T[a];
  const float b1 = tdot(s, p) * inv;
  tcross(s, T + 4, q);
  const float b2 = tdot(r.d, q) * inv, t = tdot(T + 8, q) * inv;
  const bool ok = (det != 0.0f) & (b1 >= 0.0f) & (b1 <= 1.0f) & (b2 >= 0.0f) & (b1 + b2 <= 1.0f);
  const uint32_t prim = fb(T[3]);
  if (ok && t >= 0.0f && t <= h.t && (!h.found || t < h.t || prim < h.prim)) {
    h.found = true;
    h.t = t;
    h.prim = prim;
  }
}
void leaf_test(const Ray& r, int32_t leaf, Hit& h) {
  const uint32_t lr = ~(uint32_t)leaf, first = lr >> kLeafCountBits, cnt = (lr & (kMaxLeafSize - 1)) + 1;
  for (uint32_t k = 0; k < cnt; ++k) tri_test(r, first + k, h);
}

// box entry (tmin = 0) of (lo, hi) by the precise build's slab arithmetic; false: missed
bool box_entry(const Ray& r, const float* inv, const float* lo, const float* hi, float& tn) {
  float n[3], f[3];
  for (int a = 0; a < 3; ++a) {
    const float t0 = (lo[a] - r.o[a]) * inv[a], t1 = (hi[a] - r.o[a]) * inv[a];
    n[a] = std::fmin(t0, t1);
    f[a] = std::fmax(t0, t1);
  }
  tn = std::fmax(std::fmax(n[0], n[1]), std::fmax(n[2], 0.0f));
  return tn <= std::fmin(std::fmin(f[0], f[1]), f[2]);
}

struct WalkStats {
  double calls = 0, rays = 0, int_iter = 0, int_steps = 0, leaf_iter = 0, leaf_steps = 0;
  void print(const char* what) const {
    std::printf("%s: %.0f wave calls, %.1f lanes; interior %.2f iterations/call, %.2f steps/ray, utilisation %.3f; "
                "leaf %.2f iterations/call, %.2f steps/ray, utilisation %.3f\n",
                what, calls, rays / calls, int_iter / calls, int_steps / rays, int_steps / (64.0 * int_iter),
                leaf_iter / calls, leaf_steps / rays, leaf_steps / (64.0 * leaf_iter));
  }
};

// traverse<STACK, kAllLds, false> for one wave, lanes in lock step
void walk_wave(const Ray* rays, int n, Hit* out, WalkStats& st, bool full_sort) {
  struct Lane { int32_t node, leaf; int sp; int32_t stack[64]; float inv[3]; Hit h; };
  static Lane L[kWave];
  for (int l = 0; l < n; ++l) {
    L[l].node = g_bvh.root; L[l].leaf = 0; L[l].sp = 0; L[l].h = Hit();
    for (int a = 0; a < 3; ++a) L[l].inv[a] = safe_inv(rays[l].d[a]);
    if (L[l].node < 0) { L[l].leaf = L[l].node; L[l].node = kDone; }
  }
  st.calls += 1;
  st.rays += n;
  auto pop = [](Lane& x) { const int32_t v = x.sp > 0 ? x.stack[x.sp - 1] : kDone; x.sp = std::max(x.sp - 1, 0); return v; };
  auto interior = [&](Lane& x, const Ray& r) {
    const float* nd = &g_bvh.nodes[32 * (size_t)x.node];
    float t[4]; int32_t c[4];
    const float tmax = x.h.t * kCull;
    for (int k = 0; k < 4; ++k) {
      const float lo[3] = {nd[k], nd[8 + k], nd[16 + k]}, hi[3] = {nd[4 + k], nd[12 + k], nd[20 + k]};
      float tn;
      c[k] = (int32_t)fb(nd[24 + k]);
      t[k] = (c[k] != kEmptyChild && box_entry(r, x.inv, lo, hi, tn) && tn <= tmax) ? tn : kInf;
    }
    auto ce = [&](int i, int j) { if (t[j] < t[i]) { std::swap(t[i], t[j]); std::swap(c[i], c[j]); } };
    if (full_sort) { ce(0, 1); ce(2, 3); ce(0, 2); ce(1, 3); ce(1, 2); }
    else { ce(0, 1); ce(0, 2); ce(0, 3); }
    for (int k = 3; k >= 1; --k) if (t[k] < kInf) x.stack[x.sp++] = c[k];
    return t[0] < kInf ? c[0] : pop(x);
  };
  for (;;) {
    bool any = false, in[kWave];
    for (int l = 0; l < n; ++l) any |= L[l].node != kDone || L[l].leaf != 0;
    if (!any) break;
    for (int l = 0; l < n; ++l) in[l] = L[l].node != kDone && L[l].node >= 0;
    for (;;) {
      int act = 0;
      for (int l = 0; l < n; ++l) act += in[l];
      if (!act) break;
      st.int_iter += 1;
      st.int_steps += act;
      bool seeking = false;
      for (int l = 0; l < n; ++l) if (in[l]) {
        Lane& x = L[l];
        x.node = interior(x, rays[l]);
        if (x.node < 0 && x.leaf == 0) { x.leaf = x.node; x.node = pop(x); }
        seeking |= x.leaf == 0;
      }
      if (!seeking) break;   // every lane in the loop holds a leaf
      for (int l = 0; l < n; ++l) in[l] = in[l] && L[l].node != kDone && L[l].node >= 0;
    }
    for (;;) {
      int act = 0;
      for (int l = 0; l < n; ++l) act += L[l].leaf < 0;
      if (!act) break;
      st.leaf_iter += 1;
      st.leaf_steps += act;
      for (int l = 0; l < n; ++l) if (L[l].leaf < 0) {
        Lane& x = L[l];
        leaf_test(rays[l], x.leaf, x.h);
        x.leaf = 0;
        if (x.node < 0) { x.leaf = x.node; x.node = pop(x); }
      }
    }
  }
  for (int l = 0; l < n; ++l) out[l] = L[l].h;
}

struct SweepStats { double calls = 0, rays = 0, tests[3] = {0, 0, 0}, rounds = 0, mismatches = 0; };

// sweep_nearest for one wave
void sweep_wave(const Ray* rays, int n, Hit* out, SweepStats& st) {
  const uint32_t N = (uint32_t)(g_sweep.size() / 8), kNone = 0xFFFFFFFFu;
  uint32_t k1[kWave], k2[kWave], rest[kWave];
  float inv[kWave][3];
  st.calls += 1;
  st.rays += n;
  for (int l = 0; l < n; ++l) {
    k1[l] = k2[l] = kNone; rest[l] = 0; out[l] = Hit();
    for (int a = 0; a < 3; ++a) inv[l][a] = safe_inv(rays[l].d[a]);
    for (uint32_t i = 0; i < N; ++i) {
      float te;
      const bool hit = box_entry(rays[l], inv[l], &g_sweep[8 * i], &g_sweep[8 * i + 4], te);
      const uint32_t key = hit ? ((fb(te) & ~31u) | i) : kNone;
      const uint32_t mid = std::max(k1[l], key);
      k1[l] = std::min(k1[l], key);
      k2[l] = std::min(k2[l], mid);
      if (hit) rest[l] |= 1u << i;
    }
    rest[l] &= ~((1u << (k1[l] & 31u)) | (1u << (k2[l] & 31u)));
  }
  auto ref = [&](uint32_t id) { return (int32_t)fb(g_sweep[8 * id + 3]); };
  bool any = false;
  for (int l = 0; l < n; ++l) if (k1[l] != kNone) { any = true; leaf_test(rays[l], ref(k1[l] & 31u), out[l]); }
  st.tests[0] += any;
  any = false;
  for (int l = 0; l < n; ++l)
    if (k2[l] != kNone && bf(k2[l] & ~31u) <= out[l].t * kCull) { any = true; leaf_test(rays[l], ref(k2[l] & 31u), out[l]); }
  st.tests[1] += any;
  for (;;) {
    bool more = false;
    any = false;
    for (int l = 0; l < n; ++l) if (rest[l]) {
      more = true;
      const uint32_t id = (uint32_t)__builtin_ctz(rest[l]);
      rest[l] &= rest[l] - 1;
      float te;
      if (box_entry(rays[l], inv[l], &g_sweep[8 * id], &g_sweep[8 * id + 4], te) && te <= out[l].t * kCull) {
        any = true;
        leaf_test(rays[l], ref(id), out[l]);
      }
    }
    if (!more) break;
    st.rounds += 1;
    st.tests[2] += any;
  }
}

// 5. sweep_nearest over a list in the pair encoding (lo.w = ka | kb << 16):
// `keys` keys kept (2 or 3), `early`: the first culled or missing key clears
// the lane's mask, `neg_zero`: every zero entry of phase 1 is taken as -0
// (the key clears the sign, so it sorts first as +0 does)
struct PairStats { double calls = 0, rays = 0, tests = 0, leaf_rounds = 0, rest_leaf_rounds = 0, cull_rounds = 0, key3_rounds = 0, mismatches = 0; };
void pairs_wave(const std::vector<float>& list, int keys, bool early, bool neg_zero, const Ray* rays, int n, Hit* out,
                PairStats& st) {
  const uint32_t N = (uint32_t)(list.size() / 8), kNone = 0xFFFFFFFFu;
  uint32_t key[kWave][3], rest[kWave];
  float inv[kWave][3];
  st.calls += 1;
  st.rays += n;
  for (int l = 0; l < n; ++l) {
    key[l][0] = key[l][1] = key[l][2] = kNone; rest[l] = 0; out[l] = Hit();
    for (int a = 0; a < 3; ++a) inv[l][a] = safe_inv(rays[l].d[a]);
    for (uint32_t i = 0; i < N; ++i) {
      float te;
      const bool hit = box_entry(rays[l], inv[l], &list[8 * i], &list[8 * i + 4], te);
      if (neg_zero && te == 0.0f) te = -0.0f;
      const uint32_t k = hit ? ((fb(te) & 0x7FFFFFE0u) | i) : kNone;
      const uint32_t mid = std::max(key[l][0], k);
      key[l][0] = std::min(key[l][0], k);
      if (keys == 3) key[l][2] = std::min(key[l][2], std::max(key[l][1], mid));
      key[l][1] = std::min(key[l][1], mid);
      if (hit) rest[l] |= 1u << i;
    }
    for (int k = 0; k < keys; ++k) rest[l] &= ~(1u << (key[l][k] & 31u));
  }
  auto test = [&](int l, uint32_t id) {
    const uint32_t w = fb(list[8 * id + 3]), ka = w & 0xFFFFu, kb = w >> 16;
    tri_test(rays[l], ka, out[l]);
    if (kb != ka) tri_test(rays[l], kb, out[l]);
    st.tests += 1;
  };
  for (int round = 0; round < keys; ++round) {
    bool any = false;
    for (int l = 0; l < n; ++l) {
      const uint32_t k = key[l][round];
      const bool pass = round == 0 ? k != kNone : bf(k & ~31u) <= out[l].t * kCull;
      if (pass) { any = true; test(l, k & 31u); }
      else if (early) rest[l] = 0;
    }
    st.leaf_rounds += any;
    if (round == 2) st.key3_rounds += any;
  }
  for (;;) {
    bool more = false, any = false;
    for (int l = 0; l < n; ++l) if (rest[l]) {
      more = true;
      const uint32_t id = (uint32_t)__builtin_ctz(rest[l]);
      rest[l] &= rest[l] - 1;
      float te;
      if (box_entry(rays[l], inv[l], &list[8 * id], &list[8 * id + 4], te) && te <= out[l].t * kCull) { any = true; test(l, id); }
    }
    if (!more) break;
    st.cull_rounds += 1;
    st.leaf_rounds += any;
    st.rest_leaf_rounds += any;
  }
}
std::vector<float> g_pairs, g_unpaired;   // sweep_pairs.h: the kernels' list, and one record per leaf in its encoding
struct PairVariant { const char* name; const std::vector<float>* list; int keys; bool early; };
const PairVariant kPairVariants[6] = {
    {"today", &g_unpaired, 2, false},   {"A", &g_pairs, 2, false},         {"B alone", &g_unpaired, 2, true},
    {"A + B", &g_pairs, 2, true},       {"A + B + C", &g_pairs, 3, true},  {"B + C without A", &g_unpaired, 3, true}};
bool differs(const Hit& a, const Hit& b) {
  return a.found != b.found || (a.found && (fb(a.t) != fb(b.t) || a.prim != b.prim));
}

// 6. phase 1 on the centre list (dev_sweep.h sweep_centre), in
// the fast build's arithmetic: a = fma(c, inv, -o inv), near / far =
// fma(-+e, |inv|, a) per axis.  Phase 2 is the product's (two keys, the
// early-out, pops re-tested on lo / hi with the fast build's slab form).  Per
// ray and record it also counts: records the lo / hi test hits (in either
// build's arithmetic) and the centre test misses, those of them holding a
// triangle the ray hits, and records whose lowered key lies beyond the cull
// bound of a triangle of theirs the ray hits.
std::vector<float> g_phase1;   // sweep_pairs.h sweep_phase1_records of g_pairs
struct Phase1Stats { double rays = 0, boxes = 0, extra = 0, missed = 0, missed_with_hit = 0, late_keys = 0, mismatches = 0; };
bool box_entry_fast(const Ray& r, const float* inv, const float* lo, const float* hi, float& tn) {
  float n[3], f[3];
  for (int a = 0; a < 3; ++a) {
    const float oinv = r.o[a] * inv[a], t0 = std::fmaf(lo[a], inv[a], -oinv), t1 = std::fmaf(hi[a], inv[a], -oinv);
    n[a] = std::fmin(t0, t1);
    f[a] = std::fmax(t0, t1);
  }
  tn = std::fmax(std::fmax(n[0], n[1]), std::fmax(n[2], 0.0f));
  return tn <= std::fmin(std::fmin(f[0], f[1]), f[2]);
}
bool centre_entry(const Ray& r, const float* inv, const float* c, const float* e, float& tn) {
  float n[3], f[3];
  for (int a = 0; a < 3; ++a) {
    const float oinv = r.o[a] * inv[a], m = std::fmaf(c[a], inv[a], -oinv), ia = std::fabs(inv[a]);
    n[a] = std::fmaf(-e[a], ia, m);
    f[a] = std::fmaf(e[a], ia, m);
  }
  tn = std::fmax(std::fmax(n[0], n[1]), std::fmax(n[2], 0.0f));
  return tn <= std::fmin(std::fmin(f[0], f[1]), f[2]);
}
void phase1_wave(bool neg_zero, const Ray* rays, int n, Hit* out, Phase1Stats& st) {
  const std::vector<float>& list = g_pairs;
  const uint32_t N = (uint32_t)(list.size() / 8), kNone = 0xFFFFFFFFu;
  st.rays += n;
  for (int l = 0; l < n; ++l) {
    const Ray& r = rays[l];
    uint32_t key[2] = {kNone, kNone}, rest = 0;
    float inv[3];
    out[l] = Hit();
    for (int a = 0; a < 3; ++a) inv[a] = safe_inv(r.d[a]);
    auto tris = [&](uint32_t id, Hit& h) {
      const uint32_t w = fb(list[8 * id + 3]), ka = w & 0xFFFFu, kb = w >> 16;
      tri_test(r, ka, h);
      if (kb != ka) tri_test(r, kb, h);
    };
    for (uint32_t i = 0; i < N; ++i) {
      float te, t_old;
      const bool hit = centre_entry(r, inv, &g_phase1[8 * i], &g_phase1[8 * i + 4], te);
      const bool old = box_entry(r, inv, &list[8 * i], &list[8 * i + 4], t_old) ||
                       box_entry_fast(r, inv, &list[8 * i], &list[8 * i + 4], t_old);
      if (neg_zero && te == 0.0f) te = -0.0f;
      const uint32_t k = hit ? ((fb(te) & 0x7FFFFFE0u) | i) : kNone;
      Hit own;   // the record's own triangles, with no other hit to cull them
      tris(i, own);
      st.boxes += old;
      st.extra += hit && !old;
      st.missed += old && !hit;
      st.missed_with_hit += !hit && own.found;
      st.late_keys += hit && own.found && !(bf(k & ~31u) <= own.t * kCull);
      const uint32_t mid = std::max(key[0], k);
      key[0] = std::min(key[0], k);
      key[1] = std::min(key[1], mid);
      if (hit) rest |= 1u << i;
    }
    rest &= ~((1u << (key[0] & 31u)) | (1u << (key[1] & 31u)));
    for (int round = 0; round < 2; ++round) {
      const uint32_t k = key[round];
      if (round == 0 ? k != kNone : bf(k & ~31u) <= out[l].t * kCull) tris(k & 31u, out[l]);
      else rest = 0;
    }
    while (rest) {
      const uint32_t id = (uint32_t)__builtin_ctz(rest);
      rest &= rest - 1;
      float te;
      if (box_entry_fast(r, inv, &list[8 * id], &list[8 * id + 4], te) && te <= out[l].t * kCull) tris(id, out[l]);
    }
  }
}

// leaves in order of box entry, culled against the hit so far: tests per ray,
// and the leaf boxes hit with no culling at all
struct OrderStats { double rays = 0, waves = 0, tests = 0, wave_max = 0, boxes = 0; };
void ordered_wave(const Ray* rays, int n, OrderStats& st) {
  const uint32_t N = (uint32_t)(g_sweep.size() / 8);
  int mx = 0;
  for (int l = 0; l < n; ++l) {
    float inv[3];
    for (int a = 0; a < 3; ++a) inv[a] = safe_inv(rays[l].d[a]);
    std::vector<std::pair<float, uint32_t>> c;
    for (uint32_t i = 0; i < N; ++i) {
      float te;
      if (box_entry(rays[l], inv, &g_sweep[8 * i], &g_sweep[8 * i + 4], te)) c.push_back({te, i});
    }
    std::sort(c.begin(), c.end());
    Hit h;
    int tests = 0;
    for (auto& e : c) {
      if (!(e.first <= h.t * kCull)) break;
      leaf_test(rays[l], (int32_t)fb(g_sweep[8 * e.second + 3]), h);
      ++tests;
    }
    st.tests += tests;
    st.boxes += (double)c.size();
    mx = std::max(mx, tests);
  }
  st.rays += n;
  st.waves += 1;
  st.wave_max += mx;
}

uint64_t g_rng = 0x9E3779B97F4A7C15ull;
float rnd() {
  g_rng = g_rng * 6364136223846793005ull + 1442695040888963407ull;
  return (float)((g_rng >> 40) * (1.0 / 16777216.0));
}

// the next ray of a path: a cosine-distributed direction about the hit triangle's normal
bool bounce(const Ray& r, const Hit& h, const HostScene& sc, Ray& next) {
  if (!h.found || h.t < kDistanceEpsilon) return false;
  const RefTriangleReference& tr = sc.references[h.prim];
  const float *v0 = sc.vertices[tr.tri[0]].v, *v1 = sc.vertices[tr.tri[1]].v, *v2 = sc.vertices[tr.tri[2]].v;
  float e1[3], e2[3], nrm[3];
  for (int a = 0; a < 3; ++a) { e1[a] = v1[a] - v0[a]; e2[a] = v2[a] - v0[a]; }
  tcross(e1, e2, nrm);
  const float len = std::sqrt(tdot(nrm, nrm));
  if (!(len > 0.0f)) return false;
  const float flip = tdot(nrm, r.d) > 0.0f ? -1.0f : 1.0f;
  for (int a = 0; a < 3; ++a) nrm[a] *= flip / len;
  float t1[3] = {0, 0, 0}, t2[3];
  t1[std::fabs(nrm[0]) < 0.5f ? 0 : 1] = 1.0f;
  tcross(nrm, t1, t2);
  const float l2 = std::sqrt(tdot(t2, t2));
  for (int a = 0; a < 3; ++a) t2[a] /= l2;
  tcross(t2, nrm, t1);
  const float u = rnd(), phi = 2.0f * kPi * rnd(), rr = std::sqrt(u), z = std::sqrt(1.0f - u);
  for (int a = 0; a < 3; ++a) {
    next.o[a] = r.o[a] + r.d[a] * h.t + nrm[a] * kDistanceEpsilon;
    next.d[a] = t1[a] * (rr * std::cos(phi)) + t2[a] * (rr * std::sin(phi)) + nrm[a] * z;
  }
  return true;
}

Hit brute(const Ray& r) {
  Hit h;
  for (uint32_t k = 0; k < (uint32_t)(g_bvh.tris.size() / 12); ++k) tri_test(r, k, h);
  return h;
}

struct Totals {
  WalkStats walk, sorted;
  SweepStats sweep;
  OrderStats ordered;
  PairStats pairs[6];
  Phase1Stats phase1;
};

// one wave of bounce-`level` rays: every query shape on the same rays
void run_wave(const std::vector<Ray>& w, Totals& T, Hit* hits, bool stats_only_walk) {
  const int n = (int)w.size();
  walk_wave(w.data(), n, hits, T.walk, false);
  if (stats_only_walk) return;
  Hit tmp[kWave];
  walk_wave(w.data(), n, tmp, T.sorted, true);
  ordered_wave(w.data(), n, T.ordered);
  sweep_wave(w.data(), n, tmp, T.sweep);
  for (int l = 0; l < n; ++l)
    T.sweep.mismatches += tmp[l].found != hits[l].found || (tmp[l].found && (fb(tmp[l].t) != fb(hits[l].t) || tmp[l].prim != hits[l].prim));
  for (int v = 0; v < 6; ++v) {
    const PairVariant& pv = kPairVariants[v];
    pairs_wave(*pv.list, pv.keys, pv.early, false, w.data(), n, tmp, T.pairs[v]);
    for (int l = 0; l < n; ++l) T.pairs[v].mismatches += differs(tmp[l], hits[l]);
  }
  phase1_wave(false, w.data(), n, tmp, T.phase1);
  for (int l = 0; l < n; ++l) T.phase1.mismatches += differs(tmp[l], hits[l]);
}

// 5. the adversarial set: origins at the centre, at the face centres, inside
// and on the faces of every record box, eight directions each; every variant,
// with phase 1's zero entries as they come and forced to -0
std::vector<Ray> adversarial_set() {
  std::vector<Ray> set;
  g_rng = 0xD1B54A32D192ED03ull;
  auto dirs = [&](const float* o) {
    for (int k = 0; k < 8; ++k) {
      Ray r;
      float len;
      do {
        for (int a = 0; a < 3; ++a) r.d[a] = 2.0f * rnd() - 1.0f;
        len = std::sqrt(tdot(r.d, r.d));
      } while (!(len > 1e-3f) || len > 1.0f);
      for (int a = 0; a < 3; ++a) { r.o[a] = o[a]; r.d[a] /= len; }
      if (k == 0) r.d[1] = r.d[2] = 0.0f, r.d[0] = 1.0f;   // along an axis: the other slabs' planes at infinity
      set.push_back(r);
    }
  };
  for (const std::vector<float>* list : {&g_pairs, &g_unpaired})
    for (size_t i = 0; i < list->size() / 8; ++i) {
      const float *lo = &(*list)[8 * i], *hi = lo + 4;
      float o[3];
      for (int a = 0; a < 3; ++a) o[a] = 0.5f * (lo[a] + hi[a]);
      dirs(o);
      for (int f = 0; f < 6; ++f) {   // face centres, then random points of the faces
        for (int rep = 0; rep < 3; ++rep) {
          for (int a = 0; a < 3; ++a) o[a] = rep == 0 ? 0.5f * (lo[a] + hi[a]) : lo[a] + (hi[a] - lo[a]) * rnd();
          o[f / 2] = (f & 1) ? hi[f / 2] : lo[f / 2];
          dirs(o);
        }
      }
      for (int rep = 0; rep < 6; ++rep) {   // inside
        for (int a = 0; a < 3; ++a) o[a] = lo[a] + (hi[a] - lo[a]) * rnd();
        dirs(o);
      }
    }
  return set;
}
void adversarial(double& rays, double& mismatches) {
  const std::vector<Ray> set = adversarial_set();
  WalkStats scratch;
  Hit ref[kWave], tmp[kWave];
  for (size_t at = 0; at < set.size(); at += kWave) {
    const int n = (int)std::min<size_t>(kWave, set.size() - at);
    walk_wave(&set[at], n, ref, scratch, false);
    rays += n;
    for (int v = 0; v < 6; ++v)
      for (int nz = 0; nz < 2; ++nz) {
        PairStats ps;
        pairs_wave(*kPairVariants[v].list, kPairVariants[v].keys, kPairVariants[v].early, nz != 0, &set[at], n, tmp, ps);
        for (int l = 0; l < n; ++l) mismatches += differs(tmp[l], ref[l]);
      }
  }
}

// 6. the adversarial set of part 5, and each of its rays again with one or two
// direction components replaced by 0, -0, 1e-20 or -1e-20 (safe_inv's +-1e20:
// the axis' planes at +-infinity or, from an origin on a face, at 0 * 1e20),
// phase 1's zero entries as they come and forced to -0
std::vector<Ray> adversarial_set_with_zeros() {
  std::vector<Ray> set = adversarial_set();
  const size_t base = set.size();
  const float tiny[4] = {0.0f, -0.0f, 1e-20f, -1e-20f};
  for (size_t k = 0; k < base; ++k) {
    Ray r = set[k];
    const int a = (int)(k % 3), b = (int)((k / 3) % 3);
    r.d[a] = tiny[(k / 9) % 4];
    if (b != a) r.d[b] = tiny[(k / 36) % 4];   // two components (one when b == a)
    float len = 0.0f;   // the other components: a unit vector again (along an axis if they were zero)
    for (int c = 0; c < 3; ++c) if (c != a && c != b) len += r.d[c] * r.d[c];
    len = std::sqrt(len);
    for (int c = 0, first = 1; c < 3; ++c) if (c != a && c != b) { r.d[c] = len > 0.0f ? r.d[c] / len : (float)first; first = 0; }
    set.push_back(r);
  }
  return set;
}
void adversarial_phase1(Phase1Stats& st) {
  const std::vector<Ray> set = adversarial_set_with_zeros();
  WalkStats scratch;
  Hit ref[kWave], tmp[kWave];
  for (size_t at = 0; at < set.size(); at += kWave) {
    const int n = (int)std::min<size_t>(kWave, set.size() - at);
    walk_wave(&set[at], n, ref, scratch, false);
    for (int nz = 0; nz < 2; ++nz) {
      Phase1Stats one;
      phase1_wave(nz != 0, &set[at], n, tmp, one);
      for (int l = 0; l < n; ++l) one.mismatches += differs(tmp[l], ref[l]);
      if (nz == 0) { st.rays += one.rays; st.boxes += one.boxes; st.extra += one.extra; }
      st.missed += one.missed; st.missed_with_hit += one.missed_with_hit; st.late_keys += one.late_keys;
      st.mismatches += one.mismatches;
    }
  }
}

// 7. the acceptance predicates' two forms on part 6's adversarial rays
struct AcceptStats { double rays = 0, tests = 0, bary = 0, nearest = 0; };
void adversarial_accept(AcceptStats& st) {
  const std::vector<Ray> set = adversarial_set_with_zeros();
  const uint32_t T = (uint32_t)(g_bvh.tris.size() / 12);
  struct H { float t, u, v; uint32_t prim; bool found; };
  for (const Ray& r : set) {
    st.rays += 1;
    for (int fma = 0; fma < 2; ++fma) {   // the precise build's arithmetic, then the fast build's contractions
      auto mad = [&](float a, float b, float c) { return fma ? std::fmaf(a, b, c) : a * b + c; };
      auto dot = [&](const float* a, const float* b) { return mad(a[2], b[2], mad(a[1], b[1], a[0] * b[0])); };
      auto cross = [&](const float* a, const float* b, float* c) {
        c[0] = mad(a[1], b[2], -(a[2] * b[1]));
        c[1] = mad(a[2], b[0], -(a[0] * b[2]));
        c[2] = mad(a[0], b[1], -(a[1] * b[0]));
      };
      H full{kInf, 0.0f, 0.0f, kNoPrim, false}, brief = full;
      for (uint32_t k = 0; k < T; ++k) {
        const float* tri = &g_bvh.tris[12 * (size_t)k];
        float p[3], s[3], q[3];
        cross(r.d, tri + 8, p);
        const float det = dot(tri + 4, p), inv = 1.0f / det;
        for (int a = 0; a < 3; ++a) s[a] = r.o[a] - tri[a];
        const float b1 = dot(s, p) * inv;
        cross(s, tri + 4, q);
        const float dq = dot(r.d, q), b2 = dq * inv, t = dot(tri + 8, q) * inv;
        const float sum = fma ? std::fmaf(dq, inv, b1) : b1 + b2;
        const bool ok = bary_inside(det, b1, b2, sum), ok_s = bary_inside_short(det, b1, b2, sum);
        const uint32_t prim = fb(tri[3]);
        st.tests += 1;
        st.bary += ok != ok_s;
        if (nearest_accepts(ok, t, 0.0f, full.t, full.found, prim, full.prim)) full = H{t, (1.0f - b1) - b2, b1, prim, true};
        if (nearest_accepts_short(ok_s, t, 0.0f, brief.t, prim, brief.prim)) brief = H{t, (1.0f - b1) - b2, b1, prim, false};
        st.nearest += fb(full.t) != fb(brief.t) || fb(full.u) != fb(brief.u) || fb(full.v) != fb(brief.v) ||
                      full.prim != brief.prim || full.found != (brief.prim != kNoPrim);
      }
    }
  }
}

// the wave-local queue policy over `blocks` camera blocks; bins = 1 or 8 (octant)
// bounded: today's 128 slots per level; else a bin waits until it holds a whole wave (8 x the slots)
void simulate(const HostScene& sc, int blocks, int bins, bool bounded, Totals& T) {
  constexpr int kLevels = 2;   // bounces 1 and 2 walk (L = 4)
  std::vector<Ray> q[kLevels][8];
  g_rng = 0x9E3779B97F4A7C15ull;
  Hit hits[kWave];
  auto bin_of = [&](const Ray& r) {
    return bins == 1 ? 0 : (int)((fb(r.d[0]) >> 31) | ((fb(r.d[1]) >> 31) << 1) | ((fb(r.d[2]) >> 31) << 2));
  };
  auto run = [&](int lvl, int b, size_t count) {
    std::vector<Ray>& Q = q[lvl][b];
    std::vector<Ray> w(Q.end() - (long)count, Q.end());
    Q.resize(Q.size() - count);
    run_wave(w, T, hits, bins != 1);
    if (lvl + 1 < kLevels)
      for (size_t l = 0; l < w.size(); ++l) {
        Ray nx;
        if (bounce(w[l], hits[l], sc, nx)) q[lvl + 1][bin_of(nx)].push_back(nx);
      }
  };
  // a level holding 64 rays runs (its slots, kStreamCap = 128 per level, leave
  // no room to wait for more): binned, its fullest bin, as a partial wave if need be
  auto deepest_full = [&](int& lvl, int& b) {
    for (lvl = kLevels - 1; lvl >= 0; --lvl) {
      size_t total = 0;
      b = 0;
      for (int k = 0; k < bins; ++k) {
        total += q[lvl][k].size();
        if (q[lvl][k].size() > q[lvl][b].size()) b = k;
      }
      if (bounded ? total >= (size_t)kWave : q[lvl][b].size() >= (size_t)kWave) return true;
    }
    return false;
  };
  const int bx = 240;   // 1080p: 240 x 135 blocks of 8 x 8 pixels
  for (int blk = 0; blk < blocks;) {
    int lvl, b;
    if (deepest_full(lvl, b)) { run(lvl, b, std::min<size_t>(kWave, q[lvl][b].size())); continue; }
    // camera rays of one block, spread over the frame (rayGenerator's pinhole, no jitter)
    const int bi = (int)(((long long)blk * 32400) / blocks), px = (bi % bx) * 8, py = (bi / bx) * 8;
    ++blk;
    for (int i = 0; i < kWave; ++i) {
      const float x = ((float)(px + i % 8) + rnd()) / 1920.0f * 2.0f - 1.0f;
      const float y = ((float)(py + i / 8) + rnd()) / 1080.0f * 2.0f - 1.0f;
      Ray r;
      r.o[0] = kCameraX; r.o[1] = kCameraY; r.o[2] = kCameraZ;
      const float d[3] = {x * (1920.0f / 1080.0f) * 0.4f, y * 0.4f, -1.0f}, len = std::sqrt(tdot(d, d));
      for (int a = 0; a < 3; ++a) r.d[a] = d[a] / len;
      Ray nx;
      if (bounce(r, brute(r), sc, nx)) q[0][bin_of(nx)].push_back(nx);
    }
  }
  for (int lvl = 0; lvl < kLevels; ++lvl)   // the remainders: partial waves
    for (int b = 0; b < bins; ++b)
      while (!q[lvl][b].empty()) run(lvl, b, std::min<size_t>(kWave, q[lvl][b].size()));
}

// 4. Recycling: a pass of the sweep tests key 1, key 2 (culled)
// and then at most `cap` pops of the rest mask; a lane whose mask is still
// non-zero goes back on its own level's queue with its partial hit and the
// mask, and a later pass of that level continues it (phase 1 is wave-uniform:
// a resumed lane rides through it and ignores its keys).  keys_pop: a resumed
// lane spends the key-1 and key-2 rounds on its next two pops.  The rays are
// the same for every cap: a ray carries its own random state, so what a path
// does next does not depend on the pass it finished in.
constexpr int kStreamCap = 128;   // kernels.h: a level's slots
struct RRay { Ray r; uint64_t seed = 0; Hit h; uint32_t rest = 0, passes = 0; };
struct RecycleStats {
  double calls = 0, lanes = 0, rays = 0, leaf_rounds = 0, cull_rounds = 0, tests = 0, recycled = 0, resumed_calls = 0;
  double mismatches = 0;
  uint32_t max_passes = 0, max_queue = 0;
};

void recycle_wave(RRay* w, int n, int cap, bool keys_pop, RecycleStats& st) {
  const uint32_t N = (uint32_t)(g_sweep.size() / 8), kNone = 0xFFFFFFFFu;
  uint32_t k1[kWave], k2[kWave];
  float inv[kWave][3];
  bool resumed[kWave], any_resumed = false;
  st.calls += 1;
  st.lanes += n;
  for (int l = 0; l < n; ++l) {
    resumed[l] = w[l].rest != 0;
    any_resumed |= resumed[l];
    k1[l] = k2[l] = kNone;
    for (int a = 0; a < 3; ++a) inv[l][a] = safe_inv(w[l].r.d[a]);
    if (resumed[l]) continue;
    w[l].h = Hit();
    uint32_t rest = 0;
    for (uint32_t i = 0; i < N; ++i) {
      float te;
      const bool hit = box_entry(w[l].r, inv[l], &g_sweep[8 * i], &g_sweep[8 * i + 4], te);
      const uint32_t key = hit ? ((fb(te) & ~31u) | i) : kNone;
      const uint32_t mid = std::max(k1[l], key);
      k1[l] = std::min(k1[l], key);
      k2[l] = std::min(k2[l], mid);
      if (hit) rest |= 1u << i;
    }
    w[l].rest = rest & ~((1u << (k1[l] & 31u)) | (1u << (k2[l] & 31u)));
  }
  st.resumed_calls += any_resumed;
  auto ref = [&](uint32_t id) { return (int32_t)fb(g_sweep[8 * id + 3]); };
  auto pop = [&](int l) {   // the lowest masked leaf, culled by its recomputed entry
    const uint32_t id = (uint32_t)__builtin_ctz(w[l].rest);
    w[l].rest &= w[l].rest - 1;
    float te;
    if (!(box_entry(w[l].r, inv[l], &g_sweep[8 * id], &g_sweep[8 * id + 4], te) && te <= w[l].h.t * kCull)) return false;
    leaf_test(w[l].r, ref(id), w[l].h);
    st.tests += 1;
    return true;
  };
  for (int round = 0; round < 2; ++round) {
    bool any = false, culls = false;
    for (int l = 0; l < n; ++l) {
      if (resumed[l]) {
        if (keys_pop && w[l].rest) { culls = true; any |= pop(l); }
        continue;
      }
      const uint32_t k = round == 0 ? k1[l] : k2[l];
      if (k == kNone || (round == 1 && !(bf(k & ~31u) <= w[l].h.t * kCull))) continue;
      leaf_test(w[l].r, ref(k & 31u), w[l].h);
      st.tests += 1;
      any = true;
    }
    st.leaf_rounds += any;
    st.cull_rounds += culls;
  }
  for (int c = 0; cap < 0 || c < cap; ++c) {
    bool more = false, any = false;
    for (int l = 0; l < n; ++l)
      if (w[l].rest) { more = true; any |= pop(l); }
    if (!more) break;
    st.cull_rounds += 1;
    st.leaf_rounds += any;
  }
}

void simulate_recycle(const HostScene& sc, int blocks, int cap, bool keys_pop, RecycleStats& st) {
  constexpr int kLevels = 2;
  std::vector<RRay> q[kLevels];
  WalkStats scratch;
  auto run = [&](int lvl, size_t count) {
    std::vector<RRay>& Q = q[lvl];
    std::vector<RRay> w(Q.end() - (long)count, Q.end());
    Q.resize(Q.size() - count);
    recycle_wave(w.data(), (int)w.size(), cap, keys_pop, st);
    for (RRay& x : w)   // unfinished lanes return to their own level first (the slots the pass read)
      if (x.rest) { ++x.passes; st.recycled += 1; st.max_passes = std::max(st.max_passes, x.passes); Q.push_back(x); }
    st.max_queue = std::max<uint32_t>(st.max_queue, (uint32_t)Q.size());
    for (RRay& x : w) {
      if (x.rest) continue;
      st.rays += 1;
      Hit ref;
      walk_wave(&x.r, 1, &ref, scratch, false);
      st.mismatches += x.h.found != ref.found || (ref.found && (fb(x.h.t) != fb(ref.t) || x.h.prim != ref.prim));
      if (lvl + 1 >= kLevels) continue;
      RRay nx;
      g_rng = x.seed;
      if (bounce(x.r, x.h, sc, nx.r)) { nx.seed = g_rng; q[lvl + 1].push_back(nx); }
    }
    if (lvl + 1 < kLevels) st.max_queue = std::max<uint32_t>(st.max_queue, (uint32_t)q[lvl + 1].size());
  };
  const int bx = 240;
  for (int blk = 0; blk < blocks;) {
    int lvl = kLevels - 1;
    while (lvl >= 0 && q[lvl].size() < (size_t)kWave) --lvl;
    if (lvl >= 0) { run(lvl, kWave); continue; }
    const int bi = (int)(((long long)blk * 32400) / blocks), px = (bi % bx) * 8, py = (bi / bx) * 8;
    for (int i = 0; i < kWave; ++i) {
      uint64_t z = 0x9E3779B97F4A7C15ull * (uint64_t)(blk * kWave + i + 1);   // splitmix64: the ray's own stream
      z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
      z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
      g_rng = z ^ (z >> 31);
      const float x = ((float)(px + i % 8) + rnd()) / 1920.0f * 2.0f - 1.0f;
      const float y = ((float)(py + i / 8) + rnd()) / 1080.0f * 2.0f - 1.0f;
      Ray r;
      r.o[0] = kCameraX; r.o[1] = kCameraY; r.o[2] = kCameraZ;
      const float d[3] = {x * (1920.0f / 1080.0f) * 0.4f, y * 0.4f, -1.0f}, len = std::sqrt(tdot(d, d));
      for (int a = 0; a < 3; ++a) r.d[a] = d[a] / len;
      RRay nx;
      if (bounce(r, brute(r), sc, nx.r)) { nx.seed = g_rng; q[0].push_back(nx); }
    }
    ++blk;
    st.max_queue = std::max<uint32_t>(st.max_queue, (uint32_t)q[0].size());
  }
  for (;;) {   // the tail: the deepest non-empty level, as a partial wave
    int lvl = kLevels - 1;
    while (lvl >= 0 && q[lvl].empty()) --lvl;
    if (lvl < 0) break;
    run(lvl, std::min<size_t>(kWave, q[lvl].size()));
  }
}

}  // namespace

int main(int argc, char** argv) {
  if (argc < 2) { std::fprintf(stderr, "usage: walk_model <scene.obj> [camera blocks]\n"); return 1; }
  const int blocks = argc > 2 ? std::max(1, std::atoi(argv[2])) : 2000;
  HostScene sc;
  std::string err;
  if (!import_obj(argv[1], "", sc, err)) { std::fprintf(stderr, "%s\n", err.c_str()); return 1; }
  flatten(sc);
  BvhBuildOptions opt;   // mrt_scene_create for a small scene
  opt.width = 4;
  opt.lds_node_budget = 256;
  if (!build_bvh(sc.vertices.data()->v, sizeof(RefVertex), sc.indices.data(), (uint32_t)sc.references.size(), opt, g_bvh,
                 err)) { std::fprintf(stderr, "%s\n", err.c_str()); return 1; }
  if (g_bvh.root < 0 || g_bvh.num_leaves > kSweepLeaves) {
    std::fprintf(stderr, "the tree has %u leaves: the sweep takes at most %u under an interior root\n", g_bvh.num_leaves,
                 kSweepLeaves);
    return 1;
  }
  for (uint32_t k = 0; k < g_bvh.num_nodes; ++k) {   // the sweep list, as mrt_scene_create builds it
    const float* nd = &g_bvh.nodes[32 * (size_t)k];
    for (int c = 0; c < 4; ++c)
      if ((int32_t)fb(nd[24 + c]) < 0)
        g_sweep.insert(g_sweep.end(), {nd[c], nd[8 + c], nd[16 + c], nd[24 + c], nd[4 + c], nd[12 + c], nd[20 + c], 0.0f});
  }
  sweep_pair_records(g_sweep, true, g_pairs);
  sweep_pair_records(g_sweep, false, g_unpaired);
  sweep_phase1_records(g_pairs, g_phase1);
  std::printf("%zu triangles, %u nodes, %u leaves, %d camera blocks\n", sc.references.size(), g_bvh.num_nodes,
              g_bvh.num_leaves, blocks);
  Totals T, B[2];
  simulate(sc, blocks, 1, true, T);
  T.walk.print("walk");
  for (int k = 0; k < 2; ++k) {
    simulate(sc, blocks, 8, k == 0, B[k]);
    B[k].walk.print(k == 0 ? "1. walk, queues binned by octant, 128 slots per level" : "   the same, 1024 slots per level");
    std::printf("   wave calls x%.2f, interior iterations x%.2f, leaf iterations x%.2f in total\n",
                B[k].walk.calls / T.walk.calls, B[k].walk.int_iter / T.walk.int_iter, B[k].walk.leaf_iter / T.walk.leaf_iter);
  }
  const OrderStats& o = T.ordered;
  std::printf("2. leaf boxes hit per ray %.2f; the walk tests %.2f leaves per ray; in entry order with culling %.2f per ray, "
              "wave maximum %.2f (walk: %.2f leaf iterations)\n",
              o.boxes / o.rays, T.walk.leaf_steps / T.walk.rays, o.tests / o.rays, o.wave_max / o.waves,
              T.walk.leaf_iter / T.walk.calls);
  T.sorted.print("   walk with a full child sort");
  const SweepStats& s = T.sweep;
  std::printf("3. two-phase: %.2f leaf tests per call (%.2f + %.2f + %.2f), %.2f pop-and-cull rounds per call\n",
              (s.tests[0] + s.tests[1] + s.tests[2]) / s.calls, s.tests[0] / s.calls, s.tests[1] / s.calls,
              s.tests[2] / s.calls, s.rounds / s.calls);
  std::printf("two-phase vs walk: rays %.0f mismatches %.0f\n", s.rays, s.mismatches);
  // 4. recycling: caps 0..3 and unbounded (today's sweep on these rays), in both variants
  std::printf("4. recycling (cap: rest pops per pass; keys: resumed lanes pop in the key rounds)\n");
  double bad = 0, base_calls = 0, base_leaf = 0, base_cull = 0;
  uint32_t max_queue = 0;
  const int caps[5] = {-1, 0, 1, 2, 3};
  for (int keys = 0; keys < 2; ++keys)
    for (int cap : caps) {
      if (cap == 0 && !keys) continue;   // no progress: a resumed lane would never clear a bit
      if (cap < 0 && keys) continue;     // unbounded never resumes: one row
      RecycleStats r;
      simulate_recycle(sc, blocks, cap, keys != 0, r);
      if (cap < 0) { base_calls = r.calls; base_leaf = r.leaf_rounds; base_cull = r.cull_rounds; }
      char name[32];
      if (cap < 0) std::snprintf(name, sizeof name, "unbounded");
      else std::snprintf(name, sizeof name, "cap %d%s", cap, keys ? " keys" : "");
      std::printf("   %-11s %6.0f calls (x%.3f), %.1f lanes; leaf rounds %.2f/call (x%.3f in total), cull rounds %.2f/call "
                  "(x%.3f); %.3f tests/ray; recycled %.2f %% of rays, %.1f %% of calls hold a resumed lane, most passes %u; "
                  "longest queue %u; mismatches %.0f of %.0f\n",
                  name, r.calls, r.calls / base_calls, r.lanes / r.calls, r.leaf_rounds / r.calls, r.leaf_rounds / base_leaf,
                  r.cull_rounds / r.calls, r.cull_rounds / base_cull, r.tests / r.rays, 100.0 * r.recycled / r.rays,
                  100.0 * r.resumed_calls / r.calls, r.max_passes + 1, r.max_queue, r.mismatches, r.rays);
      bad += r.mismatches;
      max_queue = std::max(max_queue, r.max_queue);
    }
  std::printf("recycling vs walk: mismatches %.0f, longest queue %u of %d slots\n", bad, max_queue, kStreamCap);
  // 5. triangle-pair records, the culled-key early-out, the third key
  std::printf("5. triangle-pair records: %u leaves -> %zu records (per sweep call)\n", g_bvh.num_leaves, g_pairs.size() / 8);
  double pair_bad = 0;
  for (int v = 0; v < 6; ++v) {
    const PairStats& ps = T.pairs[v];
    std::printf("   %-16s %2zu records; leaf rounds %.2f (%.2f out of the rest mask), cull rounds %.2f, third key rounds %.2f; "
                "%.3f pair tests/ray; mismatches %.0f of %.0f\n",
                kPairVariants[v].name, kPairVariants[v].list->size() / 8, ps.leaf_rounds / ps.calls,
                ps.rest_leaf_rounds / ps.calls, ps.cull_rounds / ps.calls, ps.key3_rounds / ps.calls, ps.tests / ps.rays,
                ps.mismatches, ps.rays);
    pair_bad += ps.mismatches;
  }
  double adv_rays = 0, adv_bad = 0;
  adversarial(adv_rays, adv_bad);
  std::printf("   adversarial: %.0f rays from inside and on the faces of the record boxes, every variant, zero entries as "
              "they come and forced to -0: mismatches %.0f\n", adv_rays, adv_bad);
  std::printf("pairs vs walk: rays %.0f mismatches %.0f ; adversarial rays %.0f mismatches %.0f\n", T.pairs[4].rays, pair_bad,
              adv_rays, adv_bad);
  // 6. phase 1 on the centre list
  const Phase1Stats& p1 = T.phase1;
  Phase1Stats adv;
  adversarial_phase1(adv);
  std::printf("6. phase 1 on centre / half-extent records, fast-build arithmetic (per ray: lo / hi boxes hit %.2f, "
              "hit by the centre test alone %.4f, by lo / hi alone %.0f in all)\n", p1.boxes / p1.rays, p1.extra / p1.rays,
              p1.missed);
  std::printf("   adversarial: %.0f rays (part 5's, and each again with one or two direction components 0, -0, +-1e-20): "
              "lo / hi boxes hit %.2f per ray, by the centre test alone %.4f, by lo / hi alone %.0f in all (both zero "
              "settings; rays in a padded face's own plane)\n", adv.rays, adv.boxes / adv.rays, adv.extra / adv.rays,
              adv.missed);
  std::printf("phase 1 vs walk: rays %.0f mismatches %.0f ; adversarial rays %.0f mismatches %.0f ; missed records %.0f "
              "holding a hit triangle %.0f ; late keys %.0f\n", p1.rays, p1.mismatches, adv.rays, adv.mismatches,
              p1.missed + adv.missed, p1.missed_with_hit + adv.missed_with_hit, p1.late_keys + adv.late_keys);
  // 7. the acceptance predicates' short forms
  AcceptStats ac;
  adversarial_accept(ac);
  std::printf("accept forms: adversarial rays %.0f tests %.0f bary %.0f nearest %.0f\n", ac.rays, ac.tests, ac.bary, ac.nearest);
  const bool p1_ok = ac.bary + ac.nearest == 0 && p1.mismatches + adv.mismatches + p1.missed_with_hit + adv.missed_with_hit + p1.late_keys + adv.late_keys == 0;
  return s.mismatches == 0 && bad == 0 && max_queue <= (uint32_t)kStreamCap && p1_ok ? 0 : 2;
}
