// tri_accept_model — the leaf tests' acceptance predicates of tri_accept.h,
// the walk's form against the sweep's short one, on the CPU.
// Compiled twice: MODEL_FMA=0 is the precise build's arithmetic (no
// contraction), MODEL_FMA=1 puts std::fmaf where the fast build contracts
// (dot and cross products, and b1 + b2 as one fma with either product).
//   A. the cross product of special values — ±0, denormals, the neighbours of
//      0 and 1, ±inf, NaN and a few plain ones — for the range test's
//      (det, b1, b2) with b1 + b2 as each arithmetic forms it, and for the
//      nearest rule's (t, tmin, h.t, prim, h.prim) in every state the
//      invariant allows (nothing found: h.prim = 0xFFFFFFFF), and for the
//      occlusion rule's (t, tmin, t_T, prim, target) against its written-out
//      form: in [tmin, t_T], another triangle, (t, prim) below (t_T, target);
//   B. random rays against random triangles and their copies (equal t: the
//      tie rule), many aimed at a vertex or an edge, where b1, b2 and their sum
//      stand at 0 and 1: each ray folds a list of triangles into a hit with
//      both forms, in index order and reversed, and is an occlusion query
//      towards each of the triangles at its own t.
// Prints one line; every count of disagreements must be 0.
// build: g++ -O2 -std=c++17 -ffp-contract=off -DMODEL_FMA=<0|1> -I../metal-renderer_amd/csrc tri_accept_model.cpp
// usage: tri_accept_model [random cases = 1000000]
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <vector>

#include "tri_accept.h"

#ifndef MODEL_FMA
#define MODEL_FMA 0
#endif

using namespace mrt;

namespace {

uint32_t fb(float f) { uint32_t u; std::memcpy(&u, &f, 4); return u; }

float mad(float a, float b, float c) { return MODEL_FMA ? std::fmaf(a, b, c) : a * b + c; }
float tdot(const float* a, const float* b) { return mad(a[2], b[2], mad(a[1], b[1], a[0] * b[0])); }
void tcross(const float* a, const float* b, float* c) {
  c[0] = mad(a[1], b[2], -(a[2] * b[1]));
  c[1] = mad(a[2], b[0], -(a[0] * b[2]));
  c[2] = mad(a[0], b[1], -(a[1] * b[0]));
}

struct Hit { float t, u, v; uint32_t prim; bool found; };
bool same(const Hit& a, const Hit& b) {
  return fb(a.t) == fb(b.t) && fb(a.u) == fb(b.u) && fb(a.v) == fb(b.v) && a.prim == b.prim;
}

uint64_t g_rng = 0x9E3779B97F4A7C15ull;
float rnd() {
  g_rng = g_rng * 6364136223846793005ull + 1442695040888963407ull;
  return (float)((g_rng >> 40) & 0xFFFFFF) / 16777216.0f;
}

struct Counts { double tests = 0, bary = 0, nearest = 0, state = 0, occlusion = 0; };

// the occlusion rule written out: the range, then the order on (t, prim)
bool occludes(bool ok, float t, float tmin, float tT, uint32_t prim, uint32_t target) {
  if (!ok || prim == target) return false;
  if (!(t >= tmin) || !(t <= tT)) return false;
  return t < tT || prim < target;
}

// dev_math.h tri_bary's terms; `alt`: b1 + b2 contracted with b1's product instead of b2's
void tri_terms(const float* o, const float* d, const float* v0, const float* e1, const float* e2, bool alt, float& det,
               float& b1, float& b2, float& sum, float& t) {
  float p[3], s[3], q[3];
  tcross(d, e2, p);
  det = tdot(e1, p);
  const float inv = 1.0f / det;
  for (int a = 0; a < 3; ++a) s[a] = o[a] - v0[a];
  const float sp = tdot(s, p);
  b1 = sp * inv;
  tcross(s, e1, q);
  const float dq = tdot(d, q);
  b2 = dq * inv;
  t = tdot(e2, q) * inv;
  sum = !MODEL_FMA ? b1 + b2 : alt ? std::fmaf(sp, inv, b2) : std::fmaf(dq, inv, b1);
}

// one triangle into a hit, the walk's form and the short one side by side
void fold(bool ok_full, bool ok_short, float t, float u, float v, uint32_t prim, float tmin, Hit& full, Hit& brief, Counts& c) {
  c.tests += 1;
  c.bary += ok_full != ok_short;
  if (nearest_accepts(ok_full, t, tmin, full.t, full.found, prim, full.prim)) full = Hit{t, u, v, prim, true};
  if (nearest_accepts_short(ok_short, t, tmin, brief.t, prim, brief.prim)) brief = Hit{t, u, v, prim, false};
  c.nearest += !same(full, brief);
  c.state += full.found != (brief.prim != kNoPrim);
}

}  // namespace

int main(int argc, char** argv) {
  const long cases = argc > 1 ? std::atol(argv[1]) : 1000000;
  const float inf = INFINITY, nan = std::numeric_limits<float>::quiet_NaN(), dmin = std::numeric_limits<float>::denorm_min(),
              nmin = std::numeric_limits<float>::min(), dmax = std::nextafter(nmin, 0.0f);
  const float below1 = std::nextafter(1.0f, 0.0f), above1 = std::nextafter(1.0f, 2.0f);
  const std::vector<float> S = {0.0f, -0.0f, dmin, -dmin, dmax, -dmax, nmin, -nmin, below1, 1.0f, above1, -below1, -1.0f,
                                -above1, 0.5f, 0.25f, 2.0f, -2.0f, 1e-3f, 3.0e38f, -3.0e38f, inf, -inf, nan};
  const std::vector<uint32_t> P = {0u, 1u, 5u, 0xFFFFu, 0x7FFFFFFEu};
  Counts A;
  // A1. the range test: (det, b1, b2) and b1 + b2
  for (float det : {1.0f, -1.0f, 0.0f, -0.0f, dmin, inf, nan})
    for (float x : S)
      for (float y : S) {
#if MODEL_FMA
        // b1 + b2 as one fma: (dq, inv, b1) with b2 = fl(dq inv), and (sp, inv, b2) with b1 = fl(sp inv)
        for (float z : S) {
          const float b2 = x * y, s1 = std::fmaf(x, y, z);
          A.tests += 2;
          A.bary += bary_inside(det, z, b2, s1) != bary_inside_short(det, z, b2, s1);
          const float b1 = x * y, s2 = std::fmaf(x, y, z);
          A.bary += bary_inside(det, b1, z, s2) != bary_inside_short(det, b1, z, s2);
        }
#else
        A.tests += 1;
        A.bary += bary_inside(det, x, y, x + y) != bary_inside_short(det, x, y, x + y);
#endif
      }
  // A2. the nearest rule, in every state the invariant allows
  for (int ok = 0; ok < 2; ++ok)
    for (float t : S)
      for (float tmin : {0.0f, -0.0f, 1e-3f})
        for (float ht : S)
          for (uint32_t prim : P)
            for (size_t k = 0; k <= P.size(); ++k) {
              const bool found = k < P.size();
              const uint32_t hprim = found ? P[k] : kNoPrim;
              A.tests += 1;
              A.nearest += nearest_accepts(ok != 0, t, tmin, ht, found, prim, hprim) !=
                           nearest_accepts_short(ok != 0, t, tmin, ht, prim, hprim);
            }
  // A3. the occlusion rule
  for (int ok = 0; ok < 2; ++ok)
    for (float t : S)
      for (float tmin : {0.0f, -0.0f, 1e-3f})
        for (float tT : S)
          for (uint32_t prim : P)
            for (uint32_t target : P) {
              A.tests += 1;
              A.occlusion += occlusion_accepts(ok != 0, t, tT, prim, target, tmin) != occludes(ok != 0, t, tmin, tT, prim, target);
            }
  // B. random rays and triangles
  Counts B;
  for (long n = 0; n < cases; ++n) {
    float tri[4][9];   // v0, e1, e2
    uint32_t prim[4];
    for (int k = 0; k < 2; ++k) {
      for (int a = 0; a < 9; ++a) tri[k][a] = 2.0f * rnd() - 1.0f;
      for (int a = 3; a < 9; ++a) tri[k][a] *= (n & 8) ? 1e-3f : 1.0f;   // small and slanted ones too
      std::memcpy(tri[k + 2], tri[k], sizeof(tri[k]));                    // a copy: the same t, another index
      prim[k] = (uint32_t)(rnd() * 60000.0f);
      prim[k + 2] = (uint32_t)(rnd() * 60000.0f);
    }
    // the ray: from a random origin at a point of triangle 0 — a vertex, an edge, or anywhere inside or near
    float o[3], d[3], w1 = rnd(), w2 = rnd();
    switch (n % 6) {
      case 0: w1 = 1.0f; w2 = 0.0f; break;            // v1: b1 = 1
      case 1: w1 = 0.0f; w2 = 1.0f; break;            // v2
      case 2: w1 = 0.0f; w2 = 0.0f; break;            // v0
      case 3: w2 = 1.0f - w1; break;                  // the edge b1 + b2 = 1
      case 4: w2 = 0.0f; w1 = 0.5f + 0.6f * w1; break;   // along b2 = 0, through and past b1 = 1
      default: break;
    }
    float len = 0.0f;
    for (int a = 0; a < 3; ++a) {
      o[a] = 2.0f * rnd() - 1.0f;
      d[a] = (tri[0][a] + w1 * tri[0][3 + a] + w2 * tri[0][6 + a]) - o[a];
      len += d[a] * d[a];
    }
    len = std::sqrt(len);
    if (!(len > 0.0f)) continue;
    for (int a = 0; a < 3; ++a) d[a] /= len;
    for (int alt = 0; alt < (MODEL_FMA ? 2 : 1); ++alt)
      for (int rev = 0; rev < 2; ++rev) {
        Hit full{inf, 0.0f, 0.0f, kNoPrim, false}, brief = full;
        bool ok[4];
        float ts[4];
        for (int i = 0; i < 4; ++i) {
          const int k = rev ? 3 - i : i;
          float det, b1, b2, sum;
          tri_terms(o, d, tri[k], tri[k] + 3, tri[k] + 6, alt != 0, det, b1, b2, sum, ts[k]);
          ok[k] = bary_inside(det, b1, b2, sum);
          fold(ok[k], bary_inside_short(det, b1, b2, sum), ts[k], (1.0f - b1) - b2, b1, prim[k], 0.0f, full, brief, B);
        }
        for (int k = 0; k < 4; ++k)       // the occluder
          for (int T = 0; T < 4; ++T)     // the target, at its own t (its copy: the tie)
            B.occlusion += occlusion_accepts(ok[k], ts[k], ts[T], prim[k], prim[T]) !=
                           occludes(ok[k], ts[k], 0.0f, ts[T], prim[k], prim[T]);
      }
  }
  std::printf("accept forms (fma %d): special tests %.0f bary %.0f nearest %.0f occlusion %.0f ; random cases %ld tests %.0f "
              "bary %.0f nearest %.0f state %.0f occlusion %.0f\n",
              (int)MODEL_FMA, A.tests, A.bary, A.nearest, A.occlusion, cases, B.tests, B.bary, B.nearest, B.state, B.occlusion);
  return 0;
}
