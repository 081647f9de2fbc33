// firefly.hip — the outlier clamp ahead of the variance-guided filter
// (mrt_firefly_clamp).  Definition: include/mrt.h "firefly suppression",
// DESIGN.md §2.1s.  A filterable pixel whose luminance lies above
//     cap = mean + k * standard deviation
// of the luminances of its window's taps on the same surface (same material
// word, normal and plane as in mrt_reproject) is scaled down to the cap; a
// window that holds a light pixel is left alone.  Energy is removed, not
// redistributed.  One kernel, modelled on the staged A-Trous iteration: a tile
// with its halo of R pixels staged in LDS, 32 B per pixel.  The tile is 32 x 32
// pixels of a 1024-thread block (32 x 16 of 512 threads at R = 3), not the
// filter's 32 x 8: every block adds its count to ONE word, and 8100 such
// atomics at 1920x1080 took longer than the rest of the kernel (§2.1s).
// Compiled once: FMA contraction, IEEE division and sqrt.
#include "firefly.h"

#include "dev_filter.h"

namespace mrt {
namespace {

constexpr int kTileW = 32;

// Three planes with contiguous rows, so that a wave's taps read consecutive
// records: (luminance, word), (normal, position.x), (position.y, position.z).
// A light pixel is staged with its word; every other pixel that cannot count
// as a tap or serve as a centre — outside the image, a miss, a non-finite
// colour — with the miss word, which no filterable centre matches and which is
// not a light's: a tap tests one word.  The centre's colour comes from global
// memory, everything else of it from its staged records (t_p from guide_p).
// R: the window's radius; TH: the tile's height (a thread a pixel, a wave two rows).
template <int R, int TH>
__global__ __launch_bounds__(kTileW * TH) void firefly_kernel(FireflyArgs a) {
  constexpr int kBlock = kTileW * TH;
  constexpr int RW = kTileW + 2 * R, RH = TH + 2 * R, RN = RW * RH;
  __shared__ float2 lds_l[RN];
  __shared__ float4 lds_n[RN];
  __shared__ float2 lds_p[RN];
  __shared__ uint32_t lds_count[kBlock / 64];
  const int W = (int)a.width, H = (int)a.height;
  const int x0 = (int)(blockIdx.x * (uint32_t)kTileW), y0 = (int)(blockIdx.y * (uint32_t)TH);
  for (int k = (int)threadIdx.x; k < RN; k += kBlock) {
    const int ly = k / RW, lx = k - ly * RW;
    const int gx = x0 - R + lx, gy = y0 - R + ly;
    float2 l = make_float2(0.0f, __uint_as_float(kMissWord));
    float4 n = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    float2 q = make_float2(0.0f, 0.0f);
    if (gx >= 0 && gx < W && gy >= 0 && gy < H) {
      const size_t j = (size_t)gy * a.width + (uint32_t)gx;
      const float4 qc = a.image[j], qn = a.guide_n[j], qp = a.guide_p[j];
      const uint32_t word = __float_as_uint(qn.w);
      if (word >= kNotFilterable) {
        if (is_light(word)) l.y = qn.w;
      } else if (finite3(qc.x, qc.y, qc.z)) {
        l = make_float2(lum(qc.x, qc.y, qc.z), qn.w);
      }
      n = make_float4(qn.x, qn.y, qn.z, qp.x);
      q = make_float2(qp.y, qp.z);
    }
    lds_l[k] = l;
    lds_n[k] = n;
    lds_p[k] = q;
  }
  __syncthreads();
  const int tx = (int)(threadIdx.x & 31u), ty = (int)(threadIdx.x >> 5);
  const int x = x0 + tx, y = y0 + ty;
  bool changed = false;
  if (x < W && y < H) {   // no thread leaves before the barrier below
    const size_t i = (size_t)y * a.width + (uint32_t)x;
    float4 c = a.image[i];
    const int lc = (ty + R) * RW + tx + R;   // the centre's staged record; taps stay inside [0, RN)
    const float2 pl = lds_l[lc];
    const uint32_t word = __float_as_uint(pl.y);
    if (word < kNotFilterable && pl.x > 0.0f) {   // (a): filterable, finite (else staged as a miss), l_p > 0
      const float4 pn = lds_n[lc];
      const float2 pp = lds_p[lc];
      const float tol = a.plane_tolerance * a.guide_p[i].w;
      float s1 = 0.0f, s2 = 0.0f;
      uint32_t taps = 0;
      bool light = false;
#pragma unroll
      for (int dy = -R; dy <= R; ++dy) {
#pragma unroll
        for (int dx = -R; dx <= R; ++dx) {
          if (dy == 0 && dx == 0) continue;
          const int k = lc + dy * RW + dx;
          const float2 ql = lds_l[k];
          const uint32_t qw = __float_as_uint(ql.y);
          light |= is_light(qw);
          if (qw != word) continue;
          const float4 qn = lds_n[k];
          const float2 qp = lds_p[k];
          const float D = normal_dot(pn.x, pn.y, pn.z, qn.x, qn.y, qn.z);
          const float dist = plane_distance(pn.x, pn.y, pn.z, pn.w, pp.x, pp.y, qn.w, qp.x, qp.y);
          if (D >= a.normal_cos_min && dist <= tol) {   // false for a NaN guide value
            ++taps;
            s1 += ql.x;
            s2 += ql.x * ql.x;
          }
        }
      }
      if (!light && taps >= a.min_taps) {
        const float fn = (float)taps;
        const float m = s1 / fn;                                   // IEEE division and sqrt (Makefile)
        const float var = fmaxf(0.0f, s2 / fn - m * m);
        const float cap = m + a.k * sqrtf(var);
        if (pl.x > cap) {
          const float scale = cap / pl.x;
          const float r = c.x * scale, g = c.y * scale, b = c.z * scale;
          changed = __float_as_uint(r) != __float_as_uint(c.x) || __float_as_uint(g) != __float_as_uint(c.y) ||
                    __float_as_uint(b) != __float_as_uint(c.z);
          c.x = r;
          c.y = g;
          c.z = b;
        }
      }
    }
    a.out[i] = c;
  }
  if (a.clamped) {   // uniform: a popcount per wave, one atomic per block
    const uint32_t n = (uint32_t)__popcll(__ballot(changed));
    if ((threadIdx.x & 63u) == 0) lds_count[threadIdx.x >> 6] = n;
    __syncthreads();
    if (threadIdx.x == 0) {
      uint32_t total = 0;
      for (int w = 0; w < kBlock / 64; ++w) total += lds_count[w];
      if (total) atomicAdd(a.clamped, total);
    }
  }
}

template <int R, int TH>
void launch(const FireflyArgs& a, hipStream_t s) {
  const dim3 g((a.width + kTileW - 1) / kTileW, (a.height + TH - 1) / TH);
  firefly_kernel<R, TH><<<g, dim3(kTileW * TH), 0, s>>>(a);
}

}  // namespace

// Tile heights measured at 1920x1080 (tools/firefly_time.py):
// 32 rows are the fastest at R = 1 and 2; at R = 3 the kernel's 76 VGPRs leave
// one 1024-thread block to a CU, and 16 rows are faster.
hipError_t launch_firefly(const FireflyArgs& a, hipStream_t s) {
  if (a.width == 0 || a.height == 0 || a.radius < 1 || a.radius > 3) return hipErrorInvalidValue;
  if (a.radius == 1) launch<1, 32>(a, s);
  else if (a.radius == 2) launch<2, 32>(a, s);
  else launch<3, 16>(a, s);
  return hipGetLastError();
}

}  // namespace mrt
