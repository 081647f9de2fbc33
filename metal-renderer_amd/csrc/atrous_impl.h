// atrous_impl.h — one iteration of an edge-avoiding A-Trous filter over the
// first-hit guide planes, written once for the filters that share it: the plain
// one (denoise.hip) and the variance-guided one (variance.hip).  With step s,
//
//   a pixel p with word_p >= kNotFilterable (miss, light) keeps its value;
//   otherwise over (dx, dy) in {-2..2}^2, q = p + s (dx, dy), a tap counts iff
//   q is inside the image, word_q == word_p and c_q is finite, with weight
//     w = k[dx+2] k[dy+2] * max(0, n_p.n_q)^(2^e)
//           * exp(-|n_p.(x_q - x_p)| / (sigma_plane t_p)) * exp(-colour term)
//   (the colour term is 0 where the filter's centre says it does not apply), and
//   c'_p = sum w c_q / sum w (c_p if the sum is 0).
//
// A filter is a policy struct F that supplies what differs:
//   Args               the kernel's arguments; guide_n, guide_p, width, height,
//                      step, sigma_plane and normal_log2_power by those names
//   src(a)             the image c^i
//   Centre             SurfaceCentre + what the colour term needs of the centre
//   colour(a, c, g, p) fills those fields and p.colour (does the term apply)
//   colour_term(p, r, g, b, l)   the exponent's colour term of a tap: its colour, its luminance
//   store(a, i, r, g, b, alpha, v)   the result to its place
//   kStagedAutoSteps   the steps the staged kernel serves under kAtrousAuto (bit i = step 2^i)
//   kVariance          the filter carries a variance v beside the colour:
//     variance(a, j) is v_j, variance(a, j, w) the same where w = src(a)[j].w is at hand;
//     g_p, the 3x3 (1/4, 1/2, 1/4)^2 average of v around p (offsets of one
//     pixel, taps inside the image, renormalised), goes to colour();
//     v'_p = sum w^2 v_q / (sum w)^2 (v_p if the sum is 0) goes to store().
//
// Two implementations of an iteration: every tap from global memory (the tap
// offset is wave-uniform, so each tap is a coalesced 16-B-per-lane load), and
// a 32x8 tile with its halo of 2s pixels staged once in LDS (steps 1, 2, 4).
// The including unit is compiled with FMA contraction and native exp, IEEE
// division and sqrt (Makefile).
#pragma once
#include <type_traits>

#include "denoise.h"
#include "dev_filter.h"

namespace mrt {
namespace {

constexpr int kBlock = 256;

struct SurfaceCentre {
  float nx, ny, nz;
  float px, py, pz;
  float inv_plane;   // 1 / (sigma_plane t_p)
  bool colour;       // the colour term applies
  uint32_t e;
};

struct Sum {
  float w, r, g, b;
  float v;   // sum w^2 v_q (F::kVariance)
};

template <class F>
__device__ __forceinline__ typename F::Centre make_centre(const typename F::Args& a, const float4& c, const float4& n,
                                                          const float4& x, float g) {
  typename F::Centre p;
  p.nx = n.x; p.ny = n.y; p.nz = n.z;
  p.px = x.x; p.py = x.y; p.pz = x.z;
  p.inv_plane = inv_plane(a.sigma_plane, x.w);
  p.e = a.normal_log2_power;
  F::colour(a, c, g, p);
  return p;
}

// ql, qv: the tap's luminance and variance (read only where F uses them)
template <class F>
__device__ __forceinline__ void add_tap(const typename F::Centre& p, float k, float qnx, float qny, float qnz, float qpx,
                                        float qpy, float qpz, float qcx, float qcy, float qcz, float ql, float qv,
                                        Sum& s) {
  const float D = normal_weight(normal_dot(p.nx, p.ny, p.nz, qnx, qny, qnz), p.e);
  const float dist = plane_distance(p.nx, p.ny, p.nz, p.px, p.py, p.pz, qpx, qpy, qpz);
  const float term = F::colour_term(p, qcx, qcy, qcz, ql);
  const float arg = dist * p.inv_plane + (p.colour ? term : 0.0f);
  const float w = (k * D) * __expf(-arg);
  s.w += w;
  s.r += w * qcx;
  s.g += w * qcy;
  s.b += w * qcz;
  if constexpr (F::kVariance) s.v += (w * w) * qv;
}

template <class F>
__device__ __forceinline__ void keep(const typename F::Args& a, size_t i, const float4& c, float vp) {
  F::store(a, i, c.x, c.y, c.z, c.w, vp);
}

template <class F>
__device__ __forceinline__ void resolve(const typename F::Args& a, size_t i, const Sum& s, const float4& c, float vp) {
  if (!(s.w > 0.0f)) { keep<F>(a, i, c, vp); return; }
  F::store(a, i, s.r / s.w, s.g / s.w, s.b / s.w, c.w, (s.v / s.w) / s.w);   // IEEE division (Makefile)
}

// Direct version: pixel_64x4; no clamped address is read.
template <class F>
__global__ __launch_bounds__(kBlock) void atrous_direct_kernel(typename F::Args a) {
  const int W = (int)a.width, H = (int)a.height, s = (int)a.step;
  int x, y;
  size_t i;
  if (!pixel_64x4(a.width, a.height, x, y, i)) return;
  const float4* src = F::src(a);
  const float4 c = src[i], n = a.guide_n[i];
  float vp = 0.0f;
  if constexpr (F::kVariance) vp = F::variance(a, i, c.w);
  const uint32_t word = __float_as_uint(n.w);
  if (word >= kNotFilterable) { keep<F>(a, i, c, vp); return; }
  float g = 0.0f;
  if constexpr (F::kVariance) {
    float gw = 0.0f, gv = 0.0f;
#pragma unroll
    for (int dy = -1; dy <= 1; ++dy) {
      const int yy = y + dy;
      if (yy < 0 || yy >= H) continue;
#pragma unroll
      for (int dx = -1; dx <= 1; ++dx) {
        const int xx = x + dx;
        if (xx < 0 || xx >= W) continue;
        const size_t j = (size_t)yy * a.width + (uint32_t)xx;
        const float k = hat(dx) * hat(dy);
        gw += k;
        gv += k * F::variance(a, j);
      }
    }
    g = gv / gw;
  }
  const typename F::Centre p = make_centre<F>(a, c, n, a.guide_p[i], g);
  Sum sum{0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
  for (int dy = -2; dy <= 2; ++dy) {
    const int yy = y + dy * s;
    if (yy < 0 || yy >= H) continue;
#pragma unroll
    for (int dx = -2; dx <= 2; ++dx) {
      const int xx = x + dx * s;
      if (xx < 0 || xx >= W) continue;
      const size_t j = (size_t)yy * a.width + (uint32_t)xx;
      const float4 qn = a.guide_n[j];
      if (__float_as_uint(qn.w) != word) continue;
      const float4 qc = src[j];
      if (!finite3(qc.x, qc.y, qc.z)) continue;
      const float4 qp = a.guide_p[j];
      float qv = 0.0f;
      if constexpr (F::kVariance) qv = F::variance(a, j, qc.w);
      add_tap<F>(p, kern(dx) * kern(dy), qn.x, qn.y, qn.z, qp.x, qp.y, qp.z, qc.x, qc.y, qc.z, lum(qc.x, qc.y, qc.z), qv,
                 sum);
    }
  }
  resolve<F>(a, i, sum, c, vp);
}

// Staged version for step S: the block's 32 x 8 tile and its halo of 2S pixels
// are staged once in three planes whose rows are contiguous (consecutive lanes
// read consecutive records: no bank conflict) — (colour, word), (normal,
// position.x), (position.y, position.z) and, where F::kVariance, (variance,
// luminance) in the same record: 40 or 48 B per pixel.  A pixel outside the
// image or with a non-finite colour is staged with the miss word, which no
// filterable centre matches; its variance is staged all the same (0 outside
// the image), for the 3x3 average, whose taps are chosen by their coordinates.
// The centre's own records come from global memory (its colour may be
// non-finite, and t and alpha are not staged).
constexpr int kTileW = 32, kTileH = 8;
template <class F, int S>
__global__ __launch_bounds__(kBlock) void atrous_staged_kernel(typename F::Args a) {
  using Third = std::conditional_t<F::kVariance, float4, float2>;
  constexpr int RW = kTileW + 4 * S, RH = kTileH + 4 * S, R = RW * RH;
  __shared__ float4 lds_c[R];
  __shared__ float4 lds_n[R];
  __shared__ Third lds_p[R];
  const int W = (int)a.width, H = (int)a.height;
  const int x0 = (int)(blockIdx.x * (uint32_t)kTileW), y0 = (int)(blockIdx.y * (uint32_t)kTileH);
  const float4* src = F::src(a);
  for (int k = (int)threadIdx.x; k < R; k += kBlock) {
    const int ly = k / RW, lx = k - ly * RW;
    const int gx = x0 - 2 * S + lx, gy = y0 - 2 * S + ly;
    float4 c = make_float4(0.0f, 0.0f, 0.0f, __uint_as_float(kMissWord));
    float4 n = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    Third q{};
    if (gx >= 0 && gx < W && gy >= 0 && gy < H) {
      const size_t j = (size_t)gy * a.width + (uint32_t)gx;
      const float4 qc = src[j], qn = a.guide_n[j], qp = a.guide_p[j];
      // (the three loads issue before anything waits for one: left alone, the scheduler starts the plain
      // filter's guide_n load only after the colour has arrived, two round trips a record)
      __builtin_amdgcn_sched_barrier(0);
      float qv = 0.0f, l = 0.0f;
      if constexpr (F::kVariance) qv = F::variance(a, j, qc.w);
      // (selects, not a branch: into a branch the compiler sinks qn.w's part of the guide record's load)
      const bool finite = finite3(qc.x, qc.y, qc.z);
      c = make_float4(finite ? qc.x : 0.0f, finite ? qc.y : 0.0f, finite ? qc.z : 0.0f, finite ? qn.w : c.w);
      l = finite ? lum(qc.x, qc.y, qc.z) : 0.0f;
      n = make_float4(qn.x, qn.y, qn.z, qp.x);
      if constexpr (F::kVariance) q = make_float4(qp.y, qp.z, qv, l);
      else q = make_float2(qp.y, qp.z);
    }
    lds_c[k] = c;
    lds_n[k] = n;
    lds_p[k] = q;
  }
  __syncthreads();
  const int tx = (int)(threadIdx.x & 31u), ty = (int)(threadIdx.x >> 5);
  const int x = x0 + tx, y = y0 + ty;
  if (x >= W || y >= H) return;
  const size_t i = (size_t)y * a.width + (uint32_t)x;
  const float4 c = src[i], n = a.guide_n[i];
  float vp = 0.0f;
  if constexpr (F::kVariance) vp = F::variance(a, i, c.w);
  const uint32_t word = __float_as_uint(n.w);
  if (word >= kNotFilterable) { keep<F>(a, i, c, vp); return; }
  const int lc = (ty + 2 * S) * RW + tx + 2 * S;   // the centre's staged record; taps stay inside [0, R)
  float g = 0.0f;
  if constexpr (F::kVariance) {
    float gw = 0.0f, gv = 0.0f;
#pragma unroll
    for (int dy = -1; dy <= 1; ++dy) {
      if (y + dy < 0 || y + dy >= H) continue;
#pragma unroll
      for (int dx = -1; dx <= 1; ++dx) {
        if (x + dx < 0 || x + dx >= W) continue;
        const float k = hat(dx) * hat(dy);
        gw += k;
        gv += k * lds_p[lc + dy * RW + dx].z;
      }
    }
    g = gv / gw;
  }
  const typename F::Centre p = make_centre<F>(a, c, n, a.guide_p[i], g);
  Sum sum{0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
  for (int dy = -2; dy <= 2; ++dy) {
#pragma unroll
    for (int dx = -2; dx <= 2; ++dx) {
      const int k = lc + dy * S * RW + dx * S;
      const float4 qc = lds_c[k];
      if (__float_as_uint(qc.w) != word) continue;
      const float4 qn = lds_n[k];
      const Third qp = lds_p[k];
      float ql = 0.0f, qv = 0.0f;
      if constexpr (F::kVariance) {
        qv = qp.z;
        ql = qp.w;
      }
      add_tap<F>(p, kern(dx) * kern(dy), qn.x, qn.y, qn.z, qn.w, qp.x, qp.y, qc.x, qc.y, qc.z, ql, qv, sum);
    }
  }
  resolve<F>(a, i, sum, c, vp);
}

template <class F>
hipError_t launch_filter(const typename F::Args& a, uint32_t path, hipStream_t s) {
  if (a.width == 0 || a.height == 0 || a.step == 0 || (a.step & (a.step - 1))) return hipErrorInvalidValue;
  const bool staged = a.step <= kAtrousStagedMaxStep &&
                      (path == kAtrousStaged || (path == kAtrousAuto && (F::kStagedAutoSteps & a.step)));
  if (staged) {
    const dim3 g((a.width + kTileW - 1) / kTileW, (a.height + kTileH - 1) / kTileH);
    if (a.step == 1) atrous_staged_kernel<F, 1><<<g, dim3(kBlock), 0, s>>>(a);
    else if (a.step == 2) atrous_staged_kernel<F, 2><<<g, dim3(kBlock), 0, s>>>(a);
    else atrous_staged_kernel<F, 4><<<g, dim3(kBlock), 0, s>>>(a);
  } else {
    atrous_direct_kernel<F><<<grid_64x4(a.width, a.height), dim3(kBlock), 0, s>>>(a);
  }
  return hipGetLastError();
}

}  // namespace
}  // namespace mrt
