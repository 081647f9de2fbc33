// variance.hip — the spatial half of SVGF (Schied et al., HPG 2017) over the
// luminance moments the renderer accumulates beside its image: the per-pixel
// variance estimate (mrt_variance) and the edge-avoiding A-Trous filter whose
// colour term it steers (mrt_denoise_variance).  Definitions: include/mrt.h
// "variance-guided denoising", DESIGN.md §2.1p.  The filter is denoise.hip's
// with two changes — the colour weight is
//     exp(-|lum(c_q) - lum(c_p)| / (sigma_l sqrt(g_p) + 1e-6))   (1 if c_p is not finite)
// with g_p the 3x3 (1/4, 1/2, 1/4)^2 average of the current variance around p
// (offsets of one pixel, taps inside the image, renormalised), and the variance
// is filtered with the colour: v'_p = sum w^2 v_q / (sum w)^2.  Between
// iterations v travels in the fourth channel of the ping-pong images, so a tap
// stays one 16-B load.  Two implementations of an iteration, as in denoise.hip:
// every tap from global memory, and a 32x8 tile with its halo of 2s pixels
// staged in LDS (steps 1, 2, 4; the 3x3 variance taps come from the same tile).
// Compiled once: FMA contraction and native exp, IEEE division and sqrt.
#include "variance.h"

#include "denoise.h"

namespace mrt {
namespace {

constexpr int kBlock = 256;
constexpr uint32_t kNotFilterable = 0x80000000u;

__device__ __forceinline__ bool finite1(float x) { return (__float_as_uint(x) & 0x7F800000u) != 0x7F800000u; }
__device__ __forceinline__ bool finite3(float x, float y, float z) { return finite1(x) && finite1(y) && finite1(z); }

__device__ __forceinline__ float kern(int d) {   // (1/16, 1/4, 3/8, 1/4, 1/16)[d + 2]
  return d == 0 ? 0.375f : ((d == 1 || d == -1) ? 0.25f : 0.0625f);
}
__device__ __forceinline__ float hat(int d) { return d == 0 ? 0.5f : 0.25f; }   // (1/4, 1/2, 1/4)[d + 1]
__device__ __forceinline__ float lum(float r, float g, float b) { return (0.2126f * r + 0.7152f * g) + 0.0722f * b; }

__device__ __forceinline__ float normal_weight(float D, uint32_t e) {   // max(0, D)^(2^e)
  D = fmaxf(0.0f, D);
  for (uint32_t j = 0; j < e; ++j) D *= D;
  return D;
}

// ---------------------------------------------------------------------------
// mrt_variance: a block is 64 x 4 pixels, a wave one row of 64 — a tap row
// outside the image is skipped by the whole wave, a tap column by its lanes
// ---------------------------------------------------------------------------
__device__ __forceinline__ bool usable(const float4& m) { return finite1(m.x) && finite1(m.y) && m.w > 0.0f; }

__global__ __launch_bounds__(kBlock) void variance_kernel(VarianceArgs a) {
  const int W = (int)a.width, H = (int)a.height;
  const int x = (int)(blockIdx.x * 64u + (threadIdx.x & 63u)), y = (int)(blockIdx.y * 4u + (threadIdx.x >> 6));
  if (x >= W || y >= H) return;
  const size_t i = (size_t)y * a.width + (uint32_t)x;
  const float4 n = a.guide_n[i];
  const uint32_t word = __float_as_uint(n.w);
  if (word >= kNotFilterable) { a.variance[i] = 0.0f; return; }
  const float4 m = a.moments[i];
  float r;
  if (usable(m) && m.w >= a.min_frames) {   // the pixel's own history is long enough: temporal
    r = fmaxf(0.0f, m.y - m.x * m.x) / (m.w - 1.0f);
  } else {                                  // else its 7x7 neighbourhood on the same surface
    const float4 xp = a.guide_p[i];
    const float inv_plane = 1.0f / (a.sigma_plane * xp.w);
    float sw = 0.0f, s1 = 0.0f, s2 = 0.0f;
    for (int dy = -3; dy <= 3; ++dy) {
      const int yy = y + dy;
      if (yy < 0 || yy >= H) continue;
      for (int dx = -3; dx <= 3; ++dx) {
        const int xx = x + dx;
        if (xx < 0 || xx >= W) continue;
        const size_t j = (size_t)yy * a.width + (uint32_t)xx;
        const float4 qn = a.guide_n[j];
        if (__float_as_uint(qn.w) != word) continue;
        const float4 qm = a.moments[j];
        if (!usable(qm)) continue;
        const float4 qp = a.guide_p[j];
        const float D = normal_weight((n.x * qn.x + n.y * qn.y) + n.z * qn.z, a.normal_log2_power);
        const float dist = fabsf((n.x * (qp.x - xp.x) + n.y * (qp.y - xp.y)) + n.z * (qp.z - xp.z));
        const float w = (D * __expf(-(dist * inv_plane))) * qm.w;
        sw += w;
        s1 += w * qm.x;
        s2 += w * qm.y;
      }
    }
    r = 0.0f;
    if (sw > 0.0f) {
      const float a1 = s1 / sw, a2 = s2 / sw;
      r = fmaxf(0.0f, a2 - a1 * a1) / fmaxf(m.w, 1.0f);
    }
  }
  a.variance[i] = (r >= 0.0f && finite1(r)) ? r : 0.0f;   // never negative, never non-finite
}

// ---------------------------------------------------------------------------
// the filter
// ---------------------------------------------------------------------------
struct Centre {
  float nx, ny, nz;
  float px, py, pz;
  float l;           // lum(c_p)
  float inv_plane;   // 1 / (sigma_plane t_p)
  float inv_l;       // 1 / (sigma_l sqrt(g_p) + 1e-6)
  bool colour;       // the luminance term applies (c_p finite)
  uint32_t e;
};

struct Sum {
  float w, r, g, b, v;
};

__device__ __forceinline__ void add_tap(const Centre& p, float k, float qnx, float qny, float qnz, float qpx, float qpy,
                                        float qpz, float qcx, float qcy, float qcz, float ql, float qv, Sum& s) {
  const float D = normal_weight((p.nx * qnx + p.ny * qny) + p.nz * qnz, p.e);
  const float dist = fabsf((p.nx * (qpx - p.px) + p.ny * (qpy - p.py)) + p.nz * (qpz - p.pz));
  const float arg = dist * p.inv_plane + (p.colour ? fabsf(ql - p.l) * p.inv_l : 0.0f);
  const float w = (k * D) * __expf(-arg);
  s.w += w;
  s.r += w * qcx;
  s.g += w * qcy;
  s.b += w * qcz;
  s.v += (w * w) * qv;
}

__device__ __forceinline__ Centre make_centre(const SvgfArgs& a, const float4& c, const float4& n, const float4& x,
                                              float g) {
  Centre p;
  p.nx = n.x; p.ny = n.y; p.nz = n.z;
  p.px = x.x; p.py = x.y; p.pz = x.z;
  p.l = lum(c.x, c.y, c.z);
  p.inv_plane = 1.0f / (a.sigma_plane * x.w);
  p.inv_l = 1.0f / (a.sigma_luminance * sqrtf(fmaxf(g, 0.0f)) + 1e-6f);
  p.colour = finite3(c.x, c.y, c.z);
  p.e = a.normal_log2_power;
  return p;
}

// c^(i+1)_p and v^(i+1)_p to their places: the variance in the fourth channel,
// or (last iteration) the image's alpha there and the variance in its plane
__device__ __forceinline__ void store(const SvgfArgs& a, size_t i, float r, float g, float b, float v) {
  a.dst[i] = make_float4(r, g, b, a.alpha ? a.alpha[i].w : v);
  if (a.var_out) a.var_out[i] = v;
}

__device__ __forceinline__ void resolve(const SvgfArgs& a, size_t i, const Sum& s, const float4& c, float vp) {
  if (!(s.w > 0.0f)) { store(a, i, c.x, c.y, c.z, vp); return; }
  store(a, i, s.r / s.w, s.g / s.w, s.b / s.w, (s.v / s.w) / s.w);   // IEEE division (Makefile)
}

__global__ __launch_bounds__(kBlock) void svgf_direct_kernel(SvgfArgs a) {
  const int W = (int)a.width, H = (int)a.height, s = (int)a.step;
  const int x = (int)(blockIdx.x * 64u + (threadIdx.x & 63u)), y = (int)(blockIdx.y * 4u + (threadIdx.x >> 6));
  if (x >= W || y >= H) return;
  const size_t i = (size_t)y * a.width + (uint32_t)x;
  const float4 c = a.src[i], n = a.guide_n[i];
  const float vp = a.var_in ? a.var_in[i] : c.w;
  const uint32_t word = __float_as_uint(n.w);
  if (word >= kNotFilterable) { store(a, i, c.x, c.y, c.z, vp); return; }
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
      gv += k * (a.var_in ? a.var_in[j] : a.src[j].w);
    }
  }
  const Centre p = make_centre(a, c, n, a.guide_p[i], gv / gw);
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
      const float4 qc = a.src[j];
      if (!finite3(qc.x, qc.y, qc.z)) continue;
      const float4 qp = a.guide_p[j];
      const float qv = a.var_in ? a.var_in[j] : qc.w;
      add_tap(p, kern(dx) * kern(dy), qn.x, qn.y, qn.z, qp.x, qp.y, qp.z, qc.x, qc.y, qc.z, lum(qc.x, qc.y, qc.z), qv,
              sum);
    }
  }
  resolve(a, i, sum, c, vp);
}

// Staged version for step S: the block's 32 x 8 tile and its halo of 2S pixels,
// 48 B per pixel in three planes of 16-B records — (colour, word), (normal,
// position.x), (position.y, position.z, variance, luminance).  A pixel outside
// the image or with a non-finite colour is staged with word ~0u, which no
// filterable centre matches; its variance is staged all the same (0 outside the
// image), for the 3x3 average, whose taps are chosen by their coordinates.  The
// centre's own records come from global memory.
constexpr int kTileW = 32, kTileH = 8;
template <int S>
__global__ __launch_bounds__(kBlock) void svgf_staged_kernel(SvgfArgs a) {
  constexpr int RW = kTileW + 4 * S, RH = kTileH + 4 * S, R = RW * RH;
  __shared__ float4 lds_c[R];
  __shared__ float4 lds_n[R];
  __shared__ float4 lds_p[R];
  const int W = (int)a.width, H = (int)a.height;
  const int x0 = (int)(blockIdx.x * (uint32_t)kTileW), y0 = (int)(blockIdx.y * (uint32_t)kTileH);
  for (int k = (int)threadIdx.x; k < R; k += kBlock) {
    const int ly = k / RW, lx = k - ly * RW;
    const int gx = x0 - 2 * S + lx, gy = y0 - 2 * S + ly;
    float4 c = make_float4(0.0f, 0.0f, 0.0f, __uint_as_float(0xFFFFFFFFu));
    float4 n = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    float4 q = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    if (gx >= 0 && gx < W && gy >= 0 && gy < H) {
      const size_t j = (size_t)gy * a.width + (uint32_t)gx;
      const float4 qc = a.src[j], qn = a.guide_n[j], qp = a.guide_p[j];
      const float qv = a.var_in ? a.var_in[j] : qc.w;
      float l = 0.0f;
      if (finite3(qc.x, qc.y, qc.z)) {
        c = make_float4(qc.x, qc.y, qc.z, qn.w);
        l = lum(qc.x, qc.y, qc.z);
      }
      n = make_float4(qn.x, qn.y, qn.z, qp.x);
      q = make_float4(qp.y, qp.z, qv, l);
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
  const float4 c = a.src[i], n = a.guide_n[i];
  const float vp = a.var_in ? a.var_in[i] : c.w;
  const uint32_t word = __float_as_uint(n.w);
  if (word >= kNotFilterable) { store(a, i, c.x, c.y, c.z, vp); return; }
  const int lc = (ty + 2 * S) * RW + tx + 2 * S;   // the centre's staged record; taps stay inside [0, R)
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
  const Centre p = make_centre(a, c, n, a.guide_p[i], gv / gw);
  Sum sum{0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
  for (int dy = -2; dy <= 2; ++dy) {
#pragma unroll
    for (int dx = -2; dx <= 2; ++dx) {
      const int k = lc + dy * S * RW + dx * S;
      const float4 qc = lds_c[k];
      if (__float_as_uint(qc.w) != word) continue;
      const float4 qn = lds_n[k];
      const float4 qp = lds_p[k];
      add_tap(p, kern(dx) * kern(dy), qn.x, qn.y, qn.z, qn.w, qp.x, qp.y, qc.x, qc.y, qc.z, qp.w, qp.z, sum);
    }
  }
  resolve(a, i, sum, c, vp);
}

// Steps the staged path serves under kAtrousAuto (bit i = step 2^i).  Measured
// at 1920x1080, alternating in one call (tools/variance_time.py, DESIGN.md
// §2.1p): staged / direct 0.392 at step 1, 0.473 at step 2, 0.944 at step 4,
// spread at most 0.18 %.
constexpr uint32_t kStagedAutoSteps = 1u | 2u | 4u;

}  // namespace

hipError_t launch_variance(const VarianceArgs& a, hipStream_t s) {
  if (a.width == 0 || a.height == 0) return hipErrorInvalidValue;
  const dim3 g((a.width + 63) / 64, (a.height + 3) / 4);
  variance_kernel<<<g, dim3(kBlock), 0, s>>>(a);
  return hipGetLastError();
}

hipError_t launch_svgf_atrous(const SvgfArgs& a, uint32_t path, hipStream_t s) {
  if (a.width == 0 || a.height == 0 || a.step == 0 || (a.step & (a.step - 1))) return hipErrorInvalidValue;
  const bool staged = a.step <= kAtrousStagedMaxStep &&
                      (path == kAtrousStaged || (path == kAtrousAuto && (kStagedAutoSteps & a.step)));
  if (staged) {
    const dim3 g((a.width + kTileW - 1) / kTileW, (a.height + kTileH - 1) / kTileH);
    if (a.step == 1) svgf_staged_kernel<1><<<g, dim3(kBlock), 0, s>>>(a);
    else if (a.step == 2) svgf_staged_kernel<2><<<g, dim3(kBlock), 0, s>>>(a);
    else svgf_staged_kernel<4><<<g, dim3(kBlock), 0, s>>>(a);
  } else {
    const dim3 g((a.width + 63) / 64, (a.height + 3) / 4);
    svgf_direct_kernel<<<g, dim3(kBlock), 0, s>>>(a);
  }
  return hipGetLastError();
}

}  // namespace mrt
