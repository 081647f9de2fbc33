// denoise.hip — edge-avoiding A-Trous wavelet filter (Dammertz, Sewtz, Hanika,
// Lensch, HPG 2010) over the accumulation image, driven by the first-hit guide
// planes of kernels.hip guide_kernel.  One launch per iteration i, step
// s = 2^i; the definition (DESIGN.md "Denoised output"):
//
//   a pixel p with word_p >= 0x80000000 (miss, light) keeps its value;
//   otherwise over (dx, dy) in {-2..2}^2, q = p + s (dx, dy), a tap counts iff
//   q is inside the image, word_q == word_p and c_q is finite, with weight
//     k[dx+2] k[dy+2] * max(0, n_p.n_q)^(2^e)
//       * exp(-|n_p.(x_q - x_p)| / (sigma_plane t_p))
//       * exp(-|c_q - c_p|^2 / sigma_c^2)      (1 if sigma_c == 0 or c_p is not finite)
//   and c'_p = sum w c_q / sum w (c_p if the sum is 0); alpha is copied.
//
// Two implementations of an iteration: every tap from global memory (the tap
// offset is wave-uniform, so each tap is a coalesced 16-B-per-lane load), and
// a 32x8 tile with its halo of 2s pixels staged once in LDS (steps 1, 2, 4,
// where it measured faster).  Compiled once: FMA contraction and native exp as
// the fast build, IEEE division.
#include "denoise.h"

namespace mrt {
namespace {

constexpr int kBlock = 256;
constexpr uint32_t kNotFilterable = 0x80000000u;

__device__ __forceinline__ bool finite3(float x, float y, float z) {
  const uint32_t m = 0x7F800000u;
  return (__float_as_uint(x) & m) != m && (__float_as_uint(y) & m) != m && (__float_as_uint(z) & m) != m;
}

__device__ __forceinline__ float kern(int d) {   // (1/16, 1/4, 3/8, 1/4, 1/16)[d + 2]
  return d == 0 ? 0.375f : ((d == 1 || d == -1) ? 0.25f : 0.0625f);
}

struct Centre {
  float cx, cy, cz;
  float nx, ny, nz;
  float px, py, pz;
  float inv_plane;   // 1 / (sigma_plane t_p)
  float inv_c2;      // 1 / sigma_c^2
  bool colour;       // the colour term applies (sigma_c > 0 and c_p finite)
  uint32_t e;
};

struct Sum {
  float w, r, g, b;
};

__device__ __forceinline__ void add_tap(const Centre& p, float k, float qnx, float qny, float qnz, float qpx, float qpy,
                                        float qpz, float qcx, float qcy, float qcz, Sum& s) {
  float D = fmaxf(0.0f, (p.nx * qnx + p.ny * qny) + p.nz * qnz);
  for (uint32_t j = 0; j < p.e; ++j) D *= D;
  const float dist = fabsf((p.nx * (qpx - p.px) + p.ny * (qpy - p.py)) + p.nz * (qpz - p.pz));
  const float dx = qcx - p.cx, dy = qcy - p.cy, dz = qcz - p.cz;
  const float d2 = (dx * dx + dy * dy) + dz * dz;
  const float arg = dist * p.inv_plane + (p.colour ? d2 * p.inv_c2 : 0.0f);
  const float w = (k * D) * __expf(-arg);
  s.w += w;
  s.r += w * qcx;
  s.g += w * qcy;
  s.b += w * qcz;
}

__device__ __forceinline__ Centre make_centre(const AtrousArgs& a, const float4& c, const float4& n, const float4& x) {
  Centre p;
  p.cx = c.x; p.cy = c.y; p.cz = c.z;
  p.nx = n.x; p.ny = n.y; p.nz = n.z;
  p.px = x.x; p.py = x.y; p.pz = x.z;
  p.inv_plane = 1.0f / (a.sigma_plane * x.w);
  p.inv_c2 = a.inv_sigma_c2;
  p.colour = a.inv_sigma_c2 > 0.0f && finite3(c.x, c.y, c.z);
  p.e = a.normal_log2_power;
  return p;
}

__device__ __forceinline__ float4 resolve(const Sum& s, const float4& c) {
  if (!(s.w > 0.0f)) return c;
  return make_float4(s.r / s.w, s.g / s.w, s.b / s.w, c.w);   // IEEE division (Makefile)
}

// Direct version: a block is 64 x 4 pixels, a wave one row of 64 — a tap row
// outside the image is skipped by the whole wave, a tap column by its lanes;
// no clamped address is read.
__global__ __launch_bounds__(kBlock) void atrous_direct_kernel(AtrousArgs a) {
  const int W = (int)a.width, H = (int)a.height, s = (int)a.step;
  const int x = (int)(blockIdx.x * 64u + (threadIdx.x & 63u)), y = (int)(blockIdx.y * 4u + (threadIdx.x >> 6));
  if (x >= W || y >= H) return;
  const size_t i = (size_t)y * a.width + (uint32_t)x;
  const float4 c = a.image[i], n = a.guide_n[i];
  const uint32_t word = __float_as_uint(n.w);
  if (word >= kNotFilterable) { a.out[i] = c; return; }
  const Centre p = make_centre(a, c, n, a.guide_p[i]);
  Sum sum{0.0f, 0.0f, 0.0f, 0.0f};
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
      const float4 qc = a.image[j];
      if (!finite3(qc.x, qc.y, qc.z)) continue;
      const float4 qp = a.guide_p[j];
      add_tap(p, kern(dx) * kern(dy), qn.x, qn.y, qn.z, qp.x, qp.y, qp.z, qc.x, qc.y, qc.z, sum);
    }
  }
  a.out[i] = resolve(sum, c);
}

// Staged version for step S: the block's 32 x 8 tile and its halo of 2S pixels
// are staged once, 40 B per pixel in three planes whose rows are contiguous
// (consecutive lanes read consecutive 16-B records: no bank conflict) —
// (colour, word), (normal, position.x), (position.y, position.z).  A pixel
// outside the image or with a non-finite colour is staged with word ~0u, which
// no filterable centre matches.  The centre's own records come from global
// memory (its colour may be non-finite, and t and alpha are not staged).
constexpr int kTileW = 32, kTileH = 8;
template <int S>
__global__ __launch_bounds__(kBlock) void atrous_staged_kernel(AtrousArgs a) {
  constexpr int RW = kTileW + 4 * S, RH = kTileH + 4 * S, R = RW * RH;
  __shared__ float4 lds_c[R];
  __shared__ float4 lds_n[R];
  __shared__ float2 lds_p[R];
  const int W = (int)a.width, H = (int)a.height;
  const int x0 = (int)(blockIdx.x * (uint32_t)kTileW), y0 = (int)(blockIdx.y * (uint32_t)kTileH);
  for (int k = (int)threadIdx.x; k < R; k += kBlock) {
    const int ly = k / RW, lx = k - ly * RW;
    const int gx = x0 - 2 * S + lx, gy = y0 - 2 * S + ly;
    float4 c = make_float4(0.0f, 0.0f, 0.0f, __uint_as_float(0xFFFFFFFFu));
    float4 n = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    float2 q = make_float2(0.0f, 0.0f);
    if (gx >= 0 && gx < W && gy >= 0 && gy < H) {
      const size_t j = (size_t)gy * a.width + (uint32_t)gx;
      const float4 qc = a.image[j], qn = a.guide_n[j], qp = a.guide_p[j];
      if (finite3(qc.x, qc.y, qc.z)) c = make_float4(qc.x, qc.y, qc.z, qn.w);
      n = make_float4(qn.x, qn.y, qn.z, qp.x);
      q = make_float2(qp.y, qp.z);
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
  const float4 c = a.image[i], n = a.guide_n[i];
  const uint32_t word = __float_as_uint(n.w);
  if (word >= kNotFilterable) { a.out[i] = c; return; }
  const Centre p = make_centre(a, c, n, a.guide_p[i]);
  Sum sum{0.0f, 0.0f, 0.0f, 0.0f};
  const int lc = (ty + 2 * S) * RW + tx + 2 * S;   // the centre's staged record; taps stay inside [0, R)
#pragma unroll
  for (int dy = -2; dy <= 2; ++dy) {
#pragma unroll
    for (int dx = -2; dx <= 2; ++dx) {
      const int k = lc + dy * S * RW + dx * S;
      const float4 qc = lds_c[k];
      if (__float_as_uint(qc.w) != word) continue;
      const float4 qn = lds_n[k];
      const float2 qp = lds_p[k];
      add_tap(p, kern(dx) * kern(dy), qn.x, qn.y, qn.z, qn.w, qp.x, qp.y, qc.x, qc.y, qc.z, sum);
    }
  }
  a.out[i] = resolve(sum, c);
}

// Steps the staged path serves under kAtrousAuto (bit i = step 2^i).  Measured
// at 1920x1080, alternating in one call (DESIGN.md "Denoised output"): staged /
// direct 0.421 at step 1, 0.486 at step 2, 0.715 at step 4, spread at most 0.41 %.
constexpr uint32_t kStagedAutoSteps = 1u | 2u | 4u;

}  // namespace

hipError_t launch_atrous(const AtrousArgs& a, uint32_t path, hipStream_t s) {
  if (a.width == 0 || a.height == 0 || a.step == 0 || (a.step & (a.step - 1))) return hipErrorInvalidValue;
  const bool staged = a.step <= kAtrousStagedMaxStep &&
                      (path == kAtrousStaged || (path == kAtrousAuto && (kStagedAutoSteps & a.step)));
  if (staged) {
    const dim3 g((a.width + kTileW - 1) / kTileW, (a.height + kTileH - 1) / kTileH);
    if (a.step == 1) atrous_staged_kernel<1><<<g, dim3(kBlock), 0, s>>>(a);
    else if (a.step == 2) atrous_staged_kernel<2><<<g, dim3(kBlock), 0, s>>>(a);
    else atrous_staged_kernel<4><<<g, dim3(kBlock), 0, s>>>(a);
  } else {
    const dim3 g((a.width + 63) / 64, (a.height + 3) / 4);
    atrous_direct_kernel<<<g, dim3(kBlock), 0, s>>>(a);
  }
  return hipGetLastError();
}

}  // namespace mrt
