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
// stays one 16-B load.  Both filters are atrous_impl.h's two kernels (every tap
// from global memory; a 32x8 tile with its halo of 2s pixels staged in LDS at
// steps 1, 2, 4, the 3x3 variance taps from the same tile), and the two changes
// are this unit's policy, SvgfFilter.  Compiled once: FMA contraction and
// native exp, IEEE division and sqrt.
#include "variance.h"

#include "atrous_impl.h"

namespace mrt {
namespace {

// ---------------------------------------------------------------------------
// mrt_variance: one pixel per lane (pixel_64x4)
// ---------------------------------------------------------------------------
__device__ __forceinline__ bool usable(const float4& m) { return finite1(m.x) && finite1(m.y) && m.w > 0.0f; }

__global__ __launch_bounds__(kBlock) void variance_kernel(VarianceArgs a) {
  const int W = (int)a.width, H = (int)a.height;
  int x, y;
  size_t i;
  if (!pixel_64x4(a.width, a.height, x, y, i)) return;
  const float4 n = a.guide_n[i];
  const uint32_t word = __float_as_uint(n.w);
  if (word >= kNotFilterable) { a.variance[i] = 0.0f; return; }
  const float4 m = a.moments[i];
  float r;
  if (usable(m) && m.w >= a.min_frames) {   // the pixel's own history is long enough: temporal
    r = fmaxf(0.0f, m.y - m.x * m.x) / (m.w - 1.0f);
  } else {                                  // else its 7x7 neighbourhood on the same surface
    const float4 xp = a.guide_p[i];
    const float inv = inv_plane(a.sigma_plane, xp.w);
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
        const float D = normal_weight(normal_dot(n.x, n.y, n.z, qn.x, qn.y, qn.z), a.normal_log2_power);
        const float dist = plane_distance(n.x, n.y, n.z, xp.x, xp.y, xp.z, qp.x, qp.y, qp.z);
        const float w = (D * __expf(-(dist * inv))) * qm.w;
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
struct SvgfFilter {
  using Args = SvgfArgs;
  static constexpr bool kVariance = true;
  // Measured at 1920x1080, alternating in one call (tools/variance_time.py,
  // DESIGN.md §2.1p): staged / direct 0.392 at step 1, 0.473 at step 2, 0.944 at
  // step 4, spread at most 0.18 %.
  static constexpr uint32_t kStagedAutoSteps = 1u | 2u | 4u;

  struct Centre : SurfaceCentre {
    float l;       // lum(c_p)
    float inv_l;   // 1 / (sigma_l sqrt(g_p) + 1e-6)
  };

  static __device__ __forceinline__ const float4* src(const Args& a) { return a.src; }
  static __device__ __forceinline__ float variance(const Args& a, size_t j, float w) { return a.var_in ? a.var_in[j] : w; }
  static __device__ __forceinline__ float variance(const Args& a, size_t j) { return a.var_in ? a.var_in[j] : a.src[j].w; }

  static __device__ __forceinline__ void colour(const Args& a, const float4& c, float g, Centre& p) {
    p.l = lum(c.x, c.y, c.z);
    p.inv_l = 1.0f / (a.sigma_luminance * sqrtf(fmaxf(g, 0.0f)) + 1e-6f);
    p.colour = finite3(c.x, c.y, c.z);
  }

  static __device__ __forceinline__ float colour_term(const Centre& p, float, float, float, float ql) {
    return fabsf(ql - p.l) * p.inv_l;
  }

  // c^(i+1)_p and v^(i+1)_p to their places: the variance in the fourth channel,
  // or (last iteration) the image's alpha there and the variance in its plane
  static __device__ __forceinline__ void store(const Args& a, size_t i, float r, float g, float b, float, float v) {
    a.dst[i] = make_float4(r, g, b, a.alpha ? a.alpha[i].w : v);
    if (a.var_out) a.var_out[i] = v;
  }
};

}  // namespace

hipError_t launch_variance(const VarianceArgs& a, hipStream_t s) {
  if (a.width == 0 || a.height == 0) return hipErrorInvalidValue;
  variance_kernel<<<grid_64x4(a.width, a.height), dim3(kBlock), 0, s>>>(a);
  return hipGetLastError();
}

hipError_t launch_svgf_atrous(const SvgfArgs& a, uint32_t path, hipStream_t s) {
  return launch_filter<SvgfFilter>(a, path, s);
}

}  // namespace mrt
