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
// The iteration's two kernels — every tap from global memory, and a 32x8 tile
// with its halo of 2s pixels staged once in LDS (steps 1, 2, 4, where it
// measured faster) — are atrous_impl.h's; this unit is the policy that makes
// them this filter: the colour term and a plain store.  Compiled once: FMA
// contraction and native exp as the fast build, IEEE division.
#include "denoise.h"

#include "atrous_impl.h"

namespace mrt {
namespace {

struct PlainFilter {
  using Args = AtrousArgs;
  static constexpr bool kVariance = false;
  // Measured at 1920x1080, alternating in one call (DESIGN.md "Denoised output"):
  // staged / direct 0.421 at step 1, 0.486 at step 2, 0.715 at step 4, spread at
  // most 0.41 %.
  static constexpr uint32_t kStagedAutoSteps = 1u | 2u | 4u;

  struct Centre : SurfaceCentre {
    float cx, cy, cz;
    float inv_c2;   // 1 / sigma_c^2
  };

  static __device__ __forceinline__ const float4* src(const Args& a) { return a.image; }

  static __device__ __forceinline__ void colour(const Args& a, const float4& c, float, Centre& p) {
    p.cx = c.x; p.cy = c.y; p.cz = c.z;
    p.inv_c2 = a.inv_sigma_c2;
    p.colour = a.inv_sigma_c2 > 0.0f && finite3(c.x, c.y, c.z);
  }

  static __device__ __forceinline__ float colour_term(const Centre& p, float qcx, float qcy, float qcz, float) {
    const float dx = qcx - p.cx, dy = qcy - p.cy, dz = qcz - p.cz;
    return ((dx * dx + dy * dy) + dz * dz) * p.inv_c2;
  }

  static __device__ __forceinline__ void store(const Args& a, size_t i, float r, float g, float b, float alpha, float) {
    a.out[i] = make_float4(r, g, b, alpha);
  }
};

}  // namespace

hipError_t launch_atrous(const AtrousArgs& a, uint32_t path, hipStream_t s) { return launch_filter<PlainFilter>(a, path, s); }

}  // namespace mrt
