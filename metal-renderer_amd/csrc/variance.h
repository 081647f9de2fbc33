// variance.h — host-side launch interface of the variance estimate and the
// variance-guided A-Trous filter (variance.hip; the definitions are in
// include/mrt.h "variance-guided denoising" and DESIGN.md §2.1p).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace mrt {

struct VarianceArgs {
  const float4* moments;   // counted: (mean l, mean l^2, ., n)
  const float4* guide_n;   // (normal, bits(word)) of kern_stage.h guide_kernel
  const float4* guide_p;   // (position, t)
  float* variance;         // W * H
  uint32_t width, height;
  float sigma_plane;
  uint32_t normal_log2_power;
  float min_frames;        // (float)min_frames
};

// One iteration.  Between iterations the variance travels in the fourth
// channel of the ping-pong images; the first iteration takes it from the plane
// `var_in`, the last one writes the image's alpha and the plane `var_out`.
struct SvgfArgs {
  const float4* src;       // c^i: rgb + (v^i, or anything when var_in is given)
  const float* var_in;     // v^0 (first iteration), else nullptr: v^i = src.w
  const float4* guide_n;
  const float4* guide_p;
  float4* dst;             // c^(i+1): rgb + v^(i+1), or + alpha (last iteration)
  const float4* alpha;     // last iteration: the image whose alpha dst gets, else nullptr
  float* var_out;          // last iteration: v^(i+1) (may be nullptr), else nullptr
  uint32_t width, height;
  uint32_t step;           // s = 2^i
  float sigma_luminance;
  float sigma_plane;
  uint32_t normal_log2_power;
};

hipError_t launch_variance(const VarianceArgs& a, hipStream_t s);
// path: denoise.h AtrousPath (auto / direct / staged; the staged kernel serves steps <= kAtrousStagedMaxStep)
hipError_t launch_svgf_atrous(const SvgfArgs& a, uint32_t path, hipStream_t s);

}  // namespace mrt
