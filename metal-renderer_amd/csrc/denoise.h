// denoise.h — host-side launch interface of the edge-avoiding A-Trous filter
// (denoise.hip; the definition is in DESIGN.md "Denoised output").
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace mrt {

struct AtrousArgs {
  const float4* image;     // c^i: rgb + alpha
  const float4* guide_n;   // (normal, bits(word)) of kern_stage.h guide_kernel
  const float4* guide_p;   // (position, t)
  float4* out;             // c^(i+1)
  uint32_t width, height;
  uint32_t step;           // s = 2^i
  float inv_sigma_c2;      // 1 / sigma_color^2, 0 = no colour term
  float sigma_plane;
  uint32_t normal_log2_power;
};

// the two implementations of one iteration
enum AtrousPath : uint32_t {
  kAtrousAuto = 0,     // the staged path at the steps where it measured faster, else the direct one
  kAtrousDirect = 1,   // every tap from global memory
  kAtrousStaged = 2    // tile + halo staged in LDS (steps <= kAtrousStagedMaxStep, else direct)
};
constexpr uint32_t kAtrousStagedMaxStep = 4;   // 32x8 tile + halo of 2s: 46 KB of LDS at s = 4, 102 KB at s = 8

hipError_t launch_atrous(const AtrousArgs& a, uint32_t path, hipStream_t s);

}  // namespace mrt
