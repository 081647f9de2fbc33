// firefly.h — host-side launch interface of the firefly clamp (firefly.hip;
// the definition is in include/mrt.h "firefly suppression" and DESIGN.md §2.1s).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace mrt {

struct FireflyArgs {
  const float4* image;     // rgb + alpha
  const float4* guide_n;   // (normal, bits(word)) of kern_stage.h guide_kernel
  const float4* guide_p;   // (position, t)
  float4* out;
  uint32_t* clamped;       // pixels changed, added to (the caller zeroes it); may be nullptr
  uint32_t width, height;
  uint32_t radius;         // 1..3
  float k;
  uint32_t min_taps;
  float normal_cos_min;
  float plane_tolerance;
};

hipError_t launch_firefly(const FireflyArgs& a, hipStream_t s);

}  // namespace mrt
