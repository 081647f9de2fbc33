// temporal.h — host-side launch interface of the temporal history kernels
// (temporal.hip; the definitions are in include/mrt.h "temporal history" and
// DESIGN.md "Temporal reprojection").
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace mrt {

struct ResolveArgs {
  const float4* image;     // accumulation image: running mean of `frames` frames
  const float4* history;   // counted image (rgb, h), or nullptr (h = 0 everywhere)
  float4* out;             // counted image
  uint32_t count;          // W * H
  float frames;            // n
};

struct ReprojectArgs {
  const float4* prev;      // counted image seen through the previous camera
  const float4* prev_n;    // its guide planes (kern_stage.h guide_kernel)
  const float4* prev_p;
  const float4* cur_n;     // the current camera's guide planes
  const float4* cur_p;
  float4* out;             // counted image in the current view
  uint32_t width, height;
  float origin[3], right[3], up[3], forward[3];   // the previous camera
  float tan_half_fov;
  float plane_tolerance, normal_cos_min, max_history;
};

hipError_t launch_temporal_resolve(const ResolveArgs& a, hipStream_t s);
hipError_t launch_reproject(const ReprojectArgs& a, hipStream_t s);

}  // namespace mrt
