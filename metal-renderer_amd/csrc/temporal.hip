// temporal.hip — the temporal half of SVGF (Schied et al., HPG 2017): carry the
// accumulated image across a camera move by reprojecting it through the
// first-hit guide planes of the previous and the current camera (kernels.hip
// guide_kernel), and merge it with the frames accumulated since.  A COUNTED
// image is float4 (r, g, b, h): h >= 0 frames stand behind the colour, h = 0
// means no information and rgb = 0.  The definitions (include/mrt.h "temporal
// history", DESIGN.md "Temporal reprojection"):
//
// resolve, per pixel, h = history.w (0 without a history), n = frames:
//   h == 0                      -> (image.rgb, n)
//   n == 0                      -> history
//   image.rgb not all finite    -> history        (the history repairs the pixel)
//   otherwise                   -> ((h H.rgb + n I.rgb) / (h + n), h + n)
//
// reproject, per current pixel p (word_p >= 0x80000000 -> 0):
//   v = x_p - origin_prev, cz = v.forward_prev (cz <= 0 -> 0),
//   U = v.right_prev / cz, V = v.up_prev / cz, s = tan_half_fov_prev,
//   fx = (U / s + 1) (W - 1) / 2, fy = (V / (s H / W) + 1) (H - 1) / 2
//   (the inverse of camera_ray at the pixel centre), x0 = floor(fx),
//   y0 = floor(fy), ax = fx - x0, ay = fy - y0; the taps q = (x0 + i, y0 + j),
//   i, j in {0, 1}, with b = (i ? ax : 1 - ax) (j ? ay : 1 - ay), count iff q is
//   inside the image, b > 0, word_q == word_p, n_p.n_q >= normal_cos_min,
//   |n_p.(x_q - x_p)| <= plane_tolerance t_p, prev_q.w > 0 and prev_q.rgb
//   finite; B = sum b (B == 0 -> 0), rgb = sum b prev_q.rgb / B,
//   h = min(max_history, sum b prev_q.w / B).
//
// One pixel per lane; the camera and the parameters arrive by value (scalar
// registers).  Compiled once: FMA contraction as the fast build, IEEE division.
#include "temporal.h"

#include "dev_filter.h"

namespace mrt {
namespace {

constexpr int kBlock = 256;

// one load-load-store pass
__global__ __launch_bounds__(kBlock) void temporal_resolve_kernel(ResolveArgs a) {
  const uint32_t i = blockIdx.x * (uint32_t)kBlock + threadIdx.x;
  if (i >= a.count) return;
  const float4 c = a.image[i];
  const float n = a.frames;
  float4 hist = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
  if (a.history) hist = a.history[i];   // uniform branch
  const float h = hist.w;
  float4 o;
  if (!(h > 0.0f)) {
    o = make_float4(c.x, c.y, c.z, n);
  } else if (n == 0.0f || !finite3(c.x, c.y, c.z)) {
    o = hist;
  } else {
    const float t = h + n;
    o = make_float4((h * hist.x + n * c.x) / t, (h * hist.y + n * c.y) / t, (h * hist.z + n * c.z) / t, t);
  }
  a.out[i] = o;
}

// One pixel per lane (pixel_64x4, as atrous_direct_kernel): the current
// pixel's two loads and the store are 16 B per lane, coalesced.
// A tap's guide-normal record is read first; its position and its colour only
// when the word matches and the normals agree.  No clamped address is read.
__global__ __launch_bounds__(kBlock) void reproject_kernel(ReprojectArgs a) {
  const int W = (int)a.width, H = (int)a.height;
  int x, y;
  size_t i;
  if (!pixel_64x4(a.width, a.height, x, y, i)) return;
  const float4 zero = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
  const float4 n = a.cur_n[i];
  const uint32_t word = __float_as_uint(n.w);
  if (word >= kNotFilterable) { a.out[i] = zero; return; }
  const float4 p = a.cur_p[i];
  const float vx = p.x - a.origin[0], vy = p.y - a.origin[1], vz = p.z - a.origin[2];
  const float cz = (vx * a.forward[0] + vy * a.forward[1]) + vz * a.forward[2];
  if (!(cz > 0.0f)) { a.out[i] = zero; return; }
  const float U = ((vx * a.right[0] + vy * a.right[1]) + vz * a.right[2]) / cz;
  const float V = ((vx * a.up[0] + vy * a.up[1]) + vz * a.up[2]) / cz;
  const float s = a.tan_half_fov;
  const float sv = s * ((float)H / (float)W);
  const float fx = (U / s + 1.0f) * (0.5f * (float)(W - 1));
  const float fy = (V / sv + 1.0f) * (0.5f * (float)(H - 1));
  // a tap inside the image needs x0 in [-1, W - 1], y0 in [-1, H - 1] (also
  // keeps the float -> int conversions in range, and rejects a NaN)
  if (!(fx >= -1.0f && fx < (float)W && fy >= -1.0f && fy < (float)H)) { a.out[i] = zero; return; }
  const float flx = floorf(fx), fly = floorf(fy);
  const int x0 = (int)flx, y0 = (int)fly;
  const float ax = fx - flx, ay = fy - fly;
  const float tol = a.plane_tolerance * p.w;
  float B = 0.0f, r = 0.0f, g = 0.0f, bl = 0.0f, hs = 0.0f;
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int yy = y0 + j;
    if (yy < 0 || yy >= H) continue;
#pragma unroll
    for (int k = 0; k < 2; ++k) {
      const int xx = x0 + k;
      if (xx < 0 || xx >= W) continue;
      const float b = (k ? ax : 1.0f - ax) * (j ? ay : 1.0f - ay);
      if (!(b > 0.0f)) continue;
      const size_t q = (size_t)yy * a.width + (uint32_t)xx;
      const float4 qn = a.prev_n[q];
      if (__float_as_uint(qn.w) != word) continue;
      if (!(normal_dot(n.x, n.y, n.z, qn.x, qn.y, qn.z) >= a.normal_cos_min)) continue;
      const float4 qp = a.prev_p[q];
      const float dist = plane_distance(n.x, n.y, n.z, p.x, p.y, p.z, qp.x, qp.y, qp.z);
      if (!(dist <= tol)) continue;
      const float4 qc = a.prev[q];
      // (one test of the whole record, not w first: behind a branch on w the compiler loads rgb separately)
      if (!((int)(qc.w > 0.0f) & (int)finite3(qc.x, qc.y, qc.z))) continue;
      B += b;
      r += b * qc.x;
      g += b * qc.y;
      bl += b * qc.z;
      hs += b * qc.w;
    }
  }
  if (!(B > 0.0f)) { a.out[i] = zero; return; }
  const float h = fminf(a.max_history, hs / B);   // IEEE division (Makefile)
  // (max_history = 0 carries nothing: a count of 0 goes with rgb 0)
  a.out[i] = h > 0.0f ? make_float4(r / B, g / B, bl / B, h) : zero;
}

}  // namespace

hipError_t launch_temporal_resolve(const ResolveArgs& a, hipStream_t s) {
  if (a.count == 0) return hipErrorInvalidValue;
  temporal_resolve_kernel<<<dim3((a.count + kBlock - 1) / kBlock), dim3(kBlock), 0, s>>>(a);
  return hipGetLastError();
}

hipError_t launch_reproject(const ReprojectArgs& a, hipStream_t s) {
  if (a.width == 0 || a.height == 0) return hipErrorInvalidValue;
  reproject_kernel<<<grid_64x4(a.width, a.height), dim3(kBlock), 0, s>>>(a);
  return hipGetLastError();
}

}  // namespace mrt
