// stage_api.cpp — the stage-level C ABI of include/mrt.h (one call per pass of
// the reference's frame: raygen, intersect, shade, resolve, accumulate) and the
// entry points that need no renderer: camera helpers, guides, denoise, temporal
// resolve and reproject, display, tile pack / unpack, events, the noise table.
// The library's one error string lives here, behind mrt::host::fail.
#include <atomic>
#include <cmath>

#include "host_internal.h"
#include "denoise.h"
#include "firefly.h"
#include "image.h"
#include "noise.h"
#include "temporal.h"
#include "variance.h"

using namespace mrt::host;

namespace {

thread_local std::string g_last_error;   // the one string: every unit's fail() writes it, mrt_last_error reads it
std::atomic<uint32_t> g_denoise_path{mrt::kAtrousAuto};

// A buffer argument of an entry point: n bytes at p (null: an optional buffer
// that was not given, which overlaps nothing), written by the call or only read.
struct Span {
  const void* p;
  size_t n;
  bool written = false;
};
bool spans_overlap(const Span& a, const Span& b) {
  const char* p = (const char*)a.p;
  const char* q = (const char*)b.p;
  return p && q && p < q + b.n && q < p + a.n;
}
// the rule of every entry point: no written span overlaps any other span
bool written_overlap(std::initializer_list<Span> spans) {
  for (const Span* a = spans.begin(); a != spans.end(); ++a)
    for (const Span* b = a + 1; b != spans.end(); ++b)
      if ((a->written || b->written) && spans_overlap(*a, *b)) return true;
  return false;
}

// The iterations of an A-Trous filter from step 2^first_log2 on, ping-pong
// between scratch and out so that the last one writes `out`:
// launch(i, src, dst, step) is iteration i of N and returns a status.
template <class Launch>
int atrous_iterations(const float* image, float* out, float* scratch, uint32_t N, uint32_t first_log2, Launch launch) {
  const float* src = image;
  for (uint32_t i = 0; i < N; ++i) {
    float* dst = ((N - 1 - i) & 1u) ? scratch : out;
    const int rc = launch(i, reinterpret_cast<const float4*>(src), reinterpret_cast<float4*>(dst), 1u << (i + first_log2));
    if (rc) return rc;
    src = dst;
  }
  return MRT_OK;
}

// `iterations` iterations from step 2^first_log2 on, with implementation `path`
int denoise_run(const float* image, const float* guide_n, const float* guide_p, float* out, float* scratch,
                uint32_t W, uint32_t H, const mrt_denoise_params* params, uint32_t iterations, uint32_t first_log2,
                uint32_t path, void* stream) {
  if (!image || !guide_n || !guide_p || !out || !scratch || !params || W == 0 || H == 0 || W > 32768 || H > 32768)
    return fail(MRT_ERR_INVALID, "mrt_denoise: bad argument");
  const size_t bytes = (size_t)W * H * 16;
  if (written_overlap({{image, bytes}, {out, bytes, true}, {scratch, bytes, true}}))
    return fail(MRT_ERR_INVALID, "mrt_denoise: image, out and scratch must not overlap");
  if (written_overlap({{guide_n, bytes}, {guide_p, bytes}, {out, bytes, true}, {scratch, bytes, true}}))
    return fail(MRT_ERR_INVALID, "mrt_denoise: the guide planes must not overlap out or scratch");
  const int rc = mrt_denoise_params_check(params);
  if (rc) return rc;
  hipStream_t s = (hipStream_t)stream;
  if (iterations == 0) {
    HIP_TRY(hipMemcpyAsync(out, image, bytes, hipMemcpyDeviceToDevice, s));
    return MRT_OK;
  }
  mrt::AtrousArgs a{};
  a.guide_n = reinterpret_cast<const float4*>(guide_n);
  a.guide_p = reinterpret_cast<const float4*>(guide_p);
  a.width = W;
  a.height = H;
  a.inv_sigma_c2 = params->sigma_color > 0.0f ? (float)(1.0 / ((double)params->sigma_color * params->sigma_color)) : 0.0f;
  a.sigma_plane = params->sigma_plane;
  a.normal_log2_power = params->normal_log2_power;
  return atrous_iterations(image, out, scratch, iterations, first_log2,
                           [&](uint32_t, const float4* src, float4* dst, uint32_t step) -> int {
                             a.image = src;
                             a.out = dst;
                             a.step = step;
                             HIP_TRY(mrt::launch_atrous(a, path, s));
                             return MRT_OK;
                           });
}

// mrt_denoise_variance: `iterations` iterations from step 2^first_log2 on with
// implementation `path`; last: the final one writes the image's alpha and
// variance_out (else the variance stays in out's fourth channel)
int svgf_run(const float* image, const float* variance, const float* guide_n, const float* guide_p, float* out,
             float* scratch, float* variance_out, uint32_t W, uint32_t H, const mrt_svgf_params* params,
             uint32_t iterations, uint32_t first_log2, uint32_t path, bool last, void* stream) {
  // (scratch may be null for a single iteration, which writes `out` alone: the measurement entry)
  if (!image || !variance || !guide_n || !guide_p || !out || (!scratch && iterations != 1) || !params || W == 0 ||
      H == 0 || W > 32768 || H > 32768)
    return fail(MRT_ERR_INVALID, "mrt_denoise_variance: bad argument");
  const size_t bytes = (size_t)W * H * 16, plane = (size_t)W * H * 4;
  if (written_overlap({{image, bytes}, {variance, plane}, {guide_n, bytes}, {guide_p, bytes}, {out, bytes, true},
                       {scratch, bytes, true}, {variance_out, plane, true}}))
    return fail(MRT_ERR_INVALID, "mrt_denoise_variance: out, scratch and variance_out must not overlap any buffer");
  const int rc = mrt_svgf_params_check(params);
  if (rc) return rc;
  hipStream_t s = (hipStream_t)stream;
  const uint32_t N = iterations;
  if (N == 0) {
    HIP_TRY(hipMemcpyAsync(out, image, bytes, hipMemcpyDeviceToDevice, s));
    if (variance_out) HIP_TRY(hipMemcpyAsync(variance_out, variance, plane, hipMemcpyDeviceToDevice, s));
    return MRT_OK;
  }
  mrt::SvgfArgs a{};
  a.guide_n = reinterpret_cast<const float4*>(guide_n);
  a.guide_p = reinterpret_cast<const float4*>(guide_p);
  a.width = W;
  a.height = H;
  a.sigma_luminance = params->sigma_luminance;
  a.sigma_plane = params->sigma_plane;
  a.normal_log2_power = params->normal_log2_power;
  return atrous_iterations(image, out, scratch, N, first_log2,
                           [&](uint32_t i, const float4* src, float4* dst, uint32_t step) -> int {
                             const bool final = last && i + 1 == N;
                             a.src = src;
                             a.var_in = i == 0 ? variance : nullptr;
                             a.dst = dst;
                             a.alpha = final ? reinterpret_cast<const float4*>(image) : nullptr;
                             a.var_out = final ? variance_out : nullptr;
                             a.step = step;
                             HIP_TRY(mrt::launch_svgf_atrous(a, path, s));
                             return MRT_OK;
                           });
}

}  // namespace

namespace mrt {
namespace host {

int fail(int code, const std::string& msg) {
  g_last_error = msg;
  return code;
}

mrt::CameraBlock camera_block(const mrt_camera& c) {
  mrt::CameraBlock b{};
  static_assert(sizeof(mrt_camera) == 60 && sizeof(mrt_camera) <= sizeof(mrt::CameraBlock), "mrt_camera");
  std::memcpy(&b, &c, sizeof(mrt_camera));   // the same fields in the same order
  return b;
}

bool camera_is_default(const mrt_camera& c) {
  mrt_camera d;
  (void)mrt_camera_default(&d);
  return std::memcmp(&c, &d, sizeof(mrt_camera)) == 0;
}

// the camera block of a guide pass: `cam` (NULL = the default) checked, its lens
// removed; *moved: not the reference's camera, so the kernel reads the block
static int guide_camera(const mrt_camera* cam, mrt::CameraBlock* cb, bool* moved) {
  mrt_camera c;
  if (cam) {
    const int rc = mrt_camera_check(cam);
    if (rc) return rc;
    c = *cam;
  } else {
    (void)mrt_camera_default(&c);
  }
  c.lens_radius = 0.0f;   // the guide ray goes through the pinhole
  c.focus_distance = 0.0f;
  mrt_camera d;
  (void)mrt_camera_default(&d);
  d.focus_distance = 0.0f;
  *moved = std::memcmp(&c, &d, sizeof(mrt_camera)) != 0;
  *cb = camera_block(c);
  return MRT_OK;
}

// mrt_guides with the caller's stack spill (a renderer's own, so that its guide
// pass shares nothing with the stage calls on the scene or another renderer)
int guides_with_spill(const mrt_scene* scene, const mrt_camera* cam, uint32_t W, uint32_t H, float* guide_n,
                      float* guide_p, uint32_t flags, uint32_t* spill, void* stream) {
  if (!scene || !guide_n || !guide_p || guide_n == guide_p || W < 2 || H < 2 || W > 32768 || H > 32768)
    return fail(MRT_ERR_INVALID, "mrt_guides: bad argument");
  mrt::CameraBlock cb;
  bool moved = false;
  const int rc = guide_camera(cam, &cb, &moved);
  if (rc) return rc;
  HIP_TRY(MRT_BUILD_CALL(flags, launch_guides(scene->dev, W, H, moved ? &cb : nullptr, guide_n, guide_p, spill,
                                              (hipStream_t)stream)));
  return MRT_OK;
}

// mrt_guides_motion, likewise with the caller's stack spill
int guides_motion_with_spill(const mrt_scene* scene, const mrt_scene* prev_scene, const mrt_camera* cam, uint32_t W,
                             uint32_t H, float* guide_n, float* guide_p, float* motion_n, float* motion_p,
                             uint32_t flags, uint32_t* spill, void* stream) {
  if (!scene || !prev_scene || !guide_n || !guide_p || !motion_n || !motion_p || W < 2 || H < 2 || W > 32768 ||
      H > 32768)
    return fail(MRT_ERR_INVALID, "mrt_guides_motion: bad argument");
  const size_t bytes = (size_t)W * H * 16;
  if (written_overlap({{guide_n, bytes, true}, {guide_p, bytes, true}, {motion_n, bytes, true}, {motion_p, bytes, true}}))
    return fail(MRT_ERR_INVALID, "mrt_guides_motion: the four planes must not overlap");
  if (scene->device < 0 || prev_scene->device < 0)
    return fail(MRT_ERR_INVALID, "mrt_guides_motion: a host-only scene has nothing on a device");
  if (scene->device != prev_scene->device)
    return fail(MRT_ERR_INVALID, "mrt_guides_motion: the two scenes are on different devices");
  int rc = mrt_scene_motion_compatible(prev_scene, scene);
  if (rc) return rc;
  mrt::CameraBlock cb;
  bool moved = false;
  rc = guide_camera(cam, &cb, &moved);
  if (rc) return rc;
  HIP_TRY(MRT_BUILD_CALL(flags, launch_guides_motion(scene->dev, prev_scene->dev.prims, W, H, moved ? &cb : nullptr,
                                                     guide_n, guide_p, motion_n, motion_p, spill,
                                                     (hipStream_t)stream)));
  return MRT_OK;
}

}  // namespace host
}  // namespace mrt

extern "C" {

const char* mrt_last_error(void) { return g_last_error.c_str(); }
int mrt_abi_version(void) { return MRT_ABI_VERSION; }

int mrt_device_count(void) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) return 0;
  return n;
}

int mrt_shard_mask(uint32_t W, uint32_t H, uint32_t rank, uint32_t count, uint8_t* mask, uint64_t* owned) {
  if (W == 0 || H == 0) return fail(MRT_ERR_INVALID, "empty image");
  const uint32_t S = count ? count : 1;
  if (rank >= S) return fail(MRT_ERR_INVALID, "shard_rank >= shard_count");
  const uint32_t tx_n = (W + mrt::kTile - 1) / mrt::kTile, ty_n = (H + mrt::kTile - 1) / mrt::kTile;
  uint64_t n = 0;
  for (uint32_t y = 0; y < H; ++y)
    for (uint32_t x = 0; x < W; ++x) {
      const uint32_t t = (y / mrt::kTile) * tx_n + x / mrt::kTile;
      const bool mine = (t % S) == rank;
      if (mask) mask[(size_t)y * W + x] = mine ? 1 : 0;
      n += mine;
    }
  (void)ty_n;
  if (owned) *owned = n;
  return MRT_OK;
}

int mrt_display(const float* image, const float* reference, float* out, uint32_t W, uint32_t H, uint32_t flags,
                float compare_scale, void* stream) {
  const uint32_t mode = (flags >> 8) & 0xFFu;
  flags &= ~(MRT_DISPLAY_DENOISED | MRT_DISPLAY_RESOLVED);   // a renderer-level choice of the source (mrt_renderer_display)
  if (!image || !out || W == 0 || H == 0 || mode > 4 || (mode && !reference) || (flags & ~0xFF03u))
    return fail(MRT_ERR_INVALID, "mrt_display: bad argument");
  HIP_TRY(mrt::fast::launch_display(reinterpret_cast<const float4*>(image), reinterpret_cast<const float4*>(reference),
                                    reinterpret_cast<float4*>(out), W * H, flags, compare_scale, (hipStream_t)stream));
  return MRT_OK;
}

int mrt_tiles_packed_floats(uint32_t W, uint32_t H, uint32_t rank, uint32_t count, uint64_t* floats) {
  const uint32_t S = count ? count : 1;
  if (!floats || W == 0 || H == 0 || rank >= S) return fail(MRT_ERR_INVALID, "mrt_tiles_packed_floats: bad argument");
  const uint32_t T = ((W + mrt::kTile - 1) / mrt::kTile) * ((H + mrt::kTile - 1) / mrt::kTile);
  const uint64_t owned = rank < T ? (T - rank + S - 1) / S : 0;
  *floats = owned * mrt::kTile * mrt::kTile * 4;
  return MRT_OK;
}

int mrt_tiles_pack(const float* image, uint32_t W, uint32_t H, uint32_t rank, uint32_t count, float* packed,
                   void* stream) {
  const uint32_t S = count ? count : 1;
  if (!image || !packed || W == 0 || H == 0 || rank >= S) return fail(MRT_ERR_INVALID, "mrt_tiles_pack: bad argument");
  HIP_TRY(mrt::fast::launch_tiles_move(reinterpret_cast<const float4*>(image), reinterpret_cast<float4*>(packed), W, H,
                                       rank, S, true, (hipStream_t)stream));
  return MRT_OK;
}

int mrt_tiles_unpack(const float* packed, uint32_t W, uint32_t H, uint32_t rank, uint32_t count, float* image,
                     void* stream) {
  const uint32_t S = count ? count : 1;
  if (!image || !packed || W == 0 || H == 0 || rank >= S) return fail(MRT_ERR_INVALID, "mrt_tiles_unpack: bad argument");
  HIP_TRY(mrt::fast::launch_tiles_move(reinterpret_cast<const float4*>(packed), reinterpret_cast<float4*>(image), W, H,
                                       rank, S, false, (hipStream_t)stream));
  return MRT_OK;
}

int mrt_synchronize(void* stream) {
  if (stream) HIP_TRY(hipStreamSynchronize((hipStream_t)stream));
  else HIP_TRY(hipDeviceSynchronize());
  return MRT_OK;
}

int mrt_event_record(void* stream, void** event) {
  if (!event) return fail(MRT_ERR_INVALID, "null event");
  if (!*event) {
    hipEvent_t e;
    HIP_TRY(hipEventCreateWithFlags(&e, hipEventDisableTiming));
    *event = (void*)e;
  }
  HIP_TRY(hipEventRecord((hipEvent_t)*event, (hipStream_t)stream));
  return MRT_OK;
}

int mrt_event_synchronize(void* event) {
  if (!event) return fail(MRT_ERR_INVALID, "null event");
  HIP_TRY(hipEventSynchronize((hipEvent_t)event));
  return MRT_OK;
}

int mrt_event_destroy(void* event) {
  if (event) HIP_TRY(hipEventDestroy((hipEvent_t)event));
  return MRT_OK;
}

int mrt_debug_stamps(uint64_t* out8, int reset) {
  if (!out8) return fail(MRT_ERR_INVALID, "null output");
  HIP_TRY(mrt::fast::read_stamps(reinterpret_cast<unsigned long long*>(out8), reset != 0));
  return MRT_OK;
}

int mrt_debug_wave_times(uint64_t* out, size_t n) {
  if (!out) return fail(MRT_ERR_INVALID, "null output");
  HIP_TRY(mrt::fast::read_wave_times(reinterpret_cast<unsigned long long*>(out), n));
  return MRT_OK;
}

int mrt_debug_lanes(uint64_t* out, size_t n, int reset) {
  if (!out) return fail(MRT_ERR_INVALID, "null output");
  HIP_TRY(mrt::fast::read_lane_stats(reinterpret_cast<unsigned long long*>(out), n, reset != 0));
  return MRT_OK;
}

int mrt_noise_table(uint64_t seed, int64_t frame, float* out) {
  if (!out) return fail(MRT_ERR_INVALID, "null output");
  mrt::make_noise_table(seed, frame, out);
  return MRT_OK;
}

int mrt_debug_magic_div(uint32_t d, const uint32_t* n, uint32_t count, uint32_t* q) {
  if (d == 0 || (count && (!n || !q))) return fail(MRT_ERR_INVALID, "mrt_debug_magic_div: bad argument");
  const mrt::MagicDiv m = mrt::magic_div(d);
  for (uint32_t i = 0; i < count; ++i) q[i] = mrt::mdiv_host(n[i], m);
  return MRT_OK;
}

// ---------------------------------------------------------------------------
// stage-level ABI
// ---------------------------------------------------------------------------
int mrt_raygen(const mrt_scene* scene, uint32_t W, uint32_t H, const float* noise, void* rays, uint32_t flags,
               void* stream) {
  if (!scene || !noise || !rays || W < 2 || H < 2) return fail(MRT_ERR_INVALID, "mrt_raygen: bad argument");
  HIP_TRY(MRT_BUILD_CALL(flags, launch_raygen(W, H, noise, (mrt::RefRay*)rays, nullptr, (hipStream_t)stream)));
  return MRT_OK;
}

// ---- camera (include/mrt.h) -------------------------------------------------
int mrt_camera_default(mrt_camera* out) {
  if (!out) return fail(MRT_ERR_INVALID, "mrt_camera_default: null camera");
  // rayGenerator's camera (mrt_layout.h kCameraX/Y/Z), looking down -z
  *out = mrt_camera{{mrt::kCameraX, mrt::kCameraY, mrt::kCameraZ}, {1.0f, 0.0f, 0.0f}, {0.0f, 1.0f, 0.0f},
                    {0.0f, 0.0f, -1.0f}, 1.0f, 0.0f, 0.0f};
  return MRT_OK;
}

int mrt_camera_check(const mrt_camera* cam) {
  if (!cam) return fail(MRT_ERR_INVALID, "camera: null");
  const float* f = cam->origin;   // 15 consecutive floats
  for (int i = 0; i < 15; ++i)
    if (!std::isfinite(f[i])) return fail(MRT_ERR_INVALID, "camera: a field is not finite");
  auto dotd = [](const float* a, const float* b) {
    return (double)a[0] * b[0] + (double)a[1] * b[1] + (double)a[2] * b[2];
  };
  const float* ax[3] = {cam->right, cam->up, cam->forward};
  for (int i = 0; i < 3; ++i)
    for (int j = i; j < 3; ++j)
      if (std::fabs(dotd(ax[i], ax[j]) - (i == j ? 1.0 : 0.0)) > 1e-4)
        return fail(MRT_ERR_INVALID, "camera: right, up, forward are not orthonormal to 1e-4");
  const double cx[3] = {(double)cam->right[1] * cam->up[2] - (double)cam->right[2] * cam->up[1],
                        (double)cam->right[2] * cam->up[0] - (double)cam->right[0] * cam->up[2],
                        (double)cam->right[0] * cam->up[1] - (double)cam->right[1] * cam->up[0]};
  if (!(cx[0] * cam->forward[0] + cx[1] * cam->forward[1] + cx[2] * cam->forward[2] < 0.0))
    return fail(MRT_ERR_INVALID, "camera: the basis is not right-handed (right x up must be -forward)");
  if (!(cam->tan_half_fov > 0.0f)) return fail(MRT_ERR_INVALID, "camera: tan_half_fov must be positive");
  if (cam->lens_radius < 0.0f) return fail(MRT_ERR_INVALID, "camera: lens_radius must not be negative");
  if (cam->lens_radius > 0.0f && !(cam->focus_distance > 0.0f))
    return fail(MRT_ERR_INVALID, "camera: a lens needs a positive focus_distance");
  return MRT_OK;
}

int mrt_camera_look_at(const float eye[3], const float target[3], const float up[3], float fov_x_degrees,
                       mrt_camera* out) {
  if (!eye || !target || !up || !out) return fail(MRT_ERR_INVALID, "mrt_camera_look_at: null argument");
  for (int i = 0; i < 3; ++i)
    if (!std::isfinite(eye[i]) || !std::isfinite(target[i]) || !std::isfinite(up[i]))
      return fail(MRT_ERR_INVALID, "mrt_camera_look_at: an argument is not finite");
  if (!(fov_x_degrees > 0.0f && fov_x_degrees < 180.0f))
    return fail(MRT_ERR_INVALID, "mrt_camera_look_at: fov_x_degrees must lie in (0, 180)");
  double f[3] = {(double)target[0] - eye[0], (double)target[1] - eye[1], (double)target[2] - eye[2]};
  const double fl = std::sqrt(f[0] * f[0] + f[1] * f[1] + f[2] * f[2]);
  if (!(fl > 0.0)) return fail(MRT_ERR_INVALID, "mrt_camera_look_at: eye and target coincide");
  for (double& v : f) v /= fl;
  const double ul = std::sqrt((double)up[0] * up[0] + (double)up[1] * up[1] + (double)up[2] * up[2]);
  double r[3] = {f[1] * up[2] - f[2] * up[1], f[2] * up[0] - f[0] * up[2], f[0] * up[1] - f[1] * up[0]};
  const double rl = std::sqrt(r[0] * r[0] + r[1] * r[1] + r[2] * r[2]);
  if (!(ul > 0.0) || !(rl > 1e-6 * ul))
    return fail(MRT_ERR_INVALID, "mrt_camera_look_at: up is zero or parallel to the view direction");
  for (double& v : r) v /= rl;
  const double u[3] = {r[1] * f[2] - r[2] * f[1], r[2] * f[0] - r[0] * f[2], r[0] * f[1] - r[1] * f[0]};
  mrt_camera c{};
  for (int i = 0; i < 3; ++i) {
    c.origin[i] = eye[i];
    c.right[i] = (float)r[i];
    c.up[i] = (float)u[i];
    c.forward[i] = (float)f[i];
  }
  c.tan_half_fov = (float)std::tan((double)fov_x_degrees * (3.14159265358979323846 / 360.0));
  c.lens_radius = 0.0f;
  c.focus_distance = 0.0f;
  const int rc = mrt_camera_check(&c);   // (e.g. a field of view whose tangent overflows a float)
  if (rc) return rc;
  *out = c;
  return MRT_OK;
}

int mrt_raygen_camera(const mrt_scene* scene, const mrt_camera* cam, uint32_t W, uint32_t H, const float* noise,
                      void* rays, uint32_t flags, void* stream) {
  if (!scene || !cam || !noise || !rays || W < 2 || H < 2)
    return fail(MRT_ERR_INVALID, "mrt_raygen_camera: bad argument");
  const int rc = mrt_camera_check(cam);
  if (rc) return rc;
  const mrt::CameraBlock cb = camera_block(*cam);
  HIP_TRY(MRT_BUILD_CALL(flags, launch_raygen(W, H, noise, (mrt::RefRay*)rays, camera_is_default(*cam) ? nullptr : &cb,
                                              (hipStream_t)stream)));
  return MRT_OK;
}

// ---- denoised output (include/mrt.h) ---------------------------------------
int mrt_guides(const mrt_scene* scene, const mrt_camera* cam, uint32_t W, uint32_t H, float* guide_n, float* guide_p,
               uint32_t flags, void* stream) {
  return guides_with_spill(scene, cam, W, H, guide_n, guide_p, flags,
                           scene ? scene->isect_spill.as<uint32_t>() : nullptr, stream);
}

int mrt_denoise_params_default(uint64_t frames, mrt_denoise_params* out) {
  if (!out) return fail(MRT_ERR_INVALID, "mrt_denoise_params_default: null params");
  out->iterations = frames <= 2 ? 3u : (frames <= 16 ? 2u : 1u);
  out->sigma_color = (float)(2.0 / std::sqrt((double)std::max<uint64_t>(frames, 1)));
  out->sigma_plane = 0.01f;
  out->normal_log2_power = 6;
  return MRT_OK;
}

int mrt_denoise_params_check(const mrt_denoise_params* p) {
  if (!p) return fail(MRT_ERR_INVALID, "denoise params: null");
  if (p->iterations > 8) return fail(MRT_ERR_INVALID, "denoise params: iterations must be at most 8");
  if (!std::isfinite(p->sigma_color) || p->sigma_color < 0.0f)
    return fail(MRT_ERR_INVALID, "denoise params: sigma_color must be finite and not negative");
  if (!std::isfinite(p->sigma_plane) || !(p->sigma_plane > 0.0f))
    return fail(MRT_ERR_INVALID, "denoise params: sigma_plane must be finite and positive");
  if (p->normal_log2_power > 8) return fail(MRT_ERR_INVALID, "denoise params: normal_log2_power must be at most 8");
  return MRT_OK;
}

int mrt_debug_denoise_path(uint32_t path) {
  if (path > mrt::kAtrousStaged) return fail(MRT_ERR_INVALID, "mrt_debug_denoise_path: 0, 1 or 2");
  g_denoise_path.store(path);
  return MRT_OK;
}

int mrt_guides_motion(const mrt_scene* scene, const mrt_scene* prev_scene, const mrt_camera* cam, uint32_t W,
                      uint32_t H, float* guide_n, float* guide_p, float* motion_n, float* motion_p, uint32_t flags,
                      void* stream) {
  return guides_motion_with_spill(scene, prev_scene, cam, W, H, guide_n, guide_p, motion_n, motion_p, flags,
                                  scene ? scene->isect_spill.as<uint32_t>() : nullptr, stream);
}

int mrt_denoise(const float* image, const float* guide_n, const float* guide_p, float* out, float* scratch,
                uint32_t W, uint32_t H, const mrt_denoise_params* params, void* stream) {
  return denoise_run(image, guide_n, guide_p, out, scratch, W, H, params, params ? params->iterations : 0u, 0u,
                     g_denoise_path.load(), stream);
}

int mrt_debug_denoise_step(const float* image, const float* guide_n, const float* guide_p, float* out, float* scratch,
                           uint32_t W, uint32_t H, const mrt_denoise_params* params, uint32_t step_log2, uint32_t path,
                           void* stream) {
  if (step_log2 > 14 || path > mrt::kAtrousStaged)
    return fail(MRT_ERR_INVALID, "mrt_debug_denoise_step: step at most 2^14, path 0, 1 or 2");
  return denoise_run(image, guide_n, guide_p, out, scratch, W, H, params, 1u, step_log2, path, stream);
}

// ---- variance-guided denoising (include/mrt.h) ------------------------------
int mrt_svgf_params_default(mrt_svgf_params* out) {
  if (!out) return fail(MRT_ERR_INVALID, "mrt_svgf_params_default: null params");
  out->iterations = 5;
  out->sigma_luminance = 4.0f;
  out->sigma_plane = 0.01f;
  out->normal_log2_power = 6;
  out->min_frames = 4;
  return MRT_OK;
}

int mrt_svgf_params_check(const mrt_svgf_params* p) {
  if (!p) return fail(MRT_ERR_INVALID, "svgf params: null");
  if (p->iterations > 8) return fail(MRT_ERR_INVALID, "svgf params: iterations must be at most 8");
  if (!std::isfinite(p->sigma_luminance) || !(p->sigma_luminance > 0.0f))
    return fail(MRT_ERR_INVALID, "svgf params: sigma_luminance must be finite and positive");
  if (!std::isfinite(p->sigma_plane) || !(p->sigma_plane > 0.0f))
    return fail(MRT_ERR_INVALID, "svgf params: sigma_plane must be finite and positive");
  if (p->normal_log2_power > 8) return fail(MRT_ERR_INVALID, "svgf params: normal_log2_power must be at most 8");
  if (p->min_frames < 2) return fail(MRT_ERR_INVALID, "svgf params: min_frames must be at least 2");
  return MRT_OK;
}

int mrt_variance(const float* moments, const float* guide_n, const float* guide_p, float* variance, uint32_t W,
                 uint32_t H, const mrt_svgf_params* params, void* stream) {
  if (!moments || !guide_n || !guide_p || !variance || !params || W == 0 || H == 0 || W > 32768 || H > 32768)
    return fail(MRT_ERR_INVALID, "mrt_variance: bad argument");
  const size_t bytes = (size_t)W * H * 16;
  if (written_overlap({{moments, bytes}, {guide_n, bytes}, {guide_p, bytes}, {variance, bytes / 4, true}}))
    return fail(MRT_ERR_INVALID, "mrt_variance: variance must not overlap an input");
  const int rc = mrt_svgf_params_check(params);
  if (rc) return rc;
  mrt::VarianceArgs a{};
  a.moments = reinterpret_cast<const float4*>(moments);
  a.guide_n = reinterpret_cast<const float4*>(guide_n);
  a.guide_p = reinterpret_cast<const float4*>(guide_p);
  a.variance = variance;
  a.width = W;
  a.height = H;
  a.sigma_plane = params->sigma_plane;
  a.normal_log2_power = params->normal_log2_power;
  a.min_frames = (float)params->min_frames;
  HIP_TRY(mrt::launch_variance(a, (hipStream_t)stream));
  return MRT_OK;
}

int mrt_denoise_variance(const float* image, const float* variance, const float* guide_n, const float* guide_p,
                         float* out, float* scratch, float* variance_out, uint32_t W, uint32_t H,
                         const mrt_svgf_params* params, void* stream) {
  if (!scratch) return fail(MRT_ERR_INVALID, "mrt_denoise_variance: bad argument");
  return svgf_run(image, variance, guide_n, guide_p, out, scratch, variance_out, W, H, params,
                  params ? params->iterations : 0u, 0u, g_denoise_path.load(), true, stream);
}

int mrt_debug_denoise_variance_step(const float* image, const float* variance, const float* guide_n,
                                    const float* guide_p, float* out, uint32_t W, uint32_t H,
                                    const mrt_svgf_params* params, uint32_t step_log2, uint32_t path, void* stream) {
  if (step_log2 > 14 || path > mrt::kAtrousStaged)
    return fail(MRT_ERR_INVALID, "mrt_debug_denoise_variance_step: step at most 2^14, path 0, 1 or 2");
  return svgf_run(image, variance, guide_n, guide_p, out, nullptr, nullptr, W, H, params, 1u, step_log2, path, false, stream);
}

// ---- firefly suppression (include/mrt.h) -------------------------------------
int mrt_firefly_params_default(mrt_firefly_params* out) {
  if (!out) return fail(MRT_ERR_INVALID, "mrt_firefly_params_default: null params");
  out->radius = 2;
  out->k = 3.0f;
  out->min_taps = 3;
  out->normal_cos_min = 0.9f;
  out->plane_tolerance = 0.01f;
  return MRT_OK;
}

int mrt_firefly_params_check(const mrt_firefly_params* p) {
  if (!p) return fail(MRT_ERR_INVALID, "firefly params: null");
  if (p->radius < 1 || p->radius > 3) return fail(MRT_ERR_INVALID, "firefly params: radius must be 1, 2 or 3");
  if (!std::isfinite(p->k) || !(p->k > 0.0f)) return fail(MRT_ERR_INVALID, "firefly params: k must be finite and positive");
  if (p->min_taps < 1) return fail(MRT_ERR_INVALID, "firefly params: min_taps must be at least 1");
  if (!(p->normal_cos_min >= -1.0f && p->normal_cos_min <= 1.0f))
    return fail(MRT_ERR_INVALID, "firefly params: normal_cos_min must be in [-1, 1]");
  if (!std::isfinite(p->plane_tolerance) || !(p->plane_tolerance > 0.0f))
    return fail(MRT_ERR_INVALID, "firefly params: plane_tolerance must be finite and positive");
  return MRT_OK;
}

int mrt_firefly_clamp(const float* image, const float* guide_n, const float* guide_p, float* out, uint32_t* clamped,
                      uint32_t W, uint32_t H, const mrt_firefly_params* params, void* stream) {
  if (!image || !guide_n || !guide_p || !out || !params || W == 0 || H == 0 || W > 32768 || H > 32768)
    return fail(MRT_ERR_INVALID, "mrt_firefly_clamp: bad argument");
  const size_t bytes = (size_t)W * H * 16;
  const Span o{out, bytes, true}, cl{clamped, 4, true};
  for (const float* in : {image, guide_n, guide_p})
    if (spans_overlap({in, bytes}, o) || spans_overlap({in, bytes}, cl))
      return fail(MRT_ERR_INVALID, "mrt_firefly_clamp: out and clamped must not overlap an input");
  if (spans_overlap(o, cl))
    return fail(MRT_ERR_INVALID, "mrt_firefly_clamp: out and clamped must not overlap each other");
  const int rc = mrt_firefly_params_check(params);
  if (rc) return rc;
  hipStream_t s = (hipStream_t)stream;
  if (clamped) HIP_TRY(hipMemsetAsync(clamped, 0, 4, s));
  mrt::FireflyArgs a{};
  a.image = reinterpret_cast<const float4*>(image);
  a.guide_n = reinterpret_cast<const float4*>(guide_n);
  a.guide_p = reinterpret_cast<const float4*>(guide_p);
  a.out = reinterpret_cast<float4*>(out);
  a.clamped = clamped;
  a.width = W;
  a.height = H;
  a.radius = params->radius;
  a.k = params->k;
  a.min_taps = params->min_taps;
  a.normal_cos_min = params->normal_cos_min;
  a.plane_tolerance = params->plane_tolerance;
  HIP_TRY(mrt::launch_firefly(a, s));
  return MRT_OK;
}

// ---- adaptive sampling (include/mrt.h) ---------------------------------------
int mrt_adaptive_params_default(mrt_adaptive_params* out) {
  if (!out) return fail(MRT_ERR_INVALID, "mrt_adaptive_params_default: null params");
  out->luminance_floor = 0.01f;
  return MRT_OK;
}

int mrt_adaptive_params_check(const mrt_adaptive_params* p) {
  if (!p) return fail(MRT_ERR_INVALID, "adaptive params: null");
  if (!std::isfinite(p->luminance_floor) || !(p->luminance_floor > 0.0f))
    return fail(MRT_ERR_INVALID, "adaptive params: luminance_floor must be finite and positive");
  return MRT_OK;
}

int mrt_counted_merge(const float* a, const float* b, float* out, uint32_t W, uint32_t H, uint32_t flags, void* stream) {
  if (!a || !b || !out || W == 0 || H == 0 || W > 32768 || H > 32768)
    return fail(MRT_ERR_INVALID, "mrt_counted_merge: bad argument");
  const size_t bytes = (size_t)W * H * 16;
  if (spans_overlap({b, bytes}, {out, bytes}) || (out != a && spans_overlap({a, bytes}, {out, bytes})))
    return fail(MRT_ERR_INVALID, "mrt_counted_merge: out may be a itself; any other overlap with an input is invalid");
  mrt::MergeArgs m{};
  m.a = reinterpret_cast<const float4*>(a);
  m.b = reinterpret_cast<const float4*>(b);
  m.out = reinterpret_cast<float4*>(out);
  m.count = W * H;
  HIP_TRY(MRT_BUILD_CALL(flags, launch_counted_merge(m, (hipStream_t)stream)));
  return MRT_OK;
}

int mrt_tile_priority(const float* image, const float* variance, const float* guide_n, float* priority, uint32_t W,
                      uint32_t H, const mrt_adaptive_params* params, uint32_t flags, void* stream) {
  if (!image || !variance || !guide_n || !priority || !params || W == 0 || H == 0 || W > 32768 || H > 32768)
    return fail(MRT_ERR_INVALID, "mrt_tile_priority: bad argument");
  const int rc = mrt_adaptive_params_check(params);
  if (rc) return rc;
  const uint32_t tx = (W + mrt::kTile - 1) / mrt::kTile, ty = (H + mrt::kTile - 1) / mrt::kTile;
  const size_t bytes = (size_t)W * H * 16, out_bytes = (size_t)tx * ty * 4;
  if (written_overlap({{image, bytes}, {variance, bytes / 4}, {guide_n, bytes}, {priority, out_bytes, true}}))
    return fail(MRT_ERR_INVALID, "mrt_tile_priority: priority must not overlap an input");
  mrt::PriorityArgs a{};
  a.image = reinterpret_cast<const float4*>(image);
  a.variance = variance;
  a.guide_n = reinterpret_cast<const float4*>(guide_n);
  a.priority = priority;
  a.width = W;
  a.height = H;
  a.tiles_x = tx;
  a.eps2 = params->luminance_floor * params->luminance_floor;
  HIP_TRY(MRT_BUILD_CALL(flags, launch_tile_priority(a, tx * ty, (hipStream_t)stream)));
  return MRT_OK;
}

int mrt_tile_select(const float* priority, uint32_t tiles, uint32_t count, uint32_t* list, void* stream) {
  if (!priority || !list) return fail(MRT_ERR_INVALID, "mrt_tile_select: null argument");
  if (count == 0 || count > tiles || tiles > mrt::kMaxSelectTiles)
    return fail(MRT_ERR_INVALID, "mrt_tile_select: need 1 <= count <= tiles <= 16384");
  if (spans_overlap({priority, (size_t)tiles * 4}, {list, (size_t)count * 4}))
    return fail(MRT_ERR_INVALID, "mrt_tile_select: list must not overlap priority");
  HIP_TRY(mrt::fast::launch_tile_select(priority, tiles, count, list, (hipStream_t)stream));   // exact: one code in both builds
  return MRT_OK;
}

int mrt_tile_error(const float* image, const float* variance, const float* guide_n, float* mean_error, uint32_t* pixels,
                   uint32_t W, uint32_t H, const mrt_adaptive_params* params, uint32_t flags, void* stream) {
  if (!image || !variance || !guide_n || !mean_error || !pixels || !params || W == 0 || H == 0 || W > 32768 || H > 32768)
    return fail(MRT_ERR_INVALID, "mrt_tile_error: bad argument");
  const int rc = mrt_adaptive_params_check(params);
  if (rc) return rc;
  const uint32_t tx = (W + mrt::kTile - 1) / mrt::kTile, ty = (H + mrt::kTile - 1) / mrt::kTile;
  const size_t bytes = (size_t)W * H * 16, out_bytes = (size_t)tx * ty * 4;
  const Span in[] = {{image, bytes}, {variance, bytes / 4}, {guide_n, bytes}};
  const Span out[] = {{mean_error, out_bytes}, {pixels, out_bytes}};
  for (const Span& o : out)
    for (const Span& b : in)
      if (spans_overlap(o, b)) return fail(MRT_ERR_INVALID, "mrt_tile_error: an output must not overlap an input");
  if (spans_overlap(out[0], out[1])) return fail(MRT_ERR_INVALID, "mrt_tile_error: mean_error and pixels must not overlap");
  mrt::ErrorArgs a{};
  a.p.image = reinterpret_cast<const float4*>(image);
  a.p.variance = variance;
  a.p.guide_n = reinterpret_cast<const float4*>(guide_n);
  a.p.priority = mean_error;
  a.p.width = W;
  a.p.height = H;
  a.p.tiles_x = tx;
  a.p.eps2 = params->luminance_floor * params->luminance_floor;
  a.pixels = pixels;
  HIP_TRY(MRT_BUILD_CALL(flags, launch_tile_error(a, tx * ty, (hipStream_t)stream)));
  return MRT_OK;
}

static_assert(sizeof(mrt_error_summary) == sizeof(mrt::ErrorSummary) && sizeof(mrt_error_summary) == 32 &&
                  offsetof(mrt_error_summary, pixels) == offsetof(mrt::ErrorSummary, pixels),
              "mrt_error_summary and the kernels' copy of it");

int mrt_tile_threshold(const float* mean_error, const uint32_t* pixels, uint32_t tiles, float threshold,
                       uint32_t max_count, uint32_t* list, mrt_error_summary* summary, void* stream) {
  if (!mean_error || !pixels || !list || !summary) return fail(MRT_ERR_INVALID, "mrt_tile_threshold: null argument");
  if (!std::isfinite(threshold) || threshold < 0.0f)
    return fail(MRT_ERR_INVALID, "mrt_tile_threshold: threshold must be finite and not negative");
  if (tiles == 0 || tiles > mrt::kMaxSelectTiles || max_count == 0 || max_count > tiles)
    return fail(MRT_ERR_INVALID, "mrt_tile_threshold: need 1 <= max_count <= tiles <= 16384");
  const Span b[] = {{mean_error, (size_t)tiles * 4}, {pixels, (size_t)tiles * 4}, {list, (size_t)max_count * 4},
                    {summary, sizeof(mrt_error_summary)}};
  for (int i = 0; i < 4; ++i)
    for (int j = i + 1; j < 4; ++j)
      if (spans_overlap(b[i], b[j])) return fail(MRT_ERR_INVALID, "mrt_tile_threshold: the buffers must not overlap");
  mrt::ThresholdArgs a{};
  a.mean_error = mean_error;
  a.pixels = pixels;
  a.list = list;
  a.summary = reinterpret_cast<mrt::ErrorSummary*>(summary);
  a.tiles = tiles;
  a.max_count = max_count;
  a.threshold = threshold;
  HIP_TRY(mrt::fast::launch_tile_threshold(a, (hipStream_t)stream));   // exact: one code in both builds
  return MRT_OK;
}

int mrt_converge_params_default(mrt_converge_params* out) {
  if (!out) return fail(MRT_ERR_INVALID, "mrt_converge_params_default: null params");
  out->target_error = 1e-3f;
  out->frames_per_pass = 8;
  out->max_passes = 64;
  out->max_tiles = 0;
  out->max_tile_frames = 0;
  out->luminance_floor = 0.01f;
  return MRT_OK;
}

int mrt_converge_params_check(const mrt_converge_params* p) {
  if (!p) return fail(MRT_ERR_INVALID, "converge params: null");
  if (!std::isfinite(p->target_error) || !(p->target_error > 0.0f))
    return fail(MRT_ERR_INVALID, "converge params: target_error must be finite and positive");
  if (p->frames_per_pass < 1) return fail(MRT_ERR_INVALID, "converge params: frames_per_pass must be at least 1");
  if (p->max_passes < 1) return fail(MRT_ERR_INVALID, "converge params: max_passes must be at least 1");
  if (!std::isfinite(p->luminance_floor) || !(p->luminance_floor > 0.0f))
    return fail(MRT_ERR_INVALID, "converge params: luminance_floor must be finite and positive");
  return MRT_OK;
}

// ---- temporal history (include/mrt.h) --------------------------------------
int mrt_reproject_params_default(mrt_reproject_params* out) {
  if (!out) return fail(MRT_ERR_INVALID, "mrt_reproject_params_default: null params");
  out->plane_tolerance = 0.01f;
  out->normal_cos_min = 0.9f;
  out->max_history = 32.0f;
  return MRT_OK;
}

int mrt_reproject_params_check(const mrt_reproject_params* p) {
  if (!p) return fail(MRT_ERR_INVALID, "reproject params: null");
  if (!std::isfinite(p->plane_tolerance) || !(p->plane_tolerance > 0.0f))
    return fail(MRT_ERR_INVALID, "reproject params: plane_tolerance must be finite and positive");
  if (!std::isfinite(p->normal_cos_min) || p->normal_cos_min < -1.0f || p->normal_cos_min > 1.0f)
    return fail(MRT_ERR_INVALID, "reproject params: normal_cos_min must be in [-1, 1]");
  if (!std::isfinite(p->max_history) || p->max_history < 0.0f)
    return fail(MRT_ERR_INVALID, "reproject params: max_history must be finite and not negative");
  return MRT_OK;
}


int mrt_temporal_resolve(const float* image, uint64_t frames, const float* history, float* out, uint32_t W, uint32_t H,
                         void* stream) {
  if (!image || !out || W == 0 || H == 0 || W > 32768 || H > 32768)
    return fail(MRT_ERR_INVALID, "mrt_temporal_resolve: bad argument");
  const size_t bytes = (size_t)W * H * 16;
  if (written_overlap({{image, bytes}, {history, bytes}, {out, bytes, true}}))
    return fail(MRT_ERR_INVALID, "mrt_temporal_resolve: out must not overlap image or history");
  mrt::ResolveArgs a{};
  a.image = reinterpret_cast<const float4*>(image);
  a.history = reinterpret_cast<const float4*>(history);
  a.out = reinterpret_cast<float4*>(out);
  a.count = W * H;
  a.frames = (float)frames;
  HIP_TRY(mrt::launch_temporal_resolve(a, (hipStream_t)stream));
  return MRT_OK;
}

int mrt_reproject(const float* prev, const float* prev_guide_n, const float* prev_guide_p, const mrt_camera* prev_cam,
                  const float* cur_guide_n, const float* cur_guide_p, float* history_out, uint32_t W, uint32_t H,
                  const mrt_reproject_params* params, void* stream) {
  if (!prev || !prev_guide_n || !prev_guide_p || !cur_guide_n || !cur_guide_p || !history_out || !params || W < 2 ||
      H < 2 || W > 32768 || H > 32768)
    return fail(MRT_ERR_INVALID, "mrt_reproject: bad argument");
  const size_t bytes = (size_t)W * H * 16;
  if (written_overlap({{prev, bytes}, {prev_guide_n, bytes}, {prev_guide_p, bytes}, {cur_guide_n, bytes},
                       {cur_guide_p, bytes}, {history_out, bytes, true}}))
    return fail(MRT_ERR_INVALID, "mrt_reproject: history_out must not overlap an input");
  int rc = mrt_reproject_params_check(params);
  if (rc) return rc;
  mrt_camera c;
  if (prev_cam) {
    rc = mrt_camera_check(prev_cam);
    if (rc) return rc;
    c = *prev_cam;
  } else {
    (void)mrt_camera_default(&c);
  }
  mrt::ReprojectArgs a{};
  a.prev = reinterpret_cast<const float4*>(prev);
  a.prev_n = reinterpret_cast<const float4*>(prev_guide_n);
  a.prev_p = reinterpret_cast<const float4*>(prev_guide_p);
  a.cur_n = reinterpret_cast<const float4*>(cur_guide_n);
  a.cur_p = reinterpret_cast<const float4*>(cur_guide_p);
  a.out = reinterpret_cast<float4*>(history_out);
  a.width = W;
  a.height = H;
  for (int k = 0; k < 3; ++k) {
    a.origin[k] = c.origin[k];
    a.right[k] = c.right[k];
    a.up[k] = c.up[k];
    a.forward[k] = c.forward[k];
  }
  a.tan_half_fov = c.tan_half_fov;   // the lens is ignored, as the guide pass ignores it
  a.plane_tolerance = params->plane_tolerance;
  a.normal_cos_min = params->normal_cos_min;
  a.max_history = params->max_history;
  HIP_TRY(mrt::launch_reproject(a, (hipStream_t)stream));
  return MRT_OK;
}

int mrt_intersect(const mrt_scene* scene, const void* rays, uint32_t stride, uint32_t count, void* isect,
                  uint32_t flags, void* stream) {
  if (!scene || (!rays && count) || (!isect && count) || stride < 32 || (stride % 4))
    return fail(MRT_ERR_INVALID, "mrt_intersect: bad argument");
  HIP_TRY(MRT_BUILD_CALL(flags, launch_intersect(scene->dev, rays, stride, count, (mrt::RefIntersection*)isect,
                                                 scene->isect_spill.as<uint32_t>(), (hipStream_t)stream)));
  return MRT_OK;
}

int mrt_shade(const mrt_scene* scene, uint32_t W, uint32_t H, uint32_t frame_index, uint32_t L, const float* noise,
              const void* isect, void* rays, void* srays, uint32_t flags, void* stream) {
  if (!scene || !noise || !isect || !rays || !srays || W == 0 || H == 0 || L == 0)
    return fail(MRT_ERR_INVALID, "mrt_shade: bad argument");
  HIP_TRY(MRT_BUILD_CALL(flags, launch_shade(scene->dev, W, H, frame_index, L, noise, (const mrt::RefIntersection*)isect,
                                             (mrt::RefRay*)rays, (mrt::RefShadowRay*)srays,
                                             (flags & MRT_FLAG_DEBUG_MATERIAL) ? mrt::kShadeDebugMaterial : 0u,
                                             (hipStream_t)stream)));
  return MRT_OK;
}

int mrt_resolve_shadow(const mrt_scene* scene, uint32_t count, const void* isect, void* rays, const void* srays,
                       uint32_t flags, void* stream) {
  if (!scene || (count && (!isect || !rays || !srays))) return fail(MRT_ERR_INVALID, "mrt_resolve_shadow: bad argument");
  HIP_TRY(MRT_BUILD_CALL(flags, launch_resolve(count, (const mrt::RefIntersection*)isect, (mrt::RefRay*)rays,
                                               (const mrt::RefShadowRay*)srays, (hipStream_t)stream)));
  return MRT_OK;
}

int mrt_accumulate(const mrt_scene* scene, uint32_t W, uint32_t H, uint32_t frame_index, const void* rays,
                   float* image, uint32_t flags, void* stream) {
  if (!scene || !rays || !image || W == 0 || H == 0) return fail(MRT_ERR_INVALID, "mrt_accumulate: bad argument");
  HIP_TRY(MRT_BUILD_CALL(flags, launch_accumulate(W, H, frame_index, (const mrt::RefRay*)rays, image,
                                                  !(flags & MRT_FLAG_NO_ACCUMULATE), (hipStream_t)stream)));
  return MRT_OK;
}

int mrt_moments(const mrt_scene* scene, uint32_t W, uint32_t H, uint32_t frame_index, const void* rays,
                float* moments, uint32_t flags, void* stream) {
  if (!scene || !rays || !moments || W == 0 || H == 0) return fail(MRT_ERR_INVALID, "mrt_moments: bad argument");
  HIP_TRY(MRT_BUILD_CALL(flags, launch_moments(W, H, frame_index, (const mrt::RefRay*)rays, moments,
                                               (hipStream_t)stream)));
  return MRT_OK;
}

int mrt_image_load_exr(const char* path, float* rgba, size_t capacity, uint32_t* width, uint32_t* height) {
  if (!path || !width || !height) return fail(MRT_ERR_INVALID, "mrt_image_load_exr: null argument");
  std::vector<float> img;
  uint32_t W = 0, H = 0;
  std::string err;
  if (!mrt::load_exr(path, img, W, H, err)) return fail(MRT_ERR_IO, err);
  *width = W;
  *height = H;
  if (!rgba) return MRT_OK;
  if (capacity < img.size()) return fail(MRT_ERR_INVALID, "mrt_image_load_exr: buffer too small");
  std::memcpy(rgba, img.data(), img.size() * 4);
  return MRT_OK;
}

}  // extern "C"
