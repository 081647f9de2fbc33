// renderer_post.cpp — the images a renderer derives from what it accumulated
// (include/mrt.h): the guide planes, the denoised and the resolved buffer, the
// temporal history, the variance plane, the firefly clamp, the extra images and
// tile planes of adaptive sampling, the error estimate, and the display blit.
// Everything here is enqueued on the renderer's main stream, behind its draws.
// (The renderer itself, its cameras and its draw loop: renderer.cpp.)
//
// Every derived buffer is made by the first call that needs it and, once it
// exists, re-made by a resize (post_resize: the one list of them); a `*_current`
// flag says whether it was computed at the renderer's current size.
#include <cmath>

#include "host_internal.h"
#include "image.h"

using namespace mrt::host;

namespace {

size_t image_bytes(const mrt_renderer* r) { return (size_t)r->desc.width * r->desc.height * 16; }

// Size every buffer of `group` to `bytes`; the group's `current` flag falls
// when one had to be made (the first use, or the first use after a failure)
int size_group(std::initializer_list<DevBuf*> group, size_t bytes, bool* current = nullptr) {
  for (DevBuf* b : group)
    if (b->bytes != bytes || !b->p) {
      if (current) *current = false;
      HIP_TRY(b->alloc(bytes));
    }
  return MRT_OK;
}

// `type p`: *given, or the default that `dflt` writes to &p; returns what `check` finds wrong with it
#define PARAMS_OR_DEFAULT(type, p, given, dflt, check) \
  type p;                                              \
  if (given) p = *(given);                             \
  else (void)(dflt);                                   \
  if (const int bad_ = check(&p)) return bad_

// the guide planes of the camera in force, on the main stream (allocated here
// when nothing has made them yet, traced when they are not the camera's)
int ensure_guides(mrt_renderer* r) {
  const uint32_t W = r->desc.width, H = r->desc.height;
  int rc = size_group({&r->guide_n, &r->guide_p}, image_bytes(r), &r->guides_current);
  if (rc) return rc;
  if (r->guides_current) return MRT_OK;
  if (!r->guide_spill.p) HIP_TRY(alloc_isect_spill(r->guide_spill, r->scene->dev.max_stack));
  rc = guides_with_spill(r->scene, &r->camera, W, H, r->guide_n.as<float>(), r->guide_p.as<float>(),
                         r->desc.flags & MRT_FLAG_PRECISE, r->guide_spill.as<uint32_t>(), r->stream);
  if (rc) return rc;
  r->guides_current = true;
  return MRT_OK;
}

// mrt_renderer_denoise / _denoise_resolved: the A-Trous filter of `src` with the
// guide planes of the camera in force, into the (sized) denoised buffer
int atrous(mrt_renderer* r, const float* src, const mrt_denoise_params& p) {
  int rc = ensure_guides(r);
  if (rc) return rc;
  rc = mrt_denoise(src, r->guide_n.as<float>(), r->guide_p.as<float>(), r->denoised.as<float>(),
                   r->denoise_scratch.as<float>(), r->desc.width, r->desc.height, &p, r->stream);
  if (rc) return rc;
  r->denoised_current = true;
  return MRT_OK;
}

int temporal_usable(const mrt_renderer* r, const char* what) {
  if (!r) return fail(MRT_ERR_INVALID, "null renderer");
  if (r->desc.shard_count > 1)
    return fail(MRT_ERR_STATE, std::string(what) + ": a sharded renderer keeps no temporal history");
  return MRT_OK;
}

// resolve(`image`, frame_index, `history` if valid) into `out`, on the main
// stream; while the extra image E holds samples (adaptive sampling), followed
// by the counted merge with `extra`: out = merge(out, extra), in place
int resolve_into(mrt_renderer* r, const float* image, const DevBuf& history, const DevBuf& extra, DevBuf& out) {
  int rc = size_group({&out}, image_bytes(r));
  if (rc) return rc;
  rc = mrt_temporal_resolve(image, r->frame_index, r->history_valid ? history.as<float>() : nullptr, out.as<float>(),
                            r->desc.width, r->desc.height, r->stream);
  if (rc || !r->extras_valid) return rc;
  return mrt_counted_merge(out.as<float>(), extra.as<float>(), out.as<float>(), r->desc.width, r->desc.height,
                           r->desc.flags & MRT_FLAG_PRECISE, r->stream);
}
int resolve_image_into(mrt_renderer* r, DevBuf& out) { return resolve_into(r, r->image, r->history, r->extra, out); }
// the same for the moments image and its history (MRT_FLAG_MOMENTS)
int resolve_moments_into(mrt_renderer* r, DevBuf& out) {
  return resolve_into(r, r->moments.as<float>(), r->moments_history, r->extra_moments, out);
}

// What mrt_renderer_denoise_variance and mrt_renderer_refine share: the
// resolved buffer, the resolved moments and, from them and the guide planes, the
// variance plane.  clamp: while firefly suppression is on, the clamped copy of
// the resolved buffer too — ahead of the variance estimate on the stream
int variance_inputs(mrt_renderer* r, const mrt_svgf_params& p, bool clamp) {
  const uint32_t W = r->desc.width, H = r->desc.height;
  const size_t bytes = image_bytes(r);
  int rc = size_group({&r->variance}, bytes / 4, &r->variance_current);
  if (rc) return rc;
  rc = ensure_guides(r);
  if (rc) return rc;
  rc = mrt_renderer_resolve(r);
  if (rc) return rc;
  rc = resolve_moments_into(r, r->moments_resolved);
  if (rc) return rc;
  if (clamp && r->firefly_on) {   // 16 B per pixel and, behind them, the counter of changed pixels
    rc = size_group({&r->clamped}, bytes + 16, &r->clamped_current);
    if (rc) return rc;
    rc = mrt_firefly_clamp(r->resolved.as<float>(), r->guide_n.as<float>(), r->guide_p.as<float>(),
                           r->clamped.as<float>(), reinterpret_cast<uint32_t*>(r->clamped.as<char>() + bytes), W, H,
                           &r->firefly, r->stream);
    if (rc) return rc;
    r->clamped_current = true;
  }
  rc = mrt_variance(r->moments_resolved.as<float>(), r->guide_n.as<float>(), r->guide_p.as<float>(),
                    r->variance.as<float>(), W, H, &p, r->stream);
  if (rc) return rc;
  r->variance_current = true;
  return MRT_OK;
}

// ---- adaptive sampling (include/mrt.h: mrt_renderer_refine) ----
int refine_usable(const mrt_renderer* r, const char* what) {
  if (!r) return fail(MRT_ERR_INVALID, "null renderer");
  if (!(r->desc.flags & MRT_FLAG_MOMENTS))
    return fail(MRT_ERR_STATE, std::string(what) + ": the renderer was created without MRT_FLAG_MOMENTS");
  if (r->desc.shard_count > 1) return fail(MRT_ERR_STATE, std::string(what) + ": not on a sharded renderer");
  if (r->desc.flags & MRT_FLAG_STATIC_NOISE)
    return fail(MRT_ERR_STATE, std::string(what) + ": not with MRT_FLAG_STATIC_NOISE (every extra frame would repeat)");
  if (r->plan.kind == mrt::KernelKind::Bounce)
    return fail(MRT_ERR_STATE, std::string(what) + ": the per-bounce kernel has no tile-list instantiation");
  return MRT_OK;
}

// E, EM, the list, the priorities, the second noise schedule and the list's
// event: made at the first refine / draw_tiles, E and EM zeroed on the main stream
int ensure_extras(mrt_renderer* r) {
  HIP_TRY(hipSetDevice(r->scene->device));
  const size_t bytes = image_bytes(r);
  HIP_TRY(r->list_ready.ensure(hipEventDisableTiming));
  if (!r->refine_noise) {
    r->refine_noise = std::make_unique<mrt::NoiseSchedule>(r->desc.seed ^ MRT_REFINE_SEED_XOR, false);
    HIP_TRY(r->refine_noise->init());
  }
  int rc = size_group({&r->extra, &r->extra_moments}, bytes, &r->extras_current);
  if (rc) return rc;
  bool kept = true;   // a list that had to be made holds nothing
  rc = size_group({&r->tile_list, &r->tile_priority}, (size_t)r->tiles_x * r->tiles_y * 4, &kept);
  if (!kept) {
    r->priority_current = false;
    r->list_count = 0;
  }
  if (rc) return rc;
  if (!r->extras_current) {
    HIP_TRY(hipMemsetAsync(r->extra.p, 0, bytes, r->stream));
    HIP_TRY(hipMemsetAsync(r->extra_moments.p, 0, bytes, r->stream));
    r->extras_current = true;
    r->extras_valid = false;
  }
  return MRT_OK;
}

// `frames` extra frames of the `count` tiles of the device list (host_list:
// uploaded first) into E / EM, from the refine schedule at the extra-frame counter
int draw_extra(mrt_renderer* r, const uint32_t* host_list, uint32_t count, uint32_t frames) {
  DrawSource src;
  src.noise = r->refine_noise.get();
  src.f0 = r->refine_stats.extra_frames;
  src.tiles = count;
  src.list = r->tile_list.as<uint32_t>();
  src.host_list = host_list;
  src.image = r->extra.as<float>();
  src.moments = r->extra_moments.as<float>();
  r->refine_stats.extra_frames += frames;   // whatever becomes of the draw: no noise is ever read twice
  const int rc = draw_frames(r, frames, src);
  if (rc) return rc;
  r->extras_valid = true;
  r->list_count = count;
  r->refine_stats.passes += 1;
  r->refine_stats.tile_frames += (uint64_t)count * frames;
  return MRT_OK;
}

// ---- sampling to a target error (include/mrt.h: mrt_renderer_converge) -------
// everything an estimate checks, before it changes anything
int estimate_usable(mrt_renderer* r, const char* what, const mrt_svgf_params& sp, const mrt_adaptive_params& ap,
                    float threshold) {
  int rc = refine_usable(r, what);
  if (rc) return rc;
  if (r->tiles_x * r->tiles_y > mrt::kMaxSelectTiles)
    return fail(MRT_ERR_INVALID, std::string(what) + ": more than 16384 tiles");
  if (!std::isfinite(threshold) || threshold < 0.0f)
    return fail(MRT_ERR_INVALID, std::string(what) + ": the threshold must be finite and not negative");
  rc = mrt_svgf_params_check(&sp);
  if (rc) return rc;
  rc = mrt_adaptive_params_check(&ap);
  if (rc) return rc;
  if (r->frame_index < sp.min_frames && !r->history_valid)
    return fail(MRT_ERR_STATE, std::string(what) + ": fewer than min_frames frames accumulated and no valid history");
  return MRT_OK;
}

// one estimate (estimate_usable has passed): denoise_variance, the per-tile
// error, the tiles above `threshold` into the tile list, and the summary
// brought to the host — the one host wait
int estimate(mrt_renderer* r, const mrt_svgf_params& sp, const mrt_adaptive_params& ap, float threshold,
             mrt_error_summary* out) {
  const uint32_t W = r->desc.width, H = r->desc.height, T = r->tiles_x * r->tiles_y;
  int rc = ensure_extras(r);   // (the tile list lives with E and EM)
  if (rc) return rc;
  rc = size_group({&r->tile_error, &r->tile_pixels}, (size_t)T * 4, &r->tile_error_current);
  if (rc) return rc;
  if (!r->error_summary.p) HIP_TRY(r->error_summary.alloc(sizeof(mrt_error_summary)));
  HIP_TRY(r->summary_host.reserve(sizeof(mrt_error_summary), hipHostMallocDefault));
  rc = mrt_renderer_denoise_variance(r, &sp);
  if (rc) return rc;
  rc = mrt_tile_error(r->denoised.as<float>(), r->variance.as<float>(), r->guide_n.as<float>(),
                      r->tile_error.as<float>(), r->tile_pixels.as<uint32_t>(), W, H, &ap,
                      r->desc.flags & MRT_FLAG_PRECISE, r->stream);
  if (rc) return rc;
  r->tile_error_current = true;
  r->list_count = 0;   // the list is rewritten: nothing of it is known until the summary is back
  rc = mrt_tile_threshold(r->tile_error.as<float>(), r->tile_pixels.as<uint32_t>(), T, threshold, T,
                          r->tile_list.as<uint32_t>(), r->error_summary.as<mrt_error_summary>(), r->stream);
  if (rc) return rc;
  HIP_TRY(hipMemcpyAsync(r->summary_host.host(), r->error_summary.p, sizeof(mrt_error_summary), hipMemcpyDeviceToHost, r->stream));
  HIP_TRY(hipStreamSynchronize(r->stream));
  *out = *r->summary_host.host<mrt_error_summary>();
  r->list_count = out->tiles_listed;
  return MRT_OK;
}

// mrt_renderer_display / _display_enqueue: what is wrong with `flags` for this
// renderer as it stands, else the image they name in *src
int display_source(mrt_renderer* r, uint32_t flags, const float** src) {
  if (((flags >> 8) & 0xFFu) && !r->reference.p) return fail(MRT_ERR_STATE, "compare mode without a loaded reference");
  const bool denoised = (flags & MRT_DISPLAY_DENOISED) != 0;
  const bool resolved = (flags & MRT_DISPLAY_RESOLVED) != 0;
  if (denoised && resolved) return fail(MRT_ERR_INVALID, "MRT_DISPLAY_DENOISED and MRT_DISPLAY_RESOLVED are exclusive");
  if (denoised && !r->denoised_current) return fail(MRT_ERR_STATE, "MRT_DISPLAY_DENOISED without a denoise at the current size");
  if (resolved && !r->resolved_current) return fail(MRT_ERR_STATE, "MRT_DISPLAY_RESOLVED without a resolve at the current size");
  *src = denoised ? r->denoised.as<float>() : (resolved ? r->resolved.as<float>() : r->image);
  return MRT_OK;
}

// the blit of `src` into the one device blit buffer (the next blit is queued
// behind the copy out of it), then that copy to `host`
int display_to(mrt_renderer* r, const float* src, uint32_t flags, float compare_scale, float* host) {
  const size_t bytes = image_bytes(r);
  int rc = exchange_flush(r);
  if (rc) return rc;
  if (r->display.bytes < bytes) HIP_TRY(r->display.alloc(bytes));
  rc = mrt_display(src, r->reference.as<float>(), r->display.as<float>(), r->desc.width, r->desc.height, flags,
                   compare_scale, r->stream);
  if (rc) return rc;
  HIP_TRY(hipMemcpyAsync(host, r->display.p, bytes, hipMemcpyDeviceToHost, r->stream));
  return MRT_OK;
}

// no derived plane, history or extra image describes what the renderer holds (resize, a scene swap)
void stale_all(mrt_renderer* r) {
  r->guides_current = r->denoised_current = r->history_valid = r->resolved_current = false;
  r->variance_current = r->clamped_current = r->priority_current = r->tile_error_current = false;
  r->extras_current = r->extras_valid = false;   // re-made (and zeroed) by the next refine / draw_tiles
  r->list_count = 0;
}

const char kNoExtras[] = "no refine or draw_tiles has run at the renderer's current size";

}  // namespace

namespace mrt {
namespace host {

// mrt_renderer_resize: no derived plane is of the new size, and each buffer
// that exists is re-made for it (one that does not is made by its first use)
int post_resize(mrt_renderer* r) {
  stale_all(r);
  const size_t px = image_bytes(r);
  const size_t tiles = (size_t)((r->desc.width + mrt::kTile - 1) / mrt::kTile) *   // (tiles_x / _y are still the old size's)
                       ((r->desc.height + mrt::kTile - 1) / mrt::kTile) * 4;
  const struct { DevBuf* b; size_t bytes; } all[] = {
      {&r->guide_n, px},        {&r->guide_p, px},         {&r->denoised, px},         {&r->denoise_scratch, px},
      {&r->prev_guide_n, px},   {&r->prev_guide_p, px},    {&r->temporal_prev, px},    {&r->history, px},
      {&r->resolved, px},       {&r->moments_prev, px},    {&r->moments_history, px},  {&r->moments_resolved, px},
      {&r->variance, px / 4},   {&r->clamped, px + 16},    {&r->extra, px},            {&r->extra_moments, px},
      {&r->tile_list, tiles},   {&r->tile_priority, tiles}, {&r->tile_error, tiles},   {&r->tile_pixels, tiles},
      {&r->motion_n, px},       {&r->motion_p, px}};
  for (const auto& e : all)
    if (e.b->p && e.b->bytes != e.bytes) HIP_TRY(e.b->alloc(e.bytes));
  return MRT_OK;
}

// mrt_renderer_set_scene / _move_scene: nothing derived from the old scene's
// image describes the new one; the buffers keep their size, but for the guide
// pass's stack spill where its rows were of another tree's depth (ensure_guides
// makes it again; one of the right size is kept)
int post_set_scene(mrt_renderer* r) {
  stale_all(r);
  const uint32_t depth = r->scene->dev.max_stack;
  const size_t want =   // (alloc_isect_spill's rule)
      depth <= (uint32_t)mrt::kMaxStack ? 0 : (size_t)depth * mrt::kIntersectSpillGrid * 256 * 4;
  if (r->guide_spill.bytes != want) HIP_TRY(r->guide_spill.alloc(0));
  return MRT_OK;
}

// mrt_renderer_reset: the extra samples go with the frames they refined
// (stream-ordered behind the pending draws)
int post_reset(mrt_renderer* r) {
  if (!r->extras_valid) return MRT_OK;
  HIP_TRY(hipMemsetAsync(r->extra.p, 0, image_bytes(r), r->stream));
  HIP_TRY(hipMemsetAsync(r->extra_moments.p, 0, image_bytes(r), r->stream));
  r->extras_valid = false;
  return MRT_OK;
}

}  // namespace host
}  // namespace mrt

extern "C" {

int mrt_renderer_denoise(mrt_renderer* r, const mrt_denoise_params* params) {
  if (!r) return fail(MRT_ERR_INVALID, "null renderer");
  if (r->frame_index == 0)
    return fail(MRT_ERR_STATE, "mrt_renderer_denoise: no frame accumulated since create, resize, reset or set_camera");
  PARAMS_OR_DEFAULT(mrt_denoise_params, p, params, mrt_denoise_params_default(r->frame_index, &p), mrt_denoise_params_check);
  HIP_TRY(hipSetDevice(r->scene->device));
  int rc = size_group({&r->denoised, &r->denoise_scratch}, image_bytes(r), &r->denoised_current);
  if (rc) return rc;
  rc = exchange_flush(r);   // a deferred (overlapped) exchange lands in the image first
  return rc ? rc : atrous(r, r->image, p);
}

int mrt_renderer_read_denoised(mrt_renderer* r, float* rgba, size_t count) {
  return read_back(r, rgba, count, [](const mrt_renderer* r) {
    return ReadSpec{image_bytes(r) / 4, r->denoised.p, r->denoised_current, "no denoise has run at the renderer's current size"};
  });
}

int mrt_renderer_save_denoised(mrt_renderer* r, const char* path) { return save_read(r, path, mrt_renderer_read_denoised); }

// ---- temporal history (include/mrt.h: mrt_renderer_move_camera) -------------
int mrt_renderer_move_camera(mrt_renderer* r, const mrt_camera* cam, const mrt_reproject_params* params) {
  int rc = temporal_usable(r, "mrt_renderer_move_camera");
  if (rc) return rc;
  rc = mrt_camera_check(cam);
  if (rc) return rc;
  PARAMS_OR_DEFAULT(mrt_reproject_params, p, params, mrt_reproject_params_default(&p), mrt_reproject_params_check);
  if (r->frame_index == 0 && !r->history_valid) return mrt_renderer_set_camera(r, cam);   // nothing to carry
  const uint32_t W = r->desc.width, H = r->desc.height;
  HIP_TRY(hipSetDevice(r->scene->device));
  rc = size_group({&r->prev_guide_n, &r->prev_guide_p, &r->temporal_prev, &r->history}, image_bytes(r));   // the first move only
  if (rc) return rc;
  const bool moments = (r->desc.flags & MRT_FLAG_MOMENTS) != 0;
  if (moments) {
    rc = size_group({&r->moments_prev, &r->moments_history}, image_bytes(r));
    if (rc) return rc;
  }
  // what the old camera saw: its guide planes, and everything accumulated
  // through it (a scratch image: the history itself is replaced last)
  rc = ensure_guides(r);
  if (rc) return rc;
  rc = resolve_image_into(r, r->temporal_prev);
  if (rc) return rc;
  if (moments) {   // the moments travel with the colour, through the same two kernels
    rc = resolve_moments_into(r, r->moments_prev);
    if (rc) return rc;
  }
  // the new camera, as mrt_renderer_set_camera installs it: failing here
  // leaves the previous camera in force, nothing reset, the history as it was
  const mrt_camera old = r->camera;
  rc = swap_camera(r, *cam);
  if (rc) return rc;
  std::swap(r->guide_n.p, r->prev_guide_n.p);   // equal sizes: the planes of `old` become the previous ones
  std::swap(r->guide_p.p, r->prev_guide_p.p);
  r->history_valid = false;     // from here on a failure leaves the new camera without a history, as set_camera would
  rc = mrt_renderer_reset(r);
  if (rc) return rc;
  rc = ensure_guides(r);
  if (rc) return rc;
  rc = mrt_reproject(r->temporal_prev.as<float>(), r->prev_guide_n.as<float>(), r->prev_guide_p.as<float>(), &old,
                     r->guide_n.as<float>(), r->guide_p.as<float>(), r->history.as<float>(), W, H, &p, r->stream);
  if (rc) return rc;
  if (moments) {
    rc = mrt_reproject(r->moments_prev.as<float>(), r->prev_guide_n.as<float>(), r->prev_guide_p.as<float>(), &old,
                       r->guide_n.as<float>(), r->guide_p.as<float>(), r->moments_history.as<float>(), W, H, &p,
                       r->stream);
    if (rc) return rc;
  }
  r->history_valid = true;
  return MRT_OK;
}

// ---- moving geometry (include/mrt.h: mrt_renderer_move_scene) ----------------
int mrt_renderer_move_scene(mrt_renderer* r, const mrt_scene* scene, const mrt_camera* cam,
                            const mrt_reproject_params* params) {
  int rc = temporal_usable(r, "mrt_renderer_move_scene");
  if (rc) return rc;
  if (!scene) return fail(MRT_ERR_INVALID, "mrt_renderer_move_scene: null scene");
  if (cam) {
    rc = mrt_camera_check(cam);
    if (rc) return rc;
  }
  PARAMS_OR_DEFAULT(mrt_reproject_params, p, params, mrt_reproject_params_default(&p), mrt_reproject_params_check);
  if (scene->device != r->scene->device)
    return fail(MRT_ERR_INVALID, scene->device < 0 ? "mrt_renderer_move_scene: a host-only scene has nothing on a device"
                                                   : "mrt_renderer_move_scene: the scene is on another device than the renderer");
  rc = mrt_scene_motion_compatible(r->scene, scene);
  if (rc) return rc;
  if (r->frame_index == 0 && !r->history_valid) return swap_scene(r, scene, cam);   // nothing to carry
  const uint32_t W = r->desc.width, H = r->desc.height;
  HIP_TRY(hipSetDevice(r->scene->device));
  rc = size_group({&r->prev_guide_n, &r->prev_guide_p, &r->temporal_prev, &r->history, &r->motion_n, &r->motion_p},
                  image_bytes(r));   // the first move only
  if (rc) return rc;
  const bool moments = (r->desc.flags & MRT_FLAG_MOMENTS) != 0;
  if (moments) {
    rc = size_group({&r->moments_prev, &r->moments_history}, image_bytes(r));
    if (rc) return rc;
  }
  // as mrt_renderer_move_camera: what the old camera saw of the old scene
  rc = ensure_guides(r);
  if (rc) return rc;
  rc = resolve_image_into(r, r->temporal_prev);
  if (rc) return rc;
  if (moments) {
    rc = resolve_moments_into(r, r->moments_prev);
    if (rc) return rc;
  }
  // the swap, behind the call's one host wait: failing before it leaves the
  // renderer as it was; from it on a failure leaves the new scene in force
  // without a history, as mrt_renderer_set_scene would
  const mrt_scene* old_scene = r->scene;
  const mrt_camera old = r->camera;
  const bool had_extras = r->extras_current;
  rc = swap_scene(r, scene, cam);
  if (rc) return rc;
  if (had_extras) {   // E and EM stay readable, cleared as mrt_renderer_reset clears them
    HIP_TRY(hipMemsetAsync(r->extra.p, 0, image_bytes(r), r->stream));
    HIP_TRY(hipMemsetAsync(r->extra_moments.p, 0, image_bytes(r), r->stream));
    r->extras_current = true;
  }
  std::swap(r->guide_n.p, r->prev_guide_n.p);   // equal sizes: the old scene's planes become the previous ones
  std::swap(r->guide_p.p, r->prev_guide_p.p);
  // the new scene's guide planes and, for each pixel's surface point, where it was in the old scene
  if (!r->guide_spill.p) HIP_TRY(alloc_isect_spill(r->guide_spill, r->scene->dev.max_stack));
  rc = guides_motion_with_spill(r->scene, old_scene, &r->camera, W, H, r->guide_n.as<float>(), r->guide_p.as<float>(),
                                r->motion_n.as<float>(), r->motion_p.as<float>(), r->desc.flags & MRT_FLAG_PRECISE,
                                r->guide_spill.as<uint32_t>(), r->stream);
  if (rc) return rc;
  r->guides_current = true;
  rc = mrt_reproject(r->temporal_prev.as<float>(), r->prev_guide_n.as<float>(), r->prev_guide_p.as<float>(), &old,
                     r->motion_n.as<float>(), r->motion_p.as<float>(), r->history.as<float>(), W, H, &p, r->stream);
  if (rc) return rc;
  if (moments) {
    rc = mrt_reproject(r->moments_prev.as<float>(), r->prev_guide_n.as<float>(), r->prev_guide_p.as<float>(), &old,
                       r->motion_n.as<float>(), r->motion_p.as<float>(), r->moments_history.as<float>(), W, H, &p,
                       r->stream);
    if (rc) return rc;
  }
  r->history_valid = true;
  return MRT_OK;
}

int mrt_renderer_resolve(mrt_renderer* r) {
  int rc = temporal_usable(r, "mrt_renderer_resolve");
  if (rc) return rc;
  if (r->frame_index == 0 && !r->history_valid)
    return fail(MRT_ERR_STATE, "mrt_renderer_resolve: no frame accumulated and no valid history");
  HIP_TRY(hipSetDevice(r->scene->device));
  rc = resolve_image_into(r, r->resolved);
  if (rc) return rc;
  r->resolved_current = true;
  return MRT_OK;
}

int mrt_renderer_read_resolved(mrt_renderer* r, float* rgba, size_t count) {
  return read_back(r, rgba, count, [](const mrt_renderer* r) {
    return ReadSpec{image_bytes(r) / 4, r->resolved.p, r->resolved_current, "no resolve has run at the renderer's current size"};
  });
}

int mrt_renderer_save_resolved(mrt_renderer* r, const char* path) { return save_read(r, path, mrt_renderer_read_resolved); }

int mrt_renderer_denoise_resolved(mrt_renderer* r, const mrt_denoise_params* params) {
  int rc = temporal_usable(r, "mrt_renderer_denoise_resolved");
  if (rc) return rc;
  if (r->frame_index == 0 && !r->history_valid)
    return fail(MRT_ERR_STATE, "mrt_renderer_denoise_resolved: no frame accumulated and no valid history");
  PARAMS_OR_DEFAULT(mrt_denoise_params, p, params, mrt_denoise_params_default(std::max<uint64_t>(r->frame_index, 1), &p),
                    mrt_denoise_params_check);
  HIP_TRY(hipSetDevice(r->scene->device));
  rc = size_group({&r->denoised, &r->denoise_scratch}, image_bytes(r), &r->denoised_current);
  if (rc) return rc;
  rc = mrt_renderer_resolve(r);
  return rc ? rc : atrous(r, r->resolved.as<float>(), p);
}

// ---- variance-guided denoising (include/mrt.h: mrt_renderer_denoise_variance) ----
int mrt_renderer_read_moments(mrt_renderer* r, float* rgba, size_t count) {
  return read_back(r, rgba, count, [](const mrt_renderer* r) {
    return ReadSpec{image_bytes(r) / 4, r->moments.p, (r->desc.flags & MRT_FLAG_MOMENTS) != 0,
                    "mrt_renderer_read_moments: the renderer was created without MRT_FLAG_MOMENTS"};
  });
}

int mrt_renderer_moments(mrt_renderer* r, float** device_moments) {
  if (!r || !device_moments) return fail(MRT_ERR_INVALID, "null argument");
  if (!(r->desc.flags & MRT_FLAG_MOMENTS))
    return fail(MRT_ERR_STATE, "mrt_renderer_moments: the renderer was created without MRT_FLAG_MOMENTS");
  *device_moments = r->moments.as<float>();
  return MRT_OK;
}

int mrt_renderer_denoise_variance(mrt_renderer* r, const mrt_svgf_params* params) {
  if (!r) return fail(MRT_ERR_INVALID, "null renderer");
  if (!(r->desc.flags & MRT_FLAG_MOMENTS))
    return fail(MRT_ERR_STATE, "mrt_renderer_denoise_variance: the renderer was created without MRT_FLAG_MOMENTS");
  if (r->frame_index == 0 && !r->history_valid)
    return fail(MRT_ERR_STATE, "mrt_renderer_denoise_variance: no frame accumulated and no valid history");
  PARAMS_OR_DEFAULT(mrt_svgf_params, p, params, mrt_svgf_params_default(&p), mrt_svgf_params_check);
  HIP_TRY(hipSetDevice(r->scene->device));
  int rc = size_group({&r->denoised, &r->denoise_scratch}, image_bytes(r), &r->denoised_current);
  if (rc) return rc;
  rc = variance_inputs(r, p, true);
  if (rc) return rc;
  // with firefly suppression on, the filter's input is the clamped copy; the resolved buffer stays as it is
  const float* filtered = r->firefly_on ? r->clamped.as<float>() : r->resolved.as<float>();
  rc = mrt_denoise_variance(filtered, r->variance.as<float>(), r->guide_n.as<float>(), r->guide_p.as<float>(),
                            r->denoised.as<float>(), r->denoise_scratch.as<float>(), nullptr, r->desc.width,
                            r->desc.height, &p, r->stream);
  if (rc) return rc;
  r->denoised_current = true;
  return MRT_OK;
}

int mrt_renderer_read_variance(mrt_renderer* r, float* plane, size_t count) {
  return read_back(r, plane, count, [](const mrt_renderer* r) {
    return ReadSpec{image_bytes(r) / 16, r->variance.p, r->variance_current,
                    "no mrt_renderer_denoise_variance has run at the renderer's current size"};
  });
}

// ---- firefly suppression (include/mrt.h: mrt_renderer_set_firefly) ----------
int mrt_renderer_set_firefly(mrt_renderer* r, const mrt_firefly_params* params) {
  if (!r) return fail(MRT_ERR_INVALID, "null renderer");
  if (!(r->desc.flags & MRT_FLAG_MOMENTS))
    return fail(MRT_ERR_STATE, "mrt_renderer_set_firefly: the renderer was created without MRT_FLAG_MOMENTS");
  if (!params) {
    r->firefly_on = false;
    return MRT_OK;
  }
  const int rc = mrt_firefly_params_check(params);
  if (rc) return rc;
  r->firefly = *params;
  r->firefly_on = true;
  return MRT_OK;
}

int mrt_renderer_get_firefly(const mrt_renderer* r, mrt_firefly_params* out, uint32_t* enabled) {
  if (!r) return fail(MRT_ERR_INVALID, "null renderer");
  if (out) *out = r->firefly;
  if (enabled) *enabled = r->firefly_on ? 1u : 0u;
  return MRT_OK;
}

int mrt_renderer_read_clamped(mrt_renderer* r, float* rgba, size_t count, uint32_t* clamped_pixels) {
  return read_back(r, rgba, count, [](const mrt_renderer* r) {
    return ReadSpec{image_bytes(r) / 4, r->clamped.p, r->clamped_current,
                    "no firefly clamp has run at the renderer's current size", r->clamped.as<char>() + image_bytes(r), 1};
  }, clamped_pixels);
}

// ---- adaptive sampling (include/mrt.h: mrt_renderer_refine) -----------------
int mrt_renderer_draw_tiles(mrt_renderer* r, const uint32_t* tiles, uint32_t count, uint32_t frames) {
  int rc = refine_usable(r, "mrt_renderer_draw_tiles");
  if (rc) return rc;
  const uint32_t T = r->tiles_x * r->tiles_y;
  if (!tiles || count == 0 || count > T || frames == 0)
    return fail(MRT_ERR_INVALID, "mrt_renderer_draw_tiles: need a list of 1..tiles_x * tiles_y tiles and frames >= 1");
  std::vector<bool> seen(T, false);
  for (uint32_t k = 0; k < count; ++k) {
    if (tiles[k] >= T) return fail(MRT_ERR_INVALID, "mrt_renderer_draw_tiles: tile " + std::to_string(tiles[k]) + " out of range");
    if (seen[tiles[k]]) return fail(MRT_ERR_INVALID, "mrt_renderer_draw_tiles: tile " + std::to_string(tiles[k]) + " listed twice");
    seen[tiles[k]] = true;
  }
  rc = ensure_extras(r);
  if (rc) return rc;
  return draw_extra(r, tiles, count, frames);
}

int mrt_renderer_refine(mrt_renderer* r, uint32_t frames, uint32_t tile_count, const mrt_adaptive_params* params) {
  int rc = refine_usable(r, "mrt_renderer_refine");
  if (rc) return rc;
  const uint32_t W = r->desc.width, H = r->desc.height, T = r->tiles_x * r->tiles_y;
  if (frames == 0 || tile_count == 0 || tile_count > T || T > mrt::kMaxSelectTiles)
    return fail(MRT_ERR_INVALID, "mrt_renderer_refine: need frames >= 1 and 1 <= tile_count <= tiles_x * tiles_y <= 16384");
  PARAMS_OR_DEFAULT(mrt_adaptive_params, p, params, mrt_adaptive_params_default(&p), mrt_adaptive_params_check);
  if (r->frame_index == 0 && !r->history_valid)
    return fail(MRT_ERR_STATE, "mrt_renderer_refine: no frame accumulated and no valid history");
  mrt_svgf_params sp;
  (void)mrt_svgf_params_default(&sp);
  rc = ensure_extras(r);
  if (rc) return rc;
  rc = variance_inputs(r, sp, false);
  if (rc) return rc;
  rc = mrt_tile_priority(r->resolved.as<float>(), r->variance.as<float>(), r->guide_n.as<float>(),
                         r->tile_priority.as<float>(), W, H, &p, r->desc.flags & MRT_FLAG_PRECISE, r->stream);
  if (rc) return rc;
  r->priority_current = true;
  rc = mrt_tile_select(r->tile_priority.as<float>(), T, tile_count, r->tile_list.as<uint32_t>(), r->stream);
  if (rc) return rc;
  return draw_extra(r, nullptr, tile_count, frames);
}

int mrt_renderer_read_extra(mrt_renderer* r, float* rgba, size_t count) {
  return read_back(r, rgba, count, [](const mrt_renderer* r) {
    return ReadSpec{image_bytes(r) / 4, r->extra.p, r->extras_current, kNoExtras};
  });
}

int mrt_renderer_read_extra_moments(mrt_renderer* r, float* rgba, size_t count) {
  return read_back(r, rgba, count, [](const mrt_renderer* r) {
    return ReadSpec{image_bytes(r) / 4, r->extra_moments.p, r->extras_current, kNoExtras};
  });
}

int mrt_renderer_read_tile_priority(mrt_renderer* r, float* priority, size_t count) {
  return read_back(r, priority, count, [](const mrt_renderer* r) {
    return ReadSpec{(size_t)r->tiles_x * r->tiles_y, r->tile_priority.p, r->priority_current,
                    "no refine has run at the renderer's current size"};
  });
}

// (an empty list is stale whatever the capacity: the state is looked at first)
int mrt_renderer_read_tile_list(mrt_renderer* r, uint32_t* tiles, size_t capacity, uint32_t* count) {
  const int rc = read_back(r, count ? tiles : nullptr, capacity, [](const mrt_renderer* r) {
    return ReadSpec{r->list_count, r->tile_list.p, r->list_count != 0, kNoExtras};
  });
  if (rc) return rc;
  *count = r->list_count;
  return MRT_OK;
}

int mrt_renderer_refine_stats(mrt_renderer* r, mrt_refine_stats* stats) {
  if (!r || !stats) return fail(MRT_ERR_INVALID, "null argument");
  const int rc = finalize_pending(r);   // counts the pixels of the lists not yet read back
  if (rc) return rc;
  *stats = r->refine_stats;
  return MRT_OK;
}

// ---- sampling to a target error (include/mrt.h: mrt_renderer_converge) -------
int mrt_renderer_error(mrt_renderer* r, const mrt_svgf_params* svgf, float luminance_floor, float threshold,
                       mrt_error_summary* out) {
  if (!r || !out) return fail(MRT_ERR_INVALID, "null argument");
  mrt_svgf_params sp;
  if (svgf) sp = *svgf;
  else (void)mrt_svgf_params_default(&sp);   // (checked by estimate_usable, behind the renderer's own state)
  mrt_adaptive_params ap;
  (void)mrt_adaptive_params_default(&ap);
  if (luminance_floor != 0.0f) ap.luminance_floor = luminance_floor;
  const int rc = estimate_usable(r, "mrt_renderer_error", sp, ap, threshold);
  return rc ? rc : estimate(r, sp, ap, threshold, out);
}

int mrt_renderer_read_tile_error(mrt_renderer* r, float* mean_error, uint32_t* pixels, size_t count) {
  return read_back(r, pixels ? mean_error : nullptr, count, [](const mrt_renderer* r) {
    const size_t T = (size_t)r->tiles_x * r->tiles_y;
    return ReadSpec{T, r->tile_error.p, r->tile_error_current, "no error estimate has run at the renderer's current size",
                    r->tile_pixels.p, T};
  }, pixels);
}

int mrt_renderer_converge(mrt_renderer* r, const mrt_converge_params* params, mrt_converge_result* out) {
  if (!r || !out) return fail(MRT_ERR_INVALID, "null argument");
  PARAMS_OR_DEFAULT(mrt_converge_params, p, params, mrt_converge_params_default(&p), mrt_converge_params_check);
  mrt_svgf_params sp;
  (void)mrt_svgf_params_default(&sp);
  mrt_adaptive_params ap;
  ap.luminance_floor = p.luminance_floor;
  int rc = estimate_usable(r, "mrt_renderer_converge", sp, ap, p.target_error);
  if (rc) return rc;
  const uint32_t T = r->tiles_x * r->tiles_y;
  const uint32_t cap = p.max_tiles ? std::min(p.max_tiles, T) : T;
  mrt_converge_result res{};
  for (;;) {
    mrt_error_summary s;
    rc = estimate(r, sp, ap, p.target_error, &s);
    if (rc) return rc;
    if (res.passes == 0) res.first = s;
    res.last = s;
    if (s.tiles_above == 0) {
      res.converged = 1;
      break;
    }
    uint64_t n = std::min(s.tiles_above, cap);
    if (p.max_tile_frames) n = std::min<uint64_t>(n, (p.max_tile_frames - res.tile_frames) / p.frames_per_pass);
    if (n == 0 || res.passes >= p.max_passes) break;
    rc = draw_extra(r, nullptr, (uint32_t)n, p.frames_per_pass);   // the n worst: the head of the device list
    if (rc) return rc;
    res.passes += 1;
    res.tile_frames += n * p.frames_per_pass;
  }
  *out = res;
  return MRT_OK;
}

// ---- golden comparison and display -----------------------------------------
int mrt_renderer_load_reference(mrt_renderer* r, const char* path) {
  if (!r || !path) return fail(MRT_ERR_INVALID, "null argument");
  std::vector<float> img;
  uint32_t W = 0, H = 0;
  std::string err;
  if (!mrt::load_exr(path, img, W, H, err)) return fail(MRT_ERR_IO, err);
  if (W != r->desc.width || H != r->desc.height)
    return fail(MRT_ERR_INVALID, "reference image is " + std::to_string(W) + "x" + std::to_string(H) + ", renderer " +
                                     std::to_string(r->desc.width) + "x" + std::to_string(r->desc.height));
  HIP_TRY(hipSetDevice(r->scene->device));
  HIP_TRY(hipStreamSynchronize(r->stream));
  HIP_TRY(upload(r->reference, img.data(), img.size() * 4));
  return MRT_OK;
}

int mrt_renderer_display(mrt_renderer* r, uint32_t flags, float compare_scale, float* rgba, size_t count) {
  if (!r || !rgba) return fail(MRT_ERR_INVALID, "null argument");
  if (count < image_bytes(r) / 4) return fail(MRT_ERR_INVALID, "output buffer too small");
  const float* src = nullptr;
  int rc = display_source(r, flags, &src);
  if (rc) return rc;
  rc = display_to(r, src, flags, compare_scale, rgba);
  return rc ? rc : mrt_renderer_sync(r);
}

int mrt_renderer_display_enqueue(mrt_renderer* r, uint32_t flags, float compare_scale, uint32_t slot) {
  if (!r) return fail(MRT_ERR_INVALID, "null renderer");
  if (slot >= MRT_DISPLAY_SLOTS) return fail(MRT_ERR_INVALID, "display slot >= MRT_DISPLAY_SLOTS");
  const float* src = nullptr;
  int rc = display_source(r, flags, &src);
  if (rc) return rc;
  const size_t need = image_bytes(r) / 4;
  auto& ds = r->shown[slot];
  if (ds.queued) HIP_TRY(hipEventSynchronize(ds.done));   // its previous copy may still be landing
  if (ds.floats != need) {   // (the pinned block only grows: a smaller frame uses its front)
    ds.floats = 0;
    HIP_TRY(ds.host.reserve(need * 4, hipHostMallocDefault));
    ds.floats = need;
  }
  HIP_TRY(ds.done.ensure(hipEventDisableTiming));
  rc = display_to(r, src, flags, compare_scale, ds.host.host<float>());
  if (rc) return rc;
  HIP_TRY(hipEventRecord(ds.done, r->stream));
  ds.queued = true;
  return MRT_OK;
}

int mrt_renderer_display_map(mrt_renderer* r, uint32_t slot, const float** rgba, size_t* count) {
  if (!r || !rgba) return fail(MRT_ERR_INVALID, "null argument");
  if (slot >= MRT_DISPLAY_SLOTS) return fail(MRT_ERR_INVALID, "display slot >= MRT_DISPLAY_SLOTS");
  auto& ds = r->shown[slot];
  if (!ds.queued || ds.floats != image_bytes(r) / 4) return fail(MRT_ERR_STATE, "display slot not enqueued at the current size");
  HIP_TRY(hipEventSynchronize(ds.done));
  *rgba = ds.host.host<float>();
  if (count) *count = ds.floats;
  return MRT_OK;
}

}  // extern "C"
