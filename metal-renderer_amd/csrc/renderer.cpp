// renderer.cpp — the renderer of include/mrt.h: life cycle, camera
// generations, the draw loop and its statistics, and image read-back, denoise,
// temporal resolve and display on a renderer.  (Scene: scene_api.cpp; stage
// calls: stage_api.cpp; multi-GPU exchange: exchange.cpp.)
//
// mrt_renderer_draw_n mirrors performRaytracing: (renderer/Renderer.mm:500-585)
// frame by frame, restructured for MI355X as a wavefront of fused bounce
// launches (kern_bounce.h::bounce_kernel):
//   reference per frame: rayGenerator, L x {MPS intersect, intersectionHandler,
//                        MPS intersect (shadow), lightSamplingHandler},
//                        accumulateImage                       = 2 + 4L passes
//   here per frame:      L bounce launches over a compacted SoA ray queue
//                        (raygen fused into bounce 0, shadow resolve and
//                        accumulation fused into the bounce where the path
//                        ends)                                 = L launches
#include <cmath>
#include <cstdio>
#include <cstdlib>

#include "host_internal.h"
#include "diag_env.h"
#include "image.h"
#include "primary.h"

using namespace mrt::host;

namespace {

// pixels of tile t inside the image
uint64_t tile_pixels(const mrt_renderer* r, uint32_t t) {
  const uint32_t tx = t % r->tiles_x, ty = t / r->tiles_x;
  return (uint64_t)std::min<uint32_t>(mrt::kTile, r->desc.width - tx * mrt::kTile) *
         std::min<uint32_t>(mrt::kTile, r->desc.height - ty * mrt::kTile);
}

int finalize_draw(mrt_renderer* r, DrawRecord& d) {
  if (!d.pending) return MRT_OK;
  HIP_TRY(hipEventSynchronize(d.stop));
  float ms = 0.0f;
  HIP_TRY(hipEventElapsedTime(&ms, d.start, d.stop));
  const CounterLayout& lay = d.layout;
  // the whole counter buffer (survivor counts, grab counters, spans) was
  // copied to pinned memory on the main stream behind the draw: no
  // synchronous copy, so the host never waits for work queued after it
  HIP_TRY(hipEventSynchronize(d.copied));
  const uint32_t* cnt = static_cast<const uint32_t*>(d.host);
  if (d.listed) {   // a refine draw: its list is on the host by now (uploaded from there, or copied back behind the draw)
    d.pixels = 0;
    for (uint32_t k = 0; k < d.listed; ++k) d.pixels += tile_pixels(r, d.list_host[k]);
    r->refine_stats.paths += d.pixels * d.frames;
  }
  uint64_t active = d.pixels * d.frames;   // bounce 0: every rendered pixel's camera ray
  for (uint32_t k = 0; k < lay.batches; ++k)
    for (uint32_t b = 0; b + 1 < lay.L; ++b) active += cnt[lay.total(k, b)];
  r->stats.active_ray_bounces += active;
  r->stats.last_draw_ms = ms;
  const uint64_t paths = d.pixels * d.frames;
  r->stats.mpaths_per_s = ms > 0.0f ? (double)paths / (ms * 1e-3) / 1e6 : 0.0;
  r->stats.kernel_launches += (uint64_t)lay.batches * (r->path_mode || r->stream_mode ? 1u : lay.L);
  for (uint32_t k = 0; k < lay.batches; ++k) {
    unsigned long long sp[2];
    std::memcpy(sp, static_cast<const char*>(d.host) + lay.span(k), 16);
    const unsigned long long t0 = ~sp[0], t1 = sp[1];
    if (sp[0] && t1 >= t0 && r->wall_khz > 0.0) {
      r->stats.span_ms += (double)(t1 - t0) / r->wall_khz;
      r->stats.spans += 1;
    }
  }
  if (r->desc.flags & MRT_FLAG_PROFILE) {
    for (size_t k = 0; k + 1 < d.events; k += 2) {
      float ms_k = 0.0f;
      HIP_TRY(hipEventElapsedTime(&ms_k, d.kernel_events[k], d.kernel_events[k + 1]));
      r->stats.kernel_ms += ms_k;
      r->stats.timed_launches += 1;
    }
  }
  d.pending = false;
  return MRT_OK;
}

// read back every pending draw, oldest first
int finalize_pending(mrt_renderer* r) {
  for (int i = 0; i < kDrawRing; ++i) {
    const int rc = finalize_draw(r, r->draws[(r->draw_next + i) % kDrawRing]);
    if (rc) return rc;
  }
  return MRT_OK;
}

// the noise chunks of frames [f0, f0 + n): generated (host threads, unless
// the worker already has) and uploaded asynchronously; never waits for the GPU
// (of schedule `noise`: the renderer's, or the refine draws' own)
int acquire_noise(mrt_renderer* r, mrt::NoiseSchedule* noise, int64_t f0, uint32_t n,
                  std::vector<mrt::NoiseSchedule::Chunk*>* out) {
  using NS = mrt::NoiseSchedule;
  const int64_t k0 = NS::chunk_of(f0), k1 = NS::chunk_of(f0 + (int64_t)n - 1);
  HIP_TRY(noise->poll(k0, k1));   // (never evicts a chunk this draw reads)
  const uint64_t waits = noise->counters().waits;
  for (int64_t k = k0; k <= k1; ++k) {
    NS::Chunk* c = nullptr;
    HIP_TRY(noise->acquire(k, r->draw_seq, &c));
    if (out) out->push_back(c);
  }
  if (noise->counters().waits != waits) r->stats.noise_waits += 1;
  // the next chunk's tables are generated while these frames render
  noise->prefetch(k1 + 1);
  return MRT_OK;
}

// Put r->camera in force: build its candidate lists (wavefront kernels only,
// primary_allowed, the cap, a pinhole camera) and upload them with the camera
// block into a generation no launch in flight reads.  idle: nothing of this
// renderer is executing (create / resize): a synchronous copy, and every
// other generation is free.  Otherwise the copy is asynchronous on the next
// batch's render stream and the host waits for nothing — unless all
// kCameraGens generations are still read by executing draws.
int install_camera(mrt_renderer* r, bool idle) {
  const uint32_t W = r->desc.width, H = r->desc.height;
  const mrt::CameraBlock cb = camera_block(r->camera);
  const mrt::CameraBlock* cbp = r->camera_moved ? &cb : nullptr;
  mrt::PrimaryLists pl;
  const mrt::BvhResult& b = r->scene->bvh;
  const bool lists_possible = r->primary_allowed && !r->path_mode;
  const bool lists = lists_possible && mrt::build_primary_lists(b.tris.data(), (uint32_t)(b.tris.size() / 12), W, H,
                                                                r->primary_cap, cbp, pl);
  // capacity: the block and the longest buffer build_primary_lists can return
  // for this frame size, so a generation never grows between resizes
  const size_t nblocks = (size_t)((W + mrt::kPrimaryBlock - 1) / mrt::kPrimaryBlock) *
                         ((H + mrt::kPrimaryBlock - 1) / mrt::kPrimaryBlock);
  const size_t cap_bytes = sizeof(mrt::CameraBlock) + (lists_possible ? nblocks * (1 + (size_t)r->primary_cap) * 4 : 0);
  const size_t bytes = sizeof(mrt::CameraBlock) + (lists ? pl.words.size() * 4 : 0);
  if (bytes > cap_bytes) return fail(MRT_ERR_STATE, "camera: candidate lists exceed their bound");
  auto size_gen = [&](CameraGen* c) -> int {
    if (c->dev.bytes < cap_bytes) HIP_TRY(c->dev.alloc(cap_bytes));
    if (c->host_bytes < cap_bytes) {
      if (c->host) HIP_TRY(hipHostFree(c->host));
      c->host = nullptr;
      c->host_bytes = 0;
      HIP_TRY(hipHostMalloc(&c->host, cap_bytes, hipHostMallocDefault));
      c->host_bytes = cap_bytes;
    }
    return MRT_OK;
  };
  CameraGen* g = nullptr;
  while (idle && r->cams.size() < kCameraGens) {   // all generations exist from create on
    r->cams.emplace_back(new CameraGen());
    CameraGen* c = r->cams.back().get();
    HIP_TRY(hipEventCreateWithFlags(&c->ready, hipEventDisableTiming));
    HIP_TRY(hipEventCreateWithFlags(&c->retired, hipEventDisableTiming));
  }
  for (auto& c : r->cams) {
    if (idle) {
      // The caller synchronised the main stream, which follows every render
      // launch — but not an upload that no draw followed (set_camera, then
      // resize): wait for it before its staging is written again.  Every
      // generation is sized for the new frame here, where allocation's
      // implicit synchronisation costs nothing, so a later set_camera never
      // allocates.
      if (c->async) HIP_TRY(hipEventSynchronize(c->ready));
      c->async = false;
      c->busy = false;
      const int rc = size_gen(c.get());
      if (rc) return rc;
    } else {
      if (c.get() == r->cam_cur) continue;
      if (c->busy && hipEventQuery(c->retired) == hipSuccess) c->busy = false;
    }
    if (!c->busy && !g) g = c.get();
  }
  if (!g) {   // every generation is read by draws still executing: wait for one
    for (auto& c : r->cams)
      if (c.get() != r->cam_cur) { g = c.get(); break; }
    HIP_TRY(hipEventSynchronize(g->retired));
    g->busy = false;
  }
  if (g->dev.bytes < cap_bytes || g->host_bytes < cap_bytes)   // sized in the idle path for this frame size
    return fail(MRT_ERR_STATE, "camera: generation smaller than the frame's bound");
  std::memcpy(g->host, &cb, sizeof(cb));
  if (lists) std::memcpy(static_cast<char*>(g->host) + sizeof(cb), pl.words.data(), pl.words.size() * 4);
  if (idle) {
    HIP_TRY(hipMemcpy(g->dev.p, g->host, bytes, hipMemcpyHostToDevice));
    g->async = false;
    g->waited_streams = ~0u;
  } else {
    const uint32_t slot = r->slot_next;
    HIP_TRY(hipMemcpyAsync(g->dev.p, g->host, bytes, hipMemcpyHostToDevice, r->slots[slot].stream));
    HIP_TRY(hipEventRecord(g->ready, r->slots[slot].stream));
    g->async = true;
    g->waited_streams = 1u << slot;
    if (CameraGen* old = r->cam_cur) {
      // (a generation replaced before any draw used it: its upload, on a
      // render stream, must also be over before it is recycled)
      if (old->async) HIP_TRY(hipStreamWaitEvent(r->stream, old->ready, 0));
      HIP_TRY(hipEventRecord(old->retired, r->stream));
      old->busy = true;
    }
  }
  g->moved = r->camera_moved;
  g->has_lists = lists;
  g->primary_bx = lists ? pl.blocks_x : 0;
  r->cam_cur = g;
  r->stats.primary_blocks = lists ? pl.listed_blocks : 0;
  r->stats.primary_mean = lists ? (float)pl.mean_count : 0.0f;
  return MRT_OK;
}

int alloc_frame_buffers(mrt_renderer* r) {
  const uint32_t W = r->desc.width, H = r->desc.height;
  const uint32_t S = std::max<uint32_t>(1, r->desc.shard_count);
  r->tiles_x = (W + mrt::kTile - 1) / mrt::kTile;
  r->tiles_y = (H + mrt::kTile - 1) / mrt::kTile;
  const uint32_t T = r->tiles_x * r->tiles_y;
  r->owned_tiles = r->desc.shard_rank < T ? (T - r->desc.shard_rank + S - 1) / S : 0;
  r->owned_pixels = 0;
  for (uint32_t t = r->desc.shard_rank; t < T; t += S) {
    const uint32_t tx = t % r->tiles_x, ty = t / r->tiles_x;
    const uint64_t w = std::min<uint32_t>(mrt::kTile, W - tx * mrt::kTile);
    const uint64_t h = std::min<uint32_t>(mrt::kTile, H - ty * mrt::kTile);
    r->owned_pixels += w * h;
  }
  // frames per launch: about 2^27 rays per launch (64 frames at 1080p, up
  // to kMaxBatch), so the launch-boundary drain (the last grabs finishing at
  // falling occupancy, ~20-40 us) is a small share of each launch: C2 at
  // 2^24 rays per launch (8 frames) 5210, 2^25 5431, 2^26 5551, 2^27 5617
  // Mpaths/s.  Memory: 64 B per queued ray x 2 queues + 16 B radiance
  // (~19.5 GB at 2^27 rays, of 288 GB).
  const size_t owned_slots = std::max<size_t>(1, (size_t)r->owned_tiles * 4096);
  r->batch = (uint32_t)std::min<size_t>(mrt::kMaxBatch, std::max<size_t>(1, ((size_t)1 << 27) / owned_slots));
  if (const char* v = mrt::diag_env("MRT_BATCH"))
    r->batch = std::max<uint32_t>(1, std::min<uint32_t>(mrt::kMaxBatch, (uint32_t)std::strtoul(v, nullptr, 0)));
  // a ray's tag holds batch * owned slots in 31 bits
  while (r->batch > 1 && owned_slots * r->batch >= ((size_t)1 << 31)) --r->batch;
  if (owned_slots >= ((size_t)1 << 31)) return fail(MRT_ERR_INVALID, "frame too large");
  // queue capacity: every owned slot of the batch + per-block rounding and
  // slack of the segments (kernels.h)
  const size_t slots = owned_slots * r->batch + (size_t)r->grid * (256 + mrt::kSegSlack);
  r->stream_mode = r->stream_allowed;
  for (FrameSlot& fs : r->slots) {
    HIP_TRY(fs.segments.alloc(((size_t)4 * r->grid + 2) * 4));   // 2 queues x 2 classes x grid + 2 chunk words
    HIP_TRY(hipMemsetAsync(fs.segments.p, 0, fs.segments.bytes, r->stream));
    // the path kernel keeps the path state in LDS: no ray queues; the
    // streaming wavefront needs only its per-wave queues
    const size_t qslots = r->stream_mode ? mrt::stream_slots(r->desc.max_path_length, r->grid) : slots;
    // (stream mode: queue[1] is unused but for its plane 0, the partial hits
    // of recycled rays — 16 B a slot, as the other planes — where the scene's
    // nearest queries sweep under a cap, kern_bounce.h bounce_wave)
    const mrt::DeviceScene& dev = r->scene->dev;
    const bool partial = r->stream_mode && dev.sweep_leaves && dev.sweep_cap < mrt::kSweepLeaves;
    for (int q = 0; q < 2; ++q)
      for (int p = 0; p < mrt::kQueuePlanes; ++p)
        HIP_TRY(fs.queue[q][p].alloc(r->path_mode || (r->stream_mode && q == 1 && !(partial && p == 0)) ? 0 : qslots * 16));
    HIP_TRY(fs.radiance.alloc(owned_slots * r->batch * 16));
    const uint32_t need = r->scene->dev.max_stack;
    // spill rows of max_stack words per lane (dev_lds.h LdsCtx::spill_lane)
    if (need > r->stack_entries && !fs.spill.p) HIP_TRY(fs.spill.alloc((size_t)need * r->grid * 256 * 4));
  }
  if (r->own_image) {
    if (r->image) (void)hipFree(r->image);
    r->image = nullptr;
    HIP_TRY(hipMalloc(&r->image, (size_t)W * H * 16));
  }
  HIP_TRY(hipMemsetAsync(r->image, 0, (size_t)W * H * 16, r->stream));
  if (r->desc.flags & MRT_FLAG_MOMENTS) {
    HIP_TRY(r->moments.alloc((size_t)W * H * 16));
    HIP_TRY(hipMemsetAsync(r->moments.p, 0, (size_t)W * H * 16, r->stream));
  }
  r->image_foreign = false;
  r->frame_index = 0;
  r->stats = mrt_stats{};
  r->noise_base = r->noise->counters();
  r->stats.owned_pixels = r->owned_pixels;
  r->stats.kernel = r->path_mode ? 1u : (r->stream_mode ? 2u : 0u);
  r->stats.inflight = r->inflight;
  {
    const int rc = install_camera(r, true);
    if (rc) return rc;
  }
  // the render streams do not wait on the main stream: its memsets above
  // (segments, image) complete before any batch is queued
  HIP_TRY(hipStreamSynchronize(r->stream));
  return MRT_OK;
}

// A draw's frame batches: up to r->batch frames each, none crossing a noise
// chunk (64 frames, a multiple of the batch): a 64-frame draw from a multiple
// of 64 is one batch.  f0: the draw's first frame; chunks: those of the draw's
// frames, in order
struct Batch { uint64_t f; uint32_t frames; mrt::NoiseSchedule::Chunk* noise; };
std::vector<Batch> plan_batches(const mrt_renderer* r, uint64_t f0, uint32_t n,
                                const std::vector<mrt::NoiseSchedule::Chunk*>& chunks) {
  using NS = mrt::NoiseSchedule;
  std::vector<Batch> batches;
  for (uint64_t f = f0, end = f0 + n; f < end;) {
    const int64_t k = NS::chunk_of((int64_t)f);
    const uint64_t chunk_end = (uint64_t)(k + 1) * NS::kChunkFrames;
    const uint32_t b = (uint32_t)std::min<uint64_t>({(uint64_t)r->batch, end - f, chunk_end - f});
    batches.push_back({f, b, chunks[(size_t)(k - NS::chunk_of((int64_t)f0))]});
    f += b;
  }
  return batches;
}

// Size a ring entry for d.layout: the counter buffer and its pinned copy (both
// only grow) and `timed_events` profiling events.  *fresh: the counter buffer
// is new, so not zeroed by an earlier draw's folding accumulate
int size_draw_record(DrawRecord& d, size_t timed_events, bool* fresh) {
  const size_t counter_bytes = d.layout.bytes;
  *fresh = false;
  if (d.counters.bytes < counter_bytes) {
    HIP_TRY(d.counters.alloc(counter_bytes));
    *fresh = true;
  }
  if (d.host_bytes < counter_bytes) {
    if (d.host) HIP_TRY(hipHostFree(d.host));
    d.host = d.host_dev = nullptr;
    d.host_bytes = 0;
    HIP_TRY(hipHostMalloc(&d.host, counter_bytes, hipHostMallocMapped));
    HIP_TRY(hipHostGetDevicePointer(&d.host_dev, d.host, 0));
    d.host_bytes = counter_bytes;
  }
  while (d.kernel_events.size() < timed_events) {
    hipEvent_t e;
    HIP_TRY(hipEventCreate(&e));
    d.kernel_events.push_back(e);
  }
  return MRT_OK;
}

// The arguments of bounce launch b of `bt`, the draw's k-th batch, on slot
// `fs` with camera generation `cg` (path / stream kernel: the one launch, b = 0);
// src.tiles > 0: over the renderer's tile list instead of the owned tiles
int bounce_args(const mrt_renderer* r, const DrawSource& src, const DrawRecord& d, const Batch& bt, uint32_t k, uint32_t b,
                const FrameSlot& fs, const CameraGen* cg, mrt::BounceArgs& a) {
  const uint32_t L = r->desc.max_path_length;
  uint32_t* cnt = d.counters.as<uint32_t>();
  uint32_t* seg = fs.segments.as<uint32_t>();
  uint32_t* meta = seg + 4 * (size_t)r->grid;
  a.width = r->desc.width;
  a.height = r->desc.height;
  a.frame_index = (uint32_t)bt.f;
  a.batch = bt.frames;
  a.bounce = b;
  a.max_path_length = L;
  a.shard_rank = r->desc.shard_rank;
  a.shard_count = r->desc.shard_count;
  a.tiles_x = r->tiles_x;
  a.num_slots = (src.tiles ? src.tiles : r->owned_tiles) * 4096u;
  a.tile_list = src.tiles ? r->tile_list.as<uint32_t>() : nullptr;
  a.div_tiles = mrt::magic_div(a.tiles_x);
  a.div_slots = mrt::magic_div(a.num_slots);
  a.div_batch = mrt::magic_div(bt.frames);
  // (a rank that owns no tile has num_slots 0: its lanes all exit at the
  // idx < num_slots * batch bound before any quotient by it)
  if (!mrt::magic_ok(a.div_tiles, a.tiles_x) ||
      (a.num_slots && !mrt::magic_ok(a.div_slots, a.num_slots)) ||
      !mrt::magic_ok(a.div_batch, bt.frames))
    return fail(MRT_ERR_STATE, "draw: a launch divisor's magic multiplier does not divide exactly");
  a.debug = r->debug;
  a.flags = (r->desc.flags & MRT_FLAG_DEBUG_MATERIAL) ? mrt::kShadeDebugMaterial : 0u;
  a.in_segments = 2 * r->grid;   // two material classes per block
  a.in_seg_count = seg + (size_t)((b + 1) & 1) * 2 * r->grid;
  a.in_chunk = meta + ((b + 1) & 1);
  a.out_seg_count = seg + (size_t)(b & 1) * 2 * r->grid;
  a.out_chunk = meta + (b & 1);
  a.out_total = cnt + d.layout.total(k, b);
  a.grab = cnt + d.layout.grab(k, b);
  for (int p = 0; p < mrt::kQueuePlanes; ++p) {
    a.in_q.plane[p] = fs.queue[b & 1][p].as<float4>();
    a.out_q.plane[p] = fs.queue[(b + 1) & 1][p].as<float4>();
  }
  a.noise_window = static_cast<const float4*>(bt.noise->dev);
  a.noise_offset = (uint32_t)((int64_t)bt.f - mrt::NoiseSchedule::first_frame(mrt::NoiseSchedule::chunk_of((int64_t)bt.f)));
  a.radiance = fs.radiance.as<float4>();
  a.stack_spill = fs.spill.as<uint32_t>();
  a.bounce_counts = cnt + d.layout.total(k, 0);
  a.camera = cg->moved ? cg->dev.as<mrt::CameraBlock>() : nullptr;
  a.primary = cg->has_lists ? reinterpret_cast<const uint32_t*>(cg->dev.as<char>() + sizeof(mrt::CameraBlock))
                            : nullptr;
  a.primary_bx = cg->primary_bx;
  a.span = r->wall_khz > 0.0
               ? reinterpret_cast<unsigned long long*>(static_cast<char*>(d.counters.p) + d.layout.span(k))
               : nullptr;
  return MRT_OK;
}

// The arguments of batch `bt`'s accumulate; fold: the draw's last one, which
// copies the draw's statistics to the pinned copy and zeroes the counters
// src.tiles > 0: the counted accumulate over the tile list into E / EM
mrt::AccumArgs accum_args(const mrt_renderer* r, const DrawSource& src, const DrawRecord& d, const Batch& bt,
                          const FrameSlot& fs, bool fold) {
  mrt::AccumArgs acc{};
  acc.width = r->desc.width;
  acc.height = r->desc.height;
  acc.frame_index = (uint32_t)bt.f;
  acc.batch = bt.frames;
  acc.shard_rank = r->desc.shard_rank;
  acc.shard_count = r->desc.shard_count;
  acc.tiles_x = r->tiles_x;
  // (MRT_DEBUG bit 256, ablation: the accumulate launches but touches no
  // pixel — its statistics fold alone; a wrong image)
  acc.num_slots = (r->debug & 256u) ? 0u : (src.tiles ? src.tiles : r->owned_tiles) * 4096u;
  acc.radiance = fs.radiance.as<float4>();
  acc.image = reinterpret_cast<float4*>(src.image);
  acc.accumulate = (r->desc.flags & MRT_FLAG_NO_ACCUMULATE) ? 0u : 1u;
  acc.moments = reinterpret_cast<float4*>(src.moments);   // (null without MRT_FLAG_MOMENTS)
  acc.tile_list = src.tiles ? r->tile_list.as<uint32_t>() : nullptr;
  if (fold) {
    acc.counters = d.counters.as<uint32_t>();
    acc.host_counters = static_cast<uint32_t*>(d.host_dev);
    acc.copy_words = d.layout.batches * d.layout.L;
    acc.span_word = (uint32_t)(d.layout.span_off / 4);
    acc.span_words = d.layout.batches * 4;
    acc.zero_words = (uint32_t)(d.counters.bytes / 4);
  }
  return acc;
}

int write_pfm(const char* path, const std::vector<float>& rgba, uint32_t W, uint32_t H) {
  FILE* f = std::fopen(path, "wb");
  if (!f) return fail(MRT_ERR_IO, std::string("cannot write ") + path);
  std::fprintf(f, "PF\n%u %u\n-1.0\n", W, H);
  std::vector<float> row(3 * (size_t)W);
  for (uint32_t y = 0; y < H; ++y) {   // PFM scanlines are bottom-to-top == our row order
    for (uint32_t x = 0; x < W; ++x)
      for (int c = 0; c < 3; ++c) row[3 * x + c] = rgba[4 * ((size_t)y * W + x) + c];
    std::fwrite(row.data(), 4, row.size(), f);
  }
  std::fclose(f);
  return MRT_OK;
}

// Uncompressed scanline OpenEXR, FLOAT A,B,G,R channels, top-down.
int write_exr(const char* path, const std::vector<float>& rgba, uint32_t W, uint32_t H) {
  std::vector<uint8_t> out;
  auto put = [&](const void* p, size_t n) { const uint8_t* b = (const uint8_t*)p; out.insert(out.end(), b, b + n); };
  auto put_i32 = [&](int32_t v) { put(&v, 4); };
  auto put_str = [&](const char* s) { put(s, std::strlen(s) + 1); };
  auto attr = [&](const char* name, const char* type, const std::vector<uint8_t>& v) {
    put_str(name); put_str(type); put_i32((int32_t)v.size()); put(v.data(), v.size());
  };
  const uint32_t magic = 20000630u, version = 2u;
  put(&magic, 4); put(&version, 4);
  std::vector<uint8_t> ch;
  for (const char* c : {"A", "B", "G", "R"}) {
    ch.insert(ch.end(), c, c + 2);
    const int32_t pt = 2;  // FLOAT
    const uint8_t plin[4] = {0, 0, 0, 0};
    const int32_t xs = 1, ys = 1;
    ch.insert(ch.end(), (const uint8_t*)&pt, (const uint8_t*)&pt + 4);
    ch.insert(ch.end(), plin, plin + 4);
    ch.insert(ch.end(), (const uint8_t*)&xs, (const uint8_t*)&xs + 4);
    ch.insert(ch.end(), (const uint8_t*)&ys, (const uint8_t*)&ys + 4);
  }
  ch.push_back(0);
  attr("channels", "chlist", ch);
  attr("compression", "compression", {0});
  const int32_t box[4] = {0, 0, (int32_t)W - 1, (int32_t)H - 1};
  std::vector<uint8_t> bx((const uint8_t*)box, (const uint8_t*)box + 16);
  attr("dataWindow", "box2i", bx);
  attr("displayWindow", "box2i", bx);
  attr("lineOrder", "lineOrder", {0});
  const float par = 1.0f, ssw = 1.0f, swc[2] = {0.0f, 0.0f};
  attr("pixelAspectRatio", "float", std::vector<uint8_t>((const uint8_t*)&par, (const uint8_t*)&par + 4));
  attr("screenWindowCenter", "v2f", std::vector<uint8_t>((const uint8_t*)swc, (const uint8_t*)swc + 8));
  attr("screenWindowWidth", "float", std::vector<uint8_t>((const uint8_t*)&ssw, (const uint8_t*)&ssw + 4));
  out.push_back(0);
  const size_t line_bytes = (size_t)W * 4 * 4;
  uint64_t off = out.size() + 8ull * H;
  for (uint32_t y = 0; y < H; ++y) { put(&off, 8); off += 8 + line_bytes; }
  std::vector<float> line(4 * (size_t)W);
  for (uint32_t y = 0; y < H; ++y) {
    const uint32_t src = H - 1 - y;   // EXR is top-down; our row 0 is the bottom
    for (int c = 0; c < 4; ++c) {      // A, B, G, R
      const int comp = 3 - c;
      for (uint32_t x = 0; x < W; ++x) line[(size_t)c * W + x] = rgba[4 * ((size_t)src * W + x) + comp];
    }
    put_i32((int32_t)y);
    put_i32((int32_t)line_bytes);
    put(line.data(), line_bytes);
  }
  FILE* f = std::fopen(path, "wb");
  if (!f) return fail(MRT_ERR_IO, std::string("cannot write ") + path);
  std::fwrite(out.data(), 1, out.size(), f);
  std::fclose(f);
  return MRT_OK;
}

int save_rgba(const char* path, const std::vector<float>& img, uint32_t W, uint32_t H) {
  const std::string p(path);
  auto ends = [&](const char* s) { const size_t n = std::strlen(s); return p.size() >= n && p.compare(p.size() - n, n, s) == 0; };
  if (ends(".pfm")) return write_pfm(path, img, W, H);
  if (ends(".exr")) return write_exr(path, img, W, H);
  return fail(MRT_ERR_INVALID, "unsupported image extension (use .pfm or .exr)");
}

// mrt_renderer_read_denoised / _read_resolved: the derived plane `plane` to the
// host once the renderer's work is done; current: it was computed at the
// renderer's current size (else the entry point's own `stale` message)
int read_plane(mrt_renderer* r, DevBuf mrt_renderer::*plane, bool mrt_renderer::*current, const char* stale,
               float* rgba, size_t count) {
  if (!r || !rgba) return fail(MRT_ERR_INVALID, "null argument");
  const size_t need = (size_t)r->desc.width * r->desc.height * 4;
  if (count < need) return fail(MRT_ERR_INVALID, "output buffer too small");
  if (!(r->*current)) return fail(MRT_ERR_STATE, stale);
  const int rc = mrt_renderer_sync(r);
  if (rc) return rc;
  HIP_TRY(hipMemcpy(rgba, (r->*plane).p, need * 4, hipMemcpyDeviceToHost));
  return MRT_OK;
}

// mrt_renderer_save_image / _save_denoised / _save_resolved: what `read` returns, to `path`
int save_read(mrt_renderer* r, const char* path, int (*read)(mrt_renderer*, float*, size_t)) {
  if (!r || !path) return fail(MRT_ERR_INVALID, "null argument");
  const uint32_t W = r->desc.width, H = r->desc.height;
  std::vector<float> img((size_t)W * H * 4);
  const int rc = read(r, img.data(), img.size());
  if (rc) return rc;
  return save_rgba(path, img, W, H);
}

// the guide planes of the camera in force, on the main stream (allocated here
// when neither a denoise nor a move has made them yet).  The same allocation
// and trace as in mrt_renderer_denoise, which stays as it was: keep the two in
// step.  Known cost of leaving it alone: a renderer that moves before it has
// a denoised buffer (made by the first mrt_renderer_denoise or
// _denoise_resolved) has its guide planes freed (a host-synchronising
// hipFree), re-made and traced again by its first mrt_renderer_denoise, whose
// first-call test looks at the denoised buffer only.  Once per renderer and
// size, and the result is the same.
int ensure_guides(mrt_renderer* r) {
  const uint32_t W = r->desc.width, H = r->desc.height;
  const size_t bytes = (size_t)W * H * 16;
  if (r->guide_n.bytes != bytes || !r->guide_n.p || r->guide_p.bytes != bytes || !r->guide_p.p) {
    r->guides_current = false;
    HIP_TRY(r->guide_n.alloc(bytes));
    HIP_TRY(r->guide_p.alloc(bytes));
  }
  if (r->guides_current) return MRT_OK;
  if (!r->guide_spill.p) HIP_TRY(alloc_isect_spill(r->guide_spill, r->scene->dev.max_stack));
  const int rc = guides_with_spill(r->scene, &r->camera, W, H, r->guide_n.as<float>(), r->guide_p.as<float>(),
                                   r->desc.flags & MRT_FLAG_PRECISE, r->guide_spill.as<uint32_t>(), r->stream);
  if (rc) return rc;
  r->guides_current = true;
  return MRT_OK;
}

int temporal_usable(const mrt_renderer* r, const char* what) {
  if (!r) return fail(MRT_ERR_INVALID, "null renderer");
  if (r->desc.shard_count > 1)
    return fail(MRT_ERR_STATE, std::string(what) + ": a sharded renderer keeps no temporal history");
  return MRT_OK;
}

// while the extra image E holds samples (adaptive sampling), every resolve is
// followed by the counted merge with it: `out` = merge(out, extra), in place
int merge_extras(mrt_renderer* r, DevBuf& out, const DevBuf& extra) {
  if (!r->extras_valid) return MRT_OK;
  return mrt_counted_merge(out.as<float>(), extra.as<float>(), out.as<float>(), r->desc.width, r->desc.height,
                           r->desc.flags & MRT_FLAG_PRECISE, r->stream);
}

// resolve(image, frame_index, history if valid) into `out`, on the main stream
int resolve_into(mrt_renderer* r, DevBuf& out) {
  const size_t bytes = (size_t)r->desc.width * r->desc.height * 16;
  if (out.bytes != bytes || !out.p) HIP_TRY(out.alloc(bytes));
  const int rc = mrt_temporal_resolve(r->image, r->frame_index, r->history_valid ? r->history.as<float>() : nullptr,
                                      out.as<float>(), r->desc.width, r->desc.height, r->stream);
  return rc ? rc : merge_extras(r, out, r->extra);
}

// the same for the moments image and its history (MRT_FLAG_MOMENTS)
int resolve_moments_into(mrt_renderer* r, DevBuf& out) {
  const size_t bytes = (size_t)r->desc.width * r->desc.height * 16;
  if (out.bytes != bytes || !out.p) HIP_TRY(out.alloc(bytes));
  const int rc = mrt_temporal_resolve(r->moments.as<float>(), r->frame_index,
                                      r->history_valid ? r->moments_history.as<float>() : nullptr, out.as<float>(),
                                      r->desc.width, r->desc.height, r->stream);
  return rc ? rc : merge_extras(r, out, r->extra_moments);
}

int draw_frames(mrt_renderer* r, uint32_t n, const DrawSource& src);   // below

// ---- adaptive sampling (include/mrt.h: mrt_renderer_refine) ----
int refine_usable(const mrt_renderer* r, const char* what) {
  if (!r) return fail(MRT_ERR_INVALID, "null renderer");
  if (!(r->desc.flags & MRT_FLAG_MOMENTS))
    return fail(MRT_ERR_STATE, std::string(what) + ": the renderer was created without MRT_FLAG_MOMENTS");
  if (r->desc.shard_count > 1) return fail(MRT_ERR_STATE, std::string(what) + ": not on a sharded renderer");
  if (r->desc.flags & MRT_FLAG_STATIC_NOISE)
    return fail(MRT_ERR_STATE, std::string(what) + ": not with MRT_FLAG_STATIC_NOISE (every extra frame would repeat)");
  if (!r->path_mode && !r->stream_mode)
    return fail(MRT_ERR_STATE, std::string(what) + ": the per-bounce kernel has no tile-list instantiation");
  return MRT_OK;
}

// E, EM, the list, the priorities, the second noise schedule and the list's
// event: made at the first refine / draw_tiles, E and EM zeroed on the main stream
int ensure_extras(mrt_renderer* r) {
  HIP_TRY(hipSetDevice(r->scene->device));
  const size_t bytes = (size_t)r->desc.width * r->desc.height * 16;
  const size_t tile_bytes = (size_t)r->tiles_x * r->tiles_y * 4;
  if (!r->list_ready) HIP_TRY(hipEventCreateWithFlags(&r->list_ready, hipEventDisableTiming));
  if (!r->refine_noise) {
    r->refine_noise = std::make_unique<mrt::NoiseSchedule>(r->desc.seed ^ MRT_REFINE_SEED_XOR, false);
    HIP_TRY(r->refine_noise->init());
  }
  for (DevBuf* b : {&r->extra, &r->extra_moments})
    if (b->bytes != bytes || !b->p) {
      r->extras_current = false;
      HIP_TRY(b->alloc(bytes));
    }
  for (DevBuf* b : {&r->tile_list, &r->tile_priority})
    if (b->bytes != tile_bytes || !b->p) {
      r->priority_current = false;
      r->list_count = 0;
      HIP_TRY(b->alloc(tile_bytes));
    }
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

// mrt_renderer_read_extra / _read_extra_moments
int read_extra_plane(mrt_renderer* r, const DevBuf& plane, float* rgba, size_t count) {
  if (!r || !rgba) return fail(MRT_ERR_INVALID, "null argument");
  const size_t need = (size_t)r->desc.width * r->desc.height * 4;
  if (count < need) return fail(MRT_ERR_INVALID, "output buffer too small");
  if (!r->extras_current) return fail(MRT_ERR_STATE, "no refine or draw_tiles has run at the renderer's current size");
  const int rc = mrt_renderer_sync(r);
  if (rc) return rc;
  HIP_TRY(hipMemcpy(rgba, plane.p, need * 4, hipMemcpyDeviceToHost));
  return MRT_OK;
}

// Enqueue n frames of `src` (host_internal.h DrawSource): the draw loop of
// mrt_renderer_draw_n and of the refine draws.  The caller advances its own
// frame counter and statistics.
int draw_frames(mrt_renderer* r, uint32_t n, const DrawSource& src) {
  DrawRecord& d = r->draws[r->draw_next];
  // at most kDrawRing (3) draws in flight: the ring entry's previous draw must
  // have finished — the reference's MaxBuffersInFlight semaphore
  // (renderer/Renderer.mm:16, :593-600), the only host wait of a draw
  if (d.pending && hipEventQuery(d.copied) == hipErrorNotReady) r->stats.inflight_waits += 1;
  int rc = finalize_draw(r, d);
  if (rc) return rc;
  r->draw_seq += 1;
  std::vector<mrt::NoiseSchedule::Chunk*> chunks;
  rc = acquire_noise(r, src.noise, (int64_t)src.f0, n, &chunks);
  if (rc) return rc;
  const std::vector<Batch> batches = plan_batches(r, src.f0, n, chunks);
  const uint32_t nb = (uint32_t)batches.size();
  d.layout = CounterLayout(nb, r->desc.max_path_length);   // (the entry's previous draw is read back: nothing reads its layout)
  const uint32_t launches_per_batch = r->path_mode || r->stream_mode ? 1u : r->desc.max_path_length;
  const bool profile = (r->desc.flags & MRT_FLAG_PROFILE) != 0;
  bool fresh = false;
  rc = size_draw_record(d, profile ? (size_t)2 * nb * launches_per_batch : 0, &fresh);   // at most every batch is timed
  if (rc) return rc;
  if (src.tiles) {
    // the list: a host list goes to the device from the entry's pinned staging;
    // one chosen on the device comes back to it behind the draw (finalize_draw
    // counts its pixels).  On the main stream, which follows every launch that
    // read the previous list; the render streams wait for it through the event
    const uint32_t T = r->tiles_x * r->tiles_y;
    if (d.list_cap < T) {
      if (d.list_host) HIP_TRY(hipHostFree(d.list_host));
      d.list_host = nullptr;
      d.list_cap = 0;
      HIP_TRY(hipHostMalloc(reinterpret_cast<void**>(&d.list_host), (size_t)T * 4, hipHostMallocDefault));
      d.list_cap = T;
    }
    if (src.host_list) {
      std::memcpy(d.list_host, src.host_list, (size_t)src.tiles * 4);
      HIP_TRY(hipMemcpyAsync(r->tile_list.p, d.list_host, (size_t)src.tiles * 4, hipMemcpyHostToDevice, r->stream));
    } else {
      HIP_TRY(hipMemcpyAsync(d.list_host, r->tile_list.p, (size_t)src.tiles * 4, hipMemcpyDeviceToHost, r->stream));
    }
    HIP_TRY(hipEventRecord(r->list_ready, r->stream));
  }
  HIP_TRY(hipEventRecord(d.start, r->stream));
  // The render launches never wait on the main stream (it only carries
  // accumulates and image work; a noise chunk's upload is waited for through
  // its own event): the counters are cleared on the first batch's render
  // stream and the draw's other render streams wait for that.
  // The draw's last accumulate copies its statistics to the pinned host copy
  // and zeroes the counters for the ring entry's next draw (whose host side
  // has waited for that accumulate in finalize_draw): a fresh buffer, or one
  // whose last draw stopped before its folding accumulate, is the only one to
  // clear here.  MRT_COUNTER_FOLD=0: memset + copy per draw.
  const uint32_t s0 = r->slot_next;
  const bool clear = fresh || !d.clean || !r->counter_fold;
  d.clean = false;   // set again once this draw's folding accumulate is enqueued
  if (clear) HIP_TRY(hipMemsetAsync(d.counters.p, 0, d.counters.bytes, r->slots[s0].stream));
  if (clear && r->inflight > 1 && nb > 1) {
    HIP_TRY(hipEventRecord(d.cleared, r->slots[s0].stream));
    for (uint32_t j = 1; j < std::min(nb, r->inflight); ++j)
      HIP_TRY(hipStreamWaitEvent(r->slots[(s0 + j) % r->inflight].stream, d.cleared, 0));
  }
  size_t ev = 0;
  for (uint32_t k = 0; k < nb; ++k) {
    const Batch& bt = batches[k];
    const uint32_t slot = (s0 + k) % r->inflight;
    FrameSlot& fs = r->slots[slot];
    const bool own = fs.stream != r->stream;
    // the slot's radiance is free once the accumulate that last read it ran.
    // (Rotating batch-sized regions of it instead, so that a single-frame
    // draw waits only once per 64 frames, measured -1.1 % on the per-frame
    // cadence: the next kernel then competes with the accumulates for CUs.)
    if (own && fs.acc_recorded) HIP_TRY(hipStreamWaitEvent(fs.stream, fs.acc_done, 0));
    if (own && src.tiles) HIP_TRY(hipStreamWaitEvent(fs.stream, r->list_ready, 0));
    // the noise chunk's upload (once per chunk upload and render stream)
    if (!(bt.noise->waited_streams & (1u << slot))) {
      HIP_TRY(hipStreamWaitEvent(fs.stream, bt.noise->ready, 0));
      bt.noise->waited_streams |= 1u << slot;
    }
    // the camera generation's upload, likewise (set_camera with draws in flight)
    CameraGen* cg = r->cam_cur;
    if (!(cg->waited_streams & (1u << slot))) {
      HIP_TRY(hipStreamWaitEvent(fs.stream, cg->ready, 0));
      cg->waited_streams |= 1u << slot;
    }
    // every batch holding a frame f with f % profile_every == 0: every
    // batch of a batched draw, every 8th single-frame draw
    const bool timed = profile && ((bt.f % r->profile_every) == 0 || (bt.f % r->profile_every) + bt.frames > r->profile_every);
    for (uint32_t b = 0; b < launches_per_batch; ++b) {
      mrt::BounceArgs a{};
      rc = bounce_args(r, src, d, bt, k, b, fs, cg, a);
      if (rc) return rc;
      if (timed) HIP_TRY(hipEventRecord(d.kernel_events[ev++], fs.stream));
      if (r->path_mode)
        HIP_TRY(MRT_BUILD_CALL(r->desc.flags, launch_paths(r->scene->dev, a, r->stack_entries, r->grid, fs.stream)));
      else if (r->stream_mode)
        HIP_TRY(MRT_BUILD_CALL(r->desc.flags, launch_stream(r->scene->dev, a, r->stack_entries, r->grid, fs.stream)));
      else
        HIP_TRY(MRT_BUILD_CALL(r->desc.flags, launch_bounce(r->scene->dev, a, r->stack_entries, r->grid, fs.stream)));
      if (timed) HIP_TRY(hipEventRecord(d.kernel_events[ev++], fs.stream));
    }
    // accumulateImage for frames f .. f+batch-1 on the main stream, in batch
    // order (the running mean's order), behind this batch's render launch
    if (own) {
      HIP_TRY(hipEventRecord(fs.kernel_done, fs.stream));
      HIP_TRY(hipStreamWaitEvent(r->stream, fs.kernel_done, 0));
    }
    const bool fold = k + 1 == nb && r->counter_fold;
    if (src.tiles)
      HIP_TRY(MRT_BUILD_CALL(r->desc.flags, launch_accumulate_counted(accum_args(r, src, d, bt, fs, fold), r->stream)));
    else
      HIP_TRY(MRT_BUILD_CALL(r->desc.flags, launch_accumulate_frame(accum_args(r, src, d, bt, fs, fold), r->stream)));
    HIP_TRY(hipEventRecord(fs.acc_done, r->stream));
    fs.acc_recorded = true;
    if (fold) d.clean = true;
  }
  r->slot_next = (s0 + nb) % r->inflight;
  HIP_TRY(hipEventRecord(d.stop, r->stream));
  // the chunks' buffers are reusable once this draw's accumulates (which
  // follow every render launch of the draw) have run
  for (mrt::NoiseSchedule::Chunk* c : chunks) {
    HIP_TRY(hipEventRecord(c->last_use, r->stream));
    c->used = true;
  }
  {   // enqueued while the previous draw is still rendering (frames in flight)
    const DrawRecord& prev = r->draws[(r->draw_next + kDrawRing - 1) % kDrawRing];
    if (prev.pending && hipEventQuery(prev.stop) == hipErrorNotReady) r->stats.draws_overlapped += 1;
  }
  // (no stream of its own: a process has few hardware queues — 4 by
  // default — and two streams sharing one serialise their launches)
  if (!r->counter_fold)
    HIP_TRY(hipMemcpyAsync(d.host, d.counters.p, d.layout.bytes, hipMemcpyDeviceToHost, r->stream));
  HIP_TRY(hipEventRecord(d.copied, r->stream));
  d.pending = true;
  d.frames = n;
  d.pixels = src.tiles ? 0 : r->owned_pixels;
  d.listed = src.tiles;
  d.events = ev;
  r->draw_next = (r->draw_next + 1) % kDrawRing;
  return MRT_OK;
}

}  // namespace

extern "C" {

// ---------------------------------------------------------------------------
// renderer
// ---------------------------------------------------------------------------
int mrt_renderer_create(const mrt_renderer_desc* desc, mrt_renderer** out) {
  if (!desc || !out || !desc->scene) return fail(MRT_ERR_INVALID, "mrt_renderer_create: null argument");
  *out = nullptr;
  if (desc->width < 2 || desc->height < 2 || desc->width > 32768 || desc->height > 32768)
    return fail(MRT_ERR_INVALID, "image size must be in [2, 32768]");
  if ((uint64_t)desc->width * desc->height >= (1ull << 31)) return fail(MRT_ERR_INVALID, "image too large");
  if (desc->max_path_length == 0 || desc->max_path_length > 64)
    return fail(MRT_ERR_INVALID, "max_path_length must be in [1, 64]");
  const uint32_t S = std::max<uint32_t>(1, desc->shard_count);
  if (desc->shard_rank >= S) return fail(MRT_ERR_INVALID, "shard_rank >= shard_count");
  constexpr uint32_t kKnownFlags = MRT_FLAG_PRECISE | MRT_FLAG_PROFILE | MRT_FLAG_STATIC_NOISE |
                                   MRT_FLAG_NO_ACCUMULATE | MRT_FLAG_DEBUG_MATERIAL | MRT_FLAG_MOMENTS;
  if (desc->flags & ~kKnownFlags) return fail(MRT_ERR_INVALID, "unknown renderer flags");
  if ((desc->flags & MRT_FLAG_MOMENTS) && (desc->flags & MRT_FLAG_NO_ACCUMULATE))
    return fail(MRT_ERR_INVALID, "MRT_FLAG_MOMENTS needs an accumulated image (not with MRT_FLAG_NO_ACCUMULATE)");
  if ((desc->flags & MRT_FLAG_MOMENTS) && S > 1)
    return fail(MRT_ERR_INVALID, "MRT_FLAG_MOMENTS: a sharded moments image is not supported (shard_count > 1)");
  std::unique_ptr<mrt_renderer> r(new mrt_renderer());
  r->scene = desc->scene;
  r->desc = *desc;
  r->desc.shard_count = S;
  HIP_TRY(hipSetDevice(desc->scene->device));
  if (desc->stream) {
    r->stream = (hipStream_t)desc->stream;
  } else {
    HIP_TRY(hipStreamCreateWithFlags(&r->stream, hipStreamNonBlocking));
    r->own_stream = true;
  }
  r->own_image = desc->image == nullptr;
  r->image = desc->image;
  r->noise = std::make_unique<mrt::NoiseSchedule>(desc->seed, (desc->flags & MRT_FLAG_STATIC_NOISE) != 0);
  for (DrawRecord& d : r->draws) {
    HIP_TRY(hipEventCreate(&d.start));
    HIP_TRY(hipEventCreate(&d.stop));
    HIP_TRY(hipEventCreateWithFlags(&d.cleared, hipEventDisableTiming));
    HIP_TRY(hipEventCreateWithFlags(&d.copied, hipEventDisableTiming));
  }
  // LDS stack capacity: the BVH's bound rounded up to 8/16 entries when it is
  // <= 16; deeper BVHs keep 8 entries in LDS and spill the rest to global
  // memory (MRT_STACK overrides the cap).  LDS per block bounds the resident
  // blocks per CU, and for global-memory traversal occupancy wins: C4 with
  // 8 LDS entries + spill ran 1.5x faster than with a 32-entry LDS stack.
  // r3, with traversal slack: trees deeper than 32 entries (the 1M-triangle
  // scenes, 48) keep 12 in LDS — C4 +1.9 %; C3 (26) is best at 8 (12: -0.4 %,
  // C3g -0.9 %), and 16 entries lose everywhere (C4 -0.4 %, C3g -2.4 %)
  // the deeper of the main and the occluder tree (dev.max_stack): shadow rays
  // may traverse either
  const uint32_t need = desc->scene->dev.max_stack;
  uint32_t cap = need <= 16 ? 16 : (need > 32 ? 12 : 8);
  if (const char* v = mrt::diag_env("MRT_STACK")) cap = std::max<uint32_t>(8, (uint32_t)std::strtoul(v, nullptr, 0));
  const uint32_t want = std::min(need, cap);
  r->stack_entries = want <= 8 ? 8 : want <= 12 ? 12 : want <= 16 ? 16 : want <= 24 ? 24 : 32;
  if (need > r->stack_entries)   // spill variants: 8 / 12 (path kernel; the wavefront runs 16) / 16 / 32
    r->stack_entries = r->stack_entries <= 8 ? 8 : r->stack_entries <= 12 ? 12 : r->stack_entries <= 16 ? 16 : 32;
  if (const char* dbg = mrt::diag_env("MRT_DEBUG")) r->debug = (uint32_t)std::strtoul(dbg, nullptr, 0);
  if (const char* v = mrt::diag_env("MRT_COUNTER_FOLD")) r->counter_fold = std::atoi(v) != 0;
  if (const char* v = mrt::diag_env("MRT_PROFILE_EVERY"))
    r->profile_every = std::max<uint32_t>(1, (uint32_t)std::strtoul(v, nullptr, 0));
  {
    int khz = 0;
    if (hipDeviceGetAttribute(&khz, hipDeviceAttributeWallClockRate, desc->scene->device) == hipSuccess)
      r->wall_khz = (double)khz;
  }
  if (const char* v = mrt::diag_env("MRT_SPANS"))
    if (std::atoi(v) == 0) r->wall_khz = 0.0;
  // two frame batches in flight on their own streams (one launch's drain
  // overlaps the next launch's start): a tile share +5 % (r3.3), a whole C2
  // frame +0.9 % (9598 / 9596 / 9600 vs 9521 / 9479 / 9521 Mpaths/s,
  // alternating in one call)
  r->inflight = 2u;
  if (const char* v = mrt::diag_env("MRT_INFLIGHT")) r->inflight = (uint32_t)std::strtoul(v, nullptr, 0);
  r->inflight = std::max<uint32_t>(1, std::min<uint32_t>(8, r->inflight));
  r->slots.resize(r->inflight);
  for (uint32_t k = 0; k < r->inflight; ++k) {
    FrameSlot& fs = r->slots[k];
    if (r->inflight == 1) {   // one slot: everything in order on the main stream
      fs.stream = r->stream;
    } else {
      HIP_TRY(hipStreamCreateWithFlags(&fs.stream, hipStreamNonBlocking));
      fs.own_stream = true;
    }
    HIP_TRY(hipEventCreateWithFlags(&fs.acc_done, hipEventDisableTiming));
    HIP_TRY(hipEventCreateWithFlags(&fs.kernel_done, hipEventDisableTiming));
  }
  // kernel: scenes traversed from global memory run the path megakernel (all
  // bounces of a frame batch in one launch: C3 +15 %, C4 +1.5 % over the
  // wavefront), scenes staged whole in LDS the wavefront of per-bounce
  // launches (C2: the path kernel is 24 % slower); MRT_KERNEL=path|wave
  // overrides.
  if (const char* v = mrt::diag_env("MRT_PRIMARY")) r->primary_allowed = std::atoi(v) != 0;
  if (const char* v = mrt::diag_env("MRT_PRIMARY_CAP"))
    r->primary_cap = std::max<uint32_t>(1, std::min<uint32_t>(mrt::kPrimaryFallback - 1, (uint32_t)std::strtoul(v, nullptr, 0)));
  r->path_mode = mrt::fast::path_preferred(desc->scene->dev);
  if (const char* k = mrt::diag_env("MRT_KERNEL")) r->path_mode = std::strcmp(k, "path") == 0;
  // streaming wavefront (one launch per frame batch, per-wave ray queues)
  // for whole-scene-in-LDS scenes; MRT_STREAM=0 keeps one launch per bounce
  {
    const char* c = mrt::diag_env("MRT_STREAM");
    const bool want = !c || std::atoi(c) != 0;
    r->stream_allowed = want && !r->path_mode && desc->max_path_length <= mrt::kStreamMaxL &&
                        mrt::fast::stream_supported(desc->scene->dev, r->stack_entries);
  }
  // persistent grid of the kernel this renderer launches: the stream kernel
  // sizes it by its own LDS (the per-bounce kernel's segment scratch grows
  // with the grid: sized for that, a 24-KB scene image + stack left C2 at 4
  // instead of 5 blocks per CU)
  if (r->path_mode)
    HIP_TRY(MRT_BUILD_CALL(desc->flags, path_grid(r->scene->dev, r->stack_entries, &r->grid)));
  else if (r->stream_allowed)
    HIP_TRY(MRT_BUILD_CALL(desc->flags, stream_grid(r->scene->dev, r->stack_entries, &r->grid)));
  else
    HIP_TRY(MRT_BUILD_CALL(desc->flags, bounce_grid(r->scene->dev, r->stack_entries, 0u, &r->grid)));
  if (const char* g = mrt::diag_env("MRT_GRID")) r->grid = std::max<uint32_t>(1, (uint32_t)std::strtoul(g, nullptr, 0));
  // the noise schedule's upload stream, staging buffers and worker on the
  // renderer's device.  Created after the render streams: a process has 4
  // hardware queues and streams share them round-robin in creation order, so
  // a stream created before the render streams pushed a render stream onto a
  // queue another stream's work serialises with (C2 -10 %, C4 -7 %, measured r6)
  HIP_TRY(r->noise->init());
  (void)mrt_camera_default(&r->camera);
  int rc = alloc_frame_buffers(r.get());
  if (rc) return rc;
  *out = r.release();
  return MRT_OK;
}

int mrt_renderer_resize(mrt_renderer* r, uint32_t width, uint32_t height) {
  if (!r) return fail(MRT_ERR_INVALID, "null renderer");
  if (width < 2 || height < 2 || width > 32768 || height > 32768) return fail(MRT_ERR_INVALID, "bad size");
  if (!r->own_image) return fail(MRT_ERR_STATE, "cannot resize an externally owned image");
  int rc = finalize_pending(r);
  if (rc) return rc;
  rc = exchange_drop(r, true);   // a pending gather was packed for the old size: never unpack it into the new image
  if (rc) return rc;
  HIP_TRY(hipStreamSynchronize(r->stream));
  r->desc.width = width;
  r->desc.height = height;
  r->x.slab_floats = 0;    // the exchange buffers are re-sized for the new image at the next exchange
  r->guides_current = r->denoised_current = false;
  r->history_valid = r->resolved_current = false;
  r->variance_current = false;
  r->clamped_current = false;
  r->extras_current = r->extras_valid = r->priority_current = false;   // re-made (and zeroed) by the next refine / draw_tiles
  r->tile_error_current = false;
  r->list_count = 0;
  if (r->denoised.p) {     // a renderer that has denoised keeps its buffers, at the new size
    const size_t bytes = (size_t)width * height * 16;
    HIP_TRY(r->guide_n.alloc(bytes));
    HIP_TRY(r->guide_p.alloc(bytes));
    HIP_TRY(r->denoised.alloc(bytes));
    HIP_TRY(r->denoise_scratch.alloc(bytes));
  }
  {   // likewise the temporal history's buffers, each where it exists
    const size_t bytes = (size_t)width * height * 16;
    for (DevBuf* b : {&r->guide_n, &r->guide_p, &r->prev_guide_n, &r->prev_guide_p, &r->temporal_prev, &r->history,
                      &r->resolved, &r->moments_prev, &r->moments_history, &r->moments_resolved})
      if (b->p && b->bytes != bytes) HIP_TRY(b->alloc(bytes));
    if (r->variance.p && r->variance.bytes != bytes / 4) HIP_TRY(r->variance.alloc(bytes / 4));
    if (r->clamped.p && r->clamped.bytes != bytes + 16) HIP_TRY(r->clamped.alloc(bytes + 16));
  }
  return alloc_frame_buffers(r);
}

int mrt_renderer_reset(mrt_renderer* r) {
  if (!r) return fail(MRT_ERR_INVALID, "null renderer");
  int rc = exchange_drop(r, false);   // the pre-reset frame's deferred tiles must not land in the cleared image
  if (rc) return rc;
  // The next frame (f = 0) overwrites every pixel this renderer owns, and
  // pixels it does not own stay 0 — unless an exchange wrote other ranks'
  // tiles into the image: only then is it cleared (stream-ordered after
  // the pending draws).  An external image is always cleared.
  if (r->image_foreign || !r->own_image) {
    HIP_TRY(hipMemsetAsync(r->image, 0, (size_t)r->desc.width * r->desc.height * 16, r->stream));
    r->image_foreign = false;
  }
  if (r->extras_valid) {      // the extra samples go with the frames they refined (stream-ordered, as above)
    const size_t bytes = (size_t)r->desc.width * r->desc.height * 16;
    HIP_TRY(hipMemsetAsync(r->extra.p, 0, bytes, r->stream));
    HIP_TRY(hipMemsetAsync(r->extra_moments.p, 0, bytes, r->stream));
    r->extras_valid = false;
  }
  r->frame_index = 0;
  r->stats.frame_index = 0;   // cumulative counters (paths, A, kernel time) persist
  r->history_valid = false;   // (mrt_renderer_move_camera sets it again once it has reprojected)
  return MRT_OK;
}

int mrt_renderer_set_camera(mrt_renderer* r, const mrt_camera* cam) {
  if (!r) return fail(MRT_ERR_INVALID, "null renderer");
  int rc = mrt_camera_check(cam);
  if (rc) return rc;
  // lists and upload first: a camera that cannot be installed leaves the
  // renderer as it was — the previous camera in force, nothing reset
  const mrt_camera old = r->camera;
  const bool old_moved = r->camera_moved;
  r->camera = *cam;
  r->camera_moved = !camera_is_default(*cam);
  rc = install_camera(r, false);
  if (rc) {
    r->camera = old;
    r->camera_moved = old_moved;
    return rc;
  }
  r->guides_current = false;   // the guide planes were traced with the previous camera
  return mrt_renderer_reset(r);
}

int mrt_renderer_get_camera(const mrt_renderer* r, mrt_camera* out) {
  if (!r || !out) return fail(MRT_ERR_INVALID, "mrt_renderer_get_camera: null argument");
  *out = r->camera;
  return MRT_OK;
}

int mrt_renderer_prepare(mrt_renderer* r, uint32_t n) {
  if (!r) return fail(MRT_ERR_INVALID, "null renderer");
  return acquire_noise(r, r->noise.get(), (int64_t)r->frame_index, std::max<uint32_t>(1, n), nullptr);
}

int mrt_renderer_draw_n(mrt_renderer* r, uint32_t n) {
  if (!r) return fail(MRT_ERR_INVALID, "null renderer");
  if (r->max_frames)   // MAX_FRAMES: renderer/Renderer.mm:589-590
    n = r->frame_index >= r->max_frames ? 0u : (uint32_t)std::min<uint64_t>(n, r->max_frames - r->frame_index);
  if (n == 0) return MRT_OK;
  DrawSource src;
  src.noise = r->noise.get();
  src.f0 = r->frame_index;
  src.image = r->image;
  src.moments = r->moments.as<float>();
  const int rc = draw_frames(r, n, src);
  if (rc) return rc;
  r->stats.draws += 1;
  r->frame_index += n;
  r->stats.frame_index = r->frame_index;
  r->stats.paths += r->owned_pixels * n;
  return MRT_OK;
}

int mrt_renderer_draw(mrt_renderer* r) { return mrt_renderer_draw_n(r, 1); }

int mrt_renderer_set_max_frames(mrt_renderer* r, uint32_t max_frames) {
  if (!r) return fail(MRT_ERR_INVALID, "null renderer");
  r->max_frames = max_frames;
  return MRT_OK;
}

int mrt_renderer_sync(mrt_renderer* r) {
  if (!r) return fail(MRT_ERR_INVALID, "null renderer");
  // the last collective first, with a bound: a stream blocked by a stuck
  // peer's collective would otherwise hold this host wait forever
  int rc = exchange_wait(r);
  if (rc) return rc;
  rc = finalize_pending(r);
  if (rc) return rc;
  HIP_TRY(hipStreamSynchronize(r->stream));
  return MRT_OK;
}

int mrt_renderer_image(mrt_renderer* r, float** device_image) {
  if (!r || !device_image) return fail(MRT_ERR_INVALID, "null argument");
  *device_image = r->image;
  return MRT_OK;
}

int mrt_renderer_stream(mrt_renderer* r, void** stream) {
  if (!r || !stream) return fail(MRT_ERR_INVALID, "null argument");
  *stream = (void*)r->stream;
  return MRT_OK;
}

int mrt_renderer_read_image(mrt_renderer* r, float* rgba, size_t count) {
  if (!r || !rgba) return fail(MRT_ERR_INVALID, "null argument");
  const size_t need = (size_t)r->desc.width * r->desc.height * 4;
  if (count < need) return fail(MRT_ERR_INVALID, "output buffer too small");
  int rc = exchange_flush(r);   // a deferred (overlapped) exchange lands first
  if (rc) return rc;
  rc = mrt_renderer_sync(r);
  if (rc) return rc;
  HIP_TRY(hipMemcpy(rgba, r->image, need * 4, hipMemcpyDeviceToHost));
  return MRT_OK;
}

int mrt_renderer_save_image(mrt_renderer* r, const char* path) { return save_read(r, path, mrt_renderer_read_image); }

int mrt_renderer_denoise(mrt_renderer* r, const mrt_denoise_params* params) {
  if (!r) return fail(MRT_ERR_INVALID, "null renderer");
  if (r->frame_index == 0)
    return fail(MRT_ERR_STATE, "mrt_renderer_denoise: no frame accumulated since create, resize, reset or set_camera");
  mrt_denoise_params p;
  if (params) p = *params;
  else (void)mrt_denoise_params_default(r->frame_index, &p);
  int rc = mrt_denoise_params_check(&p);
  if (rc) return rc;
  const uint32_t W = r->desc.width, H = r->desc.height;
  const size_t bytes = (size_t)W * H * 16;
  HIP_TRY(hipSetDevice(r->scene->device));
  if (r->denoised.bytes != bytes || !r->denoised.p) {   // first denoise (resize re-makes existing buffers)
    r->guides_current = r->denoised_current = false;
    HIP_TRY(r->guide_n.alloc(bytes));
    HIP_TRY(r->guide_p.alloc(bytes));
    HIP_TRY(r->denoised.alloc(bytes));
    HIP_TRY(r->denoise_scratch.alloc(bytes));
  }
  rc = exchange_flush(r);   // a deferred (overlapped) exchange lands in the image first
  if (rc) return rc;
  if (!r->guides_current) {
    if (!r->guide_spill.p) HIP_TRY(alloc_isect_spill(r->guide_spill, r->scene->dev.max_stack));
    rc = guides_with_spill(r->scene, &r->camera, W, H, r->guide_n.as<float>(), r->guide_p.as<float>(),
                           r->desc.flags & MRT_FLAG_PRECISE, r->guide_spill.as<uint32_t>(), r->stream);
    if (rc) return rc;
    r->guides_current = true;
  }
  rc = mrt_denoise(r->image, r->guide_n.as<float>(), r->guide_p.as<float>(), r->denoised.as<float>(),
                   r->denoise_scratch.as<float>(), W, H, &p, r->stream);
  if (rc) return rc;
  r->denoised_current = true;
  return MRT_OK;
}

int mrt_renderer_read_denoised(mrt_renderer* r, float* rgba, size_t count) {
  return read_plane(r, &mrt_renderer::denoised, &mrt_renderer::denoised_current,
                    "no denoise has run at the renderer's current size", rgba, count);
}

int mrt_renderer_save_denoised(mrt_renderer* r, const char* path) { return save_read(r, path, mrt_renderer_read_denoised); }

// ---- temporal history (include/mrt.h: mrt_renderer_move_camera) -------------
int mrt_renderer_move_camera(mrt_renderer* r, const mrt_camera* cam, const mrt_reproject_params* params) {
  int rc = temporal_usable(r, "mrt_renderer_move_camera");
  if (rc) return rc;
  rc = mrt_camera_check(cam);
  if (rc) return rc;
  mrt_reproject_params p;
  if (params) p = *params;
  else (void)mrt_reproject_params_default(&p);
  rc = mrt_reproject_params_check(&p);
  if (rc) return rc;
  if (r->frame_index == 0 && !r->history_valid) return mrt_renderer_set_camera(r, cam);   // nothing to carry
  const uint32_t W = r->desc.width, H = r->desc.height;
  const size_t bytes = (size_t)W * H * 16;
  HIP_TRY(hipSetDevice(r->scene->device));
  for (DevBuf* b : {&r->prev_guide_n, &r->prev_guide_p, &r->temporal_prev, &r->history})   // the first move only
    if (b->bytes != bytes || !b->p) HIP_TRY(b->alloc(bytes));
  const bool moments = (r->desc.flags & MRT_FLAG_MOMENTS) != 0;
  if (moments)
    for (DevBuf* b : {&r->moments_prev, &r->moments_history})
      if (b->bytes != bytes || !b->p) HIP_TRY(b->alloc(bytes));
  // what the old camera saw: its guide planes, and everything accumulated
  // through it (a scratch image: the history itself is replaced last)
  rc = ensure_guides(r);
  if (rc) return rc;
  rc = resolve_into(r, r->temporal_prev);
  if (rc) return rc;
  if (moments) {   // the moments travel with the colour, through the same two kernels
    rc = resolve_moments_into(r, r->moments_prev);
    if (rc) return rc;
  }
  // the new camera, as mrt_renderer_set_camera installs it: failing here
  // leaves the previous camera in force, nothing reset, the history as it was
  const mrt_camera old = r->camera;
  const bool old_moved = r->camera_moved;
  r->camera = *cam;
  r->camera_moved = !camera_is_default(*cam);
  rc = install_camera(r, false);
  if (rc) {
    r->camera = old;
    r->camera_moved = old_moved;
    return rc;
  }
  std::swap(r->guide_n.p, r->prev_guide_n.p);   // equal sizes: the planes of `old` become the previous ones
  std::swap(r->guide_p.p, r->prev_guide_p.p);
  r->guides_current = false;
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

int mrt_renderer_resolve(mrt_renderer* r) {
  int rc = temporal_usable(r, "mrt_renderer_resolve");
  if (rc) return rc;
  if (r->frame_index == 0 && !r->history_valid)
    return fail(MRT_ERR_STATE, "mrt_renderer_resolve: no frame accumulated and no valid history");
  HIP_TRY(hipSetDevice(r->scene->device));
  rc = resolve_into(r, r->resolved);
  if (rc) return rc;
  r->resolved_current = true;
  return MRT_OK;
}

int mrt_renderer_read_resolved(mrt_renderer* r, float* rgba, size_t count) {
  return read_plane(r, &mrt_renderer::resolved, &mrt_renderer::resolved_current,
                    "no resolve has run at the renderer's current size", rgba, count);
}

int mrt_renderer_save_resolved(mrt_renderer* r, const char* path) { return save_read(r, path, mrt_renderer_read_resolved); }

int mrt_renderer_denoise_resolved(mrt_renderer* r, const mrt_denoise_params* params) {
  int rc = temporal_usable(r, "mrt_renderer_denoise_resolved");
  if (rc) return rc;
  if (r->frame_index == 0 && !r->history_valid)
    return fail(MRT_ERR_STATE, "mrt_renderer_denoise_resolved: no frame accumulated and no valid history");
  mrt_denoise_params p;
  if (params) p = *params;
  else (void)mrt_denoise_params_default(std::max<uint64_t>(r->frame_index, 1), &p);
  rc = mrt_denoise_params_check(&p);
  if (rc) return rc;
  const uint32_t W = r->desc.width, H = r->desc.height;
  const size_t bytes = (size_t)W * H * 16;
  HIP_TRY(hipSetDevice(r->scene->device));
  for (DevBuf* b : {&r->denoised, &r->denoise_scratch})
    if (b->bytes != bytes || !b->p) {
      r->denoised_current = false;
      HIP_TRY(b->alloc(bytes));
    }
  rc = mrt_renderer_resolve(r);
  if (rc) return rc;
  rc = ensure_guides(r);
  if (rc) return rc;
  rc = mrt_denoise(r->resolved.as<float>(), r->guide_n.as<float>(), r->guide_p.as<float>(), r->denoised.as<float>(),
                   r->denoise_scratch.as<float>(), W, H, &p, r->stream);
  if (rc) return rc;
  r->denoised_current = true;
  return MRT_OK;
}

// ---- variance-guided denoising (include/mrt.h: mrt_renderer_denoise_variance) ----
int mrt_renderer_read_moments(mrt_renderer* r, float* rgba, size_t count) {
  if (!r || !rgba) return fail(MRT_ERR_INVALID, "null argument");
  const size_t need = (size_t)r->desc.width * r->desc.height * 4;
  if (count < need) return fail(MRT_ERR_INVALID, "output buffer too small");
  if (!(r->desc.flags & MRT_FLAG_MOMENTS))
    return fail(MRT_ERR_STATE, "mrt_renderer_read_moments: the renderer was created without MRT_FLAG_MOMENTS");
  const int rc = mrt_renderer_sync(r);
  if (rc) return rc;
  HIP_TRY(hipMemcpy(rgba, r->moments.p, need * 4, hipMemcpyDeviceToHost));
  return MRT_OK;
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
  mrt_svgf_params p;
  if (params) p = *params;
  else (void)mrt_svgf_params_default(&p);
  int rc = mrt_svgf_params_check(&p);
  if (rc) return rc;
  const uint32_t W = r->desc.width, H = r->desc.height;
  const size_t bytes = (size_t)W * H * 16;
  HIP_TRY(hipSetDevice(r->scene->device));
  for (DevBuf* b : {&r->denoised, &r->denoise_scratch})
    if (b->bytes != bytes || !b->p) {
      r->denoised_current = false;
      HIP_TRY(b->alloc(bytes));
    }
  if (r->variance.bytes != bytes / 4 || !r->variance.p) {
    r->variance_current = false;
    HIP_TRY(r->variance.alloc(bytes / 4));
  }
  rc = ensure_guides(r);
  if (rc) return rc;
  rc = mrt_renderer_resolve(r);
  if (rc) return rc;
  rc = resolve_moments_into(r, r->moments_resolved);
  if (rc) return rc;
  const float* filtered = r->resolved.as<float>();
  if (r->firefly_on) {   // the filter's input is the clamped copy; the resolved buffer stays as it is
    if (r->clamped.bytes != bytes + 16 || !r->clamped.p) {
      r->clamped_current = false;
      HIP_TRY(r->clamped.alloc(bytes + 16));
    }
    rc = mrt_firefly_clamp(r->resolved.as<float>(), r->guide_n.as<float>(), r->guide_p.as<float>(),
                           r->clamped.as<float>(), reinterpret_cast<uint32_t*>(r->clamped.as<char>() + bytes), W, H,
                           &r->firefly, r->stream);
    if (rc) return rc;
    r->clamped_current = true;
    filtered = r->clamped.as<float>();
  }
  rc = mrt_variance(r->moments_resolved.as<float>(), r->guide_n.as<float>(), r->guide_p.as<float>(),
                    r->variance.as<float>(), W, H, &p, r->stream);
  if (rc) return rc;
  r->variance_current = true;
  rc = mrt_denoise_variance(filtered, r->variance.as<float>(), r->guide_n.as<float>(), r->guide_p.as<float>(),
                            r->denoised.as<float>(), r->denoise_scratch.as<float>(), nullptr, W, H, &p, r->stream);
  if (rc) return rc;
  r->denoised_current = true;
  return MRT_OK;
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
  const int rc = read_plane(r, &mrt_renderer::clamped, &mrt_renderer::clamped_current,
                            "no firefly clamp has run at the renderer's current size", rgba, count);
  if (rc) return rc;
  if (clamped_pixels)
    HIP_TRY(hipMemcpy(clamped_pixels, r->clamped.as<char>() + (size_t)r->desc.width * r->desc.height * 16, 4,
                      hipMemcpyDeviceToHost));
  return MRT_OK;
}

int mrt_renderer_read_variance(mrt_renderer* r, float* plane, size_t count) {
  if (!r || !plane) return fail(MRT_ERR_INVALID, "null argument");
  const size_t need = (size_t)r->desc.width * r->desc.height;
  if (count < need) return fail(MRT_ERR_INVALID, "output buffer too small");
  if (!r->variance_current)
    return fail(MRT_ERR_STATE, "no mrt_renderer_denoise_variance has run at the renderer's current size");
  const int rc = mrt_renderer_sync(r);
  if (rc) return rc;
  HIP_TRY(hipMemcpy(plane, r->variance.p, need * 4, hipMemcpyDeviceToHost));
  return MRT_OK;
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
  mrt_adaptive_params p;
  if (params) p = *params;
  else (void)mrt_adaptive_params_default(&p);
  rc = mrt_adaptive_params_check(&p);
  if (rc) return rc;
  if (r->frame_index == 0 && !r->history_valid)
    return fail(MRT_ERR_STATE, "mrt_renderer_refine: no frame accumulated and no valid history");
  mrt_svgf_params sp;
  (void)mrt_svgf_params_default(&sp);
  rc = ensure_extras(r);
  if (rc) return rc;
  const size_t bytes = (size_t)W * H * 16;
  if (r->variance.bytes != bytes / 4 || !r->variance.p) {
    r->variance_current = false;
    HIP_TRY(r->variance.alloc(bytes / 4));
  }
  rc = ensure_guides(r);
  if (rc) return rc;
  rc = mrt_renderer_resolve(r);
  if (rc) return rc;
  rc = resolve_moments_into(r, r->moments_resolved);
  if (rc) return rc;
  rc = mrt_variance(r->moments_resolved.as<float>(), r->guide_n.as<float>(), r->guide_p.as<float>(),
                    r->variance.as<float>(), W, H, &sp, r->stream);
  if (rc) return rc;
  r->variance_current = true;
  rc = mrt_tile_priority(r->resolved.as<float>(), r->variance.as<float>(), r->guide_n.as<float>(),
                         r->tile_priority.as<float>(), W, H, &p, r->desc.flags & MRT_FLAG_PRECISE, r->stream);
  if (rc) return rc;
  r->priority_current = true;
  rc = mrt_tile_select(r->tile_priority.as<float>(), T, tile_count, r->tile_list.as<uint32_t>(), r->stream);
  if (rc) return rc;
  return draw_extra(r, nullptr, tile_count, frames);
}

int mrt_renderer_read_extra(mrt_renderer* r, float* rgba, size_t count) {
  return r ? read_extra_plane(r, r->extra, rgba, count) : fail(MRT_ERR_INVALID, "null argument");
}

int mrt_renderer_read_extra_moments(mrt_renderer* r, float* rgba, size_t count) {
  return r ? read_extra_plane(r, r->extra_moments, rgba, count) : fail(MRT_ERR_INVALID, "null argument");
}

int mrt_renderer_read_tile_priority(mrt_renderer* r, float* priority, size_t count) {
  if (!r || !priority) return fail(MRT_ERR_INVALID, "null argument");
  const size_t T = (size_t)r->tiles_x * r->tiles_y;
  if (count < T) return fail(MRT_ERR_INVALID, "output buffer too small");
  if (!r->priority_current) return fail(MRT_ERR_STATE, "no refine has run at the renderer's current size");
  const int rc = mrt_renderer_sync(r);
  if (rc) return rc;
  HIP_TRY(hipMemcpy(priority, r->tile_priority.p, T * 4, hipMemcpyDeviceToHost));
  return MRT_OK;
}

int mrt_renderer_read_tile_list(mrt_renderer* r, uint32_t* tiles, size_t capacity, uint32_t* count) {
  if (!r || !tiles || !count) return fail(MRT_ERR_INVALID, "null argument");
  if (r->list_count == 0) return fail(MRT_ERR_STATE, "no refine or draw_tiles has run at the renderer's current size");
  if (capacity < r->list_count) return fail(MRT_ERR_INVALID, "output buffer too small");
  const int rc = mrt_renderer_sync(r);
  if (rc) return rc;
  HIP_TRY(hipMemcpy(tiles, r->tile_list.p, (size_t)r->list_count * 4, hipMemcpyDeviceToHost));
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
namespace {
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
  for (DevBuf* b : {&r->tile_error, &r->tile_pixels})
    if (b->bytes != (size_t)T * 4 || !b->p) {
      r->tile_error_current = false;
      HIP_TRY(b->alloc((size_t)T * 4));
    }
  if (!r->error_summary.p) HIP_TRY(r->error_summary.alloc(sizeof(mrt_error_summary)));
  if (!r->summary_host)
    HIP_TRY(hipHostMalloc(reinterpret_cast<void**>(&r->summary_host), sizeof(mrt_error_summary), hipHostMallocDefault));
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
  HIP_TRY(hipMemcpyAsync(r->summary_host, r->error_summary.p, sizeof(mrt_error_summary), hipMemcpyDeviceToHost, r->stream));
  HIP_TRY(hipStreamSynchronize(r->stream));
  *out = *r->summary_host;
  r->list_count = out->tiles_listed;
  return MRT_OK;
}
}  // namespace

int mrt_renderer_error(mrt_renderer* r, const mrt_svgf_params* svgf, float luminance_floor, float threshold,
                       mrt_error_summary* out) {
  if (!r || !out) return fail(MRT_ERR_INVALID, "null argument");
  mrt_svgf_params sp;
  if (svgf) sp = *svgf;
  else (void)mrt_svgf_params_default(&sp);
  mrt_adaptive_params ap;
  (void)mrt_adaptive_params_default(&ap);
  if (luminance_floor != 0.0f) ap.luminance_floor = luminance_floor;
  const int rc = estimate_usable(r, "mrt_renderer_error", sp, ap, threshold);
  return rc ? rc : estimate(r, sp, ap, threshold, out);
}

int mrt_renderer_read_tile_error(mrt_renderer* r, float* mean_error, uint32_t* pixels, size_t count) {
  if (!r || !mean_error || !pixels) return fail(MRT_ERR_INVALID, "null argument");
  const size_t T = (size_t)r->tiles_x * r->tiles_y;
  if (count < T) return fail(MRT_ERR_INVALID, "output buffer too small");
  if (!r->tile_error_current) return fail(MRT_ERR_STATE, "no error estimate has run at the renderer's current size");
  const int rc = mrt_renderer_sync(r);
  if (rc) return rc;
  HIP_TRY(hipMemcpy(mean_error, r->tile_error.p, T * 4, hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(pixels, r->tile_pixels.p, T * 4, hipMemcpyDeviceToHost));
  return MRT_OK;
}

int mrt_renderer_converge(mrt_renderer* r, const mrt_converge_params* params, mrt_converge_result* out) {
  if (!r || !out) return fail(MRT_ERR_INVALID, "null argument");
  mrt_converge_params p;
  if (params) p = *params;
  else (void)mrt_converge_params_default(&p);
  int rc = mrt_converge_params_check(&p);
  if (rc) return rc;
  mrt_svgf_params sp;
  (void)mrt_svgf_params_default(&sp);
  mrt_adaptive_params ap;
  ap.luminance_floor = p.luminance_floor;
  rc = estimate_usable(r, "mrt_renderer_converge", sp, ap, p.target_error);
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
  const size_t need = (size_t)r->desc.width * r->desc.height * 4;
  if (count < need) return fail(MRT_ERR_INVALID, "output buffer too small");
  if (((flags >> 8) & 0xFFu) && !r->reference.p) return fail(MRT_ERR_STATE, "compare mode without a loaded reference");
  const bool denoised = (flags & MRT_DISPLAY_DENOISED) != 0;
  const bool resolved = (flags & MRT_DISPLAY_RESOLVED) != 0;
  if (denoised && resolved) return fail(MRT_ERR_INVALID, "MRT_DISPLAY_DENOISED and MRT_DISPLAY_RESOLVED are exclusive");
  if (denoised && !r->denoised_current) return fail(MRT_ERR_STATE, "MRT_DISPLAY_DENOISED without a denoise at the current size");
  if (resolved && !r->resolved_current) return fail(MRT_ERR_STATE, "MRT_DISPLAY_RESOLVED without a resolve at the current size");
  int rc = exchange_flush(r);
  if (rc) return rc;
  if (r->display.bytes < need * 4) HIP_TRY(r->display.alloc(need * 4));
  rc = mrt_display(denoised ? r->denoised.as<float>() : (resolved ? r->resolved.as<float>() : r->image), r->reference.as<float>(), r->display.as<float>(), r->desc.width, r->desc.height, flags,
                   compare_scale, r->stream);
  if (rc) return rc;
  HIP_TRY(hipMemcpyAsync(rgba, r->display.p, need * 4, hipMemcpyDeviceToHost, r->stream));
  return mrt_renderer_sync(r);
}

int mrt_renderer_display_enqueue(mrt_renderer* r, uint32_t flags, float compare_scale, uint32_t slot) {
  if (!r) return fail(MRT_ERR_INVALID, "null renderer");
  if (slot >= MRT_DISPLAY_SLOTS) return fail(MRT_ERR_INVALID, "display slot >= MRT_DISPLAY_SLOTS");
  if (((flags >> 8) & 0xFFu) && !r->reference.p) return fail(MRT_ERR_STATE, "compare mode without a loaded reference");
  const size_t need = (size_t)r->desc.width * r->desc.height * 4;
  const bool denoised = (flags & MRT_DISPLAY_DENOISED) != 0;
  const bool resolved = (flags & MRT_DISPLAY_RESOLVED) != 0;
  if (denoised && resolved) return fail(MRT_ERR_INVALID, "MRT_DISPLAY_DENOISED and MRT_DISPLAY_RESOLVED are exclusive");
  if (denoised && !r->denoised_current) return fail(MRT_ERR_STATE, "MRT_DISPLAY_DENOISED without a denoise at the current size");
  if (resolved && !r->resolved_current) return fail(MRT_ERR_STATE, "MRT_DISPLAY_RESOLVED without a resolve at the current size");
  auto& ds = r->shown[slot];
  if (ds.queued) HIP_TRY(hipEventSynchronize(ds.done));   // its previous copy may still be landing
  if (ds.floats != need) {
    if (ds.host) HIP_TRY(hipHostFree(ds.host));
    ds.host = nullptr;
    ds.floats = 0;
    HIP_TRY(hipHostMalloc(reinterpret_cast<void**>(&ds.host), need * 4, hipHostMallocDefault));
    ds.floats = need;
  }
  if (!ds.done) HIP_TRY(hipEventCreateWithFlags(&ds.done, hipEventDisableTiming));
  int rc = exchange_flush(r);
  if (rc) return rc;
  // one device blit buffer: the next blit is queued behind this copy
  if (r->display.bytes < need * 4) HIP_TRY(r->display.alloc(need * 4));
  rc = mrt_display(denoised ? r->denoised.as<float>() : (resolved ? r->resolved.as<float>() : r->image), r->reference.as<float>(), r->display.as<float>(),
                   r->desc.width, r->desc.height, flags, compare_scale, r->stream);
  if (rc) return rc;
  HIP_TRY(hipMemcpyAsync(ds.host, r->display.p, need * 4, hipMemcpyDeviceToHost, r->stream));
  HIP_TRY(hipEventRecord(ds.done, r->stream));
  ds.queued = true;
  return MRT_OK;
}

int mrt_renderer_display_map(mrt_renderer* r, uint32_t slot, const float** rgba, size_t* count) {
  if (!r || !rgba) return fail(MRT_ERR_INVALID, "null argument");
  if (slot >= MRT_DISPLAY_SLOTS) return fail(MRT_ERR_INVALID, "display slot >= MRT_DISPLAY_SLOTS");
  auto& ds = r->shown[slot];
  if (!ds.queued || ds.floats != (size_t)r->desc.width * r->desc.height * 4)
    return fail(MRT_ERR_STATE, "display slot not enqueued at the current size");
  HIP_TRY(hipEventSynchronize(ds.done));
  *rgba = ds.host;
  if (count) *count = ds.floats;
  return MRT_OK;
}

int mrt_renderer_stats(const mrt_renderer* r, mrt_stats* stats) {
  if (!r || !stats) return fail(MRT_ERR_INVALID, "null argument");
  int rc = finalize_pending(const_cast<mrt_renderer*>(r));
  if (rc) return rc;
  *stats = r->stats;
  const mrt::NoiseSchedule::Counters& c = r->noise->counters();
  stats->noise_ms = c.gen_ms - r->noise_base.gen_ms;
  stats->noise_tables = c.tables - r->noise_base.tables;
  stats->noise_prefetched = c.prefetched - r->noise_base.prefetched;
  return MRT_OK;
}

int mrt_renderer_destroy(mrt_renderer* r) {
  if (!r) return MRT_OK;
  (void)exchange_wait(r);   // bounded: a failed communicator is aborted, not waited for
  (void)finalize_pending(r);
  if (r->stream) (void)hipStreamSynchronize(r->stream);
  for (int i = 0; i < 2; ++i) {   // an overlapped gather may still read the packed tiles
    if (r->x.gather_recorded[i]) (void)hipEventSynchronize(r->x.gather_done[i]);
    if (r->x.pack_done[i]) (void)hipEventDestroy(r->x.pack_done[i]);
    if (r->x.gather_done[i]) (void)hipEventDestroy(r->x.gather_done[i]);
  }
  if (r->x.coll_done) (void)hipEventDestroy(r->x.coll_done);
  if (r->own_image && r->image) (void)hipFree(r->image);
  for (auto& ds : r->shown) {
    if (ds.done) (void)hipEventDestroy(ds.done);
    if (ds.host) (void)hipHostFree(ds.host);
  }
  for (FrameSlot& fs : r->slots) {
    if (fs.acc_done) (void)hipEventDestroy(fs.acc_done);
    if (fs.kernel_done) (void)hipEventDestroy(fs.kernel_done);
    if (fs.own_stream) (void)hipStreamDestroy(fs.stream);
  }
  r->slots.clear();
  for (DrawRecord& d : r->draws) {
    for (hipEvent_t e : d.kernel_events) (void)hipEventDestroy(e);
    if (d.start) (void)hipEventDestroy(d.start);
    if (d.stop) (void)hipEventDestroy(d.stop);
    if (d.cleared) (void)hipEventDestroy(d.cleared);
    if (d.copied) (void)hipEventDestroy(d.copied);
    if (d.host) (void)hipHostFree(d.host);
  }
  if (r->list_ready) (void)hipEventDestroy(r->list_ready);
  if (r->summary_host) (void)hipHostFree(r->summary_host);
  for (DrawRecord& d : r->draws)
    if (d.list_host) (void)hipHostFree(d.list_host);
  r->refine_noise.reset();
  r->noise.reset();   // joins the worker; the draws reading its chunks have finished (stream synchronised above)
  if (r->own_stream) (void)hipStreamDestroy(r->stream);
  delete r;
  return MRT_OK;
}

}  // extern "C"
