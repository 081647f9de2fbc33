// renderer.cpp — the renderer of include/mrt.h: life cycle, camera
// generations, the draw loop and its statistics, and the read-back of the
// image.  (What a renderer derives from the image — filtered, resolved and
// displayed images, tile planes: renderer_post.cpp; scene: scene_api.cpp; stage
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
#include <cstdlib>

#include "host_internal.h"
#include "diag_env.h"
#include "image.h"
#include "primary.h"

using namespace mrt::host;

namespace {

// pixels of tile t inside the image
uint64_t pixels_of_tile(const mrt_renderer* r, uint32_t t) {
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
  const uint32_t* cnt = d.host.host<uint32_t>();
  if (d.listed) {   // a refine draw: its list is on the host by now (uploaded from there, or copied back behind the draw)
    d.pixels = 0;
    for (uint32_t k = 0; k < d.listed; ++k) d.pixels += pixels_of_tile(r, d.list_host.host<uint32_t>()[k]);
    r->refine_stats.paths += d.pixels * d.frames;
  }
  uint64_t active = d.pixels * d.frames;   // bounce 0: every rendered pixel's camera ray
  for (uint32_t k = 0; k < lay.batches; ++k)
    for (uint32_t b = 0; b + 1 < lay.L; ++b) active += cnt[lay.total(k, b)];
  r->stats.active_ray_bounces += active;
  r->stats.last_draw_ms = ms;
  const uint64_t paths = d.pixels * d.frames;
  r->stats.mpaths_per_s = ms > 0.0f ? (double)paths / (ms * 1e-3) / 1e6 : 0.0;
  r->stats.kernel_launches += (uint64_t)lay.batches * mrt::launches_per_batch(r->plan.kind, lay.L);
  for (uint32_t k = 0; k < lay.batches; ++k) {
    unsigned long long sp[2];
    std::memcpy(sp, d.host.host<char>() + lay.span(k), 16);
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
  const bool lists_possible = r->primary_allowed && r->plan.kind != mrt::KernelKind::Path;
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
    HIP_TRY(c->host.reserve(cap_bytes, hipHostMallocDefault));
    return MRT_OK;
  };
  CameraGen* g = nullptr;
  while (idle && r->cams.size() < kCameraGens) {   // all generations exist from create on
    r->cams.emplace_back(new CameraGen());
    CameraGen* c = r->cams.back().get();
    HIP_TRY(c->ready.create(hipEventDisableTiming));
    HIP_TRY(c->retired.create(hipEventDisableTiming));
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
  if (g->dev.bytes < cap_bytes || g->host.bytes() < cap_bytes)   // sized in the idle path for this frame size
    return fail(MRT_ERR_STATE, "camera: generation smaller than the frame's bound");
  std::memcpy(g->host.host(), &cb, sizeof(cb));
  if (lists) std::memcpy(g->host.host<char>() + sizeof(cb), pl.words.data(), pl.words.size() * 4);
  if (idle) {
    HIP_TRY(hipMemcpy(g->dev.p, g->host.host(), bytes, hipMemcpyHostToDevice));
    g->async = false;
    g->waited_streams = ~0u;
  } else {
    const uint32_t slot = r->slot_next;
    HIP_TRY(hipMemcpyAsync(g->dev.p, g->host.host(), bytes, hipMemcpyHostToDevice, r->slots[slot].stream));
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

// r->plan (kernel_plan.h): the kernel this renderer launches, decided from the
// scene (at create, and again when the scene is swapped), and what the frame
// buffers are sized for
int plan_kernel(mrt_renderer* r) {
  using mrt::KernelKind;
  const mrt::DeviceScene& dev = r->scene->dev;
  mrt::KernelPlan& p = r->plan;
  std::optional<uint32_t> cap;   // MRT_STACK overrides the stack rule's cap
  if (const char* v = mrt::diag_env("MRT_STACK")) cap = (uint32_t)std::strtoul(v, nullptr, 0);
  // kind: scenes traversed from global memory run the path megakernel (all
  // bounces of a frame batch in one launch: C3 +15 %, C4 +1.5 % over the
  // wavefront), scenes staged whole in LDS the wavefront (C2: the path kernel
  // is 24 % slower); MRT_KERNEL=path|wave overrides.
  bool path = mrt::fast::path_preferred(dev);
  if (const char* k = mrt::diag_env("MRT_KERNEL")) path = std::strcmp(k, "path") == 0;
  p.kind = path ? KernelKind::Path : KernelKind::Bounce;
  const mrt::StackChoice st = mrt::stack_rule(p.kind, dev.max_stack, cap);   // (entries and spill: the same for every kind)
  p.stack_entries = st.stack_entries;
  p.spills = st.spills;
  // the wavefront streams (one launch per frame batch, per-wave ray queues)
  // where the stream kernel supports the scene: whole in LDS, no stack spill;
  // MRT_STREAM=0 keeps one launch per bounce
  const char* c = mrt::diag_env("MRT_STREAM");
  if (!path && (!c || std::atoi(c) != 0) && r->desc.max_path_length <= mrt::kStreamMaxL &&
      mrt::fast::kernel_supported(KernelKind::Stream, dev, p.stack_entries))
    p.kind = KernelKind::Stream;
  // persistent grid of that kernel: the stream kernel sizes it by its own LDS
  // (the per-bounce kernel's segment scratch grows with the grid: sized for
  // that, a 24-KB scene image + stack left C2 at 4 instead of 5 blocks per CU)
  HIP_TRY(MRT_BUILD_CALL(r->desc.flags, kernel_grid(p.kind, dev, p.stack_entries, &p.grid)));
  if (const char* g = mrt::diag_env("MRT_GRID")) p.grid = std::max<uint32_t>(1, (uint32_t)std::strtoul(g, nullptr, 0));
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
  const size_t slots = owned_slots * r->batch + (size_t)r->plan.grid * (256 + mrt::kSegSlack);
  const bool path = r->plan.kind == mrt::KernelKind::Path, stream = r->plan.kind == mrt::KernelKind::Stream;
  // (a buffer that already has its size is kept: a scene swap, which comes here at
  // an unchanged frame size, neither frees nor allocates the radiance rows)
  auto sized = [](DevBuf& b, size_t n) { return b.bytes == n && (b.p || !n) ? hipSuccess : b.alloc(n); };
  for (FrameSlot& fs : r->slots) {
    HIP_TRY(sized(fs.segments, ((size_t)4 * r->plan.grid + 2) * 4));   // 2 queues x 2 classes x grid + 2 chunk words
    HIP_TRY(hipMemsetAsync(fs.segments.p, 0, fs.segments.bytes, r->stream));
    // the path kernel keeps the path state in LDS: no ray queues; the
    // streaming wavefront needs only its per-wave queues
    const size_t qslots = stream ? mrt::stream_slots(r->desc.max_path_length, r->plan.grid) : slots;
    // (stream mode: queue[1] is unused but for its plane 0, the partial hits
    // of recycled rays — 16 B a slot, as the other planes — where the scene's
    // nearest queries sweep under a cap, kern_bounce.h bounce_wave)
    const mrt::DeviceScene& dev = r->scene->dev;
    const bool partial = stream && dev.sweep_leaves && dev.sweep_cap < mrt::kSweepLeaves;
    for (int q = 0; q < 2; ++q)
      for (int p = 0; p < mrt::kQueuePlanes; ++p)
        HIP_TRY(sized(fs.queue[q][p], path || (stream && q == 1 && !(partial && p == 0)) ? 0 : qslots * 16));
    HIP_TRY(sized(fs.radiance, owned_slots * r->batch * 16));
    // spill rows of max_stack words per lane (dev_lds.h LdsCtx::spill_lane)
    HIP_TRY(sized(fs.spill, r->plan.spills ? (size_t)dev.max_stack * r->plan.grid * 256 * 4 : 0));
  }
  if (!r->desc.image) {
    r->image = nullptr;
    HIP_TRY(sized(r->image_buf, (size_t)W * H * 16));
    r->image = r->image_buf.as<float>();
  }
  HIP_TRY(hipMemsetAsync(r->image, 0, (size_t)W * H * 16, r->stream));
  if (r->desc.flags & MRT_FLAG_MOMENTS) {
    HIP_TRY(sized(r->moments, (size_t)W * H * 16));
    HIP_TRY(hipMemsetAsync(r->moments.p, 0, (size_t)W * H * 16, r->stream));
  }
  r->image_foreign = false;
  r->frame_index = 0;
  r->stats = mrt_stats{};
  r->noise_base = r->noise->counters();
  r->stats.owned_pixels = r->owned_pixels;
  r->stats.kernel = (uint32_t)r->plan.kind;
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
  HIP_TRY(d.host.reserve(counter_bytes, hipHostMallocMapped));
  while (d.kernel_events.size() < timed_events) {
    Event e;
    HIP_TRY(e.create(0));
    d.kernel_events.push_back(std::move(e));
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
  uint32_t* meta = seg + 4 * (size_t)r->plan.grid;
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
  a.tile_list = src.list;
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
  a.in_segments = 2 * r->plan.grid;   // two material classes per block
  a.in_seg_count = seg + (size_t)((b + 1) & 1) * 2 * r->plan.grid;
  a.in_chunk = meta + ((b + 1) & 1);
  a.out_seg_count = seg + (size_t)(b & 1) * 2 * r->plan.grid;
  a.out_chunk = meta + (b & 1);
  a.out_total = cnt + d.layout.total(k, b);
  a.grab = cnt + d.layout.grab(k, b);
  for (int p = 0; p < mrt::kQueuePlanes; ++p) {
    a.in_q.plane[p] = fs.queue[b & 1][p].as<float4>();
    a.out_q.plane[p] = fs.queue[(b + 1) & 1][p].as<float4>();
  }
  a.noise_window = bt.noise->dev.as<const float4>();
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
  acc.tile_list = src.list;
  if (fold) {
    acc.counters = d.counters.as<uint32_t>();
    acc.host_counters = static_cast<uint32_t*>(d.host.device());
    acc.copy_words = d.layout.batches * d.layout.L;
    acc.span_word = (uint32_t)(d.layout.span_off / 4);
    acc.span_words = d.layout.batches * 4;
    acc.zero_words = (uint32_t)(d.counters.bytes / 4);
  }
  return acc;
}

}  // namespace

// what renderer_post.cpp uses too (host_internal.h)
namespace mrt {
namespace host {

// read back every pending draw, oldest first
int finalize_pending(mrt_renderer* r) {
  for (int i = 0; i < kDrawRing; ++i) {
    const int rc = finalize_draw(r, r->draws[(r->draw_next + i) % kDrawRing]);
    if (rc) return rc;
  }
  return MRT_OK;
}

// Every mrt_renderer_read_*: the argument checks, the entry point's own answer
// to a plane that is not current, the wait for the renderer's work, the copy
// (host_internal.h ReadSpec; `spec` is asked once r is known not to be null)
int read_back(mrt_renderer* r, void* out, size_t count, ReadSpec (*spec)(const mrt_renderer*), void* out2) {
  if (!r || !out) return fail(MRT_ERR_INVALID, "null argument");
  const ReadSpec s = spec(r);
  if (count < s.need) return fail(MRT_ERR_INVALID, "output buffer too small");
  if (!s.current) return fail(MRT_ERR_STATE, s.stale);
  int rc = s.flush ? exchange_flush(r) : MRT_OK;
  if (rc) return rc;
  rc = mrt_renderer_sync(r);
  if (rc) return rc;
  HIP_TRY(hipMemcpy(out, s.src, s.need * 4, hipMemcpyDeviceToHost));
  if (out2) HIP_TRY(hipMemcpy(out2, s.src2, s.need2 * 4, hipMemcpyDeviceToHost));
  return MRT_OK;
}

// every mrt_renderer_save_*: what `read` returns, to `path`
int save_read(mrt_renderer* r, const char* path, int (*read)(mrt_renderer*, float*, size_t)) {
  if (!r || !path) return fail(MRT_ERR_INVALID, "null argument");
  const uint32_t W = r->desc.width, H = r->desc.height;
  std::vector<float> img((size_t)W * H * 4);
  const int rc = read(r, img.data(), img.size());
  if (rc) return rc;
  std::string err;
  bool io = false;
  return mrt::save_rgba(path, img, W, H, err, io) ? MRT_OK : fail(io ? MRT_ERR_IO : MRT_ERR_INVALID, err);
}

// mrt_renderer_set_camera / _move_camera: `cam` (checked) in force — its lists
// built and uploaded first, so a camera that cannot be installed leaves the
// renderer as it was: the previous camera in force, nothing reset
int swap_camera(mrt_renderer* r, const mrt_camera& cam) {
  const mrt_camera old = r->camera;
  const bool old_moved = r->camera_moved;
  r->camera = cam;
  r->camera_moved = !camera_is_default(cam);
  const int rc = install_camera(r, false);
  if (rc) {
    r->camera = old;
    r->camera_moved = old_moved;
    return rc;
  }
  r->guides_current = false;   // the guide planes were traced with the previous camera
  return MRT_OK;
}

// mrt_renderer_set_scene / _move_scene: mrt_renderer_resize to the same size
// with `scene` in the old one's place.  Behind the wait for the renderer's work
// the kernel is planned again for the new scene (kind, stack variant and grid
// may all change); a scene it cannot be planned for leaves the renderer as it
// was.  Then, with `cam` (checked) as the camera unless null, everything sized by
// the scene is re-made: frame queues, stack spill, the camera's candidate lists
int swap_scene(mrt_renderer* r, const mrt_scene* scene, const mrt_camera* cam) {
  HIP_TRY(hipSetDevice(r->scene->device));
  int rc = finalize_pending(r);
  if (rc) return rc;
  HIP_TRY(hipStreamSynchronize(r->stream));
  const mrt_scene* old = r->scene;
  const mrt::KernelPlan old_plan = r->plan;
  r->scene = scene;
  rc = plan_kernel(r);
  // as resize: a pending gather holds the old scene's pixels and is never unpacked
  // into the new image; dropped only once the new scene's kernel is planned
  if (!rc) rc = exchange_drop(r, true);
  if (rc) {
    r->scene = old;
    r->plan = old_plan;
    return rc;
  }
  r->desc.scene = scene;
  if (cam) {
    r->camera = *cam;
    r->camera_moved = !camera_is_default(*cam);
  }
  rc = post_set_scene(r);   // everything derived from the image: stale
  return rc ? rc : alloc_frame_buffers(r);
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
  const uint32_t launches_per_batch = mrt::launches_per_batch(r->plan.kind, r->desc.max_path_length);
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
    HIP_TRY(d.list_host.reserve((size_t)T * 4, hipHostMallocDefault));
    if (src.host_list) {
      std::memcpy(d.list_host.host(), src.host_list, (size_t)src.tiles * 4);
      HIP_TRY(hipMemcpyAsync(src.list, d.list_host.host(), (size_t)src.tiles * 4, hipMemcpyHostToDevice, r->stream));
    } else {
      HIP_TRY(hipMemcpyAsync(d.list_host.host(), src.list, (size_t)src.tiles * 4, hipMemcpyDeviceToHost, r->stream));
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
      HIP_TRY(MRT_BUILD_CALL(r->desc.flags, launch_kernel(r->plan.kind, r->scene->dev, a, r->plan.stack_entries,
                                                          r->plan.grid, fs.stream)));
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
    HIP_TRY(hipMemcpyAsync(d.host.host(), d.counters.p, d.layout.bytes, hipMemcpyDeviceToHost, r->stream));
  HIP_TRY(hipEventRecord(d.copied, r->stream));
  d.pending = true;
  d.frames = n;
  d.pixels = src.tiles ? 0 : r->owned_pixels;
  d.listed = src.tiles;
  d.events = ev;
  r->draw_next = (r->draw_next + 1) % kDrawRing;
  return MRT_OK;
}

}  // namespace host
}  // namespace mrt

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
  // (a failure from here on leaves through ~mrt_renderer: nothing made so far leaks)
  if (desc->stream)
    r->stream.borrow((hipStream_t)desc->stream);
  else
    HIP_TRY(r->stream.create());
  r->image = desc->image;   // (null: alloc_frame_buffers makes image_buf)
  r->noise = std::make_unique<mrt::NoiseSchedule>(desc->seed, (desc->flags & MRT_FLAG_STATIC_NOISE) != 0);
  for (DrawRecord& d : r->draws) {
    HIP_TRY(d.start.create(0));
    HIP_TRY(d.stop.create(0));
    HIP_TRY(d.cleared.create(hipEventDisableTiming));
    HIP_TRY(d.copied.create(hipEventDisableTiming));
  }
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
    if (r->inflight == 1)   // one slot: everything in order on the main stream
      fs.stream.borrow(r->stream);
    else
      HIP_TRY(fs.stream.create());
    HIP_TRY(fs.acc_done.create(hipEventDisableTiming));
    HIP_TRY(fs.kernel_done.create(hipEventDisableTiming));
  }
  if (const char* v = mrt::diag_env("MRT_PRIMARY")) r->primary_allowed = std::atoi(v) != 0;
  if (const char* v = mrt::diag_env("MRT_PRIMARY_CAP"))
    r->primary_cap = std::max<uint32_t>(1, std::min<uint32_t>(mrt::kPrimaryFallback - 1, (uint32_t)std::strtoul(v, nullptr, 0)));
  {
    const int rc = plan_kernel(r.get());
    if (rc) return rc;
  }
  // the noise schedule's upload stream, staging buffers and worker on the
  // renderer's device.  Created after the render streams: a process has 4
  // hardware queues and streams share them round-robin in creation order, so
  // a stream created before the render streams pushed a render stream onto a
  // queue another stream's work serialises with (C2 -10 %, C4 -7 %, measured r6).
  // So the order of creation is fixed, whatever type holds a stream: the main
  // stream, the slots' streams, this one, then refine_noise's at the first refine
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
  if (r->desc.image) return fail(MRT_ERR_STATE, "cannot resize an externally owned image");
  int rc = finalize_pending(r);
  if (rc) return rc;
  rc = exchange_drop(r, true);   // a pending gather was packed for the old size: never unpack it into the new image
  if (rc) return rc;
  HIP_TRY(hipStreamSynchronize(r->stream));
  r->desc.width = width;
  r->desc.height = height;
  r->x.slab_floats = 0;    // the exchange buffers are re-sized for the new image at the next exchange
  rc = post_resize(r);     // everything derived from the image: stale, its buffers re-made at the new size
  return rc ? rc : alloc_frame_buffers(r);
}

int mrt_renderer_set_scene(mrt_renderer* r, const mrt_scene* scene) {
  if (!r || !scene) return fail(MRT_ERR_INVALID, "mrt_renderer_set_scene: null argument");
  if (scene->device != r->scene->device)
    return fail(MRT_ERR_INVALID, scene->device < 0 ? "mrt_renderer_set_scene: a host-only scene has nothing on a device"
                                                   : "mrt_renderer_set_scene: the scene is on another device than the renderer");
  return swap_scene(r, scene, nullptr);
}

int mrt_renderer_reset(mrt_renderer* r) {
  if (!r) return fail(MRT_ERR_INVALID, "null renderer");
  int rc = exchange_drop(r, false);   // the pre-reset frame's deferred tiles must not land in the cleared image
  if (rc) return rc;
  // The next frame (f = 0) overwrites every pixel this renderer owns, and
  // pixels it does not own stay 0 — unless an exchange wrote other ranks'
  // tiles into the image: only then is it cleared (stream-ordered after
  // the pending draws).  An external image is always cleared.
  if (r->image_foreign || r->desc.image) {
    HIP_TRY(hipMemsetAsync(r->image, 0, (size_t)r->desc.width * r->desc.height * 16, r->stream));
    r->image_foreign = false;
  }
  rc = post_reset(r);   // samples beside the image go with its frames (stream-ordered, as above)
  if (rc) return rc;
  r->frame_index = 0;
  r->stats.frame_index = 0;   // cumulative counters (paths, A, kernel time) persist
  r->history_valid = false;   // (mrt_renderer_move_camera sets it again once it has reprojected)
  return MRT_OK;
}

int mrt_renderer_set_camera(mrt_renderer* r, const mrt_camera* cam) {
  if (!r) return fail(MRT_ERR_INVALID, "null renderer");
  int rc = mrt_camera_check(cam);
  if (rc) return rc;
  rc = swap_camera(r, *cam);
  return rc ? rc : mrt_renderer_reset(r);
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
  return read_back(r, rgba, count, [](const mrt_renderer* r) {   // (flush: a deferred, overlapped exchange lands first)
    return ReadSpec{(size_t)r->desc.width * r->desc.height * 4, r->image, true, nullptr, nullptr, 0, /*flush*/ true};
  });
}

int mrt_renderer_save_image(mrt_renderer* r, const char* path) { return save_read(r, path, mrt_renderer_read_image); }

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
  delete r;
  return MRT_OK;
}

}  // extern "C"

// Waits first, then the members (host_internal.h).  Also what a failed
// mrt_renderer_create leaves through, on a renderer built by half: no draw
// pending, no collective, perhaps no stream yet.
mrt_renderer::~mrt_renderer() {
  (void)exchange_wait(this);   // bounded: a failed communicator is aborted, not waited for
  (void)finalize_pending(this);
  if (stream) (void)hipStreamSynchronize(stream);
  for (int i = 0; i < 2; ++i)   // an overlapped gather may still read the packed tiles
    if (x.gather_recorded[i]) (void)hipEventSynchronize(x.gather_done[i]);
  refine_noise.reset();
  noise.reset();   // joins the worker; the draws reading its chunks have finished (stream synchronised above)
}
