// host_internal.h — what the host units behind include/mrt.h share: the error
// and HIP helpers, the one precise/fast dispatch, the objects of the C ABI
// (mrt_scene, mrt_accel, mrt_renderer, mrt_comm) and the few functions that
// cross units.  The units: scene_api.cpp (scene, accel), stage_api.cpp (the
// stage-level ABI and the standalone image entry points), renderer.cpp (the
// renderer, its cameras and its draw loop), renderer_post.cpp (the images a
// renderer derives from what it accumulated: denoised, resolved, history,
// variance, clamped, extras, tile planes, display), exchange.cpp (RCCL
// communicator, tile exchange).
// Everything shared lives in mrt::host; the units use that namespace.
#pragma once
#include <hip/hip_runtime.h>
#include <rccl/rccl.h>

#include <algorithm>
#include <cstdint>
#include <cstring>
#include <memory>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/mrt.h"
#include "bvh.h"
#include "hip_handles.h"
#include "kernels.h"
#include "noise_schedule.h"
#include "scene.h"

namespace mrt {
namespace host {

// records the calling thread's message for mrt_last_error (stage_api.cpp: the
// one definition, beside the one string it writes) and returns `code`
int fail(int code, const std::string& msg);

#define HIP_TRY(expr)                                                                             \
  do {                                                                                            \
    hipError_t e_ = (expr);                                                                       \
    if (e_ != hipSuccess)                                                                         \
      return mrt::host::fail(MRT_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(e_));     \
  } while (0)

// the one precise/fast dispatch: `call` in the build of kernels.hip that
// MRT_FLAG_PRECISE in `flags` selects (only that build's call is evaluated)
#define MRT_BUILD_CALL(flags, call) (((flags) & MRT_FLAG_PRECISE) ? mrt::precise::call : mrt::fast::call)

inline float bitsf(uint32_t u) { float f; std::memcpy(&f, &u, 4); return f; }
inline uint32_t fbits(float f) { uint32_t u; std::memcpy(&u, &f, 4); return u; }

// traversal-stack spill of the stage intersect and guide kernels (trees deeper
// than their kMaxStack-entry LDS stack): one row of max_stack words per lane of
// their persistent grid — the row stride the kernels address it with
// (dev_lds.h LdsCtx::spill_lane; a lane uses the first max_stack - 32 words)
inline hipError_t alloc_isect_spill(DevBuf& b, uint32_t max_stack) {
  if (max_stack <= (uint32_t)mrt::kMaxStack) return b.alloc(0);
  return b.alloc((size_t)max_stack * mrt::kIntersectSpillGrid * 256 * 4);
}

#define NCCL_TRY(expr)                                                                            \
  do {                                                                                            \
    ncclResult_t e_ = (expr);                                                                     \
    if (e_ != ncclSuccess)                                                                        \
      return mrt::host::fail(MRT_ERR_HIP, std::string(#expr) + ": " + ncclGetErrorString(e_));    \
  } while (0)

inline hipError_t upload(DevBuf& b, const void* src, size_t n) {
  hipError_t e = b.alloc(std::max<size_t>(n, 16));
  if (e != hipSuccess) return e;
  return n ? hipMemcpy(b.p, src, n, hipMemcpyHostToDevice) : hipSuccess;
}

// Layout of a draw's counter buffer, for `batches` frame batches of L bounces:
// the survivor totals [batches * L] and, 128-B aligned after them, the grab
// counters of every launch of the draw (zeroed by ONE memset), then the
// batches' [2] u64 spans.  draw_n addresses the buffer with it and
// finalize_draw reads the pinned copy back with it.
struct CounterLayout {
  static constexpr size_t kGrabWords = (size_t)mrt::kGrabRanges * mrt::kGrabStride;   // per launch
  uint32_t batches = 0, L = 0;
  size_t grab_off = 0;   // words
  size_t span_off = 0;   // bytes, 8-B aligned
  size_t bytes = 0;      // of the buffer this draw uses
  CounterLayout() = default;
  CounterLayout(uint32_t nb, uint32_t l) : batches(nb), L(l) {
    grab_off = ((size_t)nb * L + 31) / 32 * 32;
    span_off = (grab_off + (size_t)nb * L * kGrabWords + 1) / 2 * 8;
    bytes = span_off + (size_t)nb * 16;
  }
  size_t total(uint32_t k, uint32_t b) const { return (size_t)k * L + b; }   // word of batch k's bounce b
  size_t grab(uint32_t k, uint32_t b) const { return grab_off + total(k, b) * kGrabWords; }   // word
  size_t span(uint32_t k) const { return span_off + (size_t)k * 16; }   // byte
};

// bookkeeping of one draw_n call whose statistics are not read back yet
struct DrawRecord {
  DevBuf counters;                          // per (batch, bounce) survivor totals, then the launches' grab
                                            // counters (one buffer: one memset per draw)
  Event start, stop;
  Event cleared;                            // the counters' memset (other render streams of the draw wait on it)
  Event copied;                             // the counters' copy to `host` (read-back stream) is done
  PinnedBuf host;                           // pinned (device-mapped) copy of `counters`, written behind the draw
  std::vector<Event> kernel_events;         // MRT_FLAG_PROFILE: 2 per timed bounce launch
  uint32_t frames = 0;
  CounterLayout layout;                     // of `counters` as this draw uses it (bounce launches = batches * L)
  size_t events = 0;
  bool pending = false;
  // the counters are all zero once this entry's last draw enqueued its
  // folding accumulate (which zeroes them behind the draw); a draw that
  // returned early after its first launch leaves them dirty
  bool clean = false;
  // what the draw rendered per frame: the renderer's owned pixels, or (a refine
  // draw: listed > 0) the tiles of list_host — the pinned staging a draw_tiles
  // list is uploaded from and a refine's device-chosen list is copied back to,
  // behind the draw; its pixels are counted when the draw is read back
  uint64_t pixels = 0;
  uint32_t listed = 0;
  PinnedBuf list_host;                      // (one entry per tile of the frame)
};
constexpr int kDrawRing = 3;

// What a draw renders and where it goes (renderer.cpp draw_frames): the frames
// [f0, f0 + n) of a noise schedule, over the renderer's owned tiles into the
// accumulation image (mrt_renderer_draw_n) or over a tile list into the counted
// extra images (mrt_renderer_draw_tiles / _refine)
struct DrawSource {
  mrt::NoiseSchedule* noise = nullptr;
  uint64_t f0 = 0;
  uint32_t tiles = 0;                       // listed tiles; 0 = the owned tiles
  uint32_t* list = nullptr;                 // listed: the device list (null otherwise)
  const uint32_t* host_list = nullptr;      // listed: to upload (null: the device list is already chosen)
  float* image = nullptr;                   // accumulation image, or E
  float* moments = nullptr;                 // moments image (may be null), or EM
};

// What a reader copies to the host once the renderer is idle (read_back): `need`
// 4-B elements from `src` into the caller's buffer and, where the reader has a
// second output, need2 from src2.  stale: the entry point's own message while
// the plane is not `current` (computed at the renderer's current size)
struct ReadSpec {
  size_t need = 0;
  const void* src = nullptr;
  bool current = true;
  const char* stale = nullptr;
  const void* src2 = nullptr;
  size_t need2 = 0;
  bool flush = false;                       // a deferred exchange lands first (the image)
};

// One in-flight frame: its queues, segment counts, per-pixel path radiance and
// the stream its render launches run on.  Batches b and b+1 run on different
// slots concurrently (the reference keeps up to 3 frames in flight,
// renderer/Renderer.mm:16,593-600); their accumulations run in order on the
// main stream because the running mean is order-dependent.
struct FrameSlot {
  Stream stream;            // its own, or (one slot) the main stream, borrowed
  DevBuf queue[2][mrt::kQueuePlanes];   // ray queues (the streaming wavefront: queue[0] holds the per-wave queues)
  DevBuf segments;          // 2 queues x 2 classes x grid per-block survivor counts + 2 chunk words
  DevBuf radiance;          // W*H float4, written once per owned pixel per frame
  DevBuf spill;             // traversal stack entries beyond the LDS capacity (deep BVHs)
  Event acc_done;           // on the main stream: the accumulate that last read `radiance`
  Event kernel_done;        // on `stream`: its last render launch
  bool acc_recorded = false;
};

// One camera's device data: the CameraBlock the kernels' camera_ray reads and,
// behind it, the camera-ray candidate lists built for that camera.  A draw
// launches with pointers into the generation in force when it is enqueued;
// mrt_renderer_set_camera fills another generation (pinned staging, one
// asynchronous copy on the next batch's render stream) instead of touching
// one that launches in flight may read, and a replaced generation is recycled
// once `retired` — recorded on the main stream, behind the accumulates that
// follow every render launch of the earlier draws — has completed.
struct CameraGen {
  DevBuf dev;                     // [CameraBlock, 64 B][candidate-list words]
  PinnedBuf host;                 // pinned staging of the same bytes
  Event ready;                    // the upload, on the render stream that carried it
  Event retired;
  bool busy = false;              // replaced, `retired` not yet seen complete
  bool async = false;             // uploaded asynchronously (`ready` is recorded)
  uint32_t waited_streams = 0;    // render streams (slots) ordered behind `ready`
  bool moved = false;             // not the reference's camera: launches get the block's address
  bool has_lists = false;
  uint32_t primary_bx = 0;
};
constexpr size_t kCameraGens = 5;   // the one in force + four replaced ones whose draws may still execute

// Failure state of one RCCL communicator, shared by the communicator and the
// renderers that enqueued collectives on it (a renderer may outlive it: a
// deferred unpack after mrt_comm_destroy).  A collective that reports an
// asynchronous error (ncclCommGetAsyncError) or does not complete within the
// timeout aborts the communicator (ncclCommAbort: its pending kernels exit);
// every later use of it fails with MRT_ERR_COMM.  The reference has no
// collective (one Metal device, renderer/Renderer.mm:595) and ignores its
// command-buffer errors (:131,141,145); this is the exchange's own contract.
struct CommHealth {
  std::mutex m;
  ncclComm_t comm = nullptr;   // null once destroyed or aborted
  bool aborted = false;
  std::string error;           // why it was aborted
  double timeout_ms = 120000.0;
  uint32_t inject = 0;         // test entry mrt_debug_comm_fail: 1 async error, 2 collectives never complete
};

// Image exchange state of a renderer (mrt_renderer_exchange): the packed
// owned tiles, double-buffered so an overlapped gather of step k can still be
// reading buffer k % 2 while step k + 1 packs into the other, and on rank 0
// the gathered slabs of every rank.
struct Exchange {
  DevBuf packed[2], gathered, staging;
  Event pack_done[2], gather_done[2];
  bool gather_recorded[2] = {false, false};
  uint64_t slab_floats = 0;   // packed floats per rank (rank 0 owns the most tiles)
  int pending = -1;           // buffer whose gather awaits rank 0's unpack (overlap mode)
  uint32_t next = 0;
  const mrt_comm* comm = nullptr;
  // the communicator's shape, copied at each exchange: a deferred unpack
  // never dereferences `comm` (it may be destroyed before the flush)
  uint32_t rank = 0, nranks = 1;
  uint32_t width = 0, height = 0;   // image size the pending gather was packed at
  // the last collective enqueued (on whichever stream it ran) and the health
  // of its communicator: mrt_renderer_sync / _exchange_flush wait for it with
  // a bound instead of blocking on a stream a stuck peer never releases
  Event coll_done;
  bool coll_pending = false;
  std::shared_ptr<CommHealth> health;
};

}  // namespace host
}  // namespace mrt

// MPS-shaped acceleration structure over caller-owned device buffers
struct mrt_accel {
  mrt_accel_desc desc{};
  mrt::host::DevBuf nodes, tris;
  mrt::host::DevBuf isect_spill;       // stage intersect stack spill for trees deeper than kMaxStack
  mrt::DeviceScene dev{};
  mrt_accel_info info{};
};

struct mrt_scene {
  int device = 0;
  mrt::host::DevBuf isect_spill;       // stage intersect stack spill for trees deeper than kMaxStack
  mrt::HostScene host;
  // what motion compatibility compares, folded when the scene is flattened: the
  // material index and light status of every primitive, in order (FNV-1a, 64
  // bits), so that a per-pose call compares two words instead of two arrays
  uint64_t motion_digest = 0;
  mrt::BvhResult bvh;
  // the shadow-ray occluder tree (occluders.h) as uploaded after the main
  // tree: node refs rebased by bvh.num_nodes, leaf records by the triangle
  // count, leaf primitive ids = scene primitives (host copy for check_bvh)
  std::vector<float> occ_nodes, occ_tris;
  std::vector<uint32_t> occ_keep;   // primitives the occluder tree holds
  int32_t occ_root = 0;
  uint32_t occ_node_base = 0, occ_max_stack = 0;
  mrt::host::DevBuf nodes, tris, prims, materials, lights;
  // leaf-box sweep (mrt_layout.h DeviceScene::sweep): the main tree's leaf
  // records, 8 floats each (empty for a tree over kSweepLeaves leaves or a
  // leaf root), and whether nearest queries use them
  // sweep_pairs: the list the kernels get, derived from it (sweep_pairs.h:
  // one record per group of at most two triangles)
  // sweep_phase1: phase 1's centre / half-extent record of each of them
  // (sweep_pairs.h sweep_phase1_records), for a scene that sweeps
  std::vector<float> sweep_list, sweep_pairs, sweep_phase1;
  bool sweep_on = false;
  uint32_t sweep_cap = mrt::kSweepCap;   // DeviceScene::sweep_cap
  mrt::host::DevBuf sweep;
  mrt::DeviceScene dev{};
  mrt_scene_info info{};
};

// RCCL communicator of one rank (one process per GPU) and the stream its
// overlapped collectives run on
struct mrt_comm {
  ncclComm_t comm = nullptr;
  uint32_t nranks = 0, rank = 0;
  int device = 0;
  mrt::host::Stream stream;
  std::shared_ptr<mrt::host::CommHealth> health = std::make_shared<mrt::host::CommHealth>();
  // the health handshake, the wait for the stream's collectives and
  // ncclCommDestroy; then the members (exchange.cpp)
  ~mrt_comm();
};

struct mrt_renderer {
  // Destruction (renderer.cpp): first the waits for everything this renderer
  // enqueued, then the two noise schedules (which joins their workers), then
  // the members, last declared first.  After the waits no order among the
  // members matters to the device; they are declared so that the main stream,
  // first here, goes last, and the slots' streams after the noise schedules'.
  ~mrt_renderer();
  mrt::host::Stream stream;       // main stream (the caller's, borrowed, or its own); slot 0 runs on it
  const mrt_scene* scene = nullptr;
  mrt_renderer_desc desc{};
  float* image = nullptr;         // the accumulation image in use: the caller's (desc.image) or image_buf
  mrt::host::DevBuf image_buf;    // the image where the caller gave none (re-made by resize)
  uint32_t tiles_x = 0, tiles_y = 0, owned_tiles = 0;
  uint64_t owned_pixels = 0;
  std::vector<mrt::host::FrameSlot> slots;
  uint32_t max_frames = 0;   // MAX_FRAMES (0 = unlimited)
  // Frame batches in flight (MRT_INFLIGHT; default 1 for a whole frame, 2 for a
  // tile share).  With k >= 2 every slot renders on its own stream and the
  // accumulates run on the main stream, so batch b + 1 (of this draw or the
  // next) only waits for the accumulate that last read its slot's radiance:
  // its persistent blocks take the CUs as batch b's drain (~0.2 ms per
  // launch, whatever its length) frees them.  One GPU's 1/8 tile share of C2
  // launches 2.1-ms kernels, where that drain is 10 %.
  uint32_t inflight = 1;
  uint32_t slot_next = 0;   // slot of the next batch (rotates across draws)
  double wall_khz = 0.0;    // device wall clock (span timestamps; 0 = spans off, MRT_SPANS=0)
  bool image_foreign = false;   // the image holds pixels this renderer did not render (exchange / tiles_write)
  // the persistent kernel this renderer launches, its LDS stack and its grid
  // (kernel_plan.h; filled by renderer.cpp plan_kernel at create and again by a scene swap)
  mrt::KernelPlan plan;
  // noise tables in device chunks of 64 frames, generated ahead on a worker
  // thread and uploaded on their own stream (noise_schedule.h)
  std::unique_ptr<mrt::NoiseSchedule> noise;
  mrt::NoiseSchedule::Counters noise_base;   // the schedule's counters at the last stats reset
  uint64_t draw_seq = 0;     // draws enqueued (pins the noise chunks a draw reads)
  uint64_t frame_index = 0;
  // Draws in flight: each draw records its survivor counters and events in
  // its own ring entry, and its statistics are read back lazily (when the
  // entry is reused, or on stats / sync / read), so consecutive draws queue
  // back to back without a host round trip between them.
  mrt::host::DrawRecord draws[mrt::host::kDrawRing];
  uint32_t draw_next = 0;   // ring entry of the next draw (= the oldest pending one)
  uint32_t profile_every = 8;   // time the launches of every n-th batch (MRT_PROFILE_EVERY)
  uint32_t batch = 1;           // frames per bounce launch (frame batching)
  bool counter_fold = true;     // draw statistics copied + cleared by the last accumulate (MRT_COUNTER_FOLD)
  mrt_stats stats{};
  uint32_t debug = 0;   // MRT_DEBUG ablation bits (profiling only)
  // camera-ray candidate lists per 8x8 pixel block (primary.h), rebuilt for
  // every frame size; bounce 0 of the wavefront kernels (a wave = one block)
  // tests the block's list instead of traversing: C2 +4.6 % (alternating
  // A/B).  The path kernel refills lanes one by one, so its lists would be
  // per-lane dependent global loads at refill: C3 -4.8 %, not used there.
  // MRT_PRIMARY=0: off; MRT_PRIMARY_CAP: longest list (12)
  // The lists belong to a camera: they live in the camera's generation
  // (CameraGen), rebuilt by mrt_renderer_set_camera; none with a thin lens.
  bool primary_allowed = true;
  uint32_t primary_cap = 12;
  mrt_camera camera{};          // the camera in force (mrt_camera_default until set_camera)
  bool camera_moved = false;    // `camera` is not bitwise the default: the kernels read its block
  std::vector<std::unique_ptr<mrt::host::CameraGen>> cams;
  mrt::host::CameraGen* cam_cur = nullptr;
  mrt::host::Exchange x;
  mrt::host::DevBuf reference, display;   // comparison image (mrt_renderer_load_reference) and blit output
  // denoised output (mrt_renderer_denoise): allocated at the first denoise,
  // re-made by resize.  The guide planes belong to a size and a camera.
  mrt::host::DevBuf guide_n, guide_p, denoised, denoise_scratch;
  mrt::host::DevBuf guide_spill;              // the guide pass's own traversal-stack spill (deep trees; first denoise)
  bool guides_current = false;     // the planes hold the camera in force at the current size
  bool denoised_current = false;   // a denoise has run at the current size
  // temporal history (mrt_renderer_move_camera): allocated at the first move
  // (resolved: at the first resolve), re-made by resize.  The history is a
  // counted image beside the accumulation image, in the view of `camera`.
  mrt::host::DevBuf prev_guide_n, prev_guide_p, temporal_prev, history, resolved;
  bool history_valid = false;      // `history` holds the reprojection into the camera in force
  // moving geometry (mrt_renderer_move_scene): where each pixel's surface point
  // was in the previous scene (mrt_guides_motion), 32 B per pixel; allocated at
  // the first move_scene, re-made by resize
  mrt::host::DevBuf motion_n, motion_p;
  bool resolved_current = false;   // a resolve has run at the current size
  // variance-guided denoising (MRT_FLAG_MOMENTS): the moments image lives with
  // the image (create, resize); its scratch and history are allocated at the
  // first move, the resolved moments and the variance plane at the first
  // mrt_renderer_denoise_variance; all re-made by resize.  The moments
  // history's validity is history_valid.
  mrt::host::DevBuf moments, moments_prev, moments_history, moments_resolved, variance;
  bool variance_current = false;   // a denoise_variance has run at the current size
  // firefly suppression (mrt_renderer_set_firefly): while it is on,
  // denoise_variance filters the clamped copy of the resolved buffer — 16 B per
  // pixel and, behind them, the counter of changed pixels; made at the first
  // clamp, re-made by resize.  The setting survives reset, resize and moves.
  bool firefly_on = false;
  mrt_firefly_params firefly{2, 3.0f, 3, 0.9f, 0.01f};   // mrt_firefly_params_default
  mrt::host::DevBuf clamped;
  bool clamped_current = false;    // a clamp has run at the current size
  // adaptive sampling (mrt_renderer_refine / _draw_tiles): everything is made at
  // the first call and re-made by resize.  E and EM are counted images beside
  // the image and the moments; the second noise schedule (seed ^
  // MRT_REFINE_SEED_XOR) and the extra-frame counter are never reset.
  mrt::host::DevBuf extra, extra_moments, tile_list, tile_priority;
  std::unique_ptr<mrt::NoiseSchedule> refine_noise;
  mrt::host::Event list_ready;     // on the main stream: the list's upload or selection (render streams wait on it)
  bool extras_current = false;     // E / EM exist at the current size (zero unless extras_valid)
  bool extras_valid = false;       // E holds samples: resolves merge it
  bool priority_current = false;   // a refine has run at the current size
  uint32_t list_count = 0;         // entries of tile_list the last refine / draw_tiles drew
  mrt_refine_stats refine_stats{};
  // sampling to a target error (mrt_renderer_error / _converge): the two
  // per-tile planes of mrt_tile_error, the device summary and its pinned host
  // copy; made at the first estimate, the planes re-made by resize
  mrt::host::DevBuf tile_error, tile_pixels, error_summary;
  mrt::host::PinnedBuf summary_host;
  bool tile_error_current = false;   // an estimate has run at the current size
  struct DisplaySlot {          // mrt_renderer_display_enqueue / _map: pinned copies of the blit
    mrt::host::PinnedBuf host;
    size_t floats = 0;          // of the frame it was last enqueued for
    mrt::host::Event done;
    bool queued = false;
  } shown[MRT_DISPLAY_SLOTS];
};

// the functions that cross units
namespace mrt {
namespace host {

// stage_api.cpp (camera, guides)
mrt::CameraBlock camera_block(const mrt_camera& c);
bool camera_is_default(const mrt_camera& c);
int guides_with_spill(const mrt_scene* scene, const mrt_camera* cam, uint32_t W, uint32_t H, float* guide_n,
                      float* guide_p, uint32_t flags, uint32_t* spill, void* stream);
int guides_motion_with_spill(const mrt_scene* scene, const mrt_scene* prev_scene, const mrt_camera* cam, uint32_t W,
                             uint32_t H, float* guide_n, float* guide_p, float* motion_n, float* motion_p,
                             uint32_t flags, uint32_t* spill, void* stream);

// renderer.cpp: the draw loop and its statistics; `cam` put in force, or the
// renderer left as it was; `scene` (and `cam`, unless null) put in force at
// frame 0 behind a wait for the renderer's work, or the renderer left as it
// was; a reader's checks, wait and copy; an image to a file
int draw_frames(mrt_renderer* r, uint32_t n, const DrawSource& src);
int finalize_pending(mrt_renderer* r);
int swap_camera(mrt_renderer* r, const mrt_camera& cam);
int swap_scene(mrt_renderer* r, const mrt_scene* scene, const mrt_camera* cam);
int read_back(mrt_renderer* r, void* out, size_t count, ReadSpec (*spec)(const mrt_renderer*), void* out2 = nullptr);
int save_read(mrt_renderer* r, const char* path, int (*read)(mrt_renderer*, float*, size_t));

// renderer_post.cpp: what resize, reset and a scene swap do about the derived images
int post_resize(mrt_renderer* r);
int post_reset(mrt_renderer* r);
int post_set_scene(mrt_renderer* r);

// exchange.cpp: what the renderer's resize / reset, sync / destroy and image
// readers do about its pending collective and deferred unpack
int exchange_drop(mrt_renderer* r, bool wait);
int exchange_wait(mrt_renderer* r);
int exchange_flush(mrt_renderer* r);

}  // namespace host
}  // namespace mrt
