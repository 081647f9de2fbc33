// exchange.cpp — the RCCL communicator (mrt_comm_*) and a renderer's image
// exchange: gather or reduce of the owned tiles to rank 0, overlapped with the
// next draw or not, with bounded waits and abort on failure (CommHealth).
#include <chrono>
#include <thread>

#include "host_internal.h"

using namespace mrt::host;

namespace {

int exchange_buffers(mrt_renderer* r, const mrt_comm* c) {
  Exchange& x = r->x;
  uint64_t floats = 0;
  if (mrt_tiles_packed_floats(r->desc.width, r->desc.height, 0, c->nranks, &floats)) return MRT_ERR_INVALID;
  if (x.slab_floats == floats && x.packed[0].p) return MRT_OK;
  HIP_TRY(hipStreamSynchronize(r->stream));
  x.slab_floats = floats;
  for (int i = 0; i < 2; ++i) {
    HIP_TRY(x.packed[i].alloc(floats * 4));
    HIP_TRY(hipMemsetAsync(x.packed[i].p, 0, floats * 4, r->stream));   // ranks with fewer tiles send zero padding
    HIP_TRY(x.pack_done[i].ensure(hipEventDisableTiming));
    HIP_TRY(x.gather_done[i].ensure(hipEventDisableTiming));
    x.gather_recorded[i] = false;
  }
  if (c->rank == 0) HIP_TRY(x.gathered.alloc(floats * 4 * c->nranks));
  return MRT_OK;
}

// rank 0: unpack every other rank's slab of gather buffer `i` into the image
// (on the renderer's stream, after the gather); other ranks: order the
// renderer's stream after the gather so sync/read see it complete
int exchange_unpack(mrt_renderer* r, int i) {
  Exchange& x = r->x;
  HIP_TRY(hipStreamWaitEvent(r->stream, x.gather_done[i], 0));
  if (x.rank == 0)
    for (uint32_t k = 1; k < x.nranks; ++k)
      HIP_TRY(mrt::fast::launch_tiles_move(x.gathered.as<float4>() + (size_t)k * (x.slab_floats / 4),
                                           reinterpret_cast<float4*>(r->image), x.width, x.height, k,
                                           x.nranks, false, r->stream));
  return MRT_OK;
}

// Abort a communicator (lock held): its pending collectives are cancelled
// and every later use fails.  Returns the MRT_ERR_COMM status.
int comm_abort_locked(CommHealth& h, const std::string& why) {
  if (!h.aborted) {
    if (h.comm) (void)ncclCommAbort(h.comm);
    h.comm = nullptr;
    h.aborted = true;
    h.error = why;
  }
  return fail(MRT_ERR_COMM, "RCCL communicator aborted: " + h.error);
}

// Non-blocking health check of a communicator (lock held).
int comm_check_locked(CommHealth& h) {
  if (h.aborted) return fail(MRT_ERR_COMM, "RCCL communicator aborted: " + h.error);
  if (!h.comm) return MRT_OK;   // destroyed: nothing can fail any more
  ncclResult_t e = ncclSuccess;
  if (h.inject == 1) e = ncclSystemError;
  else if (ncclCommGetAsyncError(h.comm, &e) != ncclSuccess) e = ncclInternalError;
  if (e != ncclSuccess && e != ncclInProgress)
    return comm_abort_locked(h, std::string("asynchronous error: ") + ncclGetErrorString(e));
  return MRT_OK;
}

// The renderer's exchange state after its communicator failed: nothing is
// left to unpack or wait for (the image keeps the renderer's own tiles).
void exchange_forget(mrt_renderer* r) {
  r->x.pending = -1;
  r->x.coll_pending = false;
  r->x.comm = nullptr;
}

}  // namespace

namespace mrt {
namespace host {

// Wait, with the communicator's timeout as the bound, for the renderer's last
// collective to complete on the device; poll its asynchronous error meanwhile.
int exchange_wait(mrt_renderer* r) {
  Exchange& x = r->x;
  if (!x.coll_pending) return MRT_OK;
  std::shared_ptr<CommHealth> h = x.health;
  const auto t0 = std::chrono::steady_clock::now();
  for (uint32_t spin = 0;; ++spin) {
    double timeout_ms;
    {
      std::lock_guard<std::mutex> lk(h->m);
      if (h->inject != 2) {
        const hipError_t q = hipEventQuery(x.coll_done);
        if (q == hipSuccess) { x.coll_pending = false; return MRT_OK; }
        if (q != hipErrorNotReady) {
          exchange_forget(r);
          return fail(MRT_ERR_HIP, std::string("exchange: ") + hipGetErrorString(q));
        }
      }
      if (int rc = comm_check_locked(*h)) { exchange_forget(r); return rc; }
      timeout_ms = h->timeout_ms;
      const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
      if (ms > timeout_ms) {
        const int rc = comm_abort_locked(*h, "collective did not complete within " + std::to_string((long)timeout_ms) +
                                                  " ms (a peer stopped or the link failed)");
        exchange_forget(r);
        return rc;
      }
    }
    std::this_thread::sleep_for(std::chrono::microseconds(spin < 100 ? 20 : 500));
  }
}

// Forget a deferred (overlapped) gather without unpacking it — its tiles
// belong to an image that resize / reset discards.  The gather itself may
// still be writing the receive buffer: `wait` (resize, which may reallocate
// the exchange buffers) waits for it; reset need not (the next gather into
// the same buffer runs after it on the communicator's stream, and nothing
// else reads the buffer), so the overlap of the gather with the next draw
// is kept.
int exchange_drop(mrt_renderer* r, bool wait) {
  Exchange& x = r->x;
  if (x.pending < 0) return MRT_OK;
  x.pending = -1;
  if (wait) return exchange_wait(r);   // (the pending gather is the last collective)
  return MRT_OK;
}

int exchange_flush(mrt_renderer* r) {
  if (r->x.coll_pending && r->x.health) {   // a failed communicator surfaces at the next exchange call
    std::lock_guard<std::mutex> lk(r->x.health->m);
    if (int rc = comm_check_locked(*r->x.health)) { exchange_forget(r); return rc; }
  }
  if (r->x.pending < 0) return MRT_OK;
  const int i = r->x.pending;
  r->x.pending = -1;
  return exchange_unpack(r, i);
}

}  // namespace host
}  // namespace mrt

// Waits first, then the members (the stream): also what a failed
// mrt_comm_create leaves through, with no communicator and perhaps no stream
mrt_comm::~mrt_comm() {
  (void)hipSetDevice(device);
  {
    std::lock_guard<std::mutex> lk(health->m);
    if (health->aborted) comm = nullptr;   // ncclCommAbort already freed it
    health->comm = nullptr;                // renderers holding the health no longer touch it
  }
  if (stream && comm) (void)hipStreamSynchronize(stream);
  if (comm) (void)ncclCommDestroy(comm);
}

extern "C" {

// ---------------------------------------------------------------------------
// multi-GPU exchange (RCCL), SURVEY.md §8(e)
// ---------------------------------------------------------------------------
int mrt_comm_unique_id(void* id, size_t bytes) {
  if (!id || bytes < sizeof(ncclUniqueId)) return fail(MRT_ERR_INVALID, "mrt_comm_unique_id: need 128 bytes");
  ncclUniqueId u;
  NCCL_TRY(ncclGetUniqueId(&u));
  std::memcpy(id, &u, sizeof(u));
  return MRT_OK;
}

int mrt_comm_create(const void* id, uint32_t nranks, uint32_t rank, int device, mrt_comm** out) {
  if (!id || !out || nranks == 0 || rank >= nranks || device < 0)
    return fail(MRT_ERR_INVALID, "mrt_comm_create: bad argument");
  *out = nullptr;
  std::unique_ptr<mrt_comm> c(new mrt_comm());
  c->nranks = nranks;
  c->rank = rank;
  c->device = device;
  HIP_TRY(hipSetDevice(device));
  HIP_TRY(c->stream.create());
  ncclUniqueId u;
  std::memcpy(&u, id, sizeof(u));
  const ncclResult_t e = ncclCommInitRank(&c->comm, (int)nranks, u, (int)rank);
  if (e != ncclSuccess) {
    c->comm = nullptr;   // (nothing for ~mrt_comm to destroy)
    return fail(MRT_ERR_HIP, std::string("ncclCommInitRank: ") + ncclGetErrorString(e));
  }
  c->health->comm = c->comm;
  *out = c.release();
  return MRT_OK;
}

int mrt_comm_destroy(mrt_comm* c) {
  if (!c) return MRT_OK;
  delete c;
  return MRT_OK;
}

int mrt_comm_set_timeout(mrt_comm* c, uint32_t timeout_ms) {
  if (!c) return fail(MRT_ERR_INVALID, "null communicator");
  std::lock_guard<std::mutex> lk(c->health->m);
  c->health->timeout_ms = timeout_ms ? (double)timeout_ms : 120000.0;
  return MRT_OK;
}

int mrt_comm_check(mrt_comm* c) {
  if (!c) return fail(MRT_ERR_INVALID, "null communicator");
  std::lock_guard<std::mutex> lk(c->health->m);
  return comm_check_locked(*c->health);
}

int mrt_debug_comm_fail(mrt_comm* c, uint32_t mode) {
  if (!c || mode > 2) return fail(MRT_ERR_INVALID, "mrt_debug_comm_fail: bad argument");
  std::lock_guard<std::mutex> lk(c->health->m);
  c->health->inject = mode;
  return MRT_OK;
}


int mrt_renderer_exchange(mrt_renderer* r, mrt_comm* c, uint32_t mode) {
  if (!r || !c) return fail(MRT_ERR_INVALID, "mrt_renderer_exchange: null argument");
  const uint32_t kind = mode & 0xFFu;
  const bool overlap = (mode & MRT_EXCHANGE_OVERLAP) != 0;
  if ((kind != MRT_EXCHANGE_GATHER && kind != MRT_EXCHANGE_REDUCE) || (mode & ~0x1FFu) ||
      (overlap && kind != MRT_EXCHANGE_GATHER))
    return fail(MRT_ERR_INVALID, "mrt_renderer_exchange: bad mode");
  if (c->nranks != r->desc.shard_count || c->rank != r->desc.shard_rank)
    return fail(MRT_ERR_INVALID, "mrt_renderer_exchange: the renderer's shard (rank, count) must be the comm's");
  if (c->device != r->scene->device) return fail(MRT_ERR_INVALID, "mrt_renderer_exchange: comm on another device");
  {
    std::lock_guard<std::mutex> lk(c->health->m);
    if (int rc = comm_check_locked(*c->health)) return rc;
  }
  HIP_TRY(hipSetDevice(c->device));
  if (r->x.comm && r->x.comm != c) { int rc = exchange_flush(r); if (rc) return rc; }
  r->x.comm = c;
  int rc = exchange_flush(r);   // the previous overlapped gather's unpack (rank 0)
  if (rc) return rc;
  const uint32_t W = r->desc.width, H = r->desc.height;
  if (c->rank == 0 && c->nranks > 1) r->image_foreign = true;   // other ranks' tiles land in rank 0's image
  HIP_TRY(r->x.coll_done.ensure(hipEventDisableTiming));
  r->x.health = c->health;
  if (kind == MRT_EXCHANGE_REDUCE) {   // one in-place SUM reduce of the RGBA32F image to rank 0
    NCCL_TRY(ncclReduce(r->image, r->image, (size_t)W * H * 4, ncclFloat, ncclSum, 0, c->comm, r->stream));
    HIP_TRY(hipEventRecord(r->x.coll_done, r->stream));
    r->x.coll_pending = true;
    return MRT_OK;
  }
  rc = exchange_buffers(r, c);
  if (rc) return rc;
  Exchange& x = r->x;
  x.rank = c->rank;
  x.nranks = c->nranks;
  x.width = W;
  x.height = H;
  const int i = overlap ? (int)x.next : 0;
  x.next ^= 1u;
  // the gather two exchanges ago may still be reading packed[i]
  if (x.gather_recorded[i]) HIP_TRY(hipStreamWaitEvent(r->stream, x.gather_done[i], 0));
  HIP_TRY(mrt::fast::launch_tiles_move(reinterpret_cast<const float4*>(r->image), x.packed[i].as<float4>(), W, H,
                                       c->rank, c->nranks, true, r->stream));
  float* recv = c->rank == 0 ? x.gathered.as<float>() : x.packed[i].as<float>();
  if (overlap) {
    // the collective waits for the pack (and, on rank 0, for the previous
    // unpack, which precedes the pack on the renderer's stream) and runs on
    // the communicator's stream while the renderer's next draw proceeds.  A
    // renderer with frame batches on two render streams (a tile share) never
    // makes a render launch wait on its main stream, so there the collective
    // stays on the main stream: a process has 4 hardware queues by default,
    // and a stream sharing one with a render stream would hold that stream's
    // launches behind the collective.
    hipStream_t gs = r->inflight > 1 ? r->stream.get() : c->stream.get();
    if (gs != r->stream) {
      HIP_TRY(hipEventRecord(x.pack_done[i], r->stream));
      HIP_TRY(hipStreamWaitEvent(gs, x.pack_done[i], 0));
    }
    NCCL_TRY(ncclGather(x.packed[i].p, recv, x.slab_floats, ncclFloat, 0, c->comm, gs));
    HIP_TRY(hipEventRecord(x.gather_done[i], gs));
    HIP_TRY(hipEventRecord(x.coll_done, gs));
    x.coll_pending = true;
    x.gather_recorded[i] = true;
    x.pending = i;
    return MRT_OK;
  }
  NCCL_TRY(ncclGather(x.packed[i].p, recv, x.slab_floats, ncclFloat, 0, c->comm, r->stream));
  HIP_TRY(hipEventRecord(x.gather_done[i], r->stream));
  HIP_TRY(hipEventRecord(x.coll_done, r->stream));
  x.coll_pending = true;
  x.gather_recorded[i] = true;
  return exchange_unpack(r, i);
}

// Test entry (include/mrt.h): rank 0's half of the gather exchange without
// a communicator — `gathered` (host, nranks slabs of slab_floats packed
// floats, rank k's at k * slab_floats, as ncclGather delivers them) is copied
// into the receive buffer and unpacked by the same exchange_unpack the RCCL
// path runs, so slabs k >= 1 of an N-rank gather are exercised on one device.
int mrt_debug_exchange_unpack(mrt_renderer* r, uint32_t nranks, const float* gathered, size_t floats) {
  if (!r || !gathered) return fail(MRT_ERR_INVALID, "mrt_debug_exchange_unpack: null argument");
  if (nranks < 2 || r->desc.shard_count != nranks || r->desc.shard_rank != 0)
    return fail(MRT_ERR_INVALID, "mrt_debug_exchange_unpack: the renderer must be rank 0 of nranks >= 2");
  HIP_TRY(hipSetDevice(r->scene->device));
  int rc = exchange_flush(r);
  if (rc) return rc;
  mrt_comm c;   // shape only: exchange_buffers reads rank / nranks
  c.nranks = nranks;
  c.rank = 0;
  c.device = r->scene->device;
  rc = exchange_buffers(r, &c);
  if (rc) return rc;
  Exchange& x = r->x;
  if (floats != x.slab_floats * nranks) return fail(MRT_ERR_INVALID, "mrt_debug_exchange_unpack: need nranks * slab floats");
  x.rank = 0;
  x.nranks = nranks;
  x.width = r->desc.width;
  x.height = r->desc.height;
  r->image_foreign = true;
  HIP_TRY(hipMemcpyAsync(x.gathered.p, gathered, floats * 4, hipMemcpyHostToDevice, r->stream));
  HIP_TRY(hipEventRecord(x.gather_done[0], r->stream));   // "the gather is done"
  x.gather_recorded[0] = true;
  rc = exchange_unpack(r, 0);
  if (rc) return rc;
  HIP_TRY(hipStreamSynchronize(r->stream));
  return MRT_OK;
}

int mrt_renderer_exchange_flush(mrt_renderer* r) {
  if (!r) return fail(MRT_ERR_INVALID, "null renderer");
  int rc = exchange_flush(r);
  if (rc) return rc;
  return exchange_wait(r);   // the collective done on the device, or the communicator aborted
}

int mrt_renderer_tiles_read(mrt_renderer* r, float* host, size_t floats) {
  if (!r || !host) return fail(MRT_ERR_INVALID, "null argument");
  uint64_t n = 0;
  int rc = mrt_tiles_packed_floats(r->desc.width, r->desc.height, r->desc.shard_rank, r->desc.shard_count, &n);
  if (rc) return rc;
  if (floats < n) return fail(MRT_ERR_INVALID, "mrt_renderer_tiles_read: buffer too small");
  rc = exchange_flush(r);
  if (rc) return rc;
  if (r->x.staging.bytes < n * 4) HIP_TRY(r->x.staging.alloc(n * 4));
  HIP_TRY(mrt::fast::launch_tiles_move(reinterpret_cast<const float4*>(r->image), r->x.staging.as<float4>(),
                                       r->desc.width, r->desc.height, r->desc.shard_rank, r->desc.shard_count, true,
                                       r->stream));
  HIP_TRY(hipMemcpyAsync(host, r->x.staging.p, n * 4, hipMemcpyDeviceToHost, r->stream));
  return mrt_renderer_sync(r);
}

int mrt_renderer_tiles_write(mrt_renderer* r, uint32_t shard_rank, const float* host, size_t floats) {
  if (!r || !host) return fail(MRT_ERR_INVALID, "null argument");
  if (shard_rank >= r->desc.shard_count) return fail(MRT_ERR_INVALID, "mrt_renderer_tiles_write: shard_rank >= shard_count");
  uint64_t n = 0;
  int rc = mrt_tiles_packed_floats(r->desc.width, r->desc.height, shard_rank, r->desc.shard_count, &n);
  if (rc) return rc;
  if (floats < n) return fail(MRT_ERR_INVALID, "mrt_renderer_tiles_write: buffer too small");
  rc = exchange_flush(r);
  if (rc) return rc;
  r->image_foreign = true;
  HIP_TRY(hipStreamSynchronize(r->stream));   // the staging buffer may still feed a queued copy
  if (r->x.staging.bytes < n * 4) HIP_TRY(r->x.staging.alloc(n * 4));
  HIP_TRY(hipMemcpyAsync(r->x.staging.p, host, n * 4, hipMemcpyHostToDevice, r->stream));
  HIP_TRY(mrt::fast::launch_tiles_move(r->x.staging.as<float4>(), reinterpret_cast<float4*>(r->image), r->desc.width,
                                       r->desc.height, shard_rank, r->desc.shard_count, false, r->stream));
  return mrt_renderer_sync(r);
}

}  // extern "C"
