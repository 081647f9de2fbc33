// hip_handles.h — the host's owning types for what HIP hands out: device
// memory (DevBuf), events (Event), streams (Stream) and pinned host memory
// (PinnedBuf).  Each releases what it holds when it is destroyed; all are
// move-only and a moved-from object is empty, so an object made of them
// (a renderer, a noise chunk, a BVH build's result) needs no release list and
// a failed create leaks nothing.  No other file in csrc/ frees a HIP resource,
// except stage_api.cpp's mrt_event_destroy, whose events the caller owns.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <type_traits>
#include <utility>

namespace mrt {
namespace host {

struct DevBuf {
  void* p = nullptr;
  size_t bytes = 0;
  DevBuf() = default;
  DevBuf(DevBuf&& o) noexcept : p(std::exchange(o.p, nullptr)), bytes(std::exchange(o.bytes, 0)) {}
  DevBuf& operator=(DevBuf&& o) noexcept {
    if (this != &o) {
      if (p) (void)hipFree(p);
      p = std::exchange(o.p, nullptr);
      bytes = std::exchange(o.bytes, 0);
    }
    return *this;
  }
  ~DevBuf() { if (p) (void)hipFree(p); }
  hipError_t alloc(size_t n) {
    if (p) { (void)hipFree(p); p = nullptr; }
    bytes = n;
    return n ? hipMalloc(&p, n) : hipSuccess;
  }
  template <class T> T* as() const { return reinterpret_cast<T*>(p); }
};
static_assert(!std::is_copy_constructible_v<DevBuf> && !std::is_copy_assignable_v<DevBuf>, "DevBuf owns its memory");

// a HIP handle and whether it is this object's to destroy (what Event and
// Stream share); converts to the handle wherever HIP wants one
template <class H, hipError_t (*Destroy)(H)>
class Handle {
 public:
  Handle() = default;
  Handle(Handle&& o) noexcept : h_(std::exchange(o.h_, nullptr)), owned_(std::exchange(o.owned_, false)) {}
  Handle& operator=(Handle&& o) noexcept {
    if (this != &o) {
      reset();
      h_ = std::exchange(o.h_, nullptr);
      owned_ = std::exchange(o.owned_, false);
    }
    return *this;
  }
  ~Handle() { reset(); }
  void reset() {
    if (owned_) (void)Destroy(h_);
    h_ = nullptr;
    owned_ = false;
  }
  H get() const { return h_; }
  operator H() const { return h_; }

 protected:
  hipError_t own(hipError_t e) {   // `e`: what the create call that wrote h_ returned
    if (e != hipSuccess) h_ = nullptr;
    owned_ = h_ != nullptr;
    return e;
  }
  H h_ = nullptr;
  bool owned_ = false;
};

struct Event : Handle<hipEvent_t, hipEventDestroy> {
  // flags 0: a plain hipEventCreate (the events a time is read from)
  hipError_t create(unsigned flags) {
    reset();
    return own(flags ? hipEventCreateWithFlags(&h_, flags) : hipEventCreate(&h_));
  }
  // an event made where it is first needed: created unless it exists
  hipError_t ensure(unsigned flags) { return h_ ? hipSuccess : create(flags); }
};
static_assert(!std::is_copy_constructible_v<Event> && !std::is_copy_assignable_v<Event>, "Event owns its handle");

struct Stream : Handle<hipStream_t, hipStreamDestroy> {
  hipError_t create() {
    reset();
    return own(hipStreamCreateWithFlags(&h_, hipStreamNonBlocking));
  }
  // someone else's stream (the caller's, or the main stream as slot 0's): never destroyed here
  void borrow(hipStream_t s) {
    reset();
    h_ = s;
  }
};
static_assert(!std::is_copy_constructible_v<Stream> && !std::is_copy_assignable_v<Stream>, "Stream owns its handle");

// pinned host memory that only grows
class PinnedBuf {
 public:
  PinnedBuf() = default;
  PinnedBuf(PinnedBuf&& o) noexcept
      : host_(std::exchange(o.host_, nullptr)), dev_(std::exchange(o.dev_, nullptr)), bytes_(std::exchange(o.bytes_, 0)) {}
  PinnedBuf& operator=(PinnedBuf&& o) noexcept {
    if (this != &o) {
      (void)release();
      host_ = std::exchange(o.host_, nullptr);
      dev_ = std::exchange(o.dev_, nullptr);
      bytes_ = std::exchange(o.bytes_, 0);
    }
    return *this;
  }
  ~PinnedBuf() { (void)release(); }
  // at least `n` bytes, allocated with `flags` (hipHostMallocDefault / hipHostMallocMapped);
  // a buffer that is large enough is kept as it is; a failure leaves it empty
  hipError_t reserve(size_t n, unsigned flags) {
    if (bytes_ >= n) return hipSuccess;
    hipError_t e = release();
    if (e == hipSuccess) e = hipHostMalloc(&host_, n, flags);
    if (e == hipSuccess && (flags & hipHostMallocMapped)) e = hipHostGetDevicePointer(&dev_, host_, 0);
    if (e == hipSuccess) bytes_ = n;
    else (void)release();
    return e;
  }
  template <class T = void> T* host() const { return static_cast<T*>(host_); }
  void* device() const { return dev_; }   // of a mapped buffer: fetched once, when it was allocated
  size_t bytes() const { return bytes_; }

 private:
  hipError_t release() {
    const hipError_t e = host_ ? hipHostFree(host_) : hipSuccess;
    host_ = dev_ = nullptr;
    bytes_ = 0;
    return e;
  }
  void* host_ = nullptr;
  void* dev_ = nullptr;
  size_t bytes_ = 0;
};
static_assert(!std::is_copy_constructible_v<PinnedBuf> && !std::is_copy_assignable_v<PinnedBuf>, "PinnedBuf owns its memory");

}  // namespace host
}  // namespace mrt
