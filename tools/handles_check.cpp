// handles_check — exercises the owning types of csrc/hip_handles.h against tools/hip_stub.cpp (no
// device) and prints one line per case for tests/test_hip_handles_host.py.  In every line
// "live=E/S/P/D" are the live events / streams / pinned blocks / device blocks and "bad" the
// releases of something that was not live (a second release, or of a borrowed handle) so far.
// build: g++ -std=c++17 -D__HIP_PLATFORM_AMD__ -I/opt/rocm/include -I../metal-renderer_amd/csrc
//        handles_check.cpp hip_stub.cpp
#include <cstdio>
#include <set>
#include <vector>

#include "hip_handles.h"

namespace stub {
extern std::set<void*> events, streams, pinned, device;
extern long calls, fail_at, bad_frees;
extern unsigned pinned_flags;
}  // namespace stub

using namespace mrt::host;

namespace {

void line(const char* name, const char* note = "") {
  std::printf("%s%s live=%zu/%zu/%zu/%zu bad=%ld\n", name, note, stub::events.size(), stub::streams.size(),
              stub::pinned.size(), stub::device.size(), stub::bad_frees);
}

// what mrt_renderer_create makes, in its order: the main stream, the slots' streams, the draw
// ring's twelve events, two pinned buffers (one mapped) and the image
struct Aggregate {
  Stream stream;
  std::vector<Stream> slots;
  Event ring[12];
  PinnedBuf counters, list;
  DevBuf image;
  hipError_t create(int nslots) {
    hipError_t e = stream.create();
    for (int k = 0; k < nslots && e == hipSuccess; ++k) {
      slots.emplace_back();
      e = slots.back().create();
    }
    for (int k = 0; k < 12 && e == hipSuccess; ++k) e = ring[k].create(k % 4 < 2 ? 0 : hipEventDisableTiming);
    if (e == hipSuccess) e = counters.reserve(4096, hipHostMallocMapped);
    if (e == hipSuccess) e = list.reserve(256, hipHostMallocDefault);
    if (e == hipSuccess) e = image.alloc(64 * 64 * 16);
    return e;
  }
};
constexpr int kSlots = 8;
constexpr int kAggregateCalls = 1 + kSlots + 12 + 2 + 1 + 1;   // (the mapped buffer: two calls)

}  // namespace

int main() {
  {   // move construction and assignment: one owner, each handle released once
    Event a;
    (void)a.create(hipEventDisableTiming);
    const hipEvent_t h = a.get();
    Event b(std::move(a));
    std::printf("event_move_construct from_empty=%d to_same=%d", a.get() == nullptr, b.get() == h);
    line("");
    Event c;
    (void)c.create(0);
    c = std::move(b);   // c's own event goes, b's moves in
    std::printf("event_move_assign from_empty=%d to_same=%d", b.get() == nullptr, c.get() == h);
    line("");
    Event& same = c;
    c = std::move(same);   // (self-assignment keeps it)
    line("event_self_assign");
  }
  line("event_scope_end");
  {
    Stream a;
    (void)a.create();
    const hipStream_t h = a.get();
    Stream b(std::move(a));
    Stream c;
    c = std::move(b);
    std::printf("stream_move from_empty=%d to_same=%d", a.get() == nullptr && b.get() == nullptr, c.get() == h);
    line("");
    Stream lent;
    lent.borrow(c);
    Stream lent2(std::move(lent));
    std::printf("stream_borrow same=%d from_empty=%d", lent2.get() == h, lent.get() == nullptr);
    line("");
    lent2.reset();
    line("stream_borrow_reset");
    Stream own;
    (void)own.create();
    own.borrow(c);   // its own stream goes; c's is only lent
    line("stream_borrow_over_own");
  }
  line("stream_scope_end");
  {
    DevBuf a;
    (void)a.alloc(100);
    void* p = a.p;
    DevBuf b(std::move(a));
    std::printf("devbuf_move_construct from_empty=%d to_same=%d bytes=%zu", a.p == nullptr && a.bytes == 0, b.p == p, b.bytes);
    line("");
    DevBuf c;
    (void)c.alloc(50);
    c = std::move(b);
    std::printf("devbuf_move_assign from_empty=%d to_same=%d bytes=%zu", b.p == nullptr && b.bytes == 0, c.p == p, c.bytes);
    line("");
    (void)c.alloc(0);
    std::printf("devbuf_alloc_zero empty=%d bytes=%zu", c.p == nullptr, c.bytes);
    line("");
  }
  line("devbuf_scope_end");
  {   // ensure creates once
    Event e;
    const long before = stub::calls;
    (void)e.ensure(hipEventDisableTiming);
    const hipEvent_t h = e.get();
    (void)e.ensure(hipEventDisableTiming);
    (void)e.ensure(0);
    std::printf("event_ensure creates=%ld same=%d", stub::calls - before, e.get() == h);
    line("");
  }
  line("event_ensure_scope_end");
  {   // reserve: grows only, passes its flags on, a failed grow leaves nothing
    PinnedBuf b;
    (void)b.reserve(1000, hipHostMallocMapped);
    void* h = b.host();
    std::printf("pinned_reserve bytes=%zu mapped=%d device_set=%d", b.bytes(), stub::pinned_flags == hipHostMallocMapped,
                b.device() == h);
    line("");
    const long before = stub::calls;
    (void)b.reserve(10, hipHostMallocMapped);
    (void)b.reserve(1000, hipHostMallocMapped);
    std::printf("pinned_reserve_smaller bytes=%zu same=%d calls=%ld", b.bytes(), b.host() == h, stub::calls - before);
    line("");
    (void)b.reserve(2000, hipHostMallocDefault);
    std::printf("pinned_reserve_grow bytes=%zu default=%d device_set=%d", b.bytes(), stub::pinned_flags == hipHostMallocDefault,
                b.device() != nullptr);
    line("");
    PinnedBuf m(std::move(b));
    PinnedBuf n;
    (void)n.reserve(8, hipHostMallocDefault);
    n = std::move(m);
    std::printf("pinned_move from_empty=%d bytes=%zu", b.host() == nullptr && b.bytes() == 0 && m.host() == nullptr && m.bytes() == 0,
                n.bytes());
    line("");
    stub::fail_at = stub::calls + 1;
    const hipError_t e = n.reserve(4000, hipHostMallocDefault);
    std::printf("pinned_failed_grow failed=%d empty=%d bytes=%zu", e != hipSuccess, n.host() == nullptr && n.device() == nullptr,
                n.bytes());
    line("");
    stub::fail_at = stub::calls + 2;   // the allocation succeeds, its device address is refused
    const hipError_t e2 = n.reserve(4000, hipHostMallocMapped);
    std::printf("pinned_failed_map failed=%d empty=%d bytes=%zu", e2 != hipSuccess, n.host() == nullptr && n.device() == nullptr,
                n.bytes());
    line("");
    stub::fail_at = 0;
  }
  line("pinned_scope_end");
  // a renderer-shaped aggregate whose k-th HIP call fails, for every k (the last k: none fails)
  for (int k = 1; k <= kAggregateCalls + 1; ++k) {
    int failed;
    size_t made;
    {
      Aggregate a;
      stub::fail_at = stub::calls + k;
      failed = a.create(kSlots) != hipSuccess;
      stub::fail_at = 0;
      made = stub::events.size() + stub::streams.size() + stub::pinned.size() + stub::device.size();
    }
    std::printf("aggregate k=%d failed=%d made=%zu", k, failed, made);
    line("");
  }
  return stub::bad_frees == 0 && stub::events.empty() && stub::streams.empty() && stub::pinned.empty() && stub::device.empty() ? 0 : 1;
}
