// hip_stub — the HIP entry points csrc/hip_handles.h calls, for tools/handles_check.cpp: no device,
// each hands out tokens and keeps the set of live ones, so that a release of something not live
// (a second release, or of a borrowed handle) is seen; the n-th creating call can be told to fail.
#include <hip/hip_runtime.h>

#include <cstdlib>
#include <set>

namespace stub {
std::set<void*> events, streams, pinned, device;
long calls = 0;      // creating calls so far
long fail_at = 0;    // the creating call that fails (1-based; 0: none)
long bad_frees = 0;  // releases of what was not live
unsigned pinned_flags = 0;   // of the last pinned allocation

static hipError_t make(std::set<void*>& live, void** out, size_t bytes) {
  *out = nullptr;
  if (++calls == fail_at) return hipErrorOutOfMemory;
  *out = std::malloc(bytes ? bytes : 1);
  live.insert(*out);
  return hipSuccess;
}
static hipError_t drop(std::set<void*>& live, void* p) {
  if (!live.erase(p)) {
    ++bad_frees;
    return hipErrorInvalidValue;
  }
  std::free(p);
  return hipSuccess;
}
}  // namespace stub

extern "C" {
hipError_t hipMalloc(void** p, size_t n) { return stub::make(stub::device, p, n); }
hipError_t hipFree(void* p) { return stub::drop(stub::device, p); }
hipError_t hipHostMalloc(void** p, size_t n, unsigned int flags) {
  stub::pinned_flags = flags;
  return stub::make(stub::pinned, p, n);
}
hipError_t hipHostFree(void* p) { return stub::drop(stub::pinned, p); }
hipError_t hipHostGetDevicePointer(void** dev, void* host, unsigned int) {
  *dev = nullptr;
  if (++stub::calls == stub::fail_at) return hipErrorOutOfMemory;
  *dev = host;
  return hipSuccess;
}
hipError_t hipEventCreate(hipEvent_t* e) { return stub::make(stub::events, reinterpret_cast<void**>(e), 1); }
hipError_t hipEventCreateWithFlags(hipEvent_t* e, unsigned) { return stub::make(stub::events, reinterpret_cast<void**>(e), 1); }
hipError_t hipEventDestroy(hipEvent_t e) { return stub::drop(stub::events, e); }
hipError_t hipStreamCreateWithFlags(hipStream_t* s, unsigned int) {
  return stub::make(stub::streams, reinterpret_cast<void**>(s), 1);
}
hipError_t hipStreamDestroy(hipStream_t s) { return stub::drop(stub::streams, s); }
}
