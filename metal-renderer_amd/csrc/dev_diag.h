// dev_diag.h — the three diagnostic builds' hooks, and their empty forms for the product:
// lane statistics (MRT_LANESTATS, tools/lane_stats.py), phase stamps (MRT_STAMPS,
// tools/phase_stamps.py) and the one-pixel path trace (MRT_TRACE_PX, tools/trace_path.py).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "dev_config.h"
#include "kernels.h"

namespace mrt { namespace MRT_NS { namespace {

// ---------------------------------------------------------------------------
// Diagnostic lane statistics (MRT_LANESTATS builds only; never the product):
// per wave, for each traversal loop, the loop iterations and the active lanes
// in them (lane utilisation of that loop = lanes / (64 x iterations)), and the
// lanes entering each phase.  Kept per wave in LDS by the wave's first active
// lane, summed into g_lanes at the wave's exit.  Slots (tools/lane_stats.py):
//   0-5   nearest query: lanes, wave calls, interior iterations, interior
//         lane-steps, leaf iterations, leaf lane-steps
//   6-11  the same for occlusion queries
//   12-13 shading: wave calls, lanes;  14-15 bounce_wave: calls, active lanes
//   16-17 shadow phase: lanes with a shadow ray, wave calls with any
//   18-19 camera-ray candidate lists: wave calls, lanes
//   20-25 path kernel: service rounds, lanes serviced, traversal rounds,
//         lanes traversing in them, lanes refilled, outer iterations
//   26-27 stream kernel: camera iterations, queue-level iterations
//   30-31 leaf-box sweep (nearest queries; their leaf tests count in 4-5):
//         pop-and-cull rounds, lanes in them
//   32-33 recycling (stream kernel, capped sweep): lanes recycled, passes
//         that held a resumed lane
//   34-45 stream kernel, exposed memory waits, pairs of shader-
//         clock cycles and events as 28-29: queue planes 0-1, queue planes
//         2-3, candidate-list header + entries (per listed camera iteration),
//         the shadow query's root select, the sweep's phase-1 record loads
//         (per record), and a back-to-back pair of clock reads (the cost of
//         the measurement itself, to be subtracted per event)
//   46-47 unused, read zero (the third sweep key's rounds; DESIGN "Retired A/B switches")
//   48-51 convex shadow query, split by the wave's class (LS_SPLIT:
//         0 = camera rays, 1 = a queue level): first-face passes (the plan's one
//         pass; the per-solid loop's entry-face pass of each solid) and wave
//         calls of the query, for the camera waves (48, 49) and the levels (50, 51)
// ---------------------------------------------------------------------------
#if MRT_LANESTATS
constexpr int kLaneStats = 52;
__shared__ unsigned long long s_lanes[kBlock / 64][kLaneStats];
__shared__ uint32_t s_lane_split[kBlock / 64];   // the wave's class for the split slots
__device__ unsigned long long g_lanes[kLaneStats];
__device__ __forceinline__ void ls_add(int k, uint32_t v) {
  const uint64_t m = __ballot(1);
  if ((threadIdx.x & 63u) == (uint32_t)(__ffsll((unsigned long long)m) - 1)) s_lanes[threadIdx.x >> 6][k] += v;
}
__device__ __forceinline__ uint32_t ls_lanes() { return (uint32_t)__popcll(__ballot(1)); }
#define LS_ADD(k, v) ls_add((k), (v))
// the wave's class from here on (wave-uniform), and a count into slot k + 2 * class
__device__ __forceinline__ void ls_split(uint32_t cls) {
  const uint64_t m = __ballot(1);
  if ((threadIdx.x & 63u) == (uint32_t)(__ffsll((unsigned long long)m) - 1)) s_lane_split[threadIdx.x >> 6] = cls;
}
#define LS_SPLIT(cls) ls_split((cls))
#define LS_ADD_SPLIT(k, v) ls_add((k) + 2 * (int)s_lane_split[threadIdx.x >> 6], (v))
#define LS_INIT() do { if ((threadIdx.x & 63u) < (uint32_t)kLaneStats) s_lanes[threadIdx.x >> 6][threadIdx.x & 63u] = 0; \
    if ((threadIdx.x & 63u) == 0u) s_lane_split[threadIdx.x >> 6] = 0; } while (0)
#define LS_FLUSH() do { const uint32_t l_ = threadIdx.x & 63u; \
    if (l_ < (uint32_t)kLaneStats && s_lanes[threadIdx.x >> 6][l_]) atomicAdd(&g_lanes[l_], s_lanes[threadIdx.x >> 6][l_]); } while (0)
// the shader clock, read and waited for (the wait is for the scalar and LDS
// counter only: outstanding vector memory operations stay outstanding)
__device__ __forceinline__ uint64_t ls_clock() {
  uint64_t t;
  asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t)::"memory");
  return t;
}
#define LS_T0() const uint64_t ls_t0_ = ls_clock()
// cycles since LS_T0 into slot k, one event into slot k + 1
#define LS_T1(k) do { LS_ADD((k), (uint32_t)(ls_clock() - ls_t0_)); LS_ADD((k) + 1, 1); } while (0)
// LS_T1 once a scalar load's first and last word (a, b) have arrived
#define LS_T1_LOADED(k, a, b) do { asm volatile("" ::"s"(a), "s"(b)); LS_T1(k); } while (0)
// cycles the wave waits here for its outstanding vector memory operations
#define LS_WAIT_VM(k) do { LS_T0(); asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); LS_T1(k); } while (0)
#else
#define LS_ADD(k, v) do {} while (0)
#define LS_SPLIT(cls) do {} while (0)
#define LS_ADD_SPLIT(k, v) do {} while (0)
#define LS_INIT() do {} while (0)
#define LS_FLUSH() do {} while (0)
#define LS_T0() do {} while (0)
#define LS_T1(k) do {} while (0)
#define LS_T1_LOADED(k, a, b) do {} while (0)
#define LS_WAIT_VM(k) do {} while (0)
#endif

// ---------------------------------------------------------------------------
// Diagnostic phase stamps (MRT_STAMPS builds only; never in the product):
// s_memtime around each wave-uniform phase of the bounce loop, summed per
// wave in SGPRs and stored once per wave (plain stores into g_wave_t) at
// exit, with the wave's launch timeline.  The stamp waits for
// vmcnt/lgkmcnt(0), so read the SHARES, not the length.
// ---------------------------------------------------------------------------
#ifndef MRT_STAMPS
#define MRT_STAMPS 0
#endif
#if MRT_STAMPS
__device__ __forceinline__ uint64_t stamp_now() {
  uint64_t t;
  __builtin_amdgcn_sched_barrier(0);
  asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)\n\ts_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t)::"memory");
  __builtin_amdgcn_sched_barrier(0);
  return t;
}
// per-wave timeline of the last launch of each bounce index (b % 4), in
// s_memrealtime ticks (100 MHz, chip-wide), wave id = block * 4 + wave:
// {first iteration start, exit, iterations | exit reason << 32 (1 = input
// exhausted, 2 = output segment full), last grab, end of the last grab's
// work, summed grab latency, max grab latency, last grab's latency, phase
// cycles 0..4 (s_memtime), kernel entry (before the LDS staging)} — plain stores, so the exit is not a storm of
// atomics on a few words
constexpr uint32_t kStampWaves = 8192;
constexpr uint32_t kStampFields = 16;
__device__ unsigned long long g_wave_t[4][kStampWaves][kStampFields];
__device__ __forceinline__ uint64_t stamp_real() {
  uint64_t t;
  asm volatile("s_memrealtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t)::"memory");
  return t;
}
#define STAMP_DECL() uint64_t st_acc[6] = {0, 0, 0, 0, 0, 0}; uint64_t st_prev = 0; uint64_t st_iters = 0; \
    const uint64_t st_t0 = stamp_real(); uint64_t st_why = 0, st_grab = 0, st_work = 0, st_ab = 0, \
    st_asum = 0, st_amax = 0
#define STAMP_BEGIN() do { st_prev = stamp_now(); ++st_iters; } while (0)
#define STAMP(k) do { const uint64_t t_ = stamp_now(); st_acc[k] += t_ - st_prev; st_prev = t_; } while (0)
#define STAMP_FLUSH() do { if ((threadIdx.x & 63u) == 0) { \
    const uint32_t w_ = blockIdx.x * (blockDim.x / 64u) + threadIdx.x / 64u; \
    if (w_ < kStampWaves) { unsigned long long* e_ = g_wave_t[a.bounce & 3u][w_]; \
      e_[0] = st_t0; e_[1] = stamp_real(); e_[2] = st_iters | (st_why << 32); e_[3] = st_grab; \
      e_[4] = st_work; e_[5] = st_asum; e_[6] = st_amax; e_[7] = st_grab - st_ab; \
      for (int k_ = 0; k_ < 5; ++k_) e_[8 + k_] = st_acc[k_]; e_[13] = st_entry; } } } while (0)
#define STAMP_ENTRY() const uint64_t st_entry = stamp_real()
struct StampRef { uint64_t* acc; uint64_t* prev; };   // a kernel's phase accumulators, for a callee
#define STAMP_REF() StampRef{st_acc, &st_prev}
#define STAMP_AT(r, k) do { const uint64_t t_ = stamp_now(); (r).acc[k] += t_ - *(r).prev; *(r).prev = t_; } while (0)
#define STAMP_ATOMIC_BEGIN() do { st_ab = stamp_real(); } while (0)
#define STAMP_EXIT(got) do { st_why = (got) == 0xFFFFFFFEu ? 2u : 1u; } while (0)
#define STAMP_GRAB() do { st_grab = stamp_real(); st_asum += st_grab - st_ab; \
    st_amax = st_grab - st_ab > st_amax ? st_grab - st_ab : st_amax; } while (0)
#define STAMP_WORK() do { st_work = stamp_real(); } while (0)
#else
#define STAMP_DECL() do {} while (0)
#define STAMP_BEGIN() do {} while (0)
#define STAMP(k) do {} while (0)
#define STAMP_FLUSH() do {} while (0)
#define STAMP_EXIT(got) do {} while (0)
#define STAMP_GRAB() do {} while (0)
#define STAMP_WORK() do {} while (0)
#define STAMP_ATOMIC_BEGIN() do {} while (0)
#define STAMP_ENTRY() do {} while (0)
struct StampRef {};
#define STAMP_REF() StampRef{}
#define STAMP_AT(r, k) do {} while (0)
#endif

// Diagnostic path trace (MRT_TRACE_PX builds only, never the product): the
// queries of one pixel-frame (MRT_TRACE_X, MRT_TRACE_Y, absolute frame
// MRT_TRACE_F) printed with their float bits.
#ifndef MRT_TRACE_PX
#define MRT_TRACE_PX 0
#endif
#if MRT_TRACE_PX
__device__ __forceinline__ uint32_t mdiv(uint32_t n, MagicDiv m, uint32_t d);                          // dev_shade.h
__device__ __forceinline__ void slot_pixel_a(uint32_t s, const BounceArgs& a, uint32_t& x, uint32_t& y);
__device__ __forceinline__ bool trace_lane(const BounceArgs& a, uint32_t tagv) {
  const uint32_t gslot = tagv & 0x7FFFFFFFu;
  const uint32_t fj = a.batch == 1u ? 0u : mdiv(gslot, a.div_slots, a.num_slots);
  uint32_t x, y;
  slot_pixel_a(gslot - fj * a.num_slots, a, x, y);
  return x == MRT_TRACE_X && y == MRT_TRACE_Y && a.frame_index + fj == MRT_TRACE_F;
}
#define MRT_TRACE(tagv, ...) do { if (trace_lane(a, (tagv))) printf(__VA_ARGS__); } while (0)
#else
#define MRT_TRACE(tagv, ...) do {} while (0)
#endif

}}}  // namespace mrt::MRT_NS::(anonymous)
