// kern_stream.h — the wave-local streaming wavefront kernel
#pragma once
#include "kern_bounce.h"

namespace mrt { namespace MRT_NS { namespace {

// ---------------------------------------------------------------------------
// Wave-local streaming wavefront: every bounce of a frame batch in ONE launch
// over the persistent bounce grid, with no hand-off between waves (the
// whole-scene-in-LDS class: C1, C2).
//
// bounce_kernel ends every bounce at a launch boundary: the last grabs drain
// at falling occupancy and the next launch ramps up again — 60-110 us per
// launch on one GPU's 1/8 tile share of C2 (launches of 0.35-1 ms), 1-3 % of
// a whole-frame launch.  Here each wave keeps its own small queue per bounce
// level (kStreamCap slots in HBM, written and re-read by the same CU, so
// mostly L2 hits) and always runs a full wave of ONE bounce: the deepest
// level holding >= 64 rays, else 64 new camera rays from the launch's grab
// ranges.  Survivors go to the next level at the wave's own count (ballot +
// popcount, no atomics).  Every iteration is a coherent 64-lane wave of one
// bounce as in bounce_kernel (shading code path, noise table), the queues
// never exceed 2 * 64 - 1 rays per level (a level is run as soon as it holds
// 64 and deeper levels first), and only the end of the launch drains: once
// the camera rays are gone a wave runs its partial levels, deepest first.
// No wave ever waits for another, so any grid and any residency is safe.
// ---------------------------------------------------------------------------
template <int STACK, int MODE, bool CAM = false, bool LIST = false>
__global__ __launch_bounds__(kBlock, MRT_STREAM_WAVES) void stream_kernel(DeviceScene sc, BounceArgs a) {
  // per wave (private rows): [0] rays queued per level, [1] survivors per
  // bounce (stats).  One array, so that the one row address `cnt` serves
  // both: as two arrays the kernel spilled 6 values, as one 5 (16 scratch
  // instructions -> 10), C2 +1.0 %.  A by-product of register allocation,
  // which nothing guards: re-check with tools/kres.py after a change here or
  // a compiler update
  __shared__ uint32_t s_rows[kBlock / 64][2][kStreamMaxL];
  __shared__ uint32_t s_closed;
  span_begin(a);
  LS_INIT();
  const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
  const uint32_t L = a.max_path_length;
  const LdsCtx cx = stage_lds<MODE>(sc, 0, a.stack_spill);
  for (uint32_t i = lane; i < L; i += 64u) { s_rows[wave][0][i] = 0; s_rows[wave][1][i] = 0; }
  if (tid == 0) s_closed = 0;
  __syncthreads();
  uint32_t* cnt = s_rows[wave][0];
  uint32_t* alive_cnt = cnt + kStreamMaxL;   // s_rows[wave][1]
  const uint32_t N0 = a.num_slots * a.batch;
  const uint32_t rlen = grab_range_len(N0);
  uint32_t cur_range = blockIdx.x % kGrabRanges, ranges_left = kGrabRanges;
  // this wave's queue: level k (1..L-1) at slots qbase + (k - 1) * kStreamCap
  const uint32_t qbase = (blockIdx.x * (kBlock / 64u) + wave) * (L > 1 ? L - 1 : 1u) * kStreamCap;
  uint32_t pend = 0, pend_end = 0;   // camera rays [pend, pend_end) of the wave's last grab not yet run
  bool input = true;
  STAMP_DECL();   // stamp builds: phase cycles accumulate but are not flushed for this kernel
  const StampRef st = STAMP_REF();
  for (;;) {
    // the deepest level holding a full wave (wave-uniform LDS reads)
    uint32_t lvl = 0;
    for (uint32_t k = L - 1; k >= 1; --k)
      if (cnt[k] >= 64u) { lvl = k; break; }
    if (lvl == 0 && input && pend >= pend_end) {
      // grab kGrab camera rays from the launch's ranges (bounce_kernel's grab
      // loop, its text: a shared function changes this kernel's code)
      uint32_t got = 0xFFFFFFFFu, gend = 0;
      if (lane == 0) {
        while (ranges_left) {
          const uint32_t r0 = cur_range * rlen;
          if (r0 < N0 && !(__hip_atomic_load(&s_closed, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP) & (1u << cur_range))) {
            const uint32_t i = atomicAdd(a.grab + cur_range * kGrabStride, kGrab);
            if (i < rlen && r0 + i < N0) { got = r0 + i; gend = min(N0, min(r0 + rlen, got + kGrab)); break; }
            atomicOr(&s_closed, 1u << cur_range);
          }
          cur_range = cur_range + 1 == kGrabRanges ? 0u : cur_range + 1;
          --ranges_left;
        }
      }
      got = __builtin_amdgcn_readfirstlane(got);
      cur_range = __builtin_amdgcn_readfirstlane(cur_range);
      ranges_left = __builtin_amdgcn_readfirstlane(ranges_left);
      if (got == 0xFFFFFFFFu) {
        input = false;
      } else {
        pend = got;
        pend_end = __builtin_amdgcn_readfirstlane(gend);
      }
    }
    uint32_t n, first;   // this iteration: n rays of level lvl
    bool camera = false;
    if (lvl == 0 && pend < pend_end) {
      camera = true;
      first = pend;
      n = min(64u, pend_end - pend);
      pend += n;
    } else {
      if (lvl == 0) {   // camera rays exhausted: the deepest non-empty level
        for (uint32_t k = L - 1; k >= 1; --k)
          if (cnt[k] > 0u) { lvl = k; break; }
        if (lvl == 0) break;   // every level empty: the wave is done
      }
      n = min(64u, cnt[lvl]);
      first = cnt[lvl] - n;   // run the top n, the rest stays in place
      cnt[lvl] = first;
    }
    const bool active = lane < n;
    const uint32_t idx = first + lane;                                  // camera: the launch's dense index
    const uint32_t slot = qbase + (lvl - 1u) * kStreamCap + first + lane;   // level lvl >= 1: the queue slot
    const uint32_t out = lvl + 1u < L ? qbase + lvl * kStreamCap + cnt[lvl + 1u] : 0u;
    // The wave reads rays its own lanes wrote: their stores first.  This
    // relies on gfx9 (CDNA) memory ordering: a wave's vector stores are
    // counted by vmcnt and the CU's L1 is write-through, so after
    // s_waitcnt vmcnt(0) the wave's own later loads see them.  On gfx10+
    // (stores counted by vscnt) it would need a wavefront-scope
    // release/acquire fence instead (measured within +0.5 % here, DESIGN.md
    // §2.1a).
#if MRT_LANESTATS
    // diagnostic: cycles this wait costs the wave (slot 28) over its level iterations (slot 29)
    uint64_t w0_, w1_;
    asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(w0_)::"memory");
    if (!camera) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(w1_)::"memory");
    if (!camera) { LS_ADD(28, (uint32_t)(w1_ - w0_)); LS_ADD(29, 1); }
#else
    if (!camera) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
#endif
    LS_ADD(camera ? 26 : 27, 1);
    {   // the cost of one timed pair with nothing between
      LS_T0();
      LS_T1(44);
    }
    uint32_t recycled;   // lanes back on level lvl with leaves left to test: never camera rays
    const uint32_t wrote = bounce_wave<STACK, MODE, true, CAM, LIST>(sc, cx, a, camera ? 0u : lvl, active, idx, slot,
                                                                 a.in_q, a.in_q, nullptr, out, 0u, st, recycled);
    if (lvl + 1u < L && lane == 0) {
      cnt[lvl + 1u] += wrote;
      alive_cnt[lvl] += wrote;
    }
    // at most the n lanes that left the level return to it: it stays within
    // kStreamCap, and every pass clears a mask bit of each, so they finish
    if (recycled && lane == 0) cnt[lvl] += recycled;
  }
  // stats: survivors of bounce b = rays alive at the start of bounce b + 1
  for (uint32_t b = lane; b + 1 < L; b += 64u)
    if (alive_cnt[b]) atomicAdd(a.bounce_counts + b, alive_cnt[b]);
  LS_FLUSH();
  span_end(a);
}

}}}  // namespace mrt::MRT_NS::(anonymous)
