// kern_bounce.h — the fused wavefront bounce: one wave iteration (bounce_wave) and the per-bounce kernel
#pragma once
#include "dev_diag.h"
#include "dev_shade.h"
#include "dev_shadow.h"
#include "dev_sweep.h"

namespace mrt { namespace MRT_NS { namespace {

// ---------------------------------------------------------------------------
// Fused wavefront bounce kernel (the hot path).
//
// One launch per (frame, bounce) over a persistent grid of G blocks.  Each
// ray: [bounce 0: generate the camera ray | else load its SoA state] ->
// nearest hit -> shade (NEE shadow ray, MIS emission, next direction) ->
// shadow visibility -> either accumulate the pixel (path ends: miss, near
// hit, or last bounce) or append the ray to the next queue.
//
// Queue compaction without global atomics: the N input rays are split into
// G contiguous block ranges of `chunk` rays; block g appends its survivors to
// [g*chunk, g*chunk + count_g) of the next queue with one LDS atomic per wave
// (ballot + popcount prefix inside the wave), and publishes count_g once.
// The next launch prefix-scans the G counts in LDS and maps its own dense
// index i to (segment j, offset) with a binary search.  Ray order inside a
// block segment is not deterministic; every ray carries its pixel, so the
// image is.
// ---------------------------------------------------------------------------
// exclusive prefix of v[0..n) in place (LDS), returns the total; n <= 16*kBlock
__device__ __forceinline__ uint32_t block_exclusive_scan(uint32_t* v, uint32_t n, uint32_t* wave_tmp) {
  const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
  const uint32_t per = (n + kBlock - 1) / kBlock;
  const uint32_t b = tid * per, e = min(n, b + per);
  uint32_t local = 0;
  for (uint32_t i = b; i < e; ++i) local += v[i];
  uint32_t incl = local;
  for (int off = 1; off < 64; off <<= 1) {
    const uint32_t up = __shfl_up(incl, off);
    if ((int)lane >= off) incl += up;
  }
  if (lane == 63) wave_tmp[wave] = incl;
  __syncthreads();
  uint32_t wave_prefix = 0, total = 0;
  for (uint32_t w = 0; w < kBlock / 64; ++w) {
    if (w < wave) wave_prefix += wave_tmp[w];
    total += wave_tmp[w];
  }
  uint32_t run = wave_prefix + incl - local;
  for (uint32_t i = b; i < e; ++i) {
    const uint32_t x = v[i];
    v[i] = run;
    run += x;
  }
  __syncthreads();
  return total;
}

// The wave's vector memory operations retired, as an instruction the
// compiler's own wait insertion sees (a wait written in assembly it does not):
// it then forgets the loads it still counts as pending.
__device__ __forceinline__ void wait_vmem() {
  asm volatile("" ::: "memory");
  __builtin_amdgcn_s_waitcnt(0x0F70);   // vmcnt(0), no wait on the export and LDS / scalar counters
  asm volatile("" ::: "memory");
}

// One wave iteration of the fused bounce: up to 64 rays of bounce `bounce`.
// Each active lane generates its camera ray (bounce 0: `idx` = the launch's
// dense index = global slot) or loads its ray from `slot` of `in_q`, finds
// the nearest hit, shades it (NEE shadow ray, MIS emission, next ray), writes
// the radiance of a path that ends here, appends a survivor to the block's
// output segment [out_base, out_base + cap) of `out_q` through the LDS
// cursors (class 0 = left a diffuse surface, from the front; class 1 from
// the back) and traces the shadow ray.  Returns the survivors written.
// Used by bounce_kernel (one launch per bounce) and, with WAVEQ (the wave's
// own queue: survivors at out_base + their rank among the wave's survivors,
// no cursors, no class split), by stream_kernel.
// WAVEQ, a queue level of a scene the leaf-box sweep takes: a
// pass makes at most sc.sweep_cap rest pops, and a lane left with untested
// leaves is recycled instead of shaded — its record goes back on its own
// level unchanged, with the mask in plane 1's w and the partial hit in the
// partial-hit plane (a.out_q.plane[0], which the stream kernel has no other
// use for), at the level's first slot of this pass + its rank among the
// recycled lanes.  `recycled` returns their count; they are not survivors.
// LIST: the launch renders the tiles of a.tile_list (dev_shade.h slot_pixel_l).
template <int STACK, int MODE, bool WAVEQ = false, bool CAM = false, bool LIST = false>
__device__ __forceinline__ uint32_t bounce_wave(const DeviceScene& sc, const LdsCtx& cx, const BounceArgs& a,
                                               uint32_t bounce, bool active, uint32_t idx, uint32_t slot,
                                               const RayQueue& in_q, const RayQueue& out_q, uint32_t* cursor,
                                               uint32_t out_base, uint32_t cap,
                                               StampRef st, uint32_t& recycled) {
  const uint32_t lane = threadIdx.x & 63u;
  const bool last = (bounce + 1 == a.max_path_length);
  LS_ADD(14, 1);
  LS_ADD(15, (uint32_t)__popcll(__ballot(active)));
  // -- phase 0: generate (bounce 0) or load (SoA queue planes 0-1) the ray
  PathState s;
  uint32_t tag = 0;   // tag = global owned slot | prevDiffuse << 31
  uint32_t resume = 0, unfinished = 0;   // WAVEQ: the rest mask a recycled ray came with / leaves with (sweep_nearest)
  recycled = 0;
  uint32_t pblk = 0xFFFFFFFFu;   // bounce 0: the pixel's 8x8 block (camera-ray candidate lists)
  if (active) {
    if (bounce == 0) {
      // frame fj of the batch (num_slots is a multiple of 4096: waves never
      // straddle frames, so fj is wave-uniform)
      const uint32_t fj = a.batch == 1u ? 0u : __builtin_amdgcn_readfirstlane(mdiv(idx, a.div_slots, a.num_slots));
      uint32_t x, y;
      slot_pixel_l<LIST, true>(idx - fj * a.num_slots, a, x, y);
      active = (x < a.width) && (y < a.height);
      if (active) {
        tag = idx;
        pblk = (x / kPrimaryBlock) + (y / kPrimaryBlock) * a.primary_bx;
        const float4 ns = noise_table(a, fj, 0u)[(x % kNoiseDim) + (y % kNoiseDim) * kNoiseDim];
        camera_ray<CAM>(x, y, a.width, a.height, ns, noise_table(a, fj, 0u), a.camera, s.o, s.d);
      }
    } else {
      // planes 2-3 (throughput, pdf, radiance, ior) are loaded after the
      // traversal: they are not needed there, and keeping them out of the
      // traversal's live set saves 8 VGPRs
      const float4 q0 = in_q.plane[0][slot], q1 = in_q.plane[1][slot];
      if (WAVEQ) LS_WAIT_VM(34);
      s.o = mk(q0);
      tag = fbits(q0.w);
      s.d = mk(q1);
      s.prevDiffuse = (tag >> 31) ? 1.0f : 0.0f;
      if (WAVEQ) resume = fbits(q1.w);   // a recycled ray's untested leaves (0: a survivor's record)
    }
  }
  STAMP_AT(st, 0);
  // -- phase 1: nearest hit of the path ray (MPS intersect, Renderer.mm:519-523)
  Hit h;
  h.found = false;
  bool listed = false;
  if (bounce == 0 && a.primary) {
    // a wave of camera rays is one 8x8 pixel block (slot_pixel): its
    // candidate list, when every active lane is in the same block
    const uint32_t b0 = __builtin_amdgcn_readfirstlane(pblk);
    const bool uniform = b0 != 0xFFFFFFFFu && __ballot(active && pblk != b0) == 0;
    LS_T0();
    const PrimaryWords words = (PrimaryWords)(uintptr_t)a.primary;   // header and list: scalar loads
    const uint32_t hd = uniform ? words[b0] : kPrimaryFallback;
#if MRT_LANESTATS
    asm volatile("" ::"s"(hd));
    if (WAVEQ && uniform) LS_T1(38);
#endif
    const uint32_t cnt = hd & 0xFFu;
    if (cnt != kPrimaryFallback) {
      listed = true;
      LS_ADD(18, 1);
      LS_ADD(19, (uint32_t)__popcll(__ballot(active)));
      if (active) primary_nearest<MODE>(sc, cx, words + (hd >> 8), cnt, s.o, s.d, h);
    }
  }
  if (active && !listed) {
    if (last && sc.light_shortcut && !(a.flags & kShadeDebugMaterial)) {
      // the last bounce: light triangles, then one occlusion query (last_bounce_light_hit)
      bool graze;
      if (last_bounce_light_hit<MODE>(sc, cx, s.o, s.d, h, graze)) {
        // the light hit is the target of a shadow query from s.o: the
        // occluder tree when shadow_root allows it (the other lights lost to
        // it in last_bounce_light_hit already, so no lights_occlude here)
        Hit hh;
        hh.t = h.t;
        hh.found = false;
        const int32_t root = shadow_root(sc, s.o, graze);
        if (!(a.debug & 64u) && traverse<STACK, MODE, true>(sc, cx, s.o, s.d, 0.0f, hh, h.prim, root)) h.found = false;
      }
    } else if (WAVEQ && MODE == kAllLds && sc.sweep_leaves) {   // wave-uniform (kernel argument)
      // the capped sweep; camera rays have no queue slot to return to: no cap
      h.t = __builtin_inff();
      h.u = h.v = 0.0f;
      h.prim = 0xFFFFFFFFu;
      if (resume) {
        const float4 ph = a.out_q.plane[0][slot];
        h.t = ph.x;
        h.u = ph.y;
        h.v = ph.z;
        h.prim = fbits(ph.w);
        h.found = h.prim != 0xFFFFFFFFu;
      }
      // (wave-uniform; the level comes from LDS: named scalar so that the cap holds no VGPR through the sweep)
      const uint32_t pops = __builtin_amdgcn_readfirstlane(bounce == 0 ? 0xFFFFFFFFu : sc.sweep_cap);
      unfinished = sweep_nearest<MODE, true>(sc, cx, s.o, s.d, 0.0f, h, pops, resume);
    } else {
      h = trace_nearest<STACK, MODE>(sc, cx, s.o, s.d, 0.0f, __builtin_inff());
    }
  }
  STAMP_AT(st, 1);
  // -- phase 2: intersectionHandler (Shaders.metal:105-212); a miss or a
  //    near hit ends the path (:122-126)
  const uint32_t gslot = tag & 0x7FFFFFFFu;
  if (active) {
    if (bounce == 0) {
      s.T = mk(1.0f, 1.0f, 1.0f);
      s.R = mk(0.0f, 0.0f, 0.0f);
      s.pdf = 1.0f;
      s.prevDiffuse = 0.0f;
      s.ior = 1.00029f;
    } else {
      const float4 q2 = in_q.plane[2][slot], q3 = in_q.plane[3][slot];
      if (WAVEQ) LS_WAIT_VM(36);
      s.T = mk(q2);
      s.pdf = q2.w;
      s.R = mk(q3);
      s.ior = q3.w;
    }
  }
  if (WAVEQ) {
    // recycle: the slots written are among those this pass read (rank <=
    // lane), so every lane's plane-2/3 loads above land first; the loop top's
    // wait orders the wave's later loads behind these stores
    const uint64_t rmask = __ballot(unfinished != 0u);
    if (rmask) {
      LS_ADD(32, (uint32_t)__popcll(rmask));
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      if (unfinished) {
        const uint32_t r = slot - lane + lanes_below_in(rmask);
        in_q.plane[0][r] = make_float4(s.o.x, s.o.y, s.o.z, bitsf(tag));
        in_q.plane[1][r] = make_float4(s.d.x, s.d.y, s.d.z, bitsf(unfinished));
        in_q.plane[2][r] = make_float4(s.T.x, s.T.y, s.T.z, s.pdf);
        in_q.plane[3][r] = make_float4(s.R.x, s.R.y, s.R.z, s.ior);
        a.out_q.plane[0][r] = make_float4(h.t, h.u, h.v, bitsf(h.prim));
      }
      recycled = (uint32_t)__popcll(rmask);
      active = active && !unfinished;   // neither shaded nor ended here
    }
    if (__ballot(resume != 0u)) LS_ADD(33, 1);
  }
  const bool hit_ok = active && h.found && !(h.t < kDistanceEpsilon);
  ShadowRay sh;
  sh.valid = false;
  if (__ballot(hit_ok)) {
    LS_ADD(12, 1);
    LS_ADD(13, (uint32_t)__popcll(__ballot(hit_ok)));
  }
  if (hit_ok) {
    const uint32_t fj = a.batch == 1u ? 0u : mdiv(gslot, a.div_slots, a.num_slots);   // frame in batch
    uint32_t x, y;
    slot_pixel_l<LIST>(gslot - fj * a.num_slots, a, x, y);
    const uint32_t back = (bounce % 3u) == 0 ? 0u : ((bounce % 3u) == 1 ? 2u : 1u);   // uniform
    const float4 ns = noise_table(a, fj, back)[shade_noise_cell(x, y, bounce, a.frame_index + fj)];
    if (a.debug & 2u) {   // ablation: no shading, reflect back along the ray
      s.o = add(s.o, mul(s.d, h.t * 0.999f));
      s.d = mk(-s.d.x, -s.d.y, -s.d.z);
    } else {
      shade_hit<MODE>(sc, cx, h, s, ns, bounce, a.max_path_length, !last, sh, (a.flags & kShadeDebugMaterial) != 0);
    }
  }
  STAMP_AT(st, 2);
  // -- phase 3: paths that end here (miss, near hit, last bounce: none of
  //    them carries a shadow ray) go to accumulateImage (:233-249);
  //    survivors are compacted into this block's segment of the next queue.
  //    Planes 0-2 are written before the shadow traversal so the next ray
  //    is not live across it; plane 3 (radiance, ior) after it.
  // WAVEQ: every load of this iteration has been used by now, so this wait
  // costs nothing — but without it the compiler still counts a queue load as
  // pending (presumably on the paths that skip its use: a wave without an
  // active lane) and waits for "it" at the first reuse of its registers: at
  // the start of the shadow query, behind the stores below, whose whole
  // round trip that s_waitcnt vmcnt(0) then exposed.
  if (WAVEQ) wait_vmem();
  if (active && (!hit_ok || last)) a.radiance[gslot] = make_float4(s.R.x, s.R.y, s.R.z, 0.0f);
  const bool alive = hit_ok && !last;
  // (WAVEQ: testing the survivor of the bounce before the last against the
  // lights here, so that the last level holds only rays a light accepts, was
  // built, changed no bit and measured C2 -3.4 %: removed)
  // re-sort by material between bounces: survivors that left a diffuse
  // surface (class 0) fill the block's segment from the front, the others
  // (mirror / plastic / dielectric: specular and refracted rays) from the
  // back; the next bounce reads all class-0 runs first, so its waves see
  // rays of one class (MRT_DEBUG bit 16: no partition)
  const bool cls1 = !WAVEQ && (s.prevDiffuse == 0.0f) && !(a.debug & 16u);
  const uint64_t mask0 = __ballot(alive && !cls1), mask1 = __ballot(alive && cls1);
  uint32_t o = 0, wrote = 0;
  if (mask0 | mask1) {
    uint32_t w0 = 0, w1 = 0;
    if (!WAVEQ && lane == 0) {
      if (mask0) w0 = atomicAdd(&cursor[0], (uint32_t)__popcll(mask0));
      if (mask1) w1 = atomicAdd(&cursor[1], (uint32_t)__popcll(mask1));
    }
    w0 = __shfl(w0, 0);
    w1 = __shfl(w1, 0);
    o = cls1 ? out_base + cap - 1u - (w1 + lanes_below_in(mask1)) : out_base + w0 + lanes_below_in(mask0);
    if (alive && !(a.debug & 4u)) {
      out_q.plane[0][o] = make_float4(s.o.x, s.o.y, s.o.z, bitsf(gslot | (s.prevDiffuse != 0.0f ? 0x80000000u : 0u)));
      out_q.plane[1][o] = make_float4(s.d.x, s.d.y, s.d.z, 0.0f);
      out_q.plane[2][o] = make_float4(s.T.x, s.T.y, s.T.z, s.pdf);
    }
    wrote = (uint32_t)__popcll(mask0 | mask1);
  }
  STAMP_AT(st, 3);
  // -- phase 4: shadow ray (MPS intersect :545-553 + lightSamplingHandler :214-231)
  if (__ballot(sh.valid)) {
    LS_ADD(16, (uint32_t)__popcll(__ballot(sh.valid)));
    LS_ADD(17, 1);
    LS_SPLIT(bounce == 0u ? 0u : 1u);
  }
  if (sh.valid && ((a.debug & 1u) || shadow_reaches_target<STACK, MODE>(sc, cx, sh.o, sh.d, sh.target, h.prim, sh.graze, a.debug))) {
    s.R = add(s.R, sh.L);
  }
  if (alive && !(a.debug & 4u)) out_q.plane[3][o] = make_float4(s.R.x, s.R.y, s.R.z, s.ior);
  STAMP_AT(st, 4);
  return wrote;
}

template <int STACK, int MODE, bool CAM = false>
__global__ __launch_bounds__(kBlock, MRT_BOUNCE_WAVES) void bounce_kernel(DeviceScene sc, BounceArgs a) {
  __shared__ uint32_t s_wave[kBlock / 64];
  __shared__ uint32_t s_cursor[2], s_res, s_closed;
  STAMP_ENTRY();
  span_begin(a);
  LS_INIT();
  const uint32_t tid = threadIdx.x;
  const uint32_t G = gridDim.x;
  const uint32_t nseg = (a.bounce == 0) ? 0u : a.in_segments;
  const LdsCtx cx = stage_lds<MODE>(sc, nseg + 1, a.stack_spill);
  uint32_t* seg = lds_u32() + cx.scratch_base;   // exclusive prefix of the input segments
  if (tid == 0) s_cursor[0] = s_cursor[1] = s_res = s_closed = 0;

  uint32_t N, in_chunk = 0;
  if (a.bounce == 0) {
    N = a.num_slots * a.batch;
    __syncthreads();
  } else {
    for (uint32_t i = tid; i < nseg; i += kBlock) seg[i] = a.in_seg_count[i];
    __syncthreads();
    N = block_exclusive_scan(seg, nseg, s_wave);
    if (tid == 0) seg[nseg] = N;   // sentinel: count of segment j = seg[j+1] - seg[j]
    __syncthreads();
    in_chunk = *a.in_chunk;
  }
  const uint32_t chunk = ((N + G - 1) / G + kBlock - 1) / kBlock * kBlock;
  // Work assignment (see kernels.h): dynamic — waves grab kGrab rays at a
  // time from kGrabRanges ranges, so the launch ends with at most one grab of
  // imbalance instead of a tail of slow blocks; block output capacity
  // cap = chunk + kSegSlack.  A wave reserves kGrab output slots in LDS
  // before it grabs and returns what it did not use; a wave that cannot
  // reserve stops.  A stopped block holds > cap - kGrab - 3*kGrab > chunk
  // survivors, so not every block can stop while input remains (survivors
  // <= N <= G*chunk): the input is always drained.
  // MRT_DEBUG bit 8: static interleaved assignment (64-ray groups
  // g*4 + w, + 4G, ...), capacity chunk.
  const bool dynamic = (a.debug & 8u) == 0;
  const uint32_t cap = dynamic ? chunk + kSegSlack : chunk;
  const uint32_t out_base = blockIdx.x * cap;
  const uint32_t rlen = grab_range_len(N);
  uint32_t cur_range = blockIdx.x % kGrabRanges, ranges_left = kGrabRanges;
  uint32_t static_base = blockIdx.x * kBlock + (tid & ~63u);

  const uint32_t lane = tid & 63u;

  STAMP_DECL();
  for (;;) {
    uint32_t start, end, niter;
    if (dynamic) {
      uint32_t got = 0xFFFFFFFFu;
      STAMP_ATOMIC_BEGIN();
      if (lane == 0) {
        if (atomicAdd(&s_res, kGrab) + kGrab <= cap) {
          // s_closed: ranges a wave of this block found exhausted, so the
          // block's other waves skip them without a device atomic (walking
          // the exhausted ranges one atomic at a time delayed the launch's
          // last exits by ~30 us: C2 +1.6 %, one GPU's 1/8 share +3.5 %;
          // publishing closed ranges in a launch-wide mask word measured
          // slower than the per-block mask alone)
          // (the grab loop stands in each of the three kernels because one
          // function for it, called here, changes every kernel's code: DESIGN §2.1w)
          while (ranges_left) {
            const uint32_t r0 = cur_range * rlen;
            if (r0 < N && !(__hip_atomic_load(&s_closed, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP) & (1u << cur_range))) {
              const uint32_t i = atomicAdd(a.grab + cur_range * kGrabStride, kGrab);
              if (i < rlen && r0 + i < N) { got = r0 + i; break; }
              atomicOr(&s_closed, 1u << cur_range);
            }
            cur_range = cur_range + 1 == kGrabRanges ? 0u : cur_range + 1;
            --ranges_left;
          }
          if (got == 0xFFFFFFFFu) atomicSub(&s_res, kGrab);   // input exhausted
        } else {
          got = 0xFFFFFFFEu;                                   // block's output segment full
        }
      }
      got = __builtin_amdgcn_readfirstlane(got);
      if (got >= 0xFFFFFFFEu) { STAMP_EXIT(got); break; }
      cur_range = __builtin_amdgcn_readfirstlane(cur_range);
      ranges_left = __builtin_amdgcn_readfirstlane(ranges_left);
      STAMP_GRAB();
      start = got;
      end = min(N, cur_range * rlen + rlen);
      niter = kGrab / 64;
    } else {
      if (static_base >= N) break;
      start = static_base;
      end = N;
      niter = 1;
      static_base += G * kBlock;
    }
    uint32_t wrote = 0;
    for (uint32_t it = 0; it < niter; ++it) {
      const uint32_t idx = start + it * 64u + lane;
      bool active = idx < end;
      uint32_t slot = 0;
      if (active && a.bounce != 0) {
        uint32_t lo = 0, hi = nseg;   // last j with seg[j] <= idx
        while (hi - lo > 1) { const uint32_t mid = (lo + hi) >> 1; if (seg[mid] <= idx) lo = mid; else hi = mid; }
        // segments [0, G): class 0 from the start of block j's range;
        // [G, 2G): class 1, packed at the end of block j - G's range
        const uint32_t g_in = nseg >> 1;
        slot = lo < g_in ? lo * in_chunk + (idx - seg[lo])
                         : (lo - g_in) * in_chunk + in_chunk - (seg[lo + 1] - seg[lo]) + (idx - seg[lo]);
      }
      STAMP_BEGIN();
      uint32_t none;   // (no recycling between launches)
      wrote += bounce_wave<STACK, MODE, false, CAM>(sc, cx, a, a.bounce, active, idx, slot, a.in_q, a.out_q, s_cursor,
                                               out_base, cap, STAMP_REF(), none);
    }
    STAMP_WORK();
    if (dynamic && lane == 0) atomicSub(&s_res, kGrab - wrote);
  }
  STAMP_FLUSH();
  __syncthreads();
  if (tid == 0) {
    a.out_seg_count[blockIdx.x] = s_cursor[0];
    a.out_seg_count[G + blockIdx.x] = s_cursor[1];
    const uint32_t total = s_cursor[0] + s_cursor[1];
    if (total) atomicAdd(a.out_total, total);   // stats: one atomic per block per launch
    if (blockIdx.x == 0) *a.out_chunk = cap;
  }
  LS_FLUSH();
  span_end(a);
}

}}}  // namespace mrt::MRT_NS::(anonymous)
