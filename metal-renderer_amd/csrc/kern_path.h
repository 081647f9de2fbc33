// kern_path.h — the path megakernel and its resumable traversal rounds
#pragma once
#include "dev_diag.h"
#include "dev_shade.h"
#include "dev_shadow.h"
#include "dev_traverse.h"

namespace mrt { namespace MRT_NS { namespace {

struct Trav {
  int32_t node, leaf;
  int sp;
};
__device__ __forceinline__ void trav_begin(int32_t root, Trav& tr) {
  tr.node = root;
  tr.leaf = 0;
  tr.sp = 0;
  if (tr.node < 0) { tr.leaf = tr.node; tr.node = kDone; }
}
__device__ __forceinline__ bool trav_done(const Trav& tr) { return tr.node == kDone && tr.leaf == 0; }

// One round of the while-while walk of traverse(): interior nodes (parking
// one leaf) until every lane still descending holds a leaf, then the parked
// leaves.  any = occlusion query: stops at the first triangle k != target
// with (t_k, k) < (h.t, target) and sets `occluded`.
// uv: when non-null, the nearest hit's barycentrics go to uv[0], uv[kBlock]
// (the lane's LDS path state) instead of h.u, h.v.
template <int STACK, int MODE>
__device__ __forceinline__ void trav_round(const DeviceScene& sc, const LdsCtx& cx, V3 o, V3 d, const RayBox& rb,
                                           Hit& h, bool any, uint32_t target, bool& occluded, Trav& tr,
                                           uint32_t* uv = nullptr, bool trl = false) {
  (void)trl;
#if MRT_TRACE_PX
  if (trl) printf("TR round node=%d leaf=%d sp=%d ht=%08x\n", tr.node, tr.leaf, tr.sp, fbits(h.t));
#endif
  while (tr.node != kDone && tr.node >= 0) {
    LS_ADD(2, 1);
    LS_ADD(3, (uint32_t)__popcll(__ballot(!any)));
    LS_ADD(9, (uint32_t)__popcll(__ballot(any)));
#if MRT_TRACE_PX
    const int32_t n0_ = tr.node;
#endif
    tr.node = interior_step<STACK, MODE, false>(sc, cx, tr.node, o, rb, 0.0f, h.t, tr.sp);
#if MRT_TRACE_PX
    if (trl) printf("TR   int %d -> %d sp=%d leaf=%d\n", n0_, tr.node, tr.sp, tr.leaf);
#endif
    if (tr.node < 0 && tr.leaf == 0) {
      tr.leaf = tr.node;
      tr.node = stack_pop<STACK>(cx, tr.sp);
#if MRT_TRACE_PX
      if (trl) printf("TR   park %d pop %d sp=%d\n", tr.leaf, tr.node, tr.sp);
#endif
    }
    if ((uint32_t)__popcll(__ballot(tr.leaf == 0)) <= (uint32_t)MRT_PATH_SLACK) break;
  }
  while (tr.leaf < 0) {
    LS_ADD(4, 1);
    LS_ADD(5, (uint32_t)__popcll(__ballot(!any)));
    LS_ADD(11, (uint32_t)__popcll(__ballot(any)));
    const uint32_t lr = ~(uint32_t)tr.leaf;
    const uint32_t first = lr >> kLeafCountBits, cnt = (lr & (kMaxLeafSize - 1)) + 1;
    if (leaf_tests<MODE>(sc, cx, o, d, 0.0f, first, cnt, h, any, target, uv)) {   // occluded: the query is over
      occluded = true;
      tr.node = kDone;
      tr.leaf = 0;
      break;
    }
#if MRT_TRACE_PX
    if (trl) printf("TR   leaf %d first=%u cnt=%u -> ht=%08x prim=%u\n", tr.leaf, first, cnt, fbits(h.t), h.prim);
#endif
    tr.leaf = 0;
    if (tr.node < 0) {
      tr.leaf = tr.node;
      tr.node = stack_pop<STACK>(cx, tr.sp);
#if MRT_TRACE_PX
      if (trl) printf("TR   next leaf %d pop %d sp=%d\n", tr.leaf, tr.node, tr.sp);
#endif
    }
#if MRT_LEAF_SLACK > 0
    if ((uint32_t)__popcll(__ballot(tr.leaf < 0)) <= (uint32_t)MRT_LEAF_SLACK) break;
#endif
  }
}

// ---------------------------------------------------------------------------
// Path megakernel: all MAX_PATH_LENGTH bounces of a batch of frames in ONE
// launch.  Each lane carries a whole path — camera ray, then per bounce the
// nearest-hit query, intersectionHandler, the NEE shadow query and
// lightSamplingHandler, in the reference's order (renderer/Renderer.mm:
// 500-585) — as a sequence of resumable traversal queries (trav_round); when
// MRT_PATH_SERVICE lanes have finished their query the wave services them
// together (shading or the shadow resolve, then the next query of the same
// path), and a lane whose path ended takes the next pixel sample from the
// wave's grab pool.  Compared with the wavefront of per-bounce launches there
// are no ray queues in HBM (the path state lives in LDS, 64 B per lane), no
// compaction and segment scans, and one launch (one ramp and drain) per
// batch instead of one per bounce.  The arithmetic of every path is the
// same, so the image is identical (precise build: bitwise).
// LDS path state per lane ([word][lane] after the stack): T (0-2), R (3-5),
// material pdf (6), ior (7), next-ray direction (8-10), pixel slot tag |
// prevDiffuse << 31 (11).  The next ray's origin needs no word: it is the
// shadow ray's origin (both are p + n * 1e-4, Shaders.metal:171,205), which
// stays in the lane's ray registers through the shadow query.
// ---------------------------------------------------------------------------
[[maybe_unused]] constexpr uint32_t kPathStateWords = 12;

// Start the nearest query of the lane's ray: phase 1, a full traversal.
// (The last-bounce light shortcut of the wavefront kernels,
// last_bounce_light_hit, measured C4 -1.3 % / C3 -3.4 % here: removed in r6.)
__device__ __forceinline__ void begin_nearest(const DeviceScene& sc, Hit& h, Trav& tr, uint32_t& phase) {
  phase = 1;
  trav_begin(sc.root, tr);
  h.t = __builtin_inff(); h.u = h.v = 0.0f; h.prim = 0xFFFFFFFFu; h.found = false;
}

// LIST: the launch renders the tiles of a.tile_list (dev_shade.h slot_pixel_l)
template <int STACK, int MODE, bool CAM = false, bool LIST = false>
__global__ __launch_bounds__(kBlock, MRT_PATH_WAVES) void path_kernel(DeviceScene sc, BounceArgs a) {
  __shared__ uint32_t s_closed;
  __shared__ uint32_t s_count[64];   // rays alive at the start of bounce b + 1 (stats)
  span_begin(a);
  LS_INIT();
  const uint32_t tid = threadIdx.x;
  const LdsCtx cx = stage_lds<MODE>(sc, 1, a.stack_spill);
  if (tid == 0) s_closed = 0;
  if (tid < 64) s_count[tid] = 0;
  __syncthreads();
  const uint32_t N = a.num_slots * a.batch;
  const uint32_t L = a.max_path_length;
  const uint32_t rlen = grab_range_len(N);
  uint32_t cur_range = blockIdx.x % kGrabRanges, ranges_left = kGrabRanges;
  const uint32_t lane = tid & 63u;
  uint32_t* const ps = lds_u32() + cx.stack_base + threadIdx.x + (uint32_t)(STACK < 0 ? -STACK : STACK) * kBlock;

  uint32_t pool_next = 0, pool_end = 0;   // wave-uniform pool of pixel-sample indices
  bool exhausted = false;
  uint32_t phase = 0;                     // 0 idle, 1 nearest query, 2 shadow query
  uint32_t bounce = 0;
  V3 ro = mk(0.0f, 0.0f, 0.0f), rd = mk(0.0f, 0.0f, 1.0f);
  Trav tr{kDone, 0, 0};
  Hit h;                                  // nearest: the hit; shadow: h.t = t_target, (h.u, h.v, bits h.prim) = L
  h.t = 0.0f; h.u = h.v = 0.0f; h.prim = 0u; h.found = false;
  bool occluded = false;
  uint32_t target = 0;

  for (;;) {
    LS_ADD(25, 1);
    // ---- refill idle lanes with new camera rays (rayGenerator, Shaders.metal:75-103)
    for (;;) {
      const uint64_t idle = __ballot(phase == 0);
      if (!idle || exhausted) break;
      if (pool_next >= pool_end) {
        uint32_t got = 0xFFFFFFFFu;
        if (lane == 0) {   // bounce_kernel's grab loop (its text: a shared function changes this kernel's code)
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
        }
        got = __builtin_amdgcn_readfirstlane(got);
        cur_range = __builtin_amdgcn_readfirstlane(cur_range);
        ranges_left = __builtin_amdgcn_readfirstlane(ranges_left);
        if (got == 0xFFFFFFFFu) { exhausted = true; break; }
        pool_next = got;
        pool_end = min(N, min(got + kGrab, cur_range * rlen + rlen));
      }
      const uint32_t rank = __builtin_amdgcn_mbcnt_hi((uint32_t)(idle >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)idle, 0u));
      const uint32_t take = min((uint32_t)__popcll(idle), pool_end - pool_next);
      LS_ADD(24, (uint32_t)__popcll(__ballot(phase == 0 && rank < take)));
      if (phase == 0 && rank < take) {
        const uint32_t idx = pool_next + rank;
        // sample index -> (frame fj, slot sl): frame-major, or (sc.region_grabs)
        // block-major — 8x8 pixel block, then frame, then pixel — so that a
        // grab range (1/kGrabRanges of the launch) is one band of the image
        // over all the batch's frames, and the blocks of one XCD (block ids
        // = x mod 8) start on ranges x and x + 8: their rays meet the same
        // geometry in that XCD's L2
        uint32_t fj, sl;
        if (sc.region_grabs) {
          const uint32_t q = idx >> 6, blk = mdiv(q, a.div_batch, a.batch);
          fj = q - blk * a.batch;
          sl = (blk << 6) | (idx & 63u);
        } else {
          fj = a.batch == 1u ? 0u : mdiv(idx, a.div_slots, a.num_slots);
          sl = idx - fj * a.num_slots;
        }
        uint32_t x, y;
        slot_pixel_l<LIST>(sl, a, x, y);
        if ((x < a.width) && (y < a.height)) {
          const float4 ns = noise_table(a, fj, 0u)[(x % kNoiseDim) + (y % kNoiseDim) * kNoiseDim];
          camera_ray<CAM>(x, y, a.width, a.height, ns, noise_table(a, fj, 0u), a.camera, ro, rd);
          ps[0 * kBlock] = fbits(1.0f); ps[1 * kBlock] = fbits(1.0f); ps[2 * kBlock] = fbits(1.0f);
          ps[3 * kBlock] = 0u; ps[4 * kBlock] = 0u; ps[5 * kBlock] = 0u;
          ps[6 * kBlock] = fbits(1.0f); ps[7 * kBlock] = fbits(1.00029f);
          ps[11 * kBlock] = fj * a.num_slots + sl;   // the global slot; prevDiffuse 0
          bounce = 0;
          begin_nearest(sc, h, tr, phase);
        }
      }
      pool_next += take;
    }
    if (!__any(phase != 0)) break;   // every lane idle and no samples left

    // ---- traversal rounds until enough lanes have finished their query
    bool fin = phase != 0 && trav_done(tr);
    for (;;) {
      // a finished shadow query needs no shading: its light sample is added
      // (lightSamplingHandler, Shaders.metal:214-231) and the path's next
      // nearest query starts at once, inside the traversal loop, so service
      // rounds (whose shading cost is the same however few lanes they shade)
      // are spent on finished nearest queries only
      if (fin && phase == 2) {
        MRT_TRACE(ps[11 * kBlock], "TR O inline b=%u occluded=%d\n", bounce, (int)occluded);
        if (!occluded) {
          ps[3 * kBlock] = fbits(bitsf(ps[3 * kBlock]) + h.u);
          ps[4 * kBlock] = fbits(bitsf(ps[4 * kBlock]) + h.v);
          ps[5 * kBlock] = fbits(bitsf(ps[5 * kBlock]) + bitsf(h.prim));
        }
        bounce += 1;
        atomicAdd(&s_count[bounce - 1], 1u);   // stats: rays alive at the start of this bounce
        rd = mk(bitsf(ps[8 * kBlock]), bitsf(ps[9 * kBlock]), bitsf(ps[10 * kBlock]));
        begin_nearest(sc, h, tr, phase);
        fin = trav_done(tr);
      }
      // (phase 3 — the last-bounce light shortcut's occlusion query — no
      // longer occurs here; this check of it stays because without it the
      // compiler allocates the kernel worse: SGPR spills 26 -> 34, scratch
      // 20 -> 36 B per lane, r6)
      if (fin && phase == 3) {
        h.found = !occluded;
        phase = 1;
      }
      const uint64_t going = __ballot(phase != 0 && !fin);
      if (!going) break;
      if ((uint32_t)__popcll(__ballot(fin)) >= (exhausted ? 1u : (uint32_t)MRT_PATH_SERVICE)) break;
      LS_ADD(22, 1);
      LS_ADD(23, (uint32_t)__popcll(going));
      if (phase != 0 && !fin) {
        const RayBox rb = make_raybox(ro, rd);
#if MRT_TRACE_PX
        const bool trl = phase == 1 && bounce == MRT_TRACE_B && trace_lane(a, ps[11 * kBlock]);
#else
        const bool trl = false;
#endif
        trav_round<STACK, MODE>(sc, cx, ro, rd, rb, h, phase >= 2, target, occluded, tr, nullptr, trl);
        fin = trav_done(tr);
      }
    }
    if (!__any(fin)) continue;
    LS_ADD(20, 1);
    LS_ADD(21, (uint32_t)__popcll(__ballot(fin)));

    // ---- service: finished shadow queries (MPS nearest hit + lightSamplingHandler,
    //      Shaders.metal:214-231), then the path's next bounce
    bool next_query = false;
    if (fin && phase == 2) {
      MRT_TRACE(ps[11 * kBlock], "TR O service b=%u occluded=%d\n", bounce, (int)occluded);
      if (!occluded) {
        ps[3 * kBlock] = fbits(bitsf(ps[3 * kBlock]) + h.u);
        ps[4 * kBlock] = fbits(bitsf(ps[4 * kBlock]) + h.v);
        ps[5 * kBlock] = fbits(bitsf(ps[5 * kBlock]) + bitsf(h.prim));
      }
      next_query = true;
    }
    // ---- service: finished nearest queries (intersectionHandler, Shaders.metal:105-212)
    if (fin && phase == 1) {
      PathState s;
      s.o = ro;
      s.d = rd;
      s.T = mk(bitsf(ps[0 * kBlock]), bitsf(ps[1 * kBlock]), bitsf(ps[2 * kBlock]));
      s.R = mk(bitsf(ps[3 * kBlock]), bitsf(ps[4 * kBlock]), bitsf(ps[5 * kBlock]));
      s.pdf = bitsf(ps[6 * kBlock]);
      s.ior = bitsf(ps[7 * kBlock]);
      const uint32_t tagv = ps[11 * kBlock];
      s.prevDiffuse = (tagv >> 31) ? 1.0f : 0.0f;
      const uint32_t gslot = tagv & 0x7FFFFFFFu;
      const bool last = bounce + 1 == L;
      const bool hit_ok = h.found && !(h.t < kDistanceEpsilon);   // :122-126
      MRT_TRACE(tagv, "TR N b=%u found=%d t=%08x prim=%u u=%08x v=%08x o=%08x %08x %08x d=%08x %08x %08x\n", bounce,
                (int)h.found, fbits(h.t), h.prim, fbits(h.u), fbits(h.v), fbits(ro.x), fbits(ro.y), fbits(ro.z),
                fbits(rd.x), fbits(rd.y), fbits(rd.z));
      ShadowRay sh;
      sh.valid = false;
      LS_ADD(13, (uint32_t)__popcll(__ballot(hit_ok)));
      if (hit_ok) {
        const uint32_t fj = a.batch == 1u ? 0u : mdiv(gslot, a.div_slots, a.num_slots);
        uint32_t x, y;
        slot_pixel_l<LIST>(gslot - fj * a.num_slots, a, x, y);
        const uint32_t back = (bounce % 3u) == 0 ? 0u : ((bounce % 3u) == 1 ? 2u : 1u);
        const float4 ns = noise_table(a, fj, back)[shade_noise_cell(x, y, bounce, a.frame_index + fj)];
        shade_hit<MODE>(sc, cx, h, s, ns, bounce, L, !last, sh, (a.flags & kShadeDebugMaterial) != 0);
      }
      if (!hit_ok || last) {   // the path ends: accumulateImage input (Shaders.metal:233-249)
        // streamed once to the accumulate pass: a non-temporal store, so the
        // 2 GB of radiance per launch do not evict BVH lines from L2 (C4
        // +1.2 %, 1960 -> 1984 Mpaths/s, A/B twice in one call)
        typedef float v4f __attribute__((ext_vector_type(4)));
        __builtin_nontemporal_store(v4f{s.R.x, s.R.y, s.R.z, 0.0f}, reinterpret_cast<v4f*>(a.radiance + gslot));
        MRT_TRACE(tagv, "TR E b=%u R=%08x %08x %08x\n", bounce, fbits(s.R.x), fbits(s.R.y), fbits(s.R.z));
        phase = 0;
      } else {
        ps[0 * kBlock] = fbits(s.T.x); ps[1 * kBlock] = fbits(s.T.y); ps[2 * kBlock] = fbits(s.T.z);
        ps[3 * kBlock] = fbits(s.R.x); ps[4 * kBlock] = fbits(s.R.y); ps[5 * kBlock] = fbits(s.R.z);
        ps[6 * kBlock] = fbits(s.pdf); ps[7 * kBlock] = fbits(s.ior);
        ps[8 * kBlock] = fbits(s.d.x); ps[9 * kBlock] = fbits(s.d.y); ps[10 * kBlock] = fbits(s.d.z);
        ps[11 * kBlock] = gslot | (s.prevDiffuse != 0.0f ? 0x80000000u : 0u);
        ro = s.o;   // the next ray's origin (also the shadow ray's, below)
        // the shadow ray: MPS nearest hit == target test + occlusion query
        // (MRT_DEBUG bit 1, ablation only: no shadow queries)
        bool shadow = false;
        if (sh.valid && !(a.debug & 1u)) {
          const float4 P1 = fetch_prim<MODE>(sc, cx, sh.target, 1);   // .w: the target's light index
          const V3 p0 = mk(fetch_prim<MODE>(sc, cx, sh.target, 0)), p1 = mk(P1);
          const V3 p2 = mk(fetch_prim<MODE>(sc, cx, sh.target, 2));
          float tT, u, v;
          const int32_t sroot = shadow_root_select(sc, ro, sh.graze);
          if (tri_test(ro, sh.d, p0, sub(p1, p0), sub(p2, p0), 0.0f, __builtin_inff(), tT, u, v) &&
              !(tT < kDistanceEpsilon) && !origin_occludes<MODE>(sc, cx, ro, sh.d, h.prim, sh.target, tT) &&
              !(sc.occ_lights && sroot == sc.occ_root &&
                lights_occlude<MODE>(sc, cx, ro, sh.d, sh.target, fbits(P1.w), tT))) {
            shadow = true;
            phase = 2;
            MRT_TRACE(tagv, "TR S b=%u target=%u tT=%08x root=%d L=%08x %08x %08x\n", bounce, sh.target, fbits(tT),
                      sroot, fbits(sh.L.x), fbits(sh.L.y), fbits(sh.L.z));
            rd = sh.d;   // ro = s.o = sh.o
            trav_begin(sroot, tr);
            h.t = tT;
            h.u = sh.L.x;
            h.v = sh.L.y;
            h.prim = fbits(sh.L.z);
            h.found = false;
            target = sh.target;
            occluded = false;
          }
        }
        next_query = !shadow;
      }
    }
    // ---- the path's next bounce: its nearest-hit query
    if (next_query) {
      bounce += 1;
      atomicAdd(&s_count[bounce - 1], 1u);   // stats: rays alive at the start of this bounce
      // ro already holds the next ray's origin (set at shading, unchanged by a shadow query)
      rd = mk(bitsf(ps[8 * kBlock]), bitsf(ps[9 * kBlock]), bitsf(ps[10 * kBlock]));
      begin_nearest(sc, h, tr, phase);
    }
  }
  __syncthreads();
  if (tid < 64 && tid + 1 < L && s_count[tid]) atomicAdd(a.bounce_counts + tid, s_count[tid]);
  LS_FLUSH();
  span_end(a);
}

}}}  // namespace mrt::MRT_NS::(anonymous)
