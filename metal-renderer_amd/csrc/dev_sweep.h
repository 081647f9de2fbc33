// dev_sweep.h — the leaf-box sweep of small all-in-LDS scenes, and trace_nearest (sweep or walk)
#pragma once
#include "dev_traverse.h"

namespace mrt { namespace MRT_NS { namespace {

// Leaf-box sweep: the nearest hit of a small all-in-LDS tree without a walk
// (DESIGN §2.1i).  The while-while walk parks a lane's first leaf and pushes
// the rest before any h.t exists, so its culling removes almost nothing in a
// shallow tree and the wave runs as many leaf rounds as its unluckiest lane.
// Phase 1 tests every box of the sweep list (DeviceScene::sweep: one record
// per pair of triangles, sweep_pairs.h; the records are wave-uniform: scalar
// loads into SGPRs, no VGPR or LDS traffic) and keeps, per lane, the two
// nearest records by box entry as packed keys (entry bits with the sign and
// the low five cleared | record id: non-negative floats order as unsigned
// integers, an entry of -0 is +0, and lowering an entry only culls less) and
// the other hit records as a bit mask, both in the lanes that hit only.  The
// precise build tests the lo / hi records with the walk's own slab arithmetic
// in the compiler's exec-masked block; the fast build tests the centre /
// half-extent records (sweep_centre) under v_cmpx with no branch (§2.1m).
// Phase 2 tests the nearest record's triangles, the second key's while its
// entry is within h.t (1 + 2^-11), then the masked ones, lowest id first, each
// culled by its recomputed entry under the same rule.  A masked record's key
// is no smaller than the second key's, so its entry is no smaller than that
// key's lowered one: the first key that is missing or culled ends the lane
// with no pop (§2.1l; h.t only shrinks).  The triangles tested are among those
// whose boxes the ray hits, and a record left out lies behind h.t by more than
// the walk's own slack, so the answer is the walk's: the minimum of (t, prim)
// over the box-hit leaves' triangles, independent of the order and of the
// grouping (§3.1).  The variants that lost — a third key, no early-out,
// selects in every lane, lo / hi records in the fast build — are in DESIGN
// §2.1l, §2.1m and "Retired A/B switches".
__device__ __forceinline__ bool sweep_box(float4 lo, float4 hi, V3 o, const RayBox& rb, float tmin, float& tnear) {
#if MRT_PRECISE
  const float ox = o.x, oy = o.y, oz = o.z, oix = 0.0f, oiy = 0.0f, oiz = 0.0f;
#else
  const float ox = 0.0f, oy = 0.0f, oz = 0.0f, oix = rb.oinv.x, oiy = rb.oinv.y, oiz = rb.oinv.z;
  (void)o;
#endif
  // slab distances are monotone in the plane coordinate: min / max of the
  // pair are the (near, far) planes box4 reads from the ray's quadrant copy
  const float x0 = slab(lo.x, ox, rb.inv.x, oix), x1 = slab(hi.x, ox, rb.inv.x, oix);
  const float y0 = slab(lo.y, oy, rb.inv.y, oiy), y1 = slab(hi.y, oy, rb.inv.y, oiy);
  const float z0 = slab(lo.z, oz, rb.inv.z, oiz), z1 = slab(hi.z, oz, rb.inv.z, oiz);
  tnear = fmaxf(fmaxf(fminf(x0, x1), fminf(y0, y1)), fmaxf(fminf(z0, z1), tmin));
  const float tfar = fminf(fminf(fmaxf(x0, x1), fmaxf(y0, y1)), fmaxf(z0, z1));
  return tnear <= tfar;
}

typedef float SweepRec __attribute__((ext_vector_type(8)));           // one record
typedef const __attribute__((address_space(4))) SweepRec* SweepList;   // constant address space: scalar loads

// Phase 1's slab test on a record of the centre list (sweep_pairs.h
// sweep_phase1_records: c.xyz, bits(id), e.xyz, bits(1 << id), with
// [c - e, c + e] containing the record's padded [lo, hi]): three fma per axis,
// no min / max to order the planes — the half-extent times |inv| is the
// distance from the centre's plane to either, whatever the ray's sign.  One
// rounding more than sweep_box, inside the boxes' padding:
// conservative, which is all phase 1 needs; pop() re-tests with sweep_box.
#if !MRT_PRECISE   // (the precise build keeps the lo / hi records)
__device__ __forceinline__ bool sweep_centre(SweepRec rec, const RayBox& rb, float tmin, float& tnear, float& tfar) {
  const float ax = fmaf(rec[0], rb.inv.x, -rb.oinv.x), ay = fmaf(rec[1], rb.inv.y, -rb.oinv.y),
              az = fmaf(rec[2], rb.inv.z, -rb.oinv.z);
  const float ix = fabsf(rb.inv.x), iy = fabsf(rb.inv.y), iz = fabsf(rb.inv.z);
  tnear = fmaxf(fmaxf(fmaf(-rec[4], ix, ax), fmaf(-rec[5], iy, ay)), fmaxf(fmaf(-rec[6], iz, az), tmin));
  tfar = fminf(fminf(fmaf(rec[4], ix, ax), fmaf(rec[5], iy, ay)), fmaf(rec[6], iz, az));
  return tnear <= tfar;
}
#endif

// the triangles of a record (ref = ka | kb << 16, kb == ka: one): one pair, no loop
template <int MODE>
__device__ __forceinline__ void sweep_leaf(const DeviceScene& sc, const LdsCtx& cx, V3 o, V3 d, float tmin,
                                           uint32_t ref, Hit& h) {
  LS_ADD(4, 1);
  LS_ADD(5, ls_lanes());
  const uint32_t ka = ref & 0xFFFFu, kb = ref >> 16;
  tri_pair_nearest<MODE>(sc, cx, o, d, tmin, ka, kb, kb != ka, h);
}

// CAP (the stream kernel's queue levels): a pass makes at most
// `cap` pops of the rest mask and returns the mask it leaves; the caller puts
// a lane with a non-zero mask back on its queue with h as it stands, and a
// later pass continues it with `resume` = that mask and h = that partial hit.
// A resumed lane rides through phase 1 (wave-uniform) and ignores its keys
// (it never takes their early-out: its mask is what an earlier pass left);
// it spends the key rounds on its next pops, so every pass clears a
// bit of every unfinished lane's mask even with cap = 0.  The tested records
// and the cull rule are those of one uncapped pass, so is the answer.
template <int MODE, bool CAP = false>
__device__ __forceinline__ uint32_t sweep_nearest(const DeviceScene& sc, const LdsCtx& cx, V3 o, V3 d, float tmin,
                                                  Hit& h, uint32_t cap = 0xFFFFFFFFu, uint32_t resume = 0u) {
  const RayBox rb = make_raybox(o, d);
  LS_ADD(0, ls_lanes());
  LS_ADD(1, 1);
  constexpr uint32_t kNone = 0xFFFFFFFFu;
  // two keys, ascending ([2] is never touched; as a two-entry array the kernels' registers are
  // allocated differently, and the code object is kept as it was measured)
  uint32_t key_of[3] = {kNone, kNone, kNone};
  uint32_t rest = 0u;   // in phase 1 every record hit, then those beyond the keys
  const uint32_t n = sc.sweep_leaves;
  // the fast build's centre list stands kSweepLeaves records behind the lo / hi one, in the same buffer
  const SweepList list = (SweepList)(uintptr_t)sc.sweep + (MRT_PRECISE ? 0u : kSweepLeaves);
  // the key's entry mask in a vector register: v_and_or takes one scalar
  // operand, the record id (as a literal the mask costs an instruction of its own per record)
  uint32_t key_mask = 0x7FFFFFE0u;
  asm volatile("" : "+v"(key_mask));
#if MRT_PRECISE
  for (uint32_t i = 0; i < n; ++i) {
    // (no record loaded ahead: the eight more scalar registers of a second
    // record cost the stream kernel scalar spills inside this loop, and the
    // other resident waves cover the load: measured)
    LS_T0();
    const SweepRec rec = list[i];
    LS_T1_LOADED(42, rec[0], rec[7]);
    float te;
    const bool hit = sweep_box(make_float4(rec[0], rec[1], rec[2], rec[3]), make_float4(rec[4], rec[5], rec[6], rec[7]),
                               o, rb, tmin, te);
    const uint32_t bit = 1u << (i & 31u);
    // the bookkeeping runs in the lanes that hit only (a miss changes no key):
    // an exec-masked block of five VALU
    if (hit) {
      // entry bits, sign cleared (-0 sorts first, as +0 does), above the record id
      // (i < n <= kSweepLeaves = 32 is the id as it stands; one v_and_or with the mask from its register)
      uint32_t key = (fbits(te) & key_mask) | i;
      asm volatile("" : "+v"(key));   // (keeps the block: without it the compiler turns it into selects in every lane)
      const uint32_t mid = max(key_of[0], key);
      key_of[0] = min(key_of[0], key);
      key_of[1] = min(key_of[1], mid);
      rest |= bit;
    }
  }
#else
  // The centre list in groups of kSweepUnroll records, then the rest one by
  // one (§2.1t): the loop's add, compare and taken branch come once per group.
  // Still one record in flight, into the same eight scalar registers (a
  // second record's registers cost scalar spills inside this loop, and the
  // other resident waves cover the load: measured, §2.1i).  A record is
  // addressed by a 32-bit byte offset on the list's base; its id and mask bit
  // come from its own words 3 and 7, so no counter is kept beside the offset;
  // exec is saved once in front of the loops: their control is wave-uniform, so
  // every record starts with the exec they were entered with.
  {
    typedef const __attribute__((address_space(4))) char* SweepBytes;
    const SweepBytes base = (SweepBytes)list;
    uint64_t saved;
    asm volatile("s_mov_b64 %[sv], exec" : [sv] "=s"(saved));
    auto record = [&](uint32_t at) {
      LS_T0();
      const SweepRec rec = *(SweepList)(base + at);
      LS_T1_LOADED(42, rec[0], rec[7]);
      float te, tf;
      sweep_centre(rec, rb, tmin, te, tf);
      // the bookkeeping in the lanes that hit only, with no branch: v_cmpx
      // narrows exec to them, the five instructions run (in no lane, if none
      // hit), exec comes back
      uint32_t key, mid;
      asm volatile(
          "v_cmpx_le_f32_e32 vcc, %[te], %[tf]\n\t"
          "v_and_or_b32 %[key], %[te], %[mask], %[id]\n\t"
          "v_or_b32_e32 %[rest], %[bit], %[rest]\n\t"
          "v_max_u32_e32 %[mid], %[k0], %[key]\n\t"
          "v_min_u32_e32 %[k0], %[k0], %[key]\n\t"
          "v_min_u32_e32 %[k1], %[k1], %[mid]\n\t"
          "s_mov_b64 exec, %[sv]"
          : [key] "=&v"(key), [mid] "=&v"(mid), [k0] "+v"(key_of[0]), [k1] "+v"(key_of[1]), [rest] "+v"(rest)
          : [te] "v"(te), [tf] "v"(tf), [mask] "v"(key_mask), [id] "s"(fbits(rec[3])), [bit] "s"(fbits(rec[7])),
            [sv] "s"(saved)
          : "vcc");
    };
    constexpr uint32_t kSweepUnroll = 4;   // (2: +1.0 %, 4: +1.1 %; groups filled up with padding records lost, §2.1t)
    const uint32_t end = (n / kSweepUnroll) * (kSweepUnroll * 32u);
    uint32_t off = 0;
    for (; off < end; off += kSweepUnroll * 32u) {
#pragma unroll
      for (uint32_t u = 0; u < kSweepUnroll; ++u) record(off + u * 32u);
    }
    for (; off < n * 32u; off += 32u) record(off);
  }
#endif
  // the keys' records leave the mask (a missing key is kNone, whose id bits name record 31 — not set, or the first key's own)
  rest &= ~((1u << (key_of[0] & 31u)) | (1u << (key_of[1] & 31u)));
  // the lowest masked record leaves the mask: its triangles, and whether its recomputed entry passes the cull
  auto pop = [&](uint32_t& ref) {
    const uint32_t id = (uint32_t)__ffs((int)rest) - 1u;
    rest &= rest - 1u;
    const float4 blo = g_lds[cx.sweep_base + 2u * id], bhi = g_lds[cx.sweep_base + 2u * id + 1u];
    float te;
    ref = fbits(blo.w);
    return sweep_box(blo, bhi, o, rb, tmin, te) && te <= h.t * kCullScale;
  };
  if (CAP && resume) rest = resume;
#pragma unroll
  for (int round = 0; round < 2; ++round) {   // the key rounds, shared with the resumed lanes' pops
    const uint32_t k = key_of[round];
    // (a missing key's entry bits are a NaN: it fails the cull)
    bool test = round == 0 ? k != kNone : bitsf(k & ~31u) <= h.t * kCullScale;
    uint32_t ref = 0u;
    if (CAP && resume) {
      test = false;
      if (rest) test = pop(ref);
    } else if (test) {
      ref = fbits(g_lds[cx.sweep_base + 2u * (k & 31u)].w);
    } else {
      rest = 0u;   // every masked record lies behind this key
    }
    if (test) sweep_leaf<MODE>(sc, cx, o, d, tmin, ref, h);
  }
  for (uint32_t c = 0; rest && (!CAP || c < cap); ++c) {
    LS_ADD(30, 1);
    LS_ADD(31, ls_lanes());
    uint32_t ref;
    if (pop(ref)) sweep_leaf<MODE>(sc, cx, o, d, tmin, ref, h);
  }
  h.found = h.prim != kNoPrim;   // (not kept up by the leaf tests: tri_pair_nearest)
  return CAP ? rest : 0u;
}

template <int STACK, int MODE>
__device__ __forceinline__ Hit trace_nearest(const DeviceScene& sc, const LdsCtx& cx, V3 o, V3 d, float tmin,
                                             float tmax) {
  Hit h;
  h.t = tmax;
  h.u = h.v = 0.0f;
  h.prim = 0xFFFFFFFFu;
  h.found = false;
  if (MODE == kAllLds && sc.sweep_leaves) {   // wave-uniform (kernel argument)
    sweep_nearest<MODE>(sc, cx, o, d, tmin, h);
    return h;
  }
  traverse<STACK, MODE, false>(sc, cx, o, d, tmin, h, 0u, sc.root);
  return h;
}

}}}  // namespace mrt::MRT_NS::(anonymous)
