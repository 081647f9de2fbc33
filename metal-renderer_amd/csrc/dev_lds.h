// dev_lds.h — the block's LDS image (scene staging, per-lane stack) and the fetches that read it or global memory
#pragma once
#include "dev_math.h"
#include "kernels.h"

namespace mrt { namespace MRT_NS { namespace {

// LDS staging modes:
//   kGlobal  — only the per-lane traversal stack lives in LDS (stage ABI kernels);
//   kTopLds  — the first n BFS-ordered BVH nodes (top levels) are staged in
//              LDS; deeper nodes, leaf triangles and shading records are read
//              from global memory (L2 / Infinity Cache / HBM);
//   kAllLds  — small scenes: every node, leaf triangle, per-primitive shading
//              record, material and light entry is staged in LDS once per
//              block, so traversal and shading never leave the CU.
// LDS image: [nodes][triangles][prims][materials][lights][sweep list][convex face pairs] as float4, then the
// uint32 scratch (segment prefix), then the stack laid out [entry][lane]
// (consecutive lanes hit consecutive banks).  All LDS accesses index the
// __shared__ symbol directly so they lower to ds_read/ds_write (a pointer
// select between LDS and global lowers to flat_load).
enum LdsMode { kGlobal = 0, kTopLds = 1, kAllLds = 2 };
extern __shared__ float4 g_lds[];

struct LdsCtx {
  uint32_t n_lds_nodes;   // nodes [0, n) are in LDS
  uint32_t tri_base;      // float4 offsets (kAllLds)
  uint32_t prim_base;
  uint32_t mat_base;
  uint32_t light_base;
  uint32_t sweep_base;    // the sweep list's records (kAllLds, sc.sweep_leaves of them)
  uint32_t conv_base;     // uint32 offset of the convex solids' face pairs (kAllLds, conv_table_float4s)
  uint32_t scratch_base;  // uint32 offset of the per-block scratch
  uint32_t stack_base;    // uint32 offset of the block's stack slot 0 (lane 0's); lanes add threadIdx.x
  uint32_t* spill;        // stack entries >= STACK: the block's rows of a global [lane][word] spill
                          //   area (null when STACK covers the BVH); lane threadIdx.x's row
  uint32_t spill_lane;    //   starts threadIdx.x * spill_lane words in (one word per entry)
};

__device__ __forceinline__ uint32_t* lds_u32() { return reinterpret_cast<uint32_t*>(g_lds); }

// float4s per staged node: the all-in-LDS BVH4 stages four
// quadrant copies of the six plane rows and the refs row (consecutive copies
// start 28 banks apart, so lanes of different quadrants reading the same node
// row hit disjoint banks)
__host__ __device__ constexpr uint32_t node_stride_f4(int mode, uint32_t node_f4) {
  return (mode == kAllLds && node_f4 == 8) ? kQuadNodeF4 : node_f4;
}

// float4 counts of the staged scene image for a mode
// (node_f4 = float4s per BVH4 node: 8; nodes / tri_records include the
// occluder tree's, prims are the scene's triangles)
__host__ __device__ inline uint32_t lds_scene_float4s(int mode, uint32_t node_f4, uint32_t nodes, uint32_t lds_nodes,
                                                      uint32_t tri_records, uint32_t prims, uint32_t mats,
                                                      uint32_t lights) {
  if (mode == kAllLds) return node_stride_f4(mode, node_f4) * nodes + 3 * tri_records + 6 * prims + 2 * mats + 7 * lights;
  if (mode == kTopLds) return node_f4 * lds_nodes;
  return 0;
}
// the convex solids' face pairs as a table a lane indexes by (solid, face)
// (shadow_plan.h shadow_plan_pair_index: 8 words per solid, faces 6 and 7 hold
// "no triangles"): DeviceScene::conv_face_tris lives in the kernel arguments,
// where only wave-uniform indices are cheap
__host__ __device__ inline uint32_t conv_table_float4s(const DeviceScene& sc) { return 2u * sc.conv_count; }
// both trees' nodes and leaf-triangle records (mrt_layout.h DeviceScene)
__host__ __device__ inline uint32_t scene_nodes(const DeviceScene& sc) { return sc.num_nodes + sc.occ_nodes; }
__host__ __device__ inline uint32_t scene_tri_records(const DeviceScene& sc) { return sc.num_triangles + sc.occ_tris; }
__host__ __device__ inline uint32_t lds_scene_float4s(int mode, const DeviceScene& sc) {
  return lds_scene_float4s(mode, node_float4s(sc.width), scene_nodes(sc), sc.lds_nodes, scene_tri_records(sc),
                           sc.num_triangles, sc.num_materials, sc.num_lights + 1) +
         (mode == kAllLds ? 2 * sc.sweep_leaves + conv_table_float4s(sc) : 0u);   // the sweep list's records (sweep_nearest), the face pairs
}

// 16-B buffer load at a 32-bit byte offset from a wave-uniform descriptor
// (no 64-bit address arithmetic per access); the host keeps every buffer
// read this way below 4 GiB (mrt_scene_create)
__device__ __forceinline__ __amdgpu_buffer_rsrc_t buf_rsrc(const float* base) {
  return __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(base), 0, 0xFFFFFFFF, 0x00020000);
}
__device__ __forceinline__ float4 buf_ld4(__amdgpu_buffer_rsrc_t rs, uint32_t off) {
  const auto v = __builtin_amdgcn_raw_buffer_load_b128(rs, off, 0, 0);
  return make_float4(bitsf(v[0]), bitsf(v[1]), bitsf(v[2]), bitsf(v[3]));
}

template <int MODE>
__device__ __forceinline__ void fetch_node4(const DeviceScene& sc, const LdsCtx& cx, int32_t node, const RayBox& rb,
                                            float4* q) {
  if (MODE == kAllLds) {   // the ray's quadrant copy
    const uint32_t sz = fbits(rb.inv.z) >> 31;
#pragma unroll
    for (int i = 0; i < 4; ++i) q[i] = g_lds[kQuadNodeF4 * node + rb.quad_f4 + i];
    q[4] = g_lds[kQuadNodeF4 * node + rb.quad_f4 + 4 + sz];
    q[5] = g_lds[kQuadNodeF4 * node + rb.quad_f4 + 5 - sz];
    q[6] = g_lds[kQuadNodeF4 * node + rb.quad_f4 + 6];
  } else {
    // top-nodes mode: rows in ray order, (near, far) per axis by the direction's signs
    const bool rowsel = MODE == kTopLds;
    const uint32_t sx = rowsel ? fbits(rb.inv.x) >> 31 : 0u, sy = rowsel ? fbits(rb.inv.y) >> 31 : 0u;
    const uint32_t sz = rowsel ? fbits(rb.inv.z) >> 31 : 0u;
    const uint32_t row[6] = {sx, 1u - sx, 2u + sy, 3u - sy, 4u + sz, 5u - sz};
    if (MODE == kAllLds || (MODE == kTopLds && (uint32_t)node < cx.n_lds_nodes)) {
#pragma unroll
      for (int i = 0; i < 6; ++i) q[i] = g_lds[8 * node + row[i]];
      q[6] = g_lds[8 * node + 6];
    } else {
      // one descriptor over the node array (kernel-argument values: wave-
      // uniform); per row a 32-bit offset node * 128 + row * 16
      const __amdgpu_buffer_rsrc_t rs = buf_rsrc(sc.nodes);
      const uint32_t b = (uint32_t)node << 7;
#pragma unroll
      for (int i = 0; i < 6; ++i) q[i] = buf_ld4(rs, b + (row[i] << 4));
      q[6] = buf_ld4(rs, b + 96u);
    }
  }
}

template <int MODE>
__device__ __forceinline__ void fetch_tri(const DeviceScene& sc, const LdsCtx& cx, uint32_t k, float4& t0,
                                          float4& t1, float4& t2) {
  if (MODE == kAllLds) {
    t0 = g_lds[cx.tri_base + 3 * k];
    t1 = g_lds[cx.tri_base + 3 * k + 1];
    t2 = g_lds[cx.tri_base + 3 * k + 2];
  } else {
    const __amdgpu_buffer_rsrc_t rs = buf_rsrc(sc.tris);
    const uint32_t b = k * 48u;
    t0 = buf_ld4(rs, b);
    t1 = buf_ld4(rs, b + 16u);
    t2 = buf_ld4(rs, b + 32u);
  }
}

template <int MODE>
__device__ __forceinline__ float4 fetch_prim(const DeviceScene& sc, const LdsCtx& cx, uint32_t prim, uint32_t i) {
  if (MODE == kAllLds) return g_lds[cx.prim_base + 6 * prim + i];
  // (buffer loads here measured C4 -4 %, C3 -4.5 %: the shading records stay flat loads)
  return reinterpret_cast<const float4*>(sc.prims)[6 * (size_t)prim + i];
}
template <int MODE>
__device__ __forceinline__ float4 fetch_mat(const DeviceScene& sc, const LdsCtx& cx, uint32_t m, uint32_t i) {
  if (MODE == kAllLds) return g_lds[cx.mat_base + 2 * m + i];
  return reinterpret_cast<const float4*>(sc.materials)[2 * m + i];
}
template <int MODE>
__device__ __forceinline__ float4 fetch_light(const DeviceScene& sc, const LdsCtx& cx, uint32_t l, uint32_t i) {
  if (MODE == kAllLds) return g_lds[cx.light_base + 7 * l + i];
  return reinterpret_cast<const float4*>(sc.lights)[7 * l + i];
}

// STACK = LDS entries per lane; a negative STACK means |STACK| LDS entries
// plus the global spill area for deeper entries.
// A lane's spilled words are contiguous: its pushes and pops keep touching
// the same few cache lines (measured +1.1 % C4, +1.5 % C3 over [entry][lane]).
__device__ __forceinline__ uint32_t spill_index(const LdsCtx& cx, int w) {
  return threadIdx.x * cx.spill_lane + (uint32_t)w;
}
template <int STACK>
__device__ __forceinline__ void stack_push(const LdsCtx& cx, int sp, int32_t v) {
  constexpr int kL = STACK < 0 ? -STACK : STACK;
  if (STACK > 0 || sp < kL) lds_u32()[cx.stack_base + threadIdx.x + sp * kBlock] = (uint32_t)v;
  else cx.spill[spill_index(cx, sp - kL)] = (uint32_t)v;
}
template <int STACK>
__device__ __forceinline__ int32_t stack_get(const LdsCtx& cx, int sp) {
  constexpr int kL = STACK < 0 ? -STACK : STACK;
  if (STACK > 0 || sp < kL) return (int32_t)lds_u32()[cx.stack_base + threadIdx.x + sp * kBlock];
  uint32_t v = cx.spill[spill_index(cx, sp - kL)];
  // keeps the two loads apart: merged, they become one flat load whose wait
  // covers every outstanding global access (the spill stores included)
  asm("" : "+v"(v));
  return (int32_t)v;
}

// Stage the LDS image for `MODE` (every thread of the block calls it);
// `scratch_u32` uint32 words of per-block scratch follow the scene image.
template <int MODE>
__device__ __forceinline__ LdsCtx stage_lds(const DeviceScene& sc, uint32_t scratch_u32, uint32_t* spill = nullptr) {
  LdsCtx cx;
  const uint32_t nf4 = node_float4s(sc.width);   // float4s per node
  const uint32_t n_nodes = (MODE == kAllLds) ? scene_nodes(sc) : (MODE == kTopLds ? sc.lds_nodes : 0u);
  const uint32_t TR = (MODE == kAllLds) ? scene_tri_records(sc) : 0u;   // leaf triangles of both trees
  const uint32_t T = (MODE == kAllLds) ? sc.num_triangles : 0u;          // per-primitive records
  const uint32_t M = (MODE == kAllLds) ? sc.num_materials : 0u;
  const uint32_t NL = (MODE == kAllLds) ? sc.num_lights + 1 : 0u;
  const uint32_t SW = (MODE == kAllLds) ? sc.sweep_leaves : 0u;
  cx.n_lds_nodes = n_nodes;
  const uint32_t node_f4 = node_stride_f4(MODE, nf4);
  const bool copies = node_f4 != nf4;
  cx.tri_base = node_f4 * n_nodes;
  cx.prim_base = cx.tri_base + 3 * TR;
  cx.mat_base = cx.prim_base + 6 * T;
  cx.light_base = cx.mat_base + 2 * M;
  cx.sweep_base = cx.light_base + 7 * NL;
  const uint32_t CV = (MODE == kAllLds) ? conv_table_float4s(sc) : 0u;
  cx.conv_base = 4 * (cx.sweep_base + 2 * SW);
  const uint32_t f4 = cx.sweep_base + 2 * SW + CV;
  cx.scratch_base = 4 * f4;
  cx.stack_base = cx.scratch_base + ((scratch_u32 + 3) & ~3u);
  cx.spill_lane = sc.max_stack;
  cx.spill = spill ? spill + (size_t)blockIdx.x * kBlock * cx.spill_lane : nullptr;
  if (MODE != kGlobal) {
    const float4* src[6] = {reinterpret_cast<const float4*>(sc.nodes), reinterpret_cast<const float4*>(sc.tris),
                            reinterpret_cast<const float4*>(sc.prims), reinterpret_cast<const float4*>(sc.materials),
                            reinterpret_cast<const float4*>(sc.lights), reinterpret_cast<const float4*>(sc.sweep)};
    const uint32_t base[6] = {0u, cx.tri_base, cx.prim_base, cx.mat_base, cx.light_base, cx.sweep_base};
    const uint32_t len[6] = {nf4 * n_nodes, 3 * TR, 6 * T, 2 * M, 7 * NL, 2 * SW};
    for (int r = copies ? 1 : 0; r < 6; ++r)
      for (uint32_t i = threadIdx.x; i < len[r]; i += kBlock) g_lds[base[r] + i] = src[r][i];
    // the face pairs, a word per (solid, face); a per-lane index into the
    // kernel arguments is a vector load from their segment, once per block
    for (uint32_t i = threadIdx.x; i < 4 * CV; i += kBlock)
      lds_u32()[cx.conv_base + i] = (i & 7u) < 6u ? sc.conv_face_tris[i >> 3][i & 7u] : 0xFFFFFFFFu;
    if (copies) {   // quadrant copies: x, y rows (near, far), z rows (lo, hi), refs
      for (uint32_t i = threadIdx.x; i < node_f4 * n_nodes; i += kBlock) {
        const uint32_t node = i / node_f4, rem = i % node_f4;
        const uint32_t quad = rem / kQuadCopyF4, row = rem % kQuadCopyF4;
        const uint32_t axis = row >> 1;
        const uint32_t flip = axis < 2 ? (quad >> axis) & 1u : 0u;
        const uint32_t src_row = row < 6 ? 2 * axis + ((row & 1u) ^ flip) : 6u;
        g_lds[i] = src[0][8 * node + src_row];
      }
    }
    __syncthreads();
  }
  return cx;
}

}}}  // namespace mrt::MRT_NS::(anonymous)
