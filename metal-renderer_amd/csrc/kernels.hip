// kernels.hip — gfx950 kernels of the path-tracing hot path: the translation
// unit, with the host-side launch and dispatch code.  The device code is in
// the headers it includes, by stage: dev_config.h (build selection, tunables),
// dev_diag.h (diagnostic builds), dev_math.h, dev_lds.h, dev_traverse.h,
// dev_sweep.h, dev_shadow.h, dev_shade.h, and the kernels kern_bounce.h,
// kern_stream.h, kern_path.h, kern_stage.h, kern_adaptive.h.
//
// Compiled twice (see kernels.h): MRT_PRECISE=1 -> namespace mrt::precise,
// MRT_PRECISE=0 -> mrt::fast.  Every device function restates one
// reference function; the citation is on the function.  Evaluation order of
// every float expression follows the reference source so the precise build is
// bit-comparable with the CPU oracle.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdlib>
#include <type_traits>
#include <vector>

#include "diag_env.h"
#include "kernels.h"
#include "kern_adaptive.h"
#include "kern_bounce.h"
#include "kern_path.h"
#include "kern_stage.h"
#include "kern_stream.h"

namespace mrt {
namespace MRT_NS {
namespace {

inline uint32_t blocks_for(uint32_t n) { return (n + kBlock - 1) / kBlock; }

constexpr size_t kAllLdsBudget = 48 * 1024;   // scene bytes staged whole in LDS

int choose_mode(const DeviceScene& sc) {
  static const int forced = [] {   // MRT_MODE=0/1/2 forces kGlobal/kTopLds/kAllLds (profiling)
    const char* v = mrt::diag_env("MRT_MODE");
    return v ? std::atoi(v) : -1;
  }();
  if (forced >= 0 && forced <= 2) return forced;
  if ((size_t)lds_scene_float4s(kAllLds, sc) * 16 <= kAllLdsBudget)
    return kAllLds;
  return sc.lds_nodes > 0 ? kTopLds : kGlobal;
}

// the current device's CU count: what every persistent grid is sized from
hipError_t device_cus(uint32_t* cus) {
  int dev = 0;
  hipError_t e = hipGetDevice(&dev);
  if (e != hipSuccess) return e;
  hipDeviceProp_t prop;
  e = hipGetDeviceProperties(&prop, dev);
  if (e == hipSuccess) *cus = (uint32_t)prop.multiProcessorCount;
  return e;
}

// The stack variant of a stage kernel that walks the tree (intersect, guides)
// over `count` rays: the whole stack in LDS (STACK = kMaxStack, a block per
// kBlock rays) while the tree's depth allows, else 32 LDS entries + the global
// spill buffer on the capped persistent grid (STACK = -32), which needs `spill`.
struct StageStack {
  bool whole;      // the kMaxStack form
  uint32_t grid;
  size_t lds;      // bytes of dynamic LDS
};
hipError_t stage_stack(const DeviceScene& sc, uint32_t count, const uint32_t* spill, StageStack* v) {
  v->whole = sc.max_stack <= (uint32_t)kMaxStack;
  if (!v->whole && !spill) return hipErrorInvalidValue;
  v->grid = v->whole ? blocks_for(count) : std::min<uint32_t>(blocks_for(count), kIntersectSpillGrid);
  v->lds = (size_t)(v->whole ? kMaxStack : 32) * kBlock * 4;
  return hipSuccess;
}

// ---- the persistent kernels' host side: one skeleton for the three kinds of
// kernel_plan.h.  A unit instantiates a kind's kernels only where it names the
// kind (the split fast build: the stream kernel in its own unit, below). ----

// A block's dynamic LDS: the scene image, the stack (`stack` = |STACK| entries
// per lane) and the kind's own words — path: 16 B and the per-lane path
// state; bounce: the segment counts of a grid of `grid` blocks (2 classes) +
// sentinel; stream: the sentinel alone (no segment scratch)
size_t lds_bytes(KernelKind kind, const DeviceScene& sc, int mode, uint32_t stack, uint32_t grid) {
  const size_t scene = (size_t)lds_scene_float4s(mode, sc) * 16;
  const size_t own = kind == KernelKind::Path ? 16 + (size_t)kPathStateWords * kBlock * 4
                                              : ((size_t)2 * (kind == KernelKind::Bounce ? grid : 0) + 1 + 3) / 4 * 16;
  return scene + own + (size_t)stack * kBlock * 4;
}

// kTopLds: stage only as many top BVH nodes as keep the block's LDS within
// 1/n of the CU less a 2-KB margin for allocation granularity (the VGPR budget
// allows n = MRT_BOUNCE_WAVES resident blocks of 4 waves, the path kernel's
// MRT_PATH_WAVES); the BFS order makes any prefix the top levels.  Full
// occupancy beats more staged nodes (at 6 blocks/CU: C4 with 80 nodes 828,
// ~100 nodes (at the edge) 780, 128 nodes 715 Mpaths/s).
DeviceScene fit_lds_nodes(KernelKind kind, const DeviceScene& sc, int mode, uint32_t stack, uint32_t grid) {
  if (mode != kTopLds) return sc;
  DeviceScene f = sc;
  const bool path = kind == KernelKind::Path;
  const size_t target = 160 * 1024 / (path ? MRT_PATH_WAVES : MRT_LDS_BLOCKS) - 2048;
  // own words + stack + static (the path kernel's s_count, s_closed: + 256)
  const size_t fixed = lds_bytes(kind, sc, kGlobal, stack, grid) + 64 + (path ? 256 : 0);
  const size_t node_bytes = (size_t)node_float4s(sc.width) * 16;
  const size_t fit = fixed < target ? (target - fixed) / node_bytes : 0;
  f.lds_nodes = (uint32_t)std::min<size_t>(sc.lds_nodes, fit);
  return f;
}

// kind K's kernel; a moved camera runs the CAM instantiation, a tile list the
// LIST one (same launch bounds and LDS; the per-bounce kernel has no LIST)
template <KernelKind K, int STACK, int MODE, bool CAM = false, bool LIST = false>
constexpr auto kernel_of() -> void (*)(DeviceScene, BounceArgs) {
  if constexpr (K == KernelKind::Path) return path_kernel<STACK, MODE, CAM, LIST>;
  else if constexpr (K == KernelKind::Stream) return stream_kernel<STACK, MODE, CAM, LIST>;
  else return bounce_kernel<STACK, MODE, CAM>;
}

// the instantiation a launch's arguments select; null: there is none
template <KernelKind K, int STACK, int MODE>
auto kernel_for(const BounceArgs& a) -> void (*)(DeviceScene, BounceArgs) {
  if constexpr (K == KernelKind::Bounce) {
    if (a.tile_list) return nullptr;   // the per-bounce kernel (MRT_DIAG builds of a renderer) has no LIST instantiation
    return a.camera ? kernel_of<K, STACK, MODE, true>() : kernel_of<K, STACK, MODE>();
  } else {
    if (a.tile_list) return a.camera ? kernel_of<K, STACK, MODE, true, true>() : kernel_of<K, STACK, MODE, false, true>();
    return a.camera ? kernel_of<K, STACK, MODE, true>() : kernel_of<K, STACK, MODE>();
  }
}

template <KernelKind K, int STACK, int MODE>
hipError_t launch_t(const DeviceScene& sc, const BounceArgs& a, uint32_t grid, hipStream_t s) {
  const uint32_t stack = STACK < 0 ? -STACK : STACK;
  const DeviceScene f = fit_lds_nodes(K, sc, MODE, stack, grid);
  const size_t lds = lds_bytes(K, f, MODE, stack, grid);
  const auto kernel = kernel_for<K, STACK, MODE>(a);
  if (!kernel) return hipErrorNotSupported;
  kernel<<<dim3(grid), dim3(kBlock), lds, s>>>(f, a);
  return hipGetLastError();
}

// Resident blocks per CU of K's <STACK, MODE> kernel at its LDS for a grid of
// `grid` blocks, taken from the CAM = false, LIST = false instantiation; 0: unknown
template <KernelKind K, int STACK, int MODE>
int occupancy(const DeviceScene& sc, uint32_t grid) {
  const uint32_t stack = STACK < 0 ? -STACK : STACK;
  const size_t lds = lds_bytes(K, fit_lds_nodes(K, sc, MODE, stack, grid), MODE, stack, grid);
  int occ = 0;
  if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&occ, kernel_of<K, STACK, MODE>(), kBlock, lds) != hipSuccess) occ = 0;
  return occ;
}

// the persistent grid: every block slot the kernel's LDS and registers leave
// on a CU, at most 8 (one launch at a time; the dynamic work distribution
// leaves no tail to fill)
template <KernelKind K, int STACK, int MODE>
hipError_t grid_t(const DeviceScene& sc, uint32_t* grid) {
  uint32_t cus = 0;
  const hipError_t e = device_cus(&cus);
  if (e != hipSuccess) return e;
  if constexpr (K == KernelKind::Bounce) {
    // the LDS scratch (2 segment counts per block) depends on the grid: take
    // the largest blocks/CU n whose own LDS footprint still allows n resident
    // blocks (and the VGPR budget allows)
    uint32_t n = 1;
    for (uint32_t want = 8; want >= 1; --want)
      if (occupancy<K, STACK, MODE>(sc, cus * want) >= (int)want) { n = want; break; }
    *grid = cus * n;
  } else {
    const int occ = std::max(occupancy<K, STACK, MODE>(sc, 0), 1);
    // stream: one block slot per CU is left to the other render stream's launch
    // and the accumulate kernel (MRT_STREAM_SPARE): with 6-wave registers the
    // kernel fits 6 blocks per CU, and 5 of them persistent measured best —
    // C2 11937 vs 11740 Mpaths/s with all 6 (1344 / 1408 blocks: within
    // ±0.3 %), per-frame draws 9585 vs 8856 (r5, alternating in one call)
    const int spare = K == KernelKind::Stream && occ > 1 ? MRT_STREAM_SPARE : 0;
    *grid = cus * (uint32_t)std::min(occ - spare, 8);
  }
  return hipSuccess;
}

// the kind has a kernel for this scene with the plan's stack_entries (the
// stream kernel: whole-scene-in-LDS scenes, the whole stack in LDS)
bool variant_ok(KernelKind kind, const DeviceScene& sc, uint32_t stack_entries) {
  return sc.width == 4 && run_stack(kind, stack_entries, sc.max_stack > stack_entries) != 0 &&
         (kind != KernelKind::Stream || choose_mode(sc) == kAllLds);
}

// The one turn from run time to template arguments: op.run<STACK, MODE>() for
// the kernel K runs for this scene with the plan's stack_entries — STACK from
// the kind's list (kernel_plan.h: every entry is instantiated here, and nothing
// else), MODE by choose_mode (the stream kernel: whole-scene-in-LDS scenes only)
template <KernelKind K, int STACK, class Op>
hipError_t for_mode(int mode, const Op& op) {
  if (K == KernelKind::Stream || mode == kAllLds) return op.template run<STACK, kAllLds>();
  if constexpr (K != KernelKind::Stream)
    return mode == kTopLds ? op.template run<STACK, kTopLds>() : op.template run<STACK, kGlobal>();
  else
    return hipErrorNotSupported;
}
template <KernelKind K, class Op>
hipError_t for_stack(StackList<>, int, int, const Op&) {
  return hipErrorInvalidValue;
}
template <KernelKind K, class Op, int S0, int... S>
hipError_t for_stack(StackList<S0, S...>, int stack, int mode, const Op& op) {
  return stack == S0 ? for_mode<K, S0>(mode, op) : for_stack<K>(StackList<S...>{}, stack, mode, op);
}
template <KernelKind K, class Op>
hipError_t with_variant(const DeviceScene& sc, uint32_t stack_entries, const Op& op) {
  if (!variant_ok(K, sc, stack_entries)) return K == KernelKind::Stream ? hipErrorNotSupported : hipErrorInvalidValue;
  return for_stack<K>(stacks_of<K>(), run_stack(K, stack_entries, sc.max_stack > stack_entries), choose_mode(sc), op);
}

// the two things the host does with an instantiation
template <KernelKind K>
struct LaunchOp {
  const DeviceScene& sc;
  const BounceArgs& a;
  uint32_t grid;
  hipStream_t s;
  template <int STACK, int MODE> hipError_t run() const { return launch_t<K, STACK, MODE>(sc, a, grid, s); }
};
template <KernelKind K>
struct GridOp {
  const DeviceScene& sc;
  uint32_t* grid;
  template <int STACK, int MODE> hipError_t run() const { return grid_t<K, STACK, MODE>(sc, grid); }
};

template <KernelKind K>
hipError_t launch_of(const DeviceScene& sc, const BounceArgs& a, uint32_t stack_entries, uint32_t grid, hipStream_t s) {
  if (K == KernelKind::Stream && a.max_path_length > kStreamMaxL) return hipErrorNotSupported;
  return with_variant<K>(sc, stack_entries, LaunchOp<K>{sc, a, grid, s});
}
template <KernelKind K>
hipError_t grid_of(const DeviceScene& sc, uint32_t stack_entries, uint32_t* grid) {
  return with_variant<K>(sc, stack_entries, GridOp<K>{sc, grid});
}

}  // namespace

// the stream kernel's unit (below), which the kind switch of the main unit calls across
hipError_t stream_unit_grid(const DeviceScene& sc, uint32_t stack_entries, uint32_t* grid);
hipError_t stream_unit_launch(const DeviceScene& sc, const BounceArgs& a, uint32_t stack_entries, uint32_t grid,
                              hipStream_t s);

// Translation units (Makefile): MRT_TU 0 = every entry point (precise and
// diagnostic builds); the fast build is split in two — MRT_TU 1 everything
// but the stream kernel, MRT_TU 2 the stream kernel alone, compiled with the
// max-ILP machine scheduler (-amdgpu-sched-strategy=max-ilp: C2 +0.45 %,
// alternating in one call, while the path kernel loses 0.5 % under it).
// The persistent kernels' entry points come first, launch before grid and path
// before bounce (in the stream unit, at the end of the file, grid before
// launch): a unit's kernels are instantiated, and laid out in its code object,
// in the order the host code first names them, and this order reproduces the
// code objects of the dispatch this skeleton replaced byte for byte.
#if MRT_EMIT_MAIN
bool kernel_supported(KernelKind kind, const DeviceScene& sc, uint32_t stack_entries) {
  return variant_ok(kind, sc, stack_entries);
}

hipError_t launch_kernel(KernelKind kind, const DeviceScene& sc, const BounceArgs& a, uint32_t stack_entries,
                         uint32_t grid, hipStream_t s) {
  switch (kind) {
    case KernelKind::Path: return launch_of<KernelKind::Path>(sc, a, stack_entries, grid, s);
    case KernelKind::Bounce: return launch_of<KernelKind::Bounce>(sc, a, stack_entries, grid, s);
    case KernelKind::Stream: return stream_unit_launch(sc, a, stack_entries, grid, s);
  }
  return hipErrorInvalidValue;
}

hipError_t kernel_grid(KernelKind kind, const DeviceScene& sc, uint32_t stack_entries, uint32_t* grid) {
  switch (kind) {
    case KernelKind::Path: return grid_of<KernelKind::Path>(sc, stack_entries, grid);
    case KernelKind::Bounce: return grid_of<KernelKind::Bounce>(sc, stack_entries, grid);
    case KernelKind::Stream: return stream_unit_grid(sc, stack_entries, grid);
  }
  return hipErrorInvalidValue;
}

bool path_preferred(const DeviceScene& sc) { return choose_mode(sc) != kAllLds; }

hipError_t launch_raygen(uint32_t W, uint32_t H, const float* noise, RefRay* rays, const CameraBlock* cam,
                         hipStream_t s) {
  raygen_kernel<<<dim3(blocks_for(W * H)), dim3(kBlock), 0, s>>>(W, H,
                     reinterpret_cast<const float4*>(noise), rays, cam ? *cam : CameraBlock{}, cam ? 1u : 0u);
  return hipGetLastError();
}

hipError_t launch_intersect(const DeviceScene& sc, const void* rays, uint32_t stride, uint32_t count,
                            RefIntersection* out, uint32_t* spill, hipStream_t s) {
  if (count == 0) return hipSuccess;
  if (sc.width != 4) return hipErrorInvalidValue;
  const uint8_t* r = reinterpret_cast<const uint8_t*>(rays);
  StageStack v;
  const hipError_t e = stage_stack(sc, count, spill, &v);
  if (e != hipSuccess) return e;
  if (v.whole) intersect_kernel<kMaxStack><<<dim3(v.grid), dim3(kBlock), v.lds, s>>>(sc, r, stride, count, out, nullptr);
  else intersect_kernel<-32><<<dim3(v.grid), dim3(kBlock), v.lds, s>>>(sc, r, stride, count, out, spill);
  return hipGetLastError();
}

hipError_t launch_guides(const DeviceScene& sc, uint32_t W, uint32_t H, const CameraBlock* cam, float* guide_n,
                         float* guide_p, uint32_t* spill, hipStream_t s) {
  if (sc.width != 4 || (cam && cam->lens_radius != 0.0f)) return hipErrorInvalidValue;
  float4* gn = reinterpret_cast<float4*>(guide_n);
  float4* gp = reinterpret_cast<float4*>(guide_p);
  const CameraBlock cb = cam ? *cam : CameraBlock{};
  const uint32_t moved = cam ? 1u : 0u, count = W * H;
  StageStack v;
  const hipError_t e = stage_stack(sc, count, spill, &v);
  if (e != hipSuccess) return e;
  if (v.whole) guide_kernel<kMaxStack><<<dim3(v.grid), dim3(kBlock), v.lds, s>>>(sc, W, H, cb, moved, gn, gp, nullptr);
  else guide_kernel<-32><<<dim3(v.grid), dim3(kBlock), v.lds, s>>>(sc, W, H, cb, moved, gn, gp, spill);
  return hipGetLastError();
}

hipError_t launch_shade(const DeviceScene& sc, uint32_t W, uint32_t H, uint32_t frame_index, uint32_t max_path_length,
                        const float* noise, const RefIntersection* isect, RefRay* rays, RefShadowRay* srays,
                        uint32_t flags, hipStream_t s) {
  shade_kernel<<<dim3(blocks_for(W * H)), dim3(kBlock), 0, s>>>(sc, W, H, frame_index,
                     max_path_length, reinterpret_cast<const float4*>(noise), isect, rays, srays, flags);
  return hipGetLastError();
}

hipError_t launch_resolve(uint32_t count, const RefIntersection* isect, RefRay* rays, const RefShadowRay* srays,
                          hipStream_t s) {
  if (count == 0) return hipSuccess;
  resolve_kernel<<<dim3(blocks_for(count)), dim3(kBlock), 0, s>>>(count, isect, rays, srays);
  return hipGetLastError();
}

hipError_t launch_accumulate(uint32_t W, uint32_t H, uint32_t frame_index, const RefRay* rays, float* image,
                             bool accumulate, hipStream_t s) {
  accumulate_kernel<<<dim3(blocks_for(W * H)), dim3(kBlock), 0, s>>>(W, H, frame_index, rays,
                     reinterpret_cast<float4*>(image), accumulate);
  return hipGetLastError();
}

hipError_t launch_accumulate_frame(const AccumArgs& a, hipStream_t s) {
  const uint32_t blocks = std::max<uint32_t>(1, std::min<uint32_t>(blocks_for(a.num_slots), 4096));
  if (a.moments) accumulate_frame_kernel<true><<<dim3(blocks), dim3(kBlock), 0, s>>>(a);
  else accumulate_frame_kernel<false><<<dim3(blocks), dim3(kBlock), 0, s>>>(a);
  return hipGetLastError();
}

hipError_t launch_accumulate_counted(const AccumArgs& a, hipStream_t s) {
  if (!a.tile_list || !a.moments) return hipErrorInvalidValue;
  const uint32_t blocks = std::max<uint32_t>(1, std::min<uint32_t>(blocks_for(a.num_slots), 4096));
  accumulate_counted_kernel<<<dim3(blocks), dim3(kBlock), 0, s>>>(a);
  return hipGetLastError();
}

hipError_t launch_counted_merge(const MergeArgs& a, hipStream_t s) {
  if (a.count == 0) return hipErrorInvalidValue;
  counted_merge_kernel<<<dim3(blocks_for(a.count)), dim3(kBlock), 0, s>>>(a);
  return hipGetLastError();
}

hipError_t launch_tile_priority(const PriorityArgs& a, uint32_t tiles, hipStream_t s) {
  if (tiles == 0 || a.tiles_x == 0) return hipErrorInvalidValue;
  tile_priority_kernel<<<dim3(tiles), dim3(kBlock), 0, s>>>(a);
  return hipGetLastError();
}

hipError_t launch_tile_select(const float* priority, uint32_t tiles, uint32_t count, uint32_t* list, hipStream_t s) {
  if (count == 0 || count > tiles || tiles > kMaxSelectTiles) return hipErrorInvalidValue;
  tile_select_kernel<<<dim3(blocks_for(tiles)), dim3(kBlock), 0, s>>>(priority, tiles, count, list);
  return hipGetLastError();
}

hipError_t launch_tile_error(const ErrorArgs& a, uint32_t tiles, hipStream_t s) {
  if (tiles == 0 || a.p.tiles_x == 0) return hipErrorInvalidValue;
  tile_error_kernel<<<dim3(tiles), dim3(kBlock), 0, s>>>(a);
  return hipGetLastError();
}

hipError_t launch_tile_threshold(const ThresholdArgs& a, hipStream_t s) {
  if (a.tiles == 0 || a.tiles > kMaxSelectTiles || a.max_count == 0 || a.max_count > a.tiles) return hipErrorInvalidValue;
  tile_threshold_kernel<<<dim3(blocks_for(a.tiles)), dim3(kBlock), 0, s>>>(a);
  return hipGetLastError();
}

hipError_t launch_moments(uint32_t W, uint32_t H, uint32_t frame_index, const RefRay* rays, float* moments,
                          hipStream_t s) {
  moments_kernel<<<dim3(blocks_for(W * H)), dim3(kBlock), 0, s>>>(W, H, frame_index, rays,
                     reinterpret_cast<float4*>(moments));
  return hipGetLastError();
}

hipError_t launch_display(const float4* image, const float4* reference, float4* out, uint32_t n, uint32_t flags,
                          float compare_scale, hipStream_t s) {
  if (n == 0) return hipSuccess;
  display_kernel<<<dim3(blocks_for(n)), dim3(kBlock), 0, s>>>(image, reference, out, n, flags, compare_scale);
  return hipGetLastError();
}

hipError_t launch_tiles_move(const float4* src, float4* dst, uint32_t W, uint32_t H, uint32_t rank, uint32_t count,
                             bool pack, hipStream_t s) {
  const uint32_t tx = (W + kTile - 1) / kTile, ty = (H + kTile - 1) / kTile, T = tx * ty;
  const uint32_t owned = rank < T ? (T - rank + count - 1) / count : 0u;
  if (!owned) return hipSuccess;
  const uint32_t blocks = std::min<uint32_t>(4096u, owned * 16u);
  tiles_move_kernel<<<dim3(blocks), dim3(kBlock), 0, s>>>(src, dst, W, H, rank, count, tx, owned, pack);
  return hipGetLastError();
}

// (behind every older launcher: the unit's other kernels keep their place in its code object)
hipError_t launch_guides_motion(const DeviceScene& sc, const float* prev_prims, uint32_t W, uint32_t H,
                                const CameraBlock* cam, float* guide_n, float* guide_p, float* motion_n,
                                float* motion_p, uint32_t* spill, hipStream_t s) {
  if (sc.width != 4 || !prev_prims || (cam && cam->lens_radius != 0.0f)) return hipErrorInvalidValue;
  float4* gn = reinterpret_cast<float4*>(guide_n);
  float4* gp = reinterpret_cast<float4*>(guide_p);
  float4* mn = reinterpret_cast<float4*>(motion_n);
  float4* mp = reinterpret_cast<float4*>(motion_p);
  const float4* pp = reinterpret_cast<const float4*>(prev_prims);
  const CameraBlock cb = cam ? *cam : CameraBlock{};
  const uint32_t moved = cam ? 1u : 0u, count = W * H;
  StageStack v;
  const hipError_t e = stage_stack(sc, count, spill, &v);
  if (e != hipSuccess) return e;
  if (v.whole)
    guide_motion_kernel<kMaxStack><<<dim3(v.grid), dim3(kBlock), v.lds, s>>>(sc, pp, W, H, cb, moved, gn, gp, mn, mp, nullptr);
  else guide_motion_kernel<-32><<<dim3(v.grid), dim3(kBlock), v.lds, s>>>(sc, pp, W, H, cb, moved, gn, gp, mn, mp, spill);
  return hipGetLastError();
}

hipError_t read_wave_times(unsigned long long* out, size_t n) {
#if MRT_STAMPS
  return hipMemcpyFromSymbol(out, HIP_SYMBOL(g_wave_t), std::min(n, (size_t)4 * kStampWaves * kStampFields) * sizeof(unsigned long long));
#else
  for (size_t k = 0; k < n; ++k) out[k] = 0;
  return hipSuccess;
#endif
}

hipError_t read_lane_stats(unsigned long long* out, size_t n, bool reset) {
  for (size_t k = 0; k < n; ++k) out[k] = 0;
#if MRT_LANESTATS
  unsigned long long v[kLaneStats];
  hipError_t e = hipMemcpyFromSymbol(v, HIP_SYMBOL(g_lanes), sizeof(v));
  if (e != hipSuccess) return e;
  for (size_t k = 0; k < n && k < (size_t)kLaneStats; ++k) out[k] = v[k];
  if (reset) {
    for (int k = 0; k < kLaneStats; ++k) v[k] = 0;
    e = hipMemcpyToSymbol(HIP_SYMBOL(g_lanes), v, sizeof(v));
  }
  return e;
#else
  (void)reset;
  return hipSuccess;
#endif
}

hipError_t read_stamps(unsigned long long* out8, bool reset) {
  for (int k = 0; k < 8; ++k) out8[k] = 0;
#if MRT_STAMPS
  // phase cycles and iterations summed over the per-wave records of the last
  // launch of each bounce index
  std::vector<unsigned long long> w((size_t)4 * kStampWaves * kStampFields);
  hipError_t e = hipMemcpyFromSymbol(w.data(), HIP_SYMBOL(g_wave_t), w.size() * sizeof(unsigned long long));
  if (e != hipSuccess) return e;
  for (size_t i = 0; i < (size_t)4 * kStampWaves; ++i) {
    const unsigned long long* r = &w[i * kStampFields];
    for (int k = 0; k < 5; ++k) out8[k] += r[8 + k];
    out8[5] += r[2] & 0xFFFFFFFFull;
  }
  if (reset) {
    std::fill(w.begin(), w.end(), 0ull);
    e = hipMemcpyToSymbol(HIP_SYMBOL(g_wave_t), w.data(), w.size() * sizeof(unsigned long long));
  }
  return e;
#else
  (void)reset;
  return hipSuccess;
#endif
}

#endif  // MRT_EMIT_MAIN
#if MRT_EMIT_STREAM
hipError_t stream_unit_grid(const DeviceScene& sc, uint32_t stack_entries, uint32_t* grid) {
  return grid_of<KernelKind::Stream>(sc, stack_entries, grid);
}

hipError_t stream_unit_launch(const DeviceScene& sc, const BounceArgs& a, uint32_t stack_entries, uint32_t grid,
                              hipStream_t s) {
  return launch_of<KernelKind::Stream>(sc, a, stack_entries, grid, s);
}
#endif  // MRT_EMIT_STREAM

}  // namespace MRT_NS
}  // namespace mrt
