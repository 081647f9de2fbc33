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

size_t bounce_lds_bytes(const DeviceScene& sc, int mode, uint32_t stack, uint32_t grid) {
  const size_t scene = (size_t)lds_scene_float4s(mode, sc) * 16;
  const size_t scratch = ((size_t)2 * grid + 1 + 3) / 4 * 16;   // segment counts per block (2 classes) + sentinel
  return scene + scratch + (size_t)stack * kBlock * 4;           // stack = LDS entries (|STACK|)
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

#if MRT_EMIT_MAIN   // the per-bounce and path kernels' host side (not in the stream unit)
// kTopLds: stage only as many top BVH nodes as keep the block's LDS within
// 1/MRT_BOUNCE_WAVES of the CU less a 2-KB margin for allocation granularity
// (the VGPR budget allows MRT_BOUNCE_WAVES resident blocks of 4 waves); the
// BFS order makes any prefix the top levels.  Full occupancy beats more
// staged nodes (at 6 blocks/CU: C4 with 80 nodes 828, ~100 nodes (at the
// edge) 780, 128 nodes 715 Mpaths/s).
DeviceScene fit_lds_nodes(const DeviceScene& sc, int mode, uint32_t stack, uint32_t grid) {
  if (mode != kTopLds) return sc;
  DeviceScene f = sc;
  const size_t kLdsPerBlockTarget = 160 * 1024 / MRT_LDS_BLOCKS - 2048;
  const size_t fixed = bounce_lds_bytes(sc, kGlobal, stack, grid) + 64;   // scratch + stack + static
  const size_t node_bytes = (size_t)node_float4s(sc.width) * 16;
  const size_t fit = fixed < kLdsPerBlockTarget ? (kLdsPerBlockTarget - fixed) / node_bytes : 0;
  f.lds_nodes = (uint32_t)std::min<size_t>(sc.lds_nodes, fit);
  return f;
}

template <int STACK, int MODE>
hipError_t grid_for(const DeviceScene& sc, uint32_t blocks_per_cu, uint32_t* grid) {
  uint32_t cus = 0;
  const hipError_t e = device_cus(&cus);
  if (e != hipSuccess) return e;
  // the LDS scratch (2 segment counts per block) depends on the grid: take
  // the largest blocks/CU n whose own LDS footprint still allows n resident
  // blocks (and the VGPR budget allows)
  const int stack = STACK < 0 ? -STACK : STACK;
  int n = 1;
  for (int want = 8; want >= 1; --want) {
    const uint32_t g = cus * (uint32_t)want;
    const size_t lds = bounce_lds_bytes(fit_lds_nodes(sc, MODE, stack, g), MODE, stack, g);
    int occ = 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&occ, bounce_kernel<STACK, MODE>, kBlock, lds) != hipSuccess)
      occ = 0;
    if (occ >= want) { n = want; break; }
  }
  // one launch at a time: every resident block slot (the dynamic work
  // distribution leaves no tail to fill); with frames in flight the caller
  // asks for fewer blocks per CU per launch
  *grid = cus * (blocks_per_cu ? std::min<uint32_t>(n, blocks_per_cu) : (uint32_t)n);
  return hipSuccess;
}

// path kernel: LDS = scene image + stack + the per-lane path state; the
// kTopLds node budget fits MRT_PATH_WAVES resident blocks per CU
size_t path_lds_bytes(const DeviceScene& sc, int mode, uint32_t stack) {
  const size_t scene = (size_t)lds_scene_float4s(mode, sc) * 16;
  return scene + 16 + (size_t)stack * kBlock * 4 + (size_t)kPathStateWords * kBlock * 4;
}
DeviceScene fit_path_lds_nodes(const DeviceScene& sc, int mode, uint32_t stack) {
  if (mode != kTopLds) return sc;
  DeviceScene f = sc;
  const size_t target = 160 * 1024 / MRT_PATH_WAVES - 2048;
  const size_t fixed = path_lds_bytes(sc, kGlobal, stack) + 64 + 256;   // + static (s_count, s_closed)
  const size_t fit = fixed < target ? (target - fixed) / ((size_t)node_float4s(sc.width) * 16) : 0;
  f.lds_nodes = (uint32_t)std::min<size_t>(sc.lds_nodes, fit);
  return f;
}

template <int STACK, int MODE>
hipError_t path_grid_t(const DeviceScene& sc, uint32_t* grid) {
  uint32_t cus = 0;
  const hipError_t e = device_cus(&cus);
  if (e != hipSuccess) return e;
  const int stack = STACK < 0 ? -STACK : STACK;
  const size_t lds = path_lds_bytes(fit_path_lds_nodes(sc, MODE, stack), MODE, stack);
  int occ = 0;
  if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&occ, path_kernel<STACK, MODE>, kBlock, lds) != hipSuccess || occ < 1)
    occ = 1;
  *grid = cus * (uint32_t)std::min(occ, 8);
  return hipSuccess;
}

template <int STACK, int MODE>
hipError_t launch_path_t(const DeviceScene& sc, const BounceArgs& a, uint32_t grid, hipStream_t s) {
  const int stack = STACK < 0 ? -STACK : STACK;
  const DeviceScene f = fit_path_lds_nodes(sc, MODE, stack);
  // (a moved camera: the CAM instantiation, a tile list: the LIST one; same launch bounds and LDS)
  const size_t lds = path_lds_bytes(f, MODE, stack);
  if (a.tile_list) {
    if (a.camera) path_kernel<STACK, MODE, true, true><<<dim3(grid), dim3(kBlock), lds, s>>>(f, a);
    else path_kernel<STACK, MODE, false, true><<<dim3(grid), dim3(kBlock), lds, s>>>(f, a);
  } else if (a.camera) path_kernel<STACK, MODE, true><<<dim3(grid), dim3(kBlock), lds, s>>>(f, a);
  else path_kernel<STACK, MODE><<<dim3(grid), dim3(kBlock), lds, s>>>(f, a);
  return hipGetLastError();
}

template <int STACK>
hipError_t path_dispatch_mode(const DeviceScene& sc, const BounceArgs* a, uint32_t grid, uint32_t* grid_out,
                              hipStream_t s) {
  switch (choose_mode(sc)) {
    case kAllLds:
      return a ? launch_path_t<STACK, kAllLds>(sc, *a, grid, s) : path_grid_t<STACK, kAllLds>(sc, grid_out);
    case kTopLds:
      return a ? launch_path_t<STACK, kTopLds>(sc, *a, grid, s) : path_grid_t<STACK, kTopLds>(sc, grid_out);
    default:
      return a ? launch_path_t<STACK, kGlobal>(sc, *a, grid, s) : path_grid_t<STACK, kGlobal>(sc, grid_out);
  }
}

// LDS stack capacity variants (negative: |STACK| LDS entries + global spill)
hipError_t path_dispatch(const DeviceScene& sc, const BounceArgs* a, uint32_t stack_entries, uint32_t grid,
                         uint32_t* grid_out, hipStream_t s) {
  if (sc.width != 4) return hipErrorInvalidValue;
  if (sc.max_stack > stack_entries) {
    if (stack_entries <= 8) return path_dispatch_mode<-8>(sc, a, grid, grid_out, s);
    if (stack_entries <= 12) return path_dispatch_mode<-12>(sc, a, grid, grid_out, s);
    if (stack_entries <= 16) return path_dispatch_mode<-16>(sc, a, grid, grid_out, s);
    return path_dispatch_mode<-32>(sc, a, grid, grid_out, s);
  }
  if (stack_entries <= 8) return path_dispatch_mode<8>(sc, a, grid, grid_out, s);
  if (stack_entries <= 12) return path_dispatch_mode<12>(sc, a, grid, grid_out, s);
  if (stack_entries <= 16) return path_dispatch_mode<16>(sc, a, grid, grid_out, s);
  if (stack_entries <= 24) return path_dispatch_mode<24>(sc, a, grid, grid_out, s);
  return path_dispatch_mode<32>(sc, a, grid, grid_out, s);
}

template <int STACK, int MODE>
hipError_t launch_bounce_t(const DeviceScene& sc, const BounceArgs& a, uint32_t grid, hipStream_t s) {
  const DeviceScene f = fit_lds_nodes(sc, MODE, STACK < 0 ? -STACK : STACK, grid);
  const size_t lds = bounce_lds_bytes(f, MODE, STACK < 0 ? -STACK : STACK, grid);
  if (a.tile_list) return hipErrorNotSupported;   // the per-bounce kernel (MRT_DIAG builds of a renderer) has no LIST instantiation
  if (a.camera) bounce_kernel<STACK, MODE, true><<<dim3(grid), dim3(kBlock), lds, s>>>(f, a);
  else bounce_kernel<STACK, MODE><<<dim3(grid), dim3(kBlock), lds, s>>>(f, a);
  return hipGetLastError();
}

template <int STACK>
hipError_t dispatch_mode(const DeviceScene& sc, const BounceArgs* a, uint32_t grid, uint32_t* grid_out,
                         hipStream_t s) {
  switch (choose_mode(sc)) {
    case kAllLds:
      return a ? launch_bounce_t<STACK, kAllLds>(sc, *a, grid, s) : grid_for<STACK, kAllLds>(sc, grid, grid_out);
    case kTopLds:
      return a ? launch_bounce_t<STACK, kTopLds>(sc, *a, grid, s) : grid_for<STACK, kTopLds>(sc, grid, grid_out);
    default:
      return a ? launch_bounce_t<STACK, kGlobal>(sc, *a, grid, s) : grid_for<STACK, kGlobal>(sc, grid, grid_out);
  }
}

// stack_entries = LDS stack capacity (8/16/24/32); when the BVH's bound is
// larger, the spill variants (8, 16 or 32 LDS entries + global) are used
hipError_t dispatch(const DeviceScene& sc, const BounceArgs* a, uint32_t stack_entries, uint32_t grid,
                    uint32_t* grid_out, hipStream_t s) {
  if (sc.width != 4) return hipErrorInvalidValue;
  if (sc.max_stack > stack_entries) {
    if (stack_entries <= 8) return dispatch_mode<-8>(sc, a, grid, grid_out, s);
    if (stack_entries <= 16) return dispatch_mode<-16>(sc, a, grid, grid_out, s);
    return dispatch_mode<-32>(sc, a, grid, grid_out, s);
  }
  if (stack_entries <= 8) return dispatch_mode<8>(sc, a, grid, grid_out, s);
  if (stack_entries <= 12) return dispatch_mode<12>(sc, a, grid, grid_out, s);
  if (stack_entries <= 16) return dispatch_mode<16>(sc, a, grid, grid_out, s);
  if (stack_entries <= 24) return dispatch_mode<24>(sc, a, grid, grid_out, s);
  return dispatch_mode<32>(sc, a, grid, grid_out, s);
}

#endif  // MRT_EMIT_MAIN

// wave-local streaming wavefront: whole-scene-in-LDS scenes, the stack in LDS
template <int STACK>
hipError_t launch_stream_t(const DeviceScene& sc, const BounceArgs& a, uint32_t grid, hipStream_t s) {
  const size_t lds = bounce_lds_bytes(sc, kAllLds, STACK, 0);
  if (a.tile_list) {   // the LIST instantiations (dev_shade.h slot_pixel_l)
    if (a.camera) stream_kernel<STACK, kAllLds, true, true><<<dim3(grid), dim3(kBlock), lds, s>>>(sc, a);
    else stream_kernel<STACK, kAllLds, false, true><<<dim3(grid), dim3(kBlock), lds, s>>>(sc, a);
  } else if (a.camera)
    stream_kernel<STACK, kAllLds, true><<<dim3(grid), dim3(kBlock), lds, s>>>(sc, a);
  else
    stream_kernel<STACK, kAllLds><<<dim3(grid), dim3(kBlock), lds, s>>>(sc, a);
  return hipGetLastError();
}
// the stream kernel's own persistent grid: every block slot its LDS (scene
// image + stack, no segment scratch) and registers leave on a CU
template <int STACK>
hipError_t stream_grid_t(const DeviceScene& sc, uint32_t* grid) {
  uint32_t cus = 0;
  const hipError_t e = device_cus(&cus);
  if (e != hipSuccess) return e;
  int occ = 0;
  if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&occ, stream_kernel<STACK, kAllLds>, kBlock,
                                                   bounce_lds_bytes(sc, kAllLds, STACK, 0)) != hipSuccess || occ < 1)
    occ = 1;
  // one block slot per CU is left to the other render stream's launch and
  // the accumulate kernel (MRT_STREAM_SPARE): with 6-wave registers the
  // kernel fits 6 blocks per CU, and 5 of them persistent measured best —
  // C2 11937 vs 11740 Mpaths/s with all 6 (1344 / 1408 blocks: within
  // ±0.3 %), per-frame draws 9585 vs 8856 (r5, alternating in one call)
  const int spare = occ > 1 ? MRT_STREAM_SPARE : 0;
  *grid = cus * (uint32_t)std::min(occ - spare, 8);
  return hipSuccess;
}

bool stream_ok(const DeviceScene& sc, uint32_t stack_entries) {
  return sc.width == 4 && choose_mode(sc) == kAllLds && sc.max_stack <= stack_entries && stack_entries <= 32;
}

}  // namespace

// Translation units (Makefile): MRT_TU 0 = every entry point (precise and
// diagnostic builds); the fast build is split in two — MRT_TU 1 everything
// but the stream kernel, MRT_TU 2 the stream kernel alone, compiled with the
// max-ILP machine scheduler (-amdgpu-sched-strategy=max-ilp: C2 +0.45 %,
// alternating in one call, while the path kernel loses 0.5 % under it).
#if MRT_EMIT_MAIN
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
  if (sc.max_stack <= (uint32_t)kMaxStack) {   // whole stack in LDS
    const size_t lds = (size_t)kMaxStack * kBlock * 4;
    intersect_kernel<kMaxStack><<<dim3(blocks_for(count)), dim3(kBlock), lds, s>>>(sc, r, stride, count, out, nullptr);
  } else {                                      // 32 LDS entries + global spill, persistent grid
    if (!spill) return hipErrorInvalidValue;
    const size_t lds = (size_t)32 * kBlock * 4;
    const dim3 g(std::min<uint32_t>(blocks_for(count), kIntersectSpillGrid));
    intersect_kernel<-32><<<g, dim3(kBlock), lds, s>>>(sc, r, stride, count, out, spill);
  }
  return hipGetLastError();
}

hipError_t launch_guides(const DeviceScene& sc, uint32_t W, uint32_t H, const CameraBlock* cam, float* guide_n,
                         float* guide_p, uint32_t* spill, hipStream_t s) {
  if (sc.width != 4 || (cam && cam->lens_radius != 0.0f)) return hipErrorInvalidValue;
  float4* gn = reinterpret_cast<float4*>(guide_n);
  float4* gp = reinterpret_cast<float4*>(guide_p);
  const CameraBlock cb = cam ? *cam : CameraBlock{};
  const uint32_t moved = cam ? 1u : 0u, count = W * H;
  if (sc.max_stack <= (uint32_t)kMaxStack) {   // as launch_intersect: whole stack in LDS
    const size_t lds = (size_t)kMaxStack * kBlock * 4;
    guide_kernel<kMaxStack><<<dim3(blocks_for(count)), dim3(kBlock), lds, s>>>(sc, W, H, cb, moved, gn, gp, nullptr);
  } else {                                      // 32 LDS entries + global spill, persistent grid
    if (!spill) return hipErrorInvalidValue;
    const size_t lds = (size_t)32 * kBlock * 4;
    const dim3 g(std::min<uint32_t>(blocks_for(count), kIntersectSpillGrid));
    guide_kernel<-32><<<g, dim3(kBlock), lds, s>>>(sc, W, H, cb, moved, gn, gp, spill);
  }
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

hipError_t bounce_grid(const DeviceScene& sc, uint32_t stack_entries, uint32_t blocks_per_cu, uint32_t* grid) {
  // (dispatch passes `grid` through as blocks_per_cu when no launch is given)
  return dispatch(sc, nullptr, stack_entries, blocks_per_cu, grid, nullptr);
}

hipError_t launch_bounce(const DeviceScene& sc, const BounceArgs& a, uint32_t stack_entries, uint32_t grid,
                         hipStream_t s) {
  return dispatch(sc, &a, stack_entries, grid, nullptr, s);
}

hipError_t launch_paths(const DeviceScene& sc, const BounceArgs& a, uint32_t stack_entries, uint32_t grid,
                        hipStream_t s) {
  return path_dispatch(sc, &a, stack_entries, grid, nullptr, s);
}

hipError_t path_grid(const DeviceScene& sc, uint32_t stack_entries, uint32_t* grid) {
  return path_dispatch(sc, nullptr, stack_entries, 0, grid, nullptr);
}

bool path_preferred(const DeviceScene& sc) { return choose_mode(sc) != kAllLds; }

#endif  // MRT_EMIT_MAIN
#if MRT_EMIT_STREAM
bool stream_supported(const DeviceScene& sc, uint32_t stack_entries) { return stream_ok(sc, stack_entries); }

hipError_t stream_grid(const DeviceScene& sc, uint32_t stack_entries, uint32_t* grid) {
  if (!stream_ok(sc, stack_entries)) return hipErrorNotSupported;
  if (stack_entries <= 8) return stream_grid_t<8>(sc, grid);
  if (stack_entries <= 12) return stream_grid_t<12>(sc, grid);
  if (stack_entries <= 16) return stream_grid_t<16>(sc, grid);
  if (stack_entries <= 24) return stream_grid_t<24>(sc, grid);
  return stream_grid_t<32>(sc, grid);
}

hipError_t launch_stream(const DeviceScene& sc, const BounceArgs& a, uint32_t stack_entries, uint32_t grid,
                         hipStream_t s) {
  if (!stream_ok(sc, stack_entries) || a.max_path_length > kStreamMaxL) return hipErrorNotSupported;
  if (stack_entries <= 8) return launch_stream_t<8>(sc, a, grid, s);
  if (stack_entries <= 12) return launch_stream_t<12>(sc, a, grid, s);
  if (stack_entries <= 16) return launch_stream_t<16>(sc, a, grid, s);
  if (stack_entries <= 24) return launch_stream_t<24>(sc, a, grid, s);
  return launch_stream_t<32>(sc, a, grid, s);
}
#endif  // MRT_EMIT_STREAM

}  // namespace MRT_NS
}  // namespace mrt
