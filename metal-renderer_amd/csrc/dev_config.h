// dev_config.h — build selection (precise / fast, translation unit), block size and the numeric tunables
// of the kernels (kernels.hip); every device header starts from this one.
#pragma once

#ifndef MRT_PRECISE
#error "compile with -DMRT_PRECISE=0 or 1"
#endif
#ifndef MRT_TU
#define MRT_TU 0
#endif
// The stream kernel's entry points: in unit 2 of the split fast build, or in
// the whole-file build (0) — and in unit 1 for lane-statistics builds, whose
// counters (g_lanes) must live in the unit that reads them (unit 2 then
// emits nothing)
#ifndef MRT_LANESTATS
#define MRT_LANESTATS 0
#endif
#define MRT_EMIT_STREAM (MRT_TU == 0 || (MRT_TU == 2 && !MRT_LANESTATS) || (MRT_TU == 1 && MRT_LANESTATS))
#define MRT_EMIT_MAIN (MRT_TU != 2)
#if MRT_PRECISE
#define MRT_NS precise
#else
#define MRT_NS fast
#endif

// Minimum waves per SIMD for the bounce kernel (launch bounds; the stream
// kernel has its own, MRT_STREAM_WAVES): 5 caps it at
// 96 VGPRs with 48 B/lane of scratch spills; 6 (80 VGPRs) spills ~140 B/lane
// and 4 (no spills) hides less latency — 5 measured best with one stream.
#ifndef MRT_BOUNCE_WAVES
#define MRT_BOUNCE_WAVES 5
#endif

// Traversal slack: the interior loop of a while-while round ends once at
// most this many lanes still seek a leaf, instead of waiting for the last
// one (the lanes holding a leaf test it; the others resume next round).  The
// path kernel's rounds are resumable anyway, and in deep global-memory trees
// the last lanes' descents are long: slack 12 (of 64) measured C4 1950 ->
// 2497 Mpaths/s (+28 %), C3 +7.5 %, C3g +5 %, C5 1/8 share +28 % (8 / 16 /
// 24 / 32 / 48: C4 2456 / 2488 / 2397 / 2281 / 1904).  Shallow all-in-LDS
// trees lose by it (C2, the stream kernel: slack 2 -1.3 %, 8 -3.4 %).
// r4, with the inline shadow finishes (service 32): path slack 8 / 12 / 16
// C4 2769 / 2852 / 2873, C3 2530 / 2616 / 2660; leaf slack 4 / 8 / 12 C4
// 2795 / 2852 / 2869, C3 2574 / 2616 / 2638 (one call, alternating)
#ifndef MRT_PATH_SLACK   // trav_round(): the path kernel
#define MRT_PATH_SLACK 16
#endif
#ifndef MRT_LEAF_SLACK   // trav_round(): the leaf loop's (a kept leaf is tested next round):
#define MRT_LEAF_SLACK 12 // r3, path slack 12: C4 2480 -> 2645 (+6.7 %), C3 2340 -> 2474 (+5.7 %);
#endif                   // 2 / 4 / 12 / 16 / 24 / 32: C4 2577 / 2605 / 2645 / 2640 / 2623 / 2611

// Waves per SIMD the stream kernel's registers allow: 6 (80 VGPRs, 5 values
// spilled to scratch — 6 until §2.1n — reloaded outside the traversal loops:
// tools/scratch_sites.py) under the max-ILP scheduler of its unit (Makefile):
// C2 +1.7…+3.4 %, L = 5 +4…6 % over 5 waves (96 VGPRs, no spill); 7 / 8
// waves (23 / 37 spills) lose 6 / 27 %, and 6 waves under the default
// scheduler only tie (r5, alternating in one call); re-swept at the r6
// library: 5 / 7 waves -6 / -10 %, 0 / 2 spare block slots -2 / -1.3 %
#ifndef MRT_STREAM_WAVES
#define MRT_STREAM_WAVES 6
#endif
#ifndef MRT_STREAM_SPARE   // block slots per CU the stream kernel's persistent grid leaves free (stream_grid_t)
#define MRT_STREAM_SPARE 1
#endif

#ifndef MRT_PATH_WAVES   // 5: 96 VGPRs with 1-3 spilled values (C4 +11 %, C3 +8 % over 4 waves)
#define MRT_PATH_WAVES 5
#endif
// Service threshold: finished nearest queries a wave collects before it
// shades them together.  With finished shadow queries handled inside the
// traversal loop (r4) a service round shades 22 of
// 64 lanes on C3 instead of 16: C4 2803 -> 2849 Mpaths/s (+1.6 %), C3 2491
// -> 2601 (+4.4 %) at 24, 2848 / 2620 at 32 (16: 2770 / 2471), alternating
// in one call.
#ifndef MRT_PATH_SERVICE
#define MRT_PATH_SERVICE 32
#endif
#ifndef MRT_LDS_BLOCKS   // resident blocks per CU the kTopLds node budget is sized for (fit_lds_nodes)
#define MRT_LDS_BLOCKS MRT_BOUNCE_WAVES
#endif

// Diagnostic: 1 gives the all-in-LDS kernels the per-solid loop of the convex
// shadow query as well (dev_shadow.h convex_occlusion_loop), so that a lane-
// statistics variant can count its face passes next to the plan's
#ifndef MRT_CONVEX_LOOP
#define MRT_CONVEX_LOOP 0
#endif

namespace mrt { namespace MRT_NS { namespace {

constexpr int kBlock = 256;   // 4 waves of 64 lanes

}}}  // namespace mrt::MRT_NS::(anonymous)
