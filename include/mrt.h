/*
 * mrt.h — C ABI of the MI355X-native path tracer (libmrt.so).
 *
 * This is the drop-in boundary for the hot path of serhii-rieznik/metal-renderer.
 * The reference exposes the path through two boundaries, both reproduced here:
 *
 *   B-1  App <-> renderer:  the Objective-C `Renderer` (renderer/Renderer.h:3-8)
 *        -initWithMetalKitView:            -> mrt_renderer_create
 *        -mtkView:drawableSizeWillChange:  -> mrt_renderer_resize   (Renderer.mm:640-657)
 *        -drawInMTKView:                   -> mrt_renderer_draw     (Renderer.mm:587-638)
 *        -saveCurrentImage                 -> mrt_renderer_save_image (Renderer.mm:659-662;
 *                                             a working save, the reference's is a stub)
 *        window-title stats                -> mrt_renderer_stats    (Renderer.mm:631-637)
 *   B-2  Renderer <-> GPU:  the per-stage dispatches of performRaytracing:
 *        (renderer/Renderer.mm:500-585) over the reference AoS records
 *        (renderer/Raytracing.h:47-123):
 *        rayGenerator        (Shaders.metal:75-103)   -> mrt_raygen
 *        MPS nearest-hit     (Renderer.mm:519-523,545-553; config :464-469)
 *                                                     -> mrt_intersect
 *        MPS rebuild         (Renderer.mm:456-462)    -> mrt_scene_create (BVH build)
 *   MPS itself, over raw vertex/index buffers (Renderer.mm:456-469):
 *        MPSTriangleAccelerationStructure + rebuild -> mrt_accel_create / mrt_accel_rebuild
 *        MPSRayIntersector encodeIntersection (Nearest)  -> mrt_accel_intersect
 *        intersectionHandler (Shaders.metal:105-212)  -> mrt_shade
 *        lightSamplingHandler(Shaders.metal:214-231)  -> mrt_resolve_shadow
 *        accumulateImage     (Shaders.metal:233-249)  -> mrt_accumulate
 *
 * Conventions: every function returns 0 on success and a negative mrt_status
 * on failure; mrt_last_error() returns a thread-local message.  No exception
 * crosses the ABI.  Handles are opaque.  A handle is externally synchronised
 * (one caller thread at a time, like the MTKView main thread).  Device
 * pointers are HIP device memory on the handle's device; `stream` arguments
 * are hipStream_t (NULL = the handle's own stream).
 * Image layout: RGBA32F, W*H*4 floats, row 0 = BOTTOM of the view (the
 * reference's texture orientation, Shaders.metal:81,94).
 */
#ifndef MRT_H_
#define MRT_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MRT_ABI_VERSION 9

typedef enum mrt_status {
  MRT_OK = 0,
  MRT_ERR_INVALID = -1,   /* bad argument */
  MRT_ERR_IO = -2,        /* scene / image file error */
  MRT_ERR_HIP = -3,       /* HIP runtime error (no device, launch failure, ...) */
  MRT_ERR_NOMEM = -4,
  MRT_ERR_STATE = -5,     /* call not valid in the handle's current state */
  MRT_ERR_COMM = -6       /* ABI 9: an RCCL collective reported an asynchronous error or did not complete
                             within the communicator's timeout; the communicator is aborted and every
                             later use of it fails with this status (renderers stay usable) */
} mrt_status;

/* flags */
#define MRT_FLAG_PRECISE 1u   /* parity kernels: IEEE div/sqrt, no FMA contraction, CR sin/cos */
#define MRT_FLAG_PROFILE 2u   /* time the bounce launches of every 8th frame with HIP events (mrt_stats.kernel_ms);
                                 timing events serialise a stream's launches, so only a sample is timed */
/* The reference's compile-time switches as runtime flags (renderer/Raytracing.h:11-33,
 * renderer/Shaders.metal:7); the defaults (flag clear) are the reference's defaults. */
#define MRT_FLAG_STATIC_NOISE 4u      /* ANIMATE_NOISE 0 (Raytracing.h:20): every frame reads the initial noise
                                         table (Renderer.mm:109-129; :485-497 skipped).  Renderer flag. */
#define MRT_FLAG_NO_ACCUMULATE 8u     /* ACCUMULATE_IMAGE false (Raytracing.h:14, Shaders.metal:241): the image
                                         holds the last frame's radiance alone.  Renderer and mrt_accumulate. */
#define MRT_FLAG_DEBUG_MATERIAL 16u   /* DEBUG_MATERIAL 1 (Shaders.metal:7,142-147): at each hit the path radiance
                                         is set to fresnel(n, -wI, 1.0, 1.5) before emission and NEE add to it.
                                         Renderer and mrt_shade. */
#define MRT_FLAG_MOMENTS 32u          /* the renderer accumulates the luminance moments of its frames beside the
                                         image ("variance-guided denoising" below).  Renderer flag; not with
                                         MRT_FLAG_NO_ACCUMULATE, not with shard_count > 1. */

typedef struct mrt_scene mrt_scene;
typedef struct mrt_renderer mrt_renderer;

/* ---- scene (initRaytracing: Renderer.mm:255-470) ------------------------ */
typedef struct mrt_scene_desc {
  const char* obj_path;            /* OBJ scene (renderer/Media/<name>.obj) */
  const char* mtl_override;        /* optional .mtl used instead of the OBJ's mtllib (NULL/"" = none) */
  uint32_t procedural_triangles;   /* >0: append a seeded displaced sphere of this many triangles */
  uint64_t procedural_seed;
  uint32_t max_leaf_size;          /* BVH leaf size, 0 = default (2) */
  uint32_t lds_nodes;              /* top BVH nodes staged in LDS, 0 = default; UINT32_MAX = none */
  int device;                      /* HIP device ordinal; -1 = host only (import + BVH, no upload) */
  uint32_t bvh_width;              /* 4 = BVH4 (the binary SAH tree collapsed), 0 = default (4); other widths are rejected */
  uint32_t bvh_builder;            /* MRT_BVH_*; 0 = default (host binned SAH) */
  uint32_t no_occluder_tree;       /* 1: shadow rays always traverse the main tree (no occluder tree, see
                                      mrt_scene_info.occluder_planes); 0 = default (built for host-SAH
                                      scenes of <= 16384 triangles with culled supporting planes) */
} mrt_scene_desc;

/* BVH builders */
#define MRT_BVH_HOST_SAH 1u      /* host binned-SAH BVH2, collapsed to BVH4 (best traversal quality) */
#define MRT_BVH_DEVICE_LBVH 2u   /* device linear BVH (Morton sort + radix tree, collapsed to BVH4
                                    on the GPU; BVH4 only) — fastest build, weakest tree */
#define MRT_BVH_DEVICE_PLOC 3u   /* device PLOC (Morton sort + nearest-neighbour clustering, collapsed
                                    to BVH4 on the GPU) — near-SAH tree; builds from device buffers */

typedef struct mrt_scene_info {
  uint32_t vertices, triangles, materials, light_triangles;
  uint32_t bvh_nodes, bvh_leaves, bvh_depth, bvh_lds_nodes;
  uint32_t bvh_width, bvh_max_stack;   /* node width; traversal stack entries a ray can need */
  double bvh_sah_cost;
  double build_ms;                 /* host BVH build time */
  uint64_t device_bytes;           /* scene + BVH bytes resident on the device */
  /* shadow-ray occluder tree: triangles in supporting planes with every light
   * strictly inside (walls, floor, ceiling) cannot occlude a shadow ray from
   * an origin inside those planes; such rays traverse a second BVH over the
   * other triangles (same answers).  0 planes = no occluder tree. */
  uint32_t occluder_planes, occluder_culled, occluder_nodes;
  float occluder_margin;
  uint32_t occluder_max_stack;     /* traversal stack entries the occluder tree can need (<= bvh_max_stack:
                                      a deeper occluder tree is not built); renderers size their stack by
                                      the deeper tree.  ABI 7. */
  float occluder_cos_min;          /* shadow rays whose cosine to the target light's normal is below this
                                      traverse the main tree (bound on the light's own t error). ABI 7. */
  /* ABI 8: the culled planes (n, w; outward unit normal n, inside
   * n.x - w <= -occluder_margin), occluder_planes of them */
  float occluder_plane[8][4];
  /* ABI 9: convex occluders — every triangle of the (light-free) occluder
   * tree lies on one of convex_solids parallelepiped solids (e.g. the Cornell
   * box's blocks): shadow rays through that tree are decided per solid by a
   * segment test against its three slabs pushed out by convex_delta, and the
   * leaf test of the face the segment enters, before any walk (dev_shadow.h
   * convex_occlusion).  convex_obb[c] = three unit axis normals (9 floats),
   * then each axis's padded slab (lo, hi); convex_face_tris[c][2a + side]
   * (side 0: the lo face, 1: the hi face) = its two primitive ids, 16 bits
   * each, 0xFFFF = none. */
  uint32_t convex_solids;
  float convex_delta;
  float convex_obb[4][16];
  uint32_t convex_face_tris[4][8];
} mrt_scene_info;

int mrt_scene_create(const mrt_scene_desc* desc, mrt_scene** out);
int mrt_scene_info_get(const mrt_scene* scene, mrt_scene_info* info);
/* Copy the flattened reference-layout buffers to host memory (any pointer may
 * be NULL): Vertex[24 B], uint32 indices, Material[32 B], TriangleReference[20 B],
 * LightTriangle[100 B] (light_triangles + 1 entries, the sentinel last). */
int mrt_scene_export(const mrt_scene* scene, void* vertices, void* indices, void* materials,
                     void* references, void* lights);
int mrt_scene_destroy(mrt_scene* scene);
/* Structural check of the built BVH (host): every primitive in exactly one
 * leaf, every child box contains its subtree's triangles, depth within the
 * traversal stack.  0 = valid. */
int mrt_scene_check_bvh(const mrt_scene* scene);
/* Host only (works on device = -1 scenes).  Two scenes are MOTION-COMPATIBLE —
 * two poses of one mesh, for mrt_guides_motion and mrt_renderer_move_scene —
 * iff they have the same number of triangles and of materials and, for every
 * primitive index k, references[k].materialIndex is equal in both and
 * references[k].lightTriangleIndex is 0xFFFFFFFF in both or in neither.
 * Positions, normals, material values, the BVH, its builder and leaf size may
 * differ; a scene is compatible with itself.  MRT_OK, or MRT_ERR_INVALID with a
 * message that names the first difference.  Constant time for a compatible
 * pair: the counts and a 64-bit digest of the compared words, folded when the
 * scene is created, are what is compared; only a pair that differs is walked. */
int mrt_scene_motion_compatible(const mrt_scene* a, const mrt_scene* b);

/* ---- acceleration structure over raw buffers (the MPS interface) --------
 * MPSTriangleAccelerationStructure (Renderer.mm:456-462): vertexBuffer with
 * vertexStride = sizeof(Vertex) = 24, uint32 indexBuffer, triangleCount =
 * indices / 3, `rebuild` once; MPSRayIntersector (Renderer.mm:464-469):
 * nearest hit, cull none, ray records (origin, minDistance, direction,
 * maxDistance) at rayStride, intersections (distance, primitiveIndex, (u,v)). */
typedef struct mrt_accel mrt_accel;
typedef struct mrt_accel_desc {
  const void* vertices;            /* device pointer: 3 floats (position) at the start of every vertex */
  uint32_t vertex_stride;          /* bytes between vertices (>= 12, multiple of 4) */
  const uint32_t* indices;         /* device pointer: 3 uint32 per triangle */
  uint32_t triangle_count;
  int device;                      /* HIP device of the buffers */
  uint32_t builder;                /* MRT_BVH_*; 0 = default (MRT_BVH_DEVICE_PLOC) */
  uint32_t max_leaf_size;          /* 0 = default (2) */
  void* stream;                    /* hipStream_t of libmrt's runtime, NULL = own stream */
} mrt_accel_desc;
typedef struct mrt_accel_info {
  uint32_t triangles, bvh_nodes, bvh_leaves, bvh_levels, bvh_max_stack, builder;
  double build_ms;                 /* device time (LBVH) or host time (SAH) of the last (re)build */
  uint64_t device_bytes;
} mrt_accel_info;
/* Build the structure (the buffers must stay valid until the next rebuild). */
int mrt_accel_create(const mrt_accel_desc* desc, mrt_accel** out);
/* Rebuild from the same buffers (their contents may have changed). */
int mrt_accel_rebuild(mrt_accel* accel);
/* Nearest hit of `count` ray records of `stride` bytes (contract of mrt_intersect). */
int mrt_accel_intersect(const mrt_accel* accel, const void* rays, uint32_t stride, uint32_t count,
                        void* intersections, uint32_t flags, void* stream);
int mrt_accel_info_get(const mrt_accel* accel, mrt_accel_info* info);
int mrt_accel_destroy(mrt_accel* accel);

/* ---- stage-level ABI (B-2), reference AoS layouts, device pointers ------- */
/* rayGenerator over a W x H grid: noise = 64*64 float4 (one noise slot). */
int mrt_raygen(const mrt_scene* scene, uint32_t width, uint32_t height, const float* noise,
               void* rays /* Ray[W*H], 80 B */, uint32_t flags, void* stream);
/* MPS nearest-hit: records of `stride` bytes whose first 32 B are
 * (origin, minDistance, direction, maxDistance); cull none; distance = -1 on
 * miss or maxDistance < 0; ties -> lowest primitive index. */
int mrt_intersect(const mrt_scene* scene, const void* rays, uint32_t stride, uint32_t count,
                  void* intersections /* Intersection[count], 16 B */, uint32_t flags, void* stream);
/* intersectionHandler for iteration with SharedData.frameIndex = frame_index
 * and MAX_PATH_LENGTH = max_path_length; noise = the slot bound at index 8. */
int mrt_shade(const mrt_scene* scene, uint32_t width, uint32_t height, uint32_t frame_index,
              uint32_t max_path_length, const float* noise, const void* intersections, void* rays,
              void* shadow_rays /* LightSamplingRay[W*H], 48 B */, uint32_t flags, void* stream);
int mrt_resolve_shadow(const mrt_scene* scene, uint32_t count, const void* intersections, void* rays,
                       const void* shadow_rays, uint32_t flags, void* stream);
int mrt_accumulate(const mrt_scene* scene, uint32_t width, uint32_t height, uint32_t frame_index,
                   const void* rays, float* image_rgba, uint32_t flags, void* stream);
/* mrt_accumulate's counterpart for the luminance moments ("variance-guided
 * denoising" below): with l = lum(ray.radiance), moments[p] =
 * accumulate(moments[p], (l, l*l, 0), frame_index).  The rays are only read.
 * flags: MRT_FLAG_PRECISE. */
int mrt_moments(const mrt_scene* scene, uint32_t width, uint32_t height, uint32_t frame_index, const void* rays,
                float* moments_rgba, uint32_t flags, void* stream);

/* ---- camera ---------------------------------------------------------------
 * The reference's rayGenerator has one fixed camera; this is the same
 * construction with a pose, a field of view and a thin lens.  With (u, v) the
 * reference's jittered image-plane coordinates of a pixel (u in [-1, 1], v in
 * [-H/W, H/W]) and s = tan_half_fov:
 *   pinhole:   c = (u s, v s, -1), w = normalize(c), o = origin
 *   thin lens: (xi1, xi2) = (z, w) of the frame's raygen noise table at cell
 *              ((x + 32) % 64, (y + 32) % 64) (not the cell of the pixel's own
 *              jitter and bounce-0 samples),
 *              l = lens_radius sqrt(xi1) (cos 2 pi xi2, sin 2 pi xi2),
 *              w = normalize(c focus_distance - (l.x, l.y, 0)),
 *              o = origin + right l.x + up l.y
 *   d = right w.x + up w.y + forward (-w.z)
 * A camera bitwise equal to mrt_camera_default takes the reference's own code
 * path (bit-identical images). */
typedef struct mrt_camera {
  float origin[3];
  float right[3], up[3], forward[3];  /* orthonormal, right-handed: right x up = -forward */
  float tan_half_fov;                 /* half-width of the image plane at distance 1 (reference: 1) */
  float lens_radius;                  /* 0 = pinhole */
  float focus_distance;               /* depth (along forward) of the plane in focus; used when lens_radius > 0 */
} mrt_camera;

/* The reference's camera, exactly: origin (0, 1, 2.35), looking down -z, tan 1. */
int mrt_camera_default(mrt_camera* out);
/* Host only.  A pinhole camera at `eye` looking at `target`; fov_x_degrees is
 * the full horizontal field of view, in (0, 180).  MRT_ERR_INVALID for
 * eye == target, for `up` parallel to the view direction (or zero) and for a
 * non-finite argument.  Set lens_radius / focus_distance on the result. */
int mrt_camera_look_at(const float eye[3], const float target[3], const float up[3],
                       float fov_x_degrees, mrt_camera* out);
/* Host only.  MRT_ERR_INVALID (with a message) for a non-finite field, a basis
 * that is not orthonormal to 1e-4 or not right-handed, tan_half_fov <= 0,
 * lens_radius < 0, or lens_radius > 0 with focus_distance <= 0. */
int mrt_camera_check(const mrt_camera* cam);
/* rayGenerator of `cam` (mrt_raygen is this with mrt_camera_default). */
int mrt_raygen_camera(const mrt_scene* scene, const mrt_camera* cam, uint32_t width, uint32_t height,
                      const float* noise, void* rays, uint32_t flags, void* stream);

/* ---- denoised output -------------------------------------------------------
 * First-hit guide buffers and an edge-avoiding A-Trous filter driven by them
 * (Dammertz, Sewtz, Hanika, Lensch, HPG 2010; DESIGN.md "Denoised output").
 * Not in the reference, which only ever shows the accumulation image.
 *
 * mrt_guides: one guide ray per pixel over the whole W x H frame (index
 * y * W + x, row 0 at the bottom) — the pixel's camera ray at the pixel centre
 * (the jitter sample (0.5, 0.5)) through a pinhole: a camera with
 * lens_radius > 0 is used as if its lens were absent; NULL = mrt_camera_default.
 * Traced with tmin 0 and no tmax.  Two float4 planes (device, W*H*4 floats each):
 *   guide_n[p] = (shading normal, bits(word)), guide_p[p] = (hit position, t)
 * with position, normal and material index as mrt_shade computes them; word is
 * the material index, bit 31 set when the hit is a light triangle; a miss
 * writes (0, 0, 0, bits(0xFFFFFFFF)) and (0, 0, 0, -1).  A pixel is FILTERABLE
 * iff word < 0x80000000.  flags: MRT_FLAG_PRECISE.
 * On a scene whose tree needs more than 64 traversal-stack entries (see
 * mrt_scene_info.bvh_max_stack) mrt_guides and mrt_intersect keep the deeper
 * entries in one buffer of the scene: such calls on one scene must not run
 * concurrently on different streams.  A renderer's own guide pass
 * (mrt_renderer_denoise) uses a buffer of the renderer's. */
int mrt_guides(const mrt_scene* scene, const mrt_camera* cam /* NULL = default */, uint32_t width, uint32_t height,
               float* guide_n, float* guide_p /* W*H*4 floats each, device */, uint32_t flags, void* stream);

/* The filter.  k = (1/16, 1/4, 3/8, 1/4, 1/16), c^0 = the image's rgb; for
 * iteration i = 0 .. iterations-1 the step is s = 2^i.  A pixel p that is not
 * filterable keeps its value.  Otherwise, over (dx, dy) in {-2..2}^2 with
 * q = p + s (dx, dy), a tap counts only if q is inside the image, q is
 * filterable, word_q == word_p and every component of c^i_q is finite; its
 * weight is the product of
 *   k[dx+2] k[dy+2],
 *   D^(2^e) with D = max(0, n_p.n_q) and e = normal_log2_power,
 *   exp(-|n_p.(x_q - x_p)| / (sigma_plane t_p)),
 *   exp(-|c^i_q - c^i_p|^2 / sigma_color^2)   (1 if sigma_color == 0 or c^i_p is not finite)
 * and c^(i+1)_p = sum w c^i_q / sum w (c^i_p if the sum is 0: a non-finite
 * centre without a usable neighbour; one with usable neighbours is repaired,
 * and never spreads).  Alpha is copied; iterations = 0 copies the image. */
typedef struct mrt_denoise_params {
  uint32_t iterations;         /* 0..8 */
  float sigma_color;           /* >= 0; 0 = no colour term */
  float sigma_plane;           /* > 0 */
  uint32_t normal_log2_power;  /* e, 0..8 */
} mrt_denoise_params;
/* Host only.  iterations = 3 (frames <= 2), 2 (frames <= 16), else 1;
 * sigma_color = 2 / sqrt(max(frames, 1)); sigma_plane = 0.01; normal_log2_power = 6. */
int mrt_denoise_params_default(uint64_t frames, mrt_denoise_params* out);
/* Host only.  MRT_ERR_INVALID (with a message) for a field outside the ranges
 * above, a non-finite one included. */
int mrt_denoise_params_check(const mrt_denoise_params* p);
/* Device pointers, W*H*4 floats each.  The iterations ping-pong between `out`
 * and `scratch` so that the last one writes `out`; `image` is only read.  Any
 * aliasing among image, out and scratch, and params == NULL, is MRT_ERR_INVALID. */
int mrt_denoise(const float* image, const float* guide_n, const float* guide_p, float* out, float* scratch,
                uint32_t width, uint32_t height, const mrt_denoise_params* params, void* stream);

/* ---- temporal history -------------------------------------------------------
 * Keep what has been accumulated across a camera move: the temporal half of
 * SVGF (Schied et al., HPG 2017; DESIGN.md "Temporal reprojection"), driven by
 * the guide planes of mrt_guides.  Not in the reference.  A COUNTED IMAGE is
 * W*H float4 (r, g, b, h): h >= 0 is the number of frames behind the colour;
 * h = 0 means no information, and the rgb is then (0, 0, 0).  Device pointers
 * throughout. */
typedef struct mrt_reproject_params {
  float plane_tolerance;   /* > 0   */
  float normal_cos_min;    /* [-1,1] */
  float max_history;       /* >= 0: cap of the history length carried over a move */
} mrt_reproject_params;
/* Host only.  plane_tolerance = 0.01, normal_cos_min = 0.9, max_history = 32. */
int mrt_reproject_params_default(mrt_reproject_params* out);
/* Host only.  MRT_ERR_INVALID (with a message) for a field outside the ranges
 * above, a non-finite one included. */
int mrt_reproject_params_check(const mrt_reproject_params* p);

/* Merge the accumulation image (`frames` frames of running mean) with a counted
 * history (NULL = none) into the counted image `out`.  Per pixel, with
 * h = history.w (0 without a history) and n = (float)frames:
 *   h == 0:                            out = (image.rgb bitwise, n)
 *   n == 0 (h > 0):                    out = history, bitwise
 *   a component of image.rgb is not
 *   finite (h > 0, n > 0):             out = history, bitwise (the history repairs the pixel)
 *   otherwise:                         out.rgb = (h H.rgb + n I.rgb) / (h + n), out.w = h + n
 * `out` may not alias `image` or `history` (MRT_ERR_INVALID). */
int mrt_temporal_resolve(const float* image, uint64_t frames, const float* history /* may be NULL */, float* out,
                         uint32_t width, uint32_t height, void* stream);

/* Reproject the counted image `prev`, seen through prev_cam (NULL =
 * mrt_camera_default; its lens is ignored, as mrt_guides ignores it) with guide
 * planes prev_guide_n / prev_guide_p, into the view whose guide planes are
 * cur_guide_n / cur_guide_p (all as mrt_guides writes them).  Per current
 * pixel p:
 *   p not filterable (word_p >= 0x80000000): (0, 0, 0, 0).
 *   v = x_p - origin_prev, cz = v.forward_prev; cz <= 0: 0.
 *   U = (v.right_prev) / cz, V = (v.up_prev) / cz, s = tan_half_fov_prev,
 *   fx = (U / s + 1) (W - 1) / 2, fy = (V / (s H / W) + 1) (H - 1) / 2
 *   (the inverse of the camera ray at the pixel centre);
 *   x0 = floor(fx), y0 = floor(fy), ax = fx - x0, ay = fy - y0; the four taps
 *   q = (x0 + i, y0 + j), bilinear weight b = (i ? ax : 1 - ax)(j ? ay : 1 - ay).
 *   A tap counts iff q is inside the image, b > 0, word_q == word_p (previous
 *   guide word against current), n_p.n_q >= normal_cos_min,
 *   |n_p.(x_q - x_p)| <= plane_tolerance t_p, prev_q.w > 0 and prev_q.rgb finite.
 *   B = sum of b over the taps that count; B == 0: 0.  Otherwise
 *   rgb = sum b prev_q.rgb / B, h = min(max_history, sum b prev_q.w / B)
 *   (a count of 0, possible only with max_history = 0, goes with rgb 0).
 * The inputs are only read.  params == NULL, W < 2, H < 2, or history_out
 * overlapping an input, is MRT_ERR_INVALID.  With the guide planes of the
 * current view in cur_guide_n / cur_guide_p the geometry is taken as static;
 * with the motion planes of mrt_guides_motion in their place it moves (below). */
int mrt_reproject(const float* prev, const float* prev_guide_n, const float* prev_guide_p,
                  const mrt_camera* prev_cam /* NULL = default */, const float* cur_guide_n, const float* cur_guide_p,
                  float* history_out, uint32_t width, uint32_t height, const mrt_reproject_params* params,
                  void* stream);

/* Moving geometry.  mrt_guides of `scene` and, beside its
 * planes, two MOTION PLANES: for the surface point each pixel sees now, where
 * that point was in prev_scene — another pose of the same mesh
 * (mrt_scene_motion_compatible), on the same device.  guide_n and guide_p are
 * bitwise what mrt_guides(scene, cam, ...) writes.  For a pixel whose guide ray
 * hits primitive k of `scene` at barycentrics (u, v) and distance t, with guide
 * word `word`:
 *   motion_p[p] = (position of that point in prev_scene, t)
 *   motion_n[p] = (shading normal of that point in prev_scene, bits(word))
 * both interpolated from prev_scene's primitive k with the weights (u, v,
 * (1 - u) - v) and the expressions mrt_shade uses; a miss writes the miss
 * record of mrt_guides to all four planes.  prev_scene == scene gives motion
 * planes bitwise equal to the guide planes.
 * Passed to mrt_reproject as cur_guide_n / cur_guide_p, with prev_scene's guide
 * planes and camera as the previous ones, the motion planes make it a
 * motion-vector reprojection: the point's OLD position is projected through
 * the old camera, and each tap condition compares the old frame with itself —
 *   word_q == word_p: the old frame showed the same material there (the word
 *     of a primitive is the same in both poses);
 *   n_p.n_q >= normal_cos_min: the old frame's normal at the tap against the
 *     point's own normal as it was then, so a rotating surface keeps its taps;
 *   |n_p.(x_q - x_p)| <= plane_tolerance t_p: the surface the old frame showed
 *     at the tap lies in the point's old tangent plane — the point was visible
 *     then, not hidden behind something else (the disocclusion test), within a
 *     tolerance scaled by the point's distance now;
 *   prev_q.w > 0 and finite: the old frame had samples there.
 * MRT_ERR_INVALID (nothing is written) for scenes that are not
 * motion-compatible, scenes on different devices, a host-only scene, any two of
 * the four planes overlapping, and mrt_guides' own argument errors.  Both
 * scenes must stay alive until the stream has run the call; the stack-spill
 * rule of mrt_guides applies to `scene`.  flags: MRT_FLAG_PRECISE. */
int mrt_guides_motion(const mrt_scene* scene, const mrt_scene* prev_scene, const mrt_camera* cam /* NULL = default */,
                      uint32_t width, uint32_t height, float* guide_n, float* guide_p, float* motion_n,
                      float* motion_p /* W*H*4 floats each, device */, uint32_t flags, void* stream);

/* ---- variance-guided denoising ----------------------------------------------
 * The spatial half of SVGF (Schied et al., HPG 2017): a
 * per-pixel variance estimate from accumulated luminance moments, and an
 * A-Trous filter whose colour term it steers, so that one parameter set serves
 * every frame count.  Not in the reference.  Device pointers throughout.
 *
 * lum(c) = (0.2126 r + 0.7152 g) + 0.0722 b.  A MOMENTS IMAGE is W*H float4
 * (mean l, mean l*l, 0, 1): for every frame f, where the image gets
 * accumulate(stored, c, f) the moments image gets accumulate(stored_m,
 * (l, l*l, 0), f) with l = lum(c) — the same recurrence in the same frame
 * order; f == 0 overwrites.  In the precise build l and l*l are rounded after
 * each operation, in the order written; the fast build may contract.  As a
 * counted image (temporal history above) its fourth channel is n, and it
 * resolves and reprojects through mrt_temporal_resolve and mrt_reproject, which
 * are linear in the first three channels. */
typedef struct mrt_svgf_params {
  uint32_t iterations;         /* 0..8 */
  float sigma_luminance;       /* > 0 */
  float sigma_plane;           /* > 0 */
  uint32_t normal_log2_power;  /* e, 0..8 */
  uint32_t min_frames;         /* >= 2: counts from which a pixel's own moments are trusted */
} mrt_svgf_params;
/* Host only.  iterations = 5, sigma_luminance = 4, sigma_plane = 0.01,
 * normal_log2_power = 6, min_frames = 4. */
int mrt_svgf_params_default(mrt_svgf_params* out);
/* Host only.  MRT_ERR_INVALID (with a message naming the field) for a field
 * outside the ranges above, a non-finite one included. */
int mrt_svgf_params_check(const mrt_svgf_params* p);
/* variance[p] (W*H floats) estimates the variance of the pixel's MEAN from the
 * counted moments (mu1, mu2, ., n) = moments[p]; params->iterations and
 * sigma_luminance are not used.
 *   p not filterable (word_p >= 0x80000000): 0.
 *   p is USABLE when mu1 and mu2 are finite and n > 0.
 *   p usable and n >= min_frames: the temporal estimate max(0, mu2 - mu1^2) / (n - 1).
 *   Otherwise the spatial estimate over the 7x7 window, (dx, dy) in {-3..3}^2,
 *   dy outer and dx inner, the centre included: a tap q counts iff it is inside
 *   the image, filterable, word_q == word_p and usable, with weight
 *     w = D^(2^e) exp(-|n_p.(x_q - x_p)| / (sigma_plane t_p)) n_q,
 *   D = max(0, n_p.n_q) as in mrt_denoise; a1 = sum w mu1_q / sum w,
 *   a2 = sum w mu2_q / sum w, and the result is
 *   max(0, a2 - a1^2) / max(n_p, 1), or 0 if sum w is not > 0.
 *   A result that is negative or not finite (sums that overflow) is replaced by 0:
 *   the output is never negative and never non-finite.
 * The inputs are only read.  params == NULL, or `variance` overlapping an
 * input, is MRT_ERR_INVALID. */
int mrt_variance(const float* moments, const float* guide_n, const float* guide_p, float* variance, uint32_t width,
                 uint32_t height, const mrt_svgf_params* params, void* stream);
/* mrt_denoise's definition — the same k, steps s = 2^i, tap order and tap
 * conditions, a pixel that is not filterable keeps its value, alpha copied
 * from `image` — with two changes.  v^0 = `variance` (W*H floats).
 *   The colour weight is replaced by
 *     exp(-|lum(c^i_q) - lum(c^i_p)| / (sigma_luminance sqrt(g_p) + 1e-6))   (1 if c^i_p is not finite),
 *   g_p = the average of v^i over the 3x3 pixels around p (offsets of ONE
 *   pixel, not s) with weights (1/4, 1/2, 1/4)^2, over the taps inside the
 *   image, renormalised by the weights of those taps.
 *   The variance is filtered with the colour: c^(i+1)_p = sum w c^i_q / sum w,
 *   v^(i+1)_p = sum w^2 v^i_q / (sum w)^2 (evaluated as (sum w^2 v / sum w) /
 *   sum w); both stay as they are if the sum is 0, and a pixel that is not
 *   filterable keeps its v.
 * variance_out (W*H floats, may be NULL) receives v^iterations.  iterations = 0
 * copies image to out and variance to variance_out.  A non-finite or negative
 * input variance is outside the contract.  The iterations ping-pong between
 * `out` and `scratch` (W*H*4 floats each; between iterations their fourth
 * channel carries v).  Any overlap among out, scratch, variance_out and any
 * other buffer, and params == NULL, is MRT_ERR_INVALID.
 * mrt_debug_denoise_path selects between the two implementations of an
 * iteration here as it does for mrt_denoise. */
int mrt_denoise_variance(const float* image, const float* variance, const float* guide_n, const float* guide_p,
                         float* out, float* scratch, float* variance_out /* may be NULL */, uint32_t width,
                         uint32_t height, const mrt_svgf_params* params, void* stream);

/* ---- firefly suppression -----------------------------------------------------
 * An outlier clamp ahead of the variance-guided filter: a
 * pixel whose luminance lies far above that of its neighbours on the same
 * surface is scaled down to a cap.  The filter's luminance weight is built to
 * keep such a pixel, so without the clamp it survives the filter.  The clamp is
 * BIASED: it removes energy and does not redistribute it; it is off unless
 * asked for (mrt_renderer_set_firefly below), and it never touches the variance
 * plane.  Not in the reference.  Device pointers throughout; lum is the lum of
 * "variance-guided denoising" above. */
typedef struct mrt_firefly_params {
  uint32_t radius;          /* R, 1..3: the window is {-R..R}^2 */
  float k;                  /* > 0: cap = mean + k * standard deviation */
  uint32_t min_taps;        /* >= 1: fewer counting taps leave the pixel alone */
  float normal_cos_min;     /* [-1, 1] */
  float plane_tolerance;    /* > 0 */
} mrt_firefly_params;
/* Host only.  radius = 2, k = 3, min_taps = 3, normal_cos_min = 0.9,
 * plane_tolerance = 0.01. */
int mrt_firefly_params_default(mrt_firefly_params* out);
/* Host only.  MRT_ERR_INVALID (with a message naming the field) for a field
 * outside the ranges above, a non-finite one included. */
int mrt_firefly_params_check(const mrt_firefly_params* p);
/* image and out are W*H float4, the guide planes as mrt_guides writes them.
 * Per pixel p, out[p] = image[p] bitwise, alpha included, unless ALL of:
 *   (a) p is filterable (word_p < 0x80000000), c_p = image[p].rgb is finite and
 *       l_p = lum(c_p) > 0;
 *   (b) no pixel q of the window p + {-R..R}^2 inside the image is a light
 *       pixel, 0x80000000 <= word_q < 0xFFFFFFFF (a miss is not a light);
 *   (c) over the window's taps q != p, dy outer and dx inner, a tap COUNTS iff
 *       q is inside the image, word_q == word_p, c_q is finite,
 *       n_p.n_q >= normal_cos_min and |n_p.(x_q - x_p)| <= plane_tolerance t_p
 *       (a comparison with a NaN guide value is false); N, the number of
 *       counting taps, is at least min_taps;
 *   (d) with l_q = lum(c_q) over the counting taps, m = (sum l_q) / N,
 *       s2 = max(0, (sum l_q^2) / N - m m) and cap = m + k sqrt(s2): l_p > cap.
 * Then out[p].rgb = c_p (cap / l_p), alpha copied; cap == 0 (every counting
 * neighbour black) makes the pixel 0.  A pixel with a non-finite colour is left
 * for the filter to repair.  `clamped` (one uint32, may be NULL) is zeroed on
 * the stream and then receives the number of pixels whose rgb changed.
 * IEEE division and square root, contraction allowed: the result agrees with
 * the definition to rounding; the decision (d) may differ where l_p and cap
 * agree to rounding.  Not in place: `out` or `clamped` overlapping an input or
 * each other, and params == NULL, is MRT_ERR_INVALID (and writes nothing). */
int mrt_firefly_clamp(const float* image, const float* guide_n, const float* guide_p, float* out,
                      uint32_t* clamped /* device, may be NULL */, uint32_t width, uint32_t height,
                      const mrt_firefly_params* params, void* stream);

/* ---- adaptive sampling ------------------------------------------------------
 * Spend further samples where the variance plane says the error is: a priority
 * per 64x64 tile, the tiles of highest priority, and draws of an arbitrary
 * list of tiles into counted images beside the accumulation image
 * (mrt_renderer_refine below).  Not in the reference.  The
 * tile is the unit: tile t of a W x H frame, row-major over
 * ceil(W/64) x ceil(H/64) tiles, covers the pixels x in [64 (t % tiles_x), +64),
 * y in [64 (t / tiles_x), +64) that are inside the image.  Device pointers
 * throughout; flags: MRT_FLAG_PRECISE. */
typedef struct mrt_adaptive_params {
  float luminance_floor;   /* > 0: eps of the priority */
} mrt_adaptive_params;
/* Host only.  luminance_floor = 0.01. */
int mrt_adaptive_params_default(mrt_adaptive_params* out);
/* Host only.  MRT_ERR_INVALID (with a message) for a luminance_floor that is
 * not finite or not positive. */
int mrt_adaptive_params_check(const mrt_adaptive_params* p);
/* Merge two counted images (temporal history above) of W*H float4.  Per pixel,
 * with ha = a.w and hb = b.w:
 *   hb == 0, or a component of b.rgb not finite:            out = a, bitwise
 *   otherwise ha == 0, or a component of a.rgb not finite:  out = b, bitwise
 *   otherwise  out.rgb = (ha a.rgb + hb b.rgb) / (ha + hb), out.w = ha + hb,
 *   evaluated as written (the precise build rounds after every operation; the
 *   fast build may contract and divides through a reciprocal).
 * out == a (the same pointer) is allowed; any other overlap of out with an
 * input is MRT_ERR_INVALID. */
int mrt_counted_merge(const float* a, const float* b, float* out, uint32_t width, uint32_t height, uint32_t flags,
                      void* stream);
/* priority[t] (one float per tile) = the sum of v_p / (l_p l_p + eps^2) over the
 * tile's pixels p that are inside the image, filterable (word_p < 0x80000000 in
 * guide_n) and have a finite image[p].rgb; l_p = lum(image[p].rgb), v_p =
 * variance[p] (W*H floats, as mrt_variance writes it), eps =
 * params->luminance_floor.  A tile without such a pixel has priority 0.  The
 * summation order is not defined.  v is the variance of the pixel's MEAN and a
 * frame of a tile costs the same everywhere, so the sum is the relative squared
 * error that a further sample of the tile buys.  The inputs are only read.
 * params == NULL, or `priority` overlapping an input, is MRT_ERR_INVALID. */
int mrt_tile_priority(const float* image, const float* variance, const float* guide_n, float* priority,
                      uint32_t width, uint32_t height, const mrt_adaptive_params* params, uint32_t flags,
                      void* stream);
/* list[r] (uint32, r < count) = the tile of rank r under (priority descending,
 * tile index ascending) among `tiles` priorities; a priority that is not finite
 * or is negative counts as 0.  Exact given the priorities, and the same in both
 * builds.  count == 0, count > tiles, tiles > 16384 (an 8192 x 8192 frame), or
 * list overlapping priority, is MRT_ERR_INVALID. */
int mrt_tile_select(const float* priority, uint32_t tiles, uint32_t count, uint32_t* list, void* stream);
/* The error estimate of a stop rule (mrt_renderer_converge below; DESIGN.md
 * §2.1r).  A pixel COUNTS under mrt_tile_priority's conditions — inside the
 * image, word_p < 0x80000000, image[p].rgb finite — and its term is
 * mrt_tile_priority's, v_p / (l_p l_p + eps^2): the relative squared error of
 * the pixel's mean.  pixels[t] (uint32 per tile) = the number of the tile's
 * counted pixels; mean_error[t] (float per tile) = the sum of their terms /
 * pixels[t], or 0 when there are none (the sum in any order: the kernel adds
 * the float terms and divides in double and rounds once, in both builds).  The
 * estimate is only as good as l_p: with a noisy
 * image below the variance it understates the error severalfold (§2.1r), so
 * `image` is meant to be a denoised one.  The inputs are only read.
 * params == NULL, or an output overlapping an input or the other output, is
 * MRT_ERR_INVALID. */
int mrt_tile_error(const float* image, const float* variance, const float* guide_n, float* mean_error,
                   uint32_t* pixels, uint32_t width, uint32_t height, const mrt_adaptive_params* params,
                   uint32_t flags, void* stream);
typedef struct mrt_error_summary {
  float frame_error;       /* sum of key(t) pixels[t] / sum of pixels[t] over the tiles with pixels[t] > 0 (0 if none;
                              the sums in any order, every operation rounded, the same in both builds) */
  float max_tile_error;    /* the largest key */
  uint32_t tiles_above;    /* A */
  uint32_t tiles_listed;   /* min(A, max_count) */
  uint32_t tiles_counted;  /* tiles with pixels[t] > 0 */
  uint32_t pixels;         /* sum of pixels[t] */
  uint32_t reserved[2];    /* 0 */
} mrt_error_summary;
/* key(t) = mean_error[t] if it is finite and > 0 and pixels[t] > 0, else 0.
 * Tile t is ABOVE iff key(t) > threshold (strictly); A is the number of above
 * tiles.  list[r] (uint32), r < min(A, max_count), = the above tile of rank r
 * under (key descending, tile index ascending); entries beyond that are not
 * written.  Exact given the inputs, and the same in both builds.  `summary`
 * (device memory) is written in full.  The inputs are only read.  A threshold
 * that is not finite or is negative, tiles == 0, tiles > 16384, max_count == 0,
 * max_count > tiles, or any overlap among the four buffers, is MRT_ERR_INVALID. */
int mrt_tile_threshold(const float* mean_error, const uint32_t* pixels, uint32_t tiles, float threshold,
                       uint32_t max_count, uint32_t* list, mrt_error_summary* summary, void* stream);
typedef struct mrt_converge_params {
  float target_error;         /* > 0: a tile is done when its mean error is not above it */
  uint32_t frames_per_pass;   /* >= 1: extra frames a pass gives every tile it draws */
  uint32_t max_passes;        /* >= 1: draws at most */
  uint32_t max_tiles;         /* tiles a pass draws at most; 0 = no cap */
  uint64_t max_tile_frames;   /* tile-frames the whole call may draw; 0 = no budget */
  float luminance_floor;      /* > 0: eps of the estimate */
} mrt_converge_params;
/* Host only.  target_error = 1e-3, frames_per_pass = 8, max_passes = 64,
 * max_tiles = 0, max_tile_frames = 0, luminance_floor = 0.01. */
int mrt_converge_params_default(mrt_converge_params* out);
/* Host only.  MRT_ERR_INVALID (with a message naming the field) for a field
 * outside the ranges above, a non-finite one included. */
int mrt_converge_params_check(const mrt_converge_params* p);

/* ---- renderer (B-1) ------------------------------------------------------ */
typedef struct mrt_renderer_desc {
  const mrt_scene* scene;          /* not owned; must outlive the renderer */
  uint32_t width, height;          /* the reference's W,H = CONTENT_SCALE * drawable */
  uint32_t max_path_length;        /* MAX_PATH_LENGTH (Raytracing.h:23), 1..64 */
  uint64_t seed;                   /* replaces the clock seed (Renderer.mm:109,486) */
  uint32_t shard_rank;             /* 64x64 tile t is rendered iff t % shard_count == shard_rank */
  uint32_t shard_count;            /* 0 or 1 = the whole frame */
  uint32_t flags;                  /* MRT_FLAG_* */
  void* stream;                    /* optional external hipStream_t of the SAME HIP runtime as
                                      libmrt (NULL = own stream).  Never pass a stream created
                                      by another runtime copy (e.g. PyTorch's bundled HIP). */
  float* image;                    /* optional external device image (W*H*4 floats), else owned */
} mrt_renderer_desc;

typedef struct mrt_stats {         /* counters are cumulative since create/resize */
  uint64_t frame_index;            /* frames accumulated since create/resize/reset */
  uint64_t paths;                  /* pixel paths traced by this renderer (owned pixels x frames) */
  uint64_t active_ray_bounces;     /* A: rays alive at the start of each bounce, summed */
  double last_draw_ms;             /* GPU time of the last draw/draw_n (HIP events) */
  double mpaths_per_s;             /* paths of the last draw / last_draw_ms */
  uint64_t kernel_launches;        /* bounce-kernel launches issued */
  double kernel_ms;                /* summed durations of the timed launches (MRT_FLAG_PROFILE) */
  uint64_t owned_pixels;
  uint64_t timed_launches;         /* launches behind kernel_ms (every 8th frame's) */
  uint32_t kernel;                 /* the hot kernel: 0 = wavefront of per-bounce launches, 1 = path megakernel,
                                      2 = streaming wavefront (all bounces of a frame batch in one launch) */
  uint32_t inflight;               /* frame batches in flight (render streams); > 1: launches overlap */
  double span_ms;                  /* summed device-measured spans of the frame batches' render launches
                                      (earliest block start to latest wave end, chip wall clock) */
  uint64_t spans;                  /* frame batches behind span_ms (every batch) */
  uint32_t primary_blocks;         /* 8x8 pixel blocks whose camera rays test a candidate list instead of
                                      traversing the BVH (0 = lists off; MRT_PRIMARY=0 disables) */
  float primary_mean;              /* mean candidate-list length over those blocks */
  /* ABI 7: host cost of the noise schedule (the reference regenerates one
   * table per frame on the CPU before the frame's commit, Renderer.mm:486-496;
   * here mrt_renderer_prepare / draw_n generate a window of tables on the host
   * threads and upload it once) */
  double noise_ms;                 /* host wall time generating noise tables (ABI 8: on the schedule's worker
                                      thread, overlapped with rendering; uploads are asynchronous) */
  uint64_t noise_tables;           /* per-frame tables generated (noise_ms / noise_tables = cost per frame) */
  /* ABI 8: the per-frame cadence (drawInMTKView:, Renderer.mm:587-600).  A
   * draw enqueues its launches without waiting for the GPU: noise tables come
   * from device chunks of 64 frames generated ahead on a worker thread and
   * uploaded on their own stream; the one host wait a draw can reach is the
   * reference's in-flight bound (MaxBuffersInFlight = 3 draws, :16, :593). */
  uint64_t draws;                  /* draw / draw_n calls that enqueued frames */
  uint64_t draws_overlapped;       /* draws enqueued while the previous draw was still executing on the GPU */
  uint64_t inflight_waits;         /* draws that waited for the draw 3 back to finish (the in-flight bound) */
  uint64_t noise_waits;            /* draws (and prepares) that waited for a chunk's host generation */
  uint64_t noise_prefetched;       /* chunks the worker generated ahead and a draw found ready */
} mrt_stats;

int mrt_renderer_create(const mrt_renderer_desc* desc, mrt_renderer** out);
/* drawableSizeWillChange: reallocate, frameIndex = 0 (Renderer.mm:640-657) */
int mrt_renderer_resize(mrt_renderer* r, uint32_t width, uint32_t height);
/* mrt_renderer_resize to the same size with another scene (any scene on the
 * renderer's device: no condition on its topology) in the old one's place.
 * Waits for the renderer's queued work, as resize does; plans the kernel again
 * (kind, stack variant and grid may all change, mrt_stats.kernel with them);
 * re-makes what is sized by the scene (frame queues, stack spill, the guide
 * pass's spill); rebuilds the camera's candidate lists; restarts accumulation at
 * frame 0 and the counters of mrt_stats as resize does; invalidates every
 * derived buffer, the history and the extra images; drops a pending exchange;
 * clears an external image.  The camera, the firefly setting, the flags and
 * both noise schedules persist (the refine schedule's counter is never reset).
 * After set_scene(S); draw(n) the image and the moments are bitwise those of a
 * fresh renderer created on S with the same desc and camera after draw(n).  A
 * failure before the swap (a null, host-only or other-device scene, a kernel
 * that cannot be planned) leaves the renderer as it was.  The old scene may be
 * destroyed once the call returns. */
int mrt_renderer_set_scene(mrt_renderer* r, const mrt_scene* scene);
/* frameIndex = 0 without reallocating: the next frame overwrites every pixel
 * the renderer owns (until then the image keeps its content; pixels written
 * by an exchange or mrt_renderer_tiles_write, and an external image, are
 * cleared here); the cumulative counters of mrt_stats are kept. */
int mrt_renderer_reset(mrt_renderer* r);
/* mrt_renderer_reset plus a new camera (checked with mrt_camera_check): after
 * set_camera(C); draw(n) the image is bitwise that of a fresh renderer with
 * camera C after draw(n).  A draw uses the camera in force when it was
 * enqueued, on every render stream: draws already enqueued keep theirs.  The
 * call does not wait for the GPU: the camera and its candidate lists (rebuilt
 * on the host for a pinhole camera, under the conditions of the default
 * camera's; none with a thin lens) go to a device buffer of their own,
 * uploaded asynchronously and recycled once the draws that read it have
 * finished (five such buffers, allocated at create / resize for the frame's
 * size, so this call allocates nothing).  A camera that fails the check or
 * cannot be installed leaves the renderer as it was, not reset.  Only a host that replaces the camera more than four times while
 * the first of those cameras' draws is still executing waits for that draw.
 * The camera persists across mrt_renderer_resize and mrt_renderer_reset. */
int mrt_renderer_set_camera(mrt_renderer* r, const mrt_camera* cam);
int mrt_renderer_get_camera(const mrt_renderer* r, mrt_camera* out);
/* Generate the noise tables for frames [frame_index, frame_index+n) ahead
 * of time and enqueue their upload (the reference regenerates one slot per
 * frame on the CPU, Renderer.mm:486-496).  Blocks on host generation only.
 * draw_n does the same itself when a chunk is missing, and asks the worker
 * thread for the next chunk of 64 frames while these render. */
int mrt_renderer_prepare(mrt_renderer* r, uint32_t n);
/* One frame: 1 spp, MAX_PATH_LENGTH bounces, running-mean accumulation. */
int mrt_renderer_draw(mrt_renderer* r);
int mrt_renderer_draw_n(mrt_renderer* r, uint32_t n);
/* Wait for all queued work of the renderer. */
int mrt_renderer_sync(mrt_renderer* r);
/* Device pointer of the accumulation image (for an RCCL reduce). */
int mrt_renderer_image(mrt_renderer* r, float** device_image);
/* The renderer's main HIP stream (libmrt's runtime): work queued on it, e.g.
 * mrt_tiles_pack of the image, runs after the renderer's draws without a
 * host round trip. */
int mrt_renderer_stream(mrt_renderer* r, void** stream);
/* Synchronise and copy the image to host memory (rgba must hold W*H*4 floats). */
int mrt_renderer_read_image(mrt_renderer* r, float* rgba, size_t count);
/* MAX_FRAMES (Raytracing.h:28, Renderer.mm:589-590): once frame_index reaches
 * max_frames, draws are no-ops (0 = unlimited, the reference's default). */
int mrt_renderer_set_max_frames(mrt_renderer* r, uint32_t max_frames);
/* Save the image top-down as .pfm (float RGB) or .exr (float RGBA, uncompressed). */
int mrt_renderer_save_image(mrt_renderer* r, const char* path);
/* Denoise the accumulation image into a buffer the renderer owns; the image
 * itself is never written.  Enqueued on the renderer's stream after the draws
 * queued so far, without a host wait (draw; denoise; display_enqueue(slot |
 * MRT_DISPLAY_DENOISED); map).  params NULL = mrt_denoise_params_default for
 * the frames accumulated.  The guide planes are computed on the same stream
 * at the first denoise after create, resize or set_camera, with the camera in
 * force and the renderer's precise or fast build, and kept until the next
 * such call.  The buffers (guides 32 B, denoised 16 B, scratch 16 B per pixel)
 * are allocated at the first denoise and re-made by resize: a renderer that
 * never denoises allocates nothing.  MRT_ERR_STATE when no frame has been
 * accumulated since create, resize, reset or set_camera.  A sharded renderer
 * filters whatever its image holds, which is the whole frame only on rank 0
 * after an exchange. */
int mrt_renderer_denoise(mrt_renderer* r, const mrt_denoise_params* params);
/* The denoised buffer, as read_image / save_image give the image (read
 * synchronises).  MRT_ERR_STATE when no denoise has run at the renderer's
 * current size. */
int mrt_renderer_read_denoised(mrt_renderer* r, float* rgba, size_t count);
int mrt_renderer_save_denoised(mrt_renderer* r, const char* path);   /* .pfm / .exr */
/* Temporal history (the section of that name above).  mrt_renderer_move_camera
 * is mrt_renderer_set_camera that carries what has been accumulated into the
 * new view, as a counted history image that lives BESIDE the accumulation
 * image: the image itself is never written, and after move_camera(C); draw(n)
 * it is bitwise that of a fresh renderer with set_camera(C); draw(n).
 * Everything is enqueued on the renderer's main stream behind the draws queued
 * so far, without a host wait; the buffers (previous guides 32 B, and three
 * counted images of 16 B per pixel, beside the denoiser's guide planes, which
 * are these same ones) are allocated at the first call only and re-made by
 * resize.  In stream order: the guide planes of the camera in force are traced
 * if they are not current; prev = resolve(image, frames accumulated, history if
 * valid); the guide planes become the previous ones; the new camera is
 * installed and the accumulation reset exactly as set_camera does; the new
 * camera's guide planes are traced; history = reproject(prev, ...) with
 * params (NULL = mrt_reproject_params_default).  A camera or params that fail
 * their check, or a camera that cannot be installed, leave the renderer, its
 * image and its history as they were.  A failure after the camera is installed
 * (the reset, the new guide pass or the reprojection: a HIP error) leaves the
 * new camera in force with the history dropped, as after set_camera.  With no
 * frame accumulated and no valid
 * history there is nothing to carry: the call is set_camera.
 * mrt_renderer_set_camera, _reset, _resize and _set_scene invalidate the history.
 * MRT_ERR_STATE on a sharded renderer (shard_count > 1): its image is whole
 * only on rank 0 after an exchange, and a sharded history is not supported. */
int mrt_renderer_move_camera(mrt_renderer* r, const mrt_camera* cam, const mrt_reproject_params* params);
/* Moving geometry: mrt_renderer_move_camera across a scene change.  `scene` is
 * another pose of the scene in force (mrt_scene_motion_compatible) on the same
 * device; cam NULL keeps the camera.  In order: the checks (MRT_ERR_STATE on a
 * sharded renderer; the camera; the params; motion compatibility) — a failed
 * check changes nothing; with no frame accumulated and no valid history the
 * call is set_scene, plus set_camera when cam is given.  Otherwise, in stream
 * order: the old camera's guide planes are traced if they are not current;
 * prev = resolve(image, frames accumulated, history if valid), the extra images
 * merged in, and the same for the moments, exactly as move_camera; the call's
 * one host wait; the swap of mrt_renderer_set_scene, which keeps prev, the
 * previous guide planes and the history buffers; the new camera, if any;
 * mrt_guides_motion(scene, old scene, camera in force) into the guide planes and
 * two motion planes (32 B per pixel, allocated at the first move_scene, re-made
 * by resize); history = mrt_reproject(prev, previous guides, old camera,
 * motion_n, motion_p, params), and likewise the moments history.  The extra
 * images are cleared, as move_camera clears them.  After move_scene(S, C);
 * draw(n) the image is bitwise that of a fresh renderer on S with camera C after
 * draw(n).  A failure after the swap leaves the new scene in force without a
 * history, as set_scene would.  The OLD scene must stay alive until the renderer
 * next synchronises (mrt_renderer_sync, a read, resize, set_scene): the motion
 * pass reads it on the stream. */
int mrt_renderer_move_scene(mrt_renderer* r, const mrt_scene* scene, const mrt_camera* cam /* NULL = keep */,
                            const mrt_reproject_params* params /* NULL = default */);
/* resolved = resolve(image, frames accumulated, history if valid), into a
 * buffer the renderer owns, enqueued without a host wait.  With a valid history
 * and no new frame it is the pure reprojection: the zero-latency frame after a
 * move.  MRT_ERR_STATE when no frame has been accumulated and there is no
 * valid history; MRT_ERR_STATE on a sharded renderer. */
int mrt_renderer_resolve(mrt_renderer* r);
/* The resolved buffer, as read_denoised / save_denoised give the denoised one;
 * its fourth channel is the sample count h + n, not alpha (save writes it as
 * the .exr's A).  MRT_ERR_STATE until a resolve has run at the current size. */
int mrt_renderer_read_resolved(mrt_renderer* r, float* rgba, size_t count);
int mrt_renderer_save_resolved(mrt_renderer* r, const char* path);   /* .pfm / .exr */
/* mrt_renderer_resolve, then mrt_denoise of the resolved buffer into the
 * renderer's denoised buffer (read_denoised, MRT_DISPLAY_DENOISED).  params
 * NULL = mrt_denoise_params_default(max(frames accumulated, 1)), which ignores
 * the history's length: conservative; a host that knows better passes its own,
 * or uses mrt_renderer_denoise_variance, whose filter widths follow the variance. */
int mrt_renderer_denoise_resolved(mrt_renderer* r, const mrt_denoise_params* params);
/* Variance-guided denoising on a renderer created with MRT_FLAG_MOMENTS (the
 * section of that name above).  Such a renderer owns a moments image (16 B per
 * pixel, allocated at create, re-made by resize) that every draw updates with
 * the image, from the one read of the frames' radiance; mrt_renderer_reset
 * restarts it as it restarts the image.  mrt_renderer_move_camera also carries
 * the moments: moments_prev = resolve(moments, frames, moments history if
 * valid) and moments history = reproject(moments_prev, ...) with the guide
 * planes, camera and parameters of the colour history (two more 16-B-per-pixel
 * buffers, allocated at the first move); its validity is the colour
 * history's.  Without the flag nothing of this exists, and every call below
 * that needs it is MRT_ERR_STATE.
 * mrt_renderer_read_moments synchronises as read_image does;
 * mrt_renderer_moments returns the device pointer. */
int mrt_renderer_read_moments(mrt_renderer* r, float* rgba, size_t count);
int mrt_renderer_moments(mrt_renderer* r, float** device_moments);
/* On the main stream, without a host wait: the guide planes if they are not
 * current; resolved = resolve(image, frames, history if valid) (as
 * mrt_renderer_resolve: read_resolved gives it); M = resolve(moments, frames,
 * moments history if valid); mrt_variance(M) into a plane the renderer owns;
 * mrt_denoise_variance(resolved, variance, ...) into the denoised buffer
 * (read_denoised, save_denoised, MRT_DISPLAY_DENOISED).  params NULL =
 * mrt_svgf_params_default.  The buffers are allocated at the first call and
 * re-made by resize.  MRT_ERR_STATE without MRT_FLAG_MOMENTS, and when no frame
 * has been accumulated and there is no valid history. */
int mrt_renderer_denoise_variance(mrt_renderer* r, const mrt_svgf_params* params);
/* The variance plane (W*H floats) the last mrt_renderer_denoise_variance fed to
 * the filter (or the last mrt_renderer_refine chose its tiles by, whichever ran
 * later); synchronises.  MRT_ERR_STATE before one has run at the current size. */
int mrt_renderer_read_variance(mrt_renderer* r, float* plane, size_t count);
/* Firefly suppression on a renderer (the section of that name above).  Off by
 * default; params NULL switches it off.  The params are checked, and a failed
 * check changes nothing.  Needs MRT_FLAG_MOMENTS (MRT_ERR_STATE without it, as
 * mrt_renderer_denoise_variance).  The setting persists across reset, resize,
 * set_camera and move_camera.  While it is on, mrt_renderer_denoise_variance —
 * and through it mrt_renderer_error and mrt_renderer_converge — enqueues,
 * between the resolve and mrt_variance, on the main stream and without a host
 * wait, mrt_firefly_clamp(resolved, guide planes) into a clamped buffer the
 * renderer owns (16 B per pixel and one counter, allocated at the first such
 * call, re-made by resize), and the filter is fed that buffer instead of the
 * resolved one.  The variance plane still comes from the moments; the resolved
 * buffer (read_resolved), the accumulation image, the moments, the extra images
 * and the history are never written by it.  While it is off every call
 * enqueues exactly what it enqueues without this section.  The clamp is biased
 * (it removes energy), and so are the denoised image and the error estimate
 * built on it: DESIGN.md §2.1s.  mrt_renderer_denoise and _denoise_resolved do
 * not clamp. */
int mrt_renderer_set_firefly(mrt_renderer* r, const mrt_firefly_params* params /* NULL = off */);
/* *out = the params in force (mrt_firefly_params_default while it has never been
 * on), *enabled = 1 or 0; either may be NULL. */
int mrt_renderer_get_firefly(const mrt_renderer* r, mrt_firefly_params* out, uint32_t* enabled);
/* The clamped buffer (W*H*4 floats) and *clamped_pixels (may be NULL), the
 * count, of the last clamp; synchronises.  MRT_ERR_STATE before one has run at
 * the current size. */
int mrt_renderer_read_clamped(mrt_renderer* r, float* rgba, size_t count, uint32_t* clamped_pixels);
/* Adaptive sampling on a renderer (the section of that name above): extra
 * frames of chosen tiles, accumulated into two counted images the renderer
 * owns beside its image — E, the extra image (r, g, b, n), and EM, the extra
 * moments (mean l, mean l*l, 0, n), n = the extra samples behind the pixel.
 * The accumulation image, the moments image and mrt_stats.frame_index, .paths
 * and .draws are never touched by these calls: after any of them the image is
 * bitwise that of a renderer that never made them, and stays so through later
 * draws.  Needs MRT_FLAG_MOMENTS: MRT_ERR_STATE without it (so on every
 * sharded renderer), with MRT_FLAG_STATIC_NOISE, and on a renderer forced to
 * the per-bounce kernel (a diagnostic setting), which has no tile-list
 * instantiation.  E, EM, the list and the priorities (32 B per pixel and 8 B
 * per tile) are allocated at the first call and re-made by resize: a renderer
 * that never calls them allocates nothing.  Everything is enqueued without a
 * host wait; the render streams wait for the list through an event.
 *
 * Noise: extra samples read a second noise schedule, seeded
 * desc.seed ^ MRT_REFINE_SEED_XOR, at an extra-frame counter e of their own
 * that advances by `frames` per call whatever the list and is never reset, so
 * no draw and no other refine ever repeats their paths.  A listed tile's extra
 * frame is exactly the frame e of a renderer created with that seed: for each
 * extra frame in order, with c its radiance at pixel p and n = (uint32_t)E[p].w,
 *   E[p].rgb = accumulate(E[p].rgb, c, n), E[p].w = n + 1    (n == 0 overwrites)
 * and EM[p] the same over (l, l*l, 0), l = lum(c).
 *
 * While E holds samples every resolve merges them: resolved =
 * mrt_counted_merge(resolve(image, frames, history), E) and likewise the
 * resolved moments with EM — in mrt_renderer_resolve, _denoise_resolved and
 * _denoise_variance (whose mrt_variance therefore sees the n they add: a refined
 * tile's priority falls by itself) and in mrt_renderer_move_camera, which
 * carries the merged images into the history and then clears E and EM.
 * mrt_renderer_reset, _set_camera and _resize clear them as well.
 *
 * The diagnostic counters of mrt_stats (active_ray_bounces, kernel_launches,
 * span_ms, spans, kernel_ms, timed_launches, last_draw_ms, mpaths_per_s,
 * draws_overlapped, inflight_waits) include the refine launches. */
#define MRT_REFINE_SEED_XOR 0x9E3779B97F4A7C15ull
/* `frames` (>= 1) extra frames of the `count` tiles in the host array `tiles`:
 * distinct, each < tiles_x * tiles_y, 1 <= count.  A bad list or frames == 0 is
 * MRT_ERR_INVALID and changes nothing.  The list is copied before the call
 * returns. */
int mrt_renderer_draw_tiles(mrt_renderer* r, const uint32_t* tiles, uint32_t count, uint32_t frames);
/* One adaptive pass, in stream order: the guide planes if they are not current;
 * the merged resolved image and moments as above; mrt_variance with
 * mrt_svgf_params_default; mrt_tile_priority (params NULL =
 * mrt_adaptive_params_default); mrt_tile_select of tile_count tiles into a
 * device list; `frames` extra frames of those tiles as mrt_renderer_draw_tiles
 * draws them.  MRT_ERR_STATE when no frame has been accumulated and there is no
 * valid history; frames == 0, tile_count == 0 or tile_count above the frame's
 * tile count is MRT_ERR_INVALID. */
int mrt_renderer_refine(mrt_renderer* r, uint32_t frames, uint32_t tile_count, const mrt_adaptive_params* params);
/* E and EM (W*H*4 floats), the priorities of the last refine (one float per
 * tile) and the list of the last refine or draw_tiles (*count entries, at most
 * `capacity`).  All synchronise.  MRT_ERR_STATE before the first refine or
 * draw_tiles at the current size (the priorities: before the first refine). */
int mrt_renderer_read_extra(mrt_renderer* r, float* rgba, size_t count);
int mrt_renderer_read_extra_moments(mrt_renderer* r, float* rgba, size_t count);
int mrt_renderer_read_tile_priority(mrt_renderer* r, float* priority, size_t count);
int mrt_renderer_read_tile_list(mrt_renderer* r, uint32_t* tiles, size_t capacity, uint32_t* count);
typedef struct mrt_refine_stats {   /* cumulative since create; never reset */
  uint64_t passes;         /* refine and draw_tiles calls that enqueued frames */
  uint64_t extra_frames;   /* the extra-frame counter e */
  uint64_t tile_frames;    /* sum over those calls of tiles x frames */
  uint64_t paths;          /* pixel paths traced by them (pixels of the listed tiles inside the image x frames);
                              a refine's list is chosen on the device, so its pixels are counted when its
                              list is next read back: mrt_renderer_refine_stats synchronises */
} mrt_refine_stats;
int mrt_renderer_refine_stats(mrt_renderer* r, mrt_refine_stats* stats);
/* Sampling to a target error.  mrt_renderer_error estimates
 * and draws nothing: mrt_renderer_denoise_variance(r, svgf) (NULL = its
 * default); mrt_tile_error(the denoised buffer, the variance plane that call
 * fed to the filter, the guide normals) with eps = luminance_floor (0 = 0.01)
 * into two per-tile planes the renderer owns; mrt_tile_threshold(threshold,
 * max_count = the frame's tile count) into the renderer's tile list, which
 * then holds out->tiles_listed tiles (read_tile_list: MRT_ERR_STATE while that
 * is 0); and the summary copied to pinned host memory and WAITED FOR — the one
 * host wait of the call, which therefore also waits for every draw enqueued
 * before it.  The resolved, variance and denoised buffers are left as
 * denoise_variance leaves them.  Preconditions: those of mrt_renderer_refine
 * (MRT_FLAG_MOMENTS, not sharded, no MRT_FLAG_STATIC_NOISE, not the per-bounce
 * kernel), more than 16384 tiles is MRT_ERR_INVALID, and MRT_ERR_STATE when
 * fewer than svgf.min_frames frames have been accumulated and there is no
 * valid history: below min_frames the variance is the spatial estimate, which
 * is off by a factor of 8 to 30 as an error estimate.  Extra samples do not
 * count towards that. */
int mrt_renderer_error(mrt_renderer* r, const mrt_svgf_params* svgf, float luminance_floor, float threshold,
                       mrt_error_summary* out);
/* The two planes of the last mrt_renderer_error or _converge (one float and one
 * uint32 per tile; `count` = the capacity of each); synchronises.
 * MRT_ERR_STATE before one has run at the current size. */
int mrt_renderer_read_tile_error(mrt_renderer* r, float* mean_error, uint32_t* pixels, size_t count);
typedef struct mrt_converge_result {
  uint32_t converged;           /* 1: the last estimate found no tile above the target */
  uint32_t passes;              /* draws made */
  uint64_t tile_frames;         /* sum over them of tiles x frames_per_pass */
  mrt_error_summary first, last;   /* the first and the last estimate (the same one when passes == 0) */
} mrt_converge_result;
/* Repeats: estimate as mrt_renderer_error with the default svgf parameters,
 * eps = params->luminance_floor and threshold = params->target_error;
 * n = min(tiles_above, max_tiles or the tile count, floor(what is left of
 * max_tile_frames / frames_per_pass)); tiles_above == 0 stops with
 * converged = 1; otherwise n == 0 or max_passes draws made stops with
 * converged = 0; otherwise frames_per_pass extra frames of the first n listed
 * tiles (the n worst), from the device list exactly as mrt_renderer_refine
 * hands its list over: E, EM, the refine noise schedule and mrt_refine_stats
 * behave as documented there, and the accumulation image, the moments image and
 * mrt_stats.frame_index, .paths and .draws are never touched.  The call always
 * ends on an estimate, so the resolved, variance and denoised buffers are
 * current for everything drawn and read_denoised after it is the finished
 * picture.  One host wait per estimate.  params NULL =
 * mrt_converge_params_default; a failed parameter or state check changes
 * nothing.  The rule looks at its own estimate: a tile whose estimate happens
 * to fall low stops early and is not looked at again, so the error of the
 * tiles it declares done is, on average, above what it reports (optional
 * stopping; stated, not corrected). */
int mrt_renderer_converge(mrt_renderer* r, const mrt_converge_params* params, mrt_converge_result* out);
int mrt_renderer_stats(const mrt_renderer* r, mrt_stats* stats);
int mrt_renderer_destroy(mrt_renderer* r);

/* ---- misc ----------------------------------------------------------------- */
const char* mrt_last_error(void);
int mrt_abi_version(void);
/* The deterministic noise table of SURVEY.md A.3 for frame `frame` (-1 = the
 * initial table), 64*64*4 floats, host memory. */
int mrt_noise_table(uint64_t seed, int64_t frame, float* out16384);
/* Host helper (no device needed): the pixels a shard owns under the 64x64
 * tile round-robin (tile t -> shard t % shard_count), as a W*H byte mask
 * (row 0 = bottom); returns the number of owned pixels via *owned. */
int mrt_shard_mask(uint32_t width, uint32_t height, uint32_t shard_rank, uint32_t shard_count, uint8_t* mask,
                   uint64_t* owned);
/* Display (blitFragment, Shaders.metal:33-70): the reference's compile-time
 * blit switches as flags — tone map 1 - exp(-c) (ENABLE_TONE_MAPPING),
 * toSRGB (MANUAL_SRGB, Raytracing.h:130-135), and COMPARISON_MODE 1..4
 * against a reference image (e.g. a Mitsuba golden, Renderer.mm:162-253)
 * scaled by compare_scale (COMPARISON_SCALE = 10).  Device pointers, W*H
 * RGBA32F in and out; `reference` may be NULL when no compare mode is set. */
#define MRT_DISPLAY_TONEMAP 1u
#define MRT_DISPLAY_SRGB 2u
#define MRT_DISPLAY_DENOISED 4u   /* mrt_renderer_display / _display_enqueue: blit the denoised buffer instead of the
                                     image (MRT_ERR_STATE without a denoise at the current size); mrt_display ignores it */
#define MRT_DISPLAY_RESOLVED 8u   /* ... blit the resolved buffer (MRT_ERR_STATE without a resolve at the current size;
                                     MRT_ERR_INVALID together with MRT_DISPLAY_DENOISED); mrt_display ignores it */
#define MRT_DISPLAY_COMPARE(mode) ((uint32_t)(mode) << 8)   /* 1 abs, 2 ref-to-color, 3 color-to-ref, 4 luminance */
int mrt_display(const float* image, const float* reference, float* out, uint32_t width, uint32_t height,
                uint32_t flags, float compare_scale, void* stream);

/* Golden images: loadReferenceImage (renderer/Renderer.mm:162-253) reads
 * Media/reference/<scene>-<L>.exr (Mitsuba goldens: ZIP-compressed half RGB)
 * and flips it into the comparison texture.  mrt_image_load_exr decodes a
 * scanline OpenEXR file (NONE / ZIPS / ZIP compression, HALF / FLOAT / UINT
 * channels; R, G, B, A by name, A = 1 if absent) into host RGBA32F with
 * row 0 = BOTTOM; call with rgba = NULL to get the size first.  No device. */
int mrt_image_load_exr(const char* path, float* rgba, size_t capacity_floats, uint32_t* width, uint32_t* height);
/* The renderer's comparison image (COMPARISON_MODE != 0): the golden at
 * `path`, which must have the renderer's W x H, uploaded to the device. */
int mrt_renderer_load_reference(mrt_renderer* r, const char* path);
/* blitFragment for a host without its own GPU code: mrt_display of the
 * accumulation image (tone map / sRGB / compare mode against the loaded
 * reference) into host memory (rgba: W*H*4 floats, row 0 = bottom). */
int mrt_renderer_display(mrt_renderer* r, uint32_t flags, float compare_scale, float* rgba, size_t count);
/* The same blit without a host wait, for a frame loop that keeps frames in
 * flight as the reference does (MaxBuffersInFlight = 3, its semaphore:
 * renderer/Renderer.mm:16,593-600).  _enqueue queues the blit of the image
 * as of the draws queued so far, and its copy into display slot `slot`
 * (< MRT_DISPLAY_SLOTS; pinned host memory owned by the renderer), on the
 * renderer's stream, and returns at once.  _map waits for that slot's copy
 * and returns its pixels (W*H*4 floats, row 0 = bottom), valid until the
 * slot is enqueued again or the renderer is resized or destroyed.  Typical
 * loop: draw; enqueue(frame % 3); present map((frame - 2) % 3). */
#define MRT_DISPLAY_SLOTS 3u
int mrt_renderer_display_enqueue(mrt_renderer* r, uint32_t flags, float compare_scale, uint32_t slot);
int mrt_renderer_display_map(mrt_renderer* r, uint32_t slot, const float** rgba, size_t* count);

/* Multi-GPU exchange of the accumulation image: a shard's
 * owned 64x64 tiles packed densely, [k][64*64] RGBA32F for its k-th owned
 * tile (tile t = shard_rank + k*shard_count, row-major tiles; zeros outside
 * the image).  Device pointers; pack reads `image`, unpack writes only the
 * shard's pixels of `image`.  Bitwise moves.  mrt_tiles_packed_floats gives
 * the packed size (host, no device). */
int mrt_tiles_packed_floats(uint32_t width, uint32_t height, uint32_t shard_rank, uint32_t shard_count,
                            uint64_t* floats);
int mrt_tiles_pack(const float* image, uint32_t width, uint32_t height, uint32_t shard_rank,
                   uint32_t shard_count, float* packed, void* stream);
int mrt_tiles_unpack(const float* packed, uint32_t width, uint32_t height, uint32_t shard_rank,
                     uint32_t shard_count, float* image, void* stream);
/* ---- multi-GPU exchange through RCCL --------------------
 * One process per GPU.  Rank 0 makes a unique id, the host distributes its
 * MRT_COMM_ID_BYTES bytes to every rank (any control channel: MPI, a socket,
 * torch.distributed gloo), each rank creates its communicator on its device,
 * and a renderer created with shard_rank = rank, shard_count = nranks
 * exchanges its accumulation image with one collective, enqueued on the
 * renderer's stream (no host round trip):
 *   MRT_EXCHANGE_GATHER — pack the rank's owned 64x64 tiles densely
 *     (mrt_tiles_pack), one ncclGather of the packed tiles to rank 0
 *     (1/N of the image per rank; on xGMI rank 0 receives the N-1 slabs
 *     over N-1 links at once), rank 0 unpacks them into its image;
 *   MRT_EXCHANGE_REDUCE — one in-place ncclReduce(sum) of the RGBA32F image
 *     to rank 0 (non-owned pixels are 0, so the sum is the 1-GPU image).
 * Either way rank 0's image is bitwise the single-device render.
 * MRT_EXCHANGE_OVERLAP (gather only): the collective runs on the
 * communicator's own stream after the pack, and rank 0's unpack is deferred
 * to the next exchange (or mrt_renderer_exchange_flush), so the transfer
 * overlaps the renderer's next draw; the packed tiles are double-buffered.
 * The reference has no multi-GPU path (a single Metal device). */
#define MRT_COMM_ID_BYTES 128
#define MRT_EXCHANGE_GATHER 1u
#define MRT_EXCHANGE_REDUCE 2u
#define MRT_EXCHANGE_OVERLAP 0x100u
typedef struct mrt_comm mrt_comm;
int mrt_comm_unique_id(void* id, size_t bytes);   /* ncclGetUniqueId: bytes >= MRT_COMM_ID_BYTES */
int mrt_comm_create(const void* id, uint32_t nranks, uint32_t rank, int device, mrt_comm** out);
int mrt_comm_destroy(mrt_comm* comm);
int mrt_renderer_exchange(mrt_renderer* r, mrt_comm* comm, uint32_t mode);
/* Complete a deferred (MRT_EXCHANGE_OVERLAP) exchange on the renderer's stream
 * and wait, bounded by the communicator's timeout, for the collective to
 * complete on the device (ABI 9; mrt_renderer_sync / _read_image wait the same
 * way).  Meanwhile the communicator's asynchronous error is polled
 * (ncclCommGetAsyncError); on an error or at the timeout it is aborted
 * (ncclCommAbort) and MRT_ERR_COMM is returned with mrt_last_error() set. */
int mrt_renderer_exchange_flush(mrt_renderer* r);
/* ABI 9: the bound of those waits (0 = the default, 120000 ms), and a
 * non-blocking health check (MRT_OK, or MRT_ERR_COMM once aborted or when an
 * asynchronous error is pending — which aborts it). */
int mrt_comm_set_timeout(mrt_comm* comm, uint32_t timeout_ms);
int mrt_comm_check(mrt_comm* comm);
/* Test entry (ABI 9): inject a failure into the communicator's health checks
 * — 1: an asynchronous error is reported; 2: its collectives never complete
 * (the bounded wait reaches the timeout); 0: none.  The abort that follows is
 * the real one (ncclCommAbort). */
int mrt_debug_comm_fail(mrt_comm* comm, uint32_t mode);
/* Host-side exchange for hosts with their own transport (MPI, gloo, ...):
 * the renderer's owned tiles packed to host memory (mrt_tiles_packed_floats
 * floats for its shard), and another shard's packed tiles written into the
 * image.  Both synchronise the renderer. */
int mrt_renderer_tiles_read(mrt_renderer* r, float* host_packed, size_t floats);
int mrt_renderer_tiles_write(mrt_renderer* r, uint32_t shard_rank, const float* host_packed, size_t floats);

/* Wait for work queued by libmrt on `stream` (NULL = everything on the device
 * libmrt's runtime has queued). */
int mrt_synchronize(void* stream);
/* Stream-ordered completion markers in libmrt's runtime (the host-side
 * ordering between libmrt's work and another runtime's, e.g. the multi-GPU
 * exchange): record an event on `stream` (NULL = the default stream),
 * creating it first when *event is NULL; wait for it; destroy it. */
int mrt_event_record(void* stream, void** event);
int mrt_event_synchronize(void* event);
int mrt_event_destroy(void* event);
/* Diagnostics: cycles spent per phase of the bounce loop, summed over the
 * waves of the last launch of each bounce index % 4 (out[0..4] = load, trace, shade, shadow, finish; out[5] = wave iterations).
 * Non-zero only in the separately built stamp library (make stamps). */
int mrt_debug_stamps(uint64_t* out8, int reset);
/* Diagnostics: per-wave timeline of the last bounce launch of each bounce
 * index % 4: out[((b % 4) * 8192 + wave) * 16 + k], k = {first iteration,
 * exit, iterations | exit reason << 32 (1 input exhausted, 2 output segment
 * full), last grab, end of the last grab's work, summed grab latency, max
 * grab latency, last grab's latency, phase cycles 0..4} in 100 MHz real-time ticks; n = number
 * of uint64 to copy (at most 4 * 8192 * 16).  Zeros outside the stamp library. */
int mrt_debug_wave_times(uint64_t* out, size_t n);
/* Diagnostics (ABI 7): lane-occupancy counters of the separately built
 * lane-statistics library (make variant VNAME=lanes VFLAGS=-DMRT_LANESTATS=1):
 * out[k] for k < n (at most 64), summed over every wave of every launch since
 * the last reset — per traversal loop the wave iterations and the active
 * lanes in them (tools/lane_stats.py names the slots).  Zeros otherwise. */
int mrt_debug_lanes(uint64_t* out, size_t n, int reset);
/* Test entry: the scene's leaf-box sweep list (dev_sweep.h sweep_nearest) —
 * *count leaf records of the main tree, of which min(*count, capacity) are
 * copied to `records` (may be NULL) as 8 floats each: (lo.xyz, bits(leaf
 * ref)), (hi.xyz, 0), the leaf's child box as its parent node holds it, in
 * node and slot order; 0 records for a tree the sweep cannot take (more than
 * 32 leaves, or a leaf root).  *enabled: nearest queries of the bounce and
 * stream kernels sweep this list instead of walking the tree (the whole
 * scene is staged in LDS and MRT_SWEEP=0 is not set under MRT_DIAG=1). */
int mrt_debug_sweep_list(const mrt_scene* scene, float* records, uint32_t capacity, uint32_t* count,
                         uint32_t* enabled);
/* Test entry: the list the sweep kernels get, derived from the per-leaf list
 * above — *count records (at most 32; more, from a non-default leaf size,
 * and the scene walks), one per group of at most two triangles: a
 * two-triangle leaf, two single-triangle leaves paired (repeatedly the pair
 * whose union box has the smallest surface area, if below the sum of the
 * members' areas), a single left alone, or ceil(n / 2) records with the
 * leaf's box for a leaf of n > 2 triangles.  min(*count, capacity) are copied
 * to `records` (may be NULL) as 8 floats each: (lo.xyz, bits(ka | kb << 16)),
 * (hi.xyz, 0) — the component-wise min / max of the members' boxes and the
 * two leaf-ordered triangle indices (kb == ka: one) — and their primitive ids
 * to prims[2 i], prims[2 i + 1] (may be NULL).  A record stands at its first
 * member's position.  MRT_SWEEP_PAIRS=0 under MRT_DIAG=1: no two leaves share
 * a record. */
int mrt_debug_sweep_pairs(const mrt_scene* scene, float* records, uint32_t* prims, uint32_t capacity,
                          uint32_t* count);
/* Test entry: phase 1's list of a scene whose nearest queries sweep (none, and
 * *count = 0, for one that walks) — one record per record of
 * mrt_debug_sweep_pairs, in its order, of which min(*count, capacity) are
 * copied to `records` (may be NULL) as 8 floats each: (c.xyz, bits(id)),
 * (e.xyz, bits(1 << id)), the centre and half-extent of the record's box with
 * [c - e, c + e] containing [lo, hi] on every axis in exact arithmetic and e
 * the smallest such float.  The fast build's phase 1 tests these (three fused
 * multiply-adds per axis); phase 2 and the precise build keep lo / hi. */
int mrt_debug_sweep_phase1(const mrt_scene* scene, float* records, uint32_t capacity, uint32_t* count);
/* Test entry: the rest pops one pass of the stream kernel's queue levels makes
 * before it recycles a ray with leaves left to test (kern_bounce.h bounce_wave),
 * for a scene whose nearest queries sweep.  32: never, the default (every cap
 * measured slower); MRT_SWEEP_CAP=<n> under MRT_DIAG=1 sets another. */
int mrt_debug_sweep_cap(const mrt_scene* scene, uint32_t* cap);
/* Test entry (ABI 7): rank 0's unpack of an N-rank gather without a
 * communicator.  `gathered` (host) holds nranks slabs of
 * mrt_tiles_packed_floats(W, H, 0, nranks) floats, rank k's at slab k, as the
 * gather of MRT_EXCHANGE_GATHER delivers them; the renderer (shard_rank 0,
 * shard_count nranks) unpacks slabs 1..N-1 into its image with the RCCL
 * path's own unpack.  Synchronises the renderer. */
/* Test entry: the main tree's BVH4 nodes as the host holds them (128 bytes
 * each, mrt_layout.h); *count nodes, min(*count, capacity) copied. */
int mrt_debug_bvh_nodes(const mrt_scene* scene, float* nodes, uint32_t capacity, uint32_t* count);
int mrt_debug_exchange_unpack(mrt_renderer* r, uint32_t nranks, const float* gathered, size_t floats);
/* Test entry (ABI 9, host only, no device): the traversal culling slack each
 * ray's nearest hit needs in the scene's main tree.  For ray record i
 * (origin, minDistance, direction, maxDistance at `stride` bytes) and its
 * brute-force nearest hit intersections[i] (reference layout, distance < 0 =
 * miss): out[4i + 0..1] = the largest (t_entry - t_hit) / t_hit over the child
 * boxes on the path from the root to the hit primitive's leaf, with the slab
 * test in the precise build's arithmetic ((p - o) * inv) and the fast build's
 * (fma(p, inv, -o * inv)); out[4i + 2..3] = the same for the near ties — the
 * triangles sharing a vertex position with the hit whose triangle test passes
 * within first-order rounding bounds (4u per operation chain), each at the
 * smallest t those bounds allow, within 2^-10 of t_hit (what a differently
 * rounding triangle test may report instead).  +inf if the ray
 * misses one of those boxes altogether, -inf for none.  The kernels cull a
 * child only when its entry lies beyond h.t * (1 + 2^-11) (dev_traverse.h
 * kCullScale): every value below 2^-11 is a hit no visiting order can lose
 * (DESIGN.md §3.1). */
int mrt_debug_box_margin(const mrt_scene* scene, const void* rays, uint32_t stride, uint32_t count,
                         const void* intersections, float* out);
/* Test entry (ABI 9, host only): q[i] = n[i] / d through the kernels' exact
 * division by a launch divisor (kernels.h magic_div: the multiplier the
 * renderer passes, applied as the kernels' mulhi + shift), n[i] < 2^31. */
int mrt_debug_magic_div(uint32_t d, const uint32_t* n, uint32_t count, uint32_t* q);
/* Test / measurement entry: the implementation mrt_denoise uses for an
 * iteration, process-wide — 0: the shipped choice per step; 1: every tap from
 * global memory; 2: tile and halo staged in LDS at every step it supports
 * (s <= 4; the direct one above).  The results agree to rounding. */
int mrt_debug_denoise_path(uint32_t path);
/* Measurement entry (tools/denoise_time.py): ONE iteration of mrt_denoise at
 * step 2^step_log2 (<= 14) with implementation `path` (as above), image ->
 * out; params->iterations is not used.  Touches no process-wide state. */
int mrt_debug_denoise_step(const float* image, const float* guide_n, const float* guide_p, float* out, float* scratch,
                           uint32_t width, uint32_t height, const mrt_denoise_params* params, uint32_t step_log2,
                           uint32_t path, void* stream);
/* Measurement entry (tools/variance_time.py): ONE iteration of
 * mrt_denoise_variance at step 2^step_log2 (<= 14) with implementation `path`,
 * as a first iteration (v from `variance`) that is not the last (out.w = v');
 * params->iterations is not used.  Touches no process-wide state. */
int mrt_debug_denoise_variance_step(const float* image, const float* variance, const float* guide_n,
                                    const float* guide_p, float* out, uint32_t width, uint32_t height,
                                    const mrt_svgf_params* params, uint32_t step_log2, uint32_t path, void* stream);
/* Number of HIP devices visible (0 when none; never fails). */
int mrt_device_count(void);

#ifdef __cplusplus
}
#endif
#endif /* MRT_H_ */
