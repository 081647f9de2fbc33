/*
 * render.c — the C host of the MI355X path tracer: a command-line driver over
 * the C ABI of include/mrt.h (libmrt.so), in place of the reference's app
 * shell (macos/GameViewController.m:10-28 creates the Renderer
 * (renderer/Renderer.h:3-8), sizes it and lets the MTKView call
 * drawInMTKView: once per display refresh; the menu's "Save current image"
 * calls saveCurrentImage).  Here:
 *
 *   -initWithMetalKitView:            mrt_scene_create + mrt_renderer_create
 *   -drawInMTKView: x spp              mrt_renderer_draw_n (1 spp per frame)
 *   -saveCurrentImage                  mrt_renderer_save_image (.pfm / .exr)
 *   window-title stats                 mrt_renderer_stats
 *
 * Multi-GPU (--gpus N): the process forks N ranks BEFORE any
 * libmrt call (no HIP state crosses a fork); rank k renders the 64x64 tiles
 * t % N == k on device k, and the owned tiles reach rank 0 through
 *   --exchange rccl  libmrt's RCCL gather (mrt_comm_*; the 128-byte unique id
 *                    travels from rank 0 to the others over pipes), or
 *   --exchange host  packed tiles through host memory and pipes
 *                    (mrt_renderer_tiles_read / _write; several ranks may then
 *                    share one GPU).
 * Rank 0 writes the image.  Exit status 0 on success, 1 on any error (the
 * message from mrt_last_error on stderr).
 *
 * usage: mrt_render --scene NAME|PATH.obj [--mtl PATH] [--procedural N]
 *                   [--w W] [--h H] [--spp N] [--L L] [--seed S] [--out x.pfm|x.exr]
 *                   [--precise] [--static-noise] [--no-accumulate] [--debug-material]
 *                   [--gpus N] [--device D] [--exchange rccl|host]
 *                   [--eye x,y,z] [--target x,y,z] [--up x,y,z] [--fov DEGREES]
 *                   [--aperture LENS_RADIUS] [--focus DISTANCE]
 *                   [--denoise] [--denoise-iterations N] [--denoise-sigma-color S]
 *                   [--denoise-variance] [--svgf-iterations N] [--svgf-sigma-luminance X]
 *                   [--firefly [K]]
 *                   [--orbit-steps K --orbit-degrees D]
 *                   [--then-scene NAME|PATH.obj [--then-mtl PATH]]
 *                   [--refine-passes P --refine-frames F --refine-tiles K]
 *                   [--target-error E [--converge-frames F] [--converge-max-passes P]
 *                    [--converge-budget N]]
 * --target-error E (single rank only, not with --refine-*; the other three
 * need it): sampling to a target error.  The renderer accumulates luminance
 * moments, and after the draws mrt_renderer_converge with target_error = E,
 * frames_per_pass = F, max_passes = P and max_tile_frames = N (each the default
 * of mrt_converge_params_default when not given) draws extra frames of the
 * tiles whose estimated relative squared error is above E until none is.  One
 * line on stdout reports it: passes, tile-frames, the first and the last
 * frame_error, and converged.  --out then receives what --denoise-variance
 * gives, which holds the extra samples.
 * --refine-passes P (single rank only; --refine-frames F, default 1, and
 * --refine-tiles K, default a quarter of the frame's 64x64 tiles, imply it with
 * P = 1): adaptive sampling.  The renderer accumulates luminance moments, and
 * after the draws (with --orbit-steps after the last move's draw) P times
 * mrt_renderer_refine(F, K): F extra frames of the K tiles of highest
 * priority.  --out then receives an image that holds the extra samples: that of
 * --denoise-variance, or of --denoise (mrt_renderer_denoise_resolved), or else
 * the resolved image.
 * --orbit-steps K --orbit-degrees D (single rank only): after the first --spp
 * frames, K times: the eye turns about the vertical axis through the target
 * by D degrees (step k stands at k D from the first eye; the axis is the
 * world's y axis whatever --up says; --orbit-degrees without --orbit-steps is
 * an error), the camera moves
 * with mrt_renderer_move_camera, which carries the accumulated history along,
 * and --spp frames are drawn.  --out then receives the resolved image
 * (mrt_renderer_resolve / _save_resolved), or with --denoise the image of
 * mrt_renderer_denoise_resolved.
 * --then-scene OBJ [--then-mtl MTL] (single rank only, not with --orbit-steps):
 * moving geometry.  OBJ is another pose of --scene (the same triangles and
 * materials in the same order, mrt_scene_motion_compatible; --procedural applies
 * to both).  After the first --spp frames mrt_renderer_move_scene puts it in the
 * first scene's place, carrying the accumulated history through the motion, and
 * --spp more frames are drawn.  --out then receives the resolved image, or what
 * --denoise / --denoise-variance make of it.
 * --denoise: after the last draw (and the exchange: only rank 0, which holds
 * the whole image, denoises) mrt_renderer_denoise with the defaults for --spp
 * frames, and --out receives the denoised image (mrt_renderer_save_denoised);
 * the two other options override a default and imply --denoise.
 * --denoise-variance (single rank only, not with --denoise): the renderer
 * accumulates luminance moments (MRT_FLAG_MOMENTS) and --out receives the image
 * of mrt_renderer_denoise_variance, run after the last draw (with --orbit-steps
 * after the last move's draw); --svgf-iterations and --svgf-sigma-luminance
 * override a default of mrt_svgf_params_default and imply it.
 * --firefly [K] (with --denoise-variance or --target-error, a usage error
 * otherwise): mrt_renderer_set_firefly with mrt_firefly_params_default, k = K
 * if given — outliers are clamped ahead of the variance-guided filter (biased:
 * energy is removed, not redistributed).
 * The camera options go through mrt_camera_look_at / mrt_renderer_set_camera
 * (fov: full horizontal angle; --aperture > 0: a thin lens, focused at --focus
 * or else on the target); without any of them the reference's camera renders.
 */
#define _GNU_SOURCE
#include <errno.h>
#include <inttypes.h>
#include <limits.h>
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <sys/types.h>
#include <sys/wait.h>
#include <time.h>
#include <unistd.h>

#include "mrt.h"

typedef struct {
  const char* scene;
  const char* mtl;
  const char* then_scene;   /* moving geometry (mrt_renderer_move_scene) */
  const char* then_mtl;
  const char* out;
  const char* exchange;
  uint32_t procedural, width, height, spp, max_path_length, gpus, flags;
  int device;
  uint64_t seed;
  /* camera (mrt_camera_look_at): set_camera is called when any of these is given */
  int camera_set, pose_set, focus_set;   /* pose_set: --eye, --target, --up or --fov */
  float eye[3], target[3], up[3], fov, aperture, focus;
  /* denoised output (mrt_renderer_denoise) */
  int denoise, denoise_iterations_set, denoise_sigma_set;
  uint32_t denoise_iterations;
  float denoise_sigma_color;
  /* variance-guided denoising (mrt_renderer_denoise_variance) */
  int denoise_variance, svgf_iterations_set, svgf_sigma_set;
  uint32_t svgf_iterations;
  float svgf_sigma_luminance;
  /* firefly suppression (mrt_renderer_set_firefly) */
  int firefly, firefly_k_set;
  float firefly_k;
  /* orbit with temporal history (mrt_renderer_move_camera) */
  /* adaptive sampling (mrt_renderer_refine) */
  uint32_t refine_passes, refine_frames, refine_tiles;
  int refine_set;
  /* sampling to a target error (mrt_renderer_converge) */
  int target_set, converge_set;
  float target_error;
  uint32_t converge_frames, converge_max_passes;
  uint64_t converge_budget;
  uint32_t orbit_steps;
  int orbit_degrees_set;
  float orbit_degrees;
} options;

/* "x,y,z" -> three floats */
static int parse_vec3(const char* s, float* out) {
  char tail = 0;
  return sscanf(s, "%f,%f,%f%c", &out[0], &out[1], &out[2], &tail) == 3 ? 0 : -1;
}

static int die(const char* what) {
  fprintf(stderr, "mrt_render: %s: %s\n", what, mrt_last_error());
  return 1;
}

static void usage(void) {
  fprintf(stderr,
          "usage: mrt_render --scene NAME|PATH.obj [--mtl PATH] [--procedural N] [--w W] [--h H]\n"
          "                  [--spp N] [--L L] [--seed S] [--out x.pfm|x.exr] [--precise]\n"
          "                  [--static-noise] [--no-accumulate] [--debug-material]\n"
          "                  [--gpus N] [--device D] [--exchange rccl|host]\n"
          "                  [--eye x,y,z] [--target x,y,z] [--up x,y,z] [--fov DEGREES]\n"
          "                  [--aperture LENS_RADIUS] [--focus DISTANCE]\n"
          "                  [--denoise] [--denoise-iterations N] [--denoise-sigma-color S]\n"
          "                  [--denoise-variance] [--svgf-iterations N] [--svgf-sigma-luminance X]\n"
          "                  [--firefly [K]]\n"
          "                  [--orbit-steps K --orbit-degrees D]\n"
          "                  [--then-scene NAME|PATH.obj [--then-mtl PATH]]\n"
          "                  [--refine-passes P --refine-frames F --refine-tiles K]\n"
          "                  [--target-error E [--converge-frames F] [--converge-max-passes P] [--converge-budget N]]\n"
          "  --orbit-steps K --orbit-degrees D (one rank): after the first --spp frames, K times: turn the eye by D\n"
          "  degrees about the world's vertical (y) axis through the target, whatever --up says, move the camera\n"
          "  keeping the accumulated history, draw --spp frames; --out gets the resolved image.  --orbit-degrees\n"
          "  alone is an error.\n"
          "  --then-scene OBJ [--then-mtl MTL] (one rank, not with --orbit-steps): OBJ is another pose of --scene;\n"
          "  after the first --spp frames it takes the scene's place, the accumulated history carried through the\n"
          "  motion, and --spp more frames are drawn; --out gets the resolved image.\n"
          "  --refine-passes P --refine-frames F --refine-tiles K (one rank): after the draws, P times F extra frames\n"
          "  of the K 64x64 tiles whose variance says they need them most; --out gets an image that holds them.\n"
          "  --target-error E (one rank, not with --refine-*): after the draws, F extra frames per pass of the tiles\n"
          "  whose estimated relative squared error is above E, until none is, P passes are drawn or N tile-frames\n"
          "  are spent; prints one line about it; --out gets the --denoise-variance image.\n"
          "  --firefly [K] (with --denoise-variance or --target-error only): clamp outliers above mean + K standard\n"
          "  deviations (default 3) of their neighbourhood ahead of the variance-guided filter; biased.\n");
}

/* --scene cornellbox -> <dir of this executable>/../scenes/cornellbox.obj */
static int resolve_scene(const char* name, char* path, size_t n) {
  if (strchr(name, '/') || (strlen(name) > 4 && strcmp(name + strlen(name) - 4, ".obj") == 0)) {
    snprintf(path, n, "%s", name);
    return 0;
  }
  char exe[PATH_MAX / 2];
  const ssize_t k = readlink("/proc/self/exe", exe, sizeof exe - 1);
  if (k <= 0) return -1;
  exe[k] = 0;
  char* slash = strrchr(exe, '/');
  if (!slash) return -1;
  *slash = 0;
  snprintf(path, n, "%s/../scenes/%s.obj", exe, name);
  return 0;
}

static int parse(int argc, char** argv, options* o) {
  *o = (options){.scene = "cornellbox", .out = "render.pfm", .exchange = "rccl", .width = 800, .height = 600,
                 .spp = 16, .max_path_length = 8, .gpus = 1, .seed = 0x6D6574616C2D7274ull,
                 /* the reference's view: from (0, 1, 2.35) down -z, 90 degrees */
                 .eye = {0.0f, 1.0f, 2.35f}, .target = {0.0f, 1.0f, 1.35f}, .up = {0.0f, 1.0f, 0.0f}, .fov = 90.0f};
  for (int i = 1; i < argc; ++i) {
    const char* a = argv[i];
    const char* v = i + 1 < argc ? argv[i + 1] : NULL;
#define VAL(name) (strcmp(a, name) == 0 && v && ++i)
    if (VAL("--scene")) o->scene = v;
    else if (VAL("--mtl")) o->mtl = v;
    else if (VAL("--then-scene")) o->then_scene = v;
    else if (VAL("--then-mtl")) o->then_mtl = v;
    else if (VAL("--out")) o->out = v;
    else if (VAL("--exchange")) o->exchange = v;
    else if (VAL("--procedural")) o->procedural = (uint32_t)strtoul(v, NULL, 0);
    else if (VAL("--w")) o->width = (uint32_t)strtoul(v, NULL, 0);
    else if (VAL("--h")) o->height = (uint32_t)strtoul(v, NULL, 0);
    else if (VAL("--spp")) o->spp = (uint32_t)strtoul(v, NULL, 0);
    else if (VAL("--L")) o->max_path_length = (uint32_t)strtoul(v, NULL, 0);
    else if (VAL("--seed")) o->seed = strtoull(v, NULL, 0);
    else if (VAL("--gpus")) o->gpus = (uint32_t)strtoul(v, NULL, 0);
    else if (VAL("--device")) o->device = atoi(v);
    else if (VAL("--eye")) { if (parse_vec3(v, o->eye)) { usage(); return -1; } o->camera_set = o->pose_set = 1; }
    else if (VAL("--target")) { if (parse_vec3(v, o->target)) { usage(); return -1; } o->camera_set = o->pose_set = 1; }
    else if (VAL("--up")) { if (parse_vec3(v, o->up)) { usage(); return -1; } o->camera_set = o->pose_set = 1; }
    else if (VAL("--fov")) { o->fov = strtof(v, NULL); o->camera_set = o->pose_set = 1; }
    else if (VAL("--aperture")) { o->aperture = strtof(v, NULL); o->camera_set = 1; }
    else if (VAL("--focus")) { o->focus = strtof(v, NULL); o->camera_set = o->focus_set = 1; }
    else if (VAL("--denoise-iterations")) { o->denoise_iterations = (uint32_t)strtoul(v, NULL, 0); o->denoise = o->denoise_iterations_set = 1; }
    else if (VAL("--denoise-sigma-color")) { o->denoise_sigma_color = strtof(v, NULL); o->denoise = o->denoise_sigma_set = 1; }
    else if (VAL("--orbit-steps")) o->orbit_steps = (uint32_t)strtoul(v, NULL, 0);
    else if (VAL("--orbit-degrees")) { o->orbit_degrees = strtof(v, NULL); o->orbit_degrees_set = 1; }
    else if (VAL("--refine-passes")) { o->refine_passes = (uint32_t)strtoul(v, NULL, 0); o->refine_set = 1; }
    else if (VAL("--refine-frames")) { o->refine_frames = (uint32_t)strtoul(v, NULL, 0); o->refine_set = 1; }
    else if (VAL("--refine-tiles")) { o->refine_tiles = (uint32_t)strtoul(v, NULL, 0); o->refine_set = 1; }
    else if (VAL("--target-error")) { o->target_error = strtof(v, NULL); o->target_set = 1; }
    else if (VAL("--converge-frames")) { o->converge_frames = (uint32_t)strtoul(v, NULL, 0); o->converge_set = 1; }
    else if (VAL("--converge-max-passes")) { o->converge_max_passes = (uint32_t)strtoul(v, NULL, 0); o->converge_set = 1; }
    else if (VAL("--converge-budget")) { o->converge_budget = strtoull(v, NULL, 0); o->converge_set = 1; }
    else if (VAL("--svgf-iterations")) { o->svgf_iterations = (uint32_t)strtoul(v, NULL, 0); o->denoise_variance = o->svgf_iterations_set = 1; }
    else if (VAL("--svgf-sigma-luminance")) { o->svgf_sigma_luminance = strtof(v, NULL); o->denoise_variance = o->svgf_sigma_set = 1; }
    else if (strcmp(a, "--firefly") == 0) {   /* the value is optional: taken when the next argument is a number */
      char* end = NULL;
      const float k = v ? strtof(v, &end) : 0.0f;
      o->firefly = 1;
      if (v && end != v && *end == 0) { o->firefly_k = k; o->firefly_k_set = 1; ++i; }
    }
    else if (strcmp(a, "--denoise") == 0) o->denoise = 1;
    else if (strcmp(a, "--denoise-variance") == 0) o->denoise_variance = 1;
    else if (strcmp(a, "--precise") == 0) o->flags |= MRT_FLAG_PRECISE;
    else if (strcmp(a, "--static-noise") == 0) o->flags |= MRT_FLAG_STATIC_NOISE;
    else if (strcmp(a, "--no-accumulate") == 0) o->flags |= MRT_FLAG_NO_ACCUMULATE;
    else if (strcmp(a, "--debug-material") == 0) o->flags |= MRT_FLAG_DEBUG_MATERIAL;
    else {
      usage();
      return -1;
    }
#undef VAL
  }
  if (o->gpus == 0 || o->spp == 0 || (strcmp(o->exchange, "rccl") && strcmp(o->exchange, "host"))) {
    usage();
    return -1;
  }
  if (o->orbit_degrees_set && !o->orbit_steps) {
    fprintf(stderr, "mrt_render: --orbit-degrees needs --orbit-steps K, K > 0\n");
    return -1;
  }
  if (o->orbit_steps && o->gpus > 1) {
    fprintf(stderr, "mrt_render: --orbit-steps is single rank only (a sharded renderer keeps no temporal history)\n");
    return -1;
  }
  if (o->then_mtl && !o->then_scene) {
    fprintf(stderr, "mrt_render: --then-mtl needs --then-scene OBJ\n");
    return -1;
  }
  if (o->then_scene && (o->gpus > 1 || o->orbit_steps)) {
    fprintf(stderr, "mrt_render: --then-scene is single rank only and excludes --orbit-steps\n");
    return -1;
  }
  if (o->denoise_variance && o->denoise) {
    fprintf(stderr, "mrt_render: --denoise-variance and --denoise exclude each other\n");
    return -1;
  }
  if (o->denoise_variance && o->gpus > 1) {
    fprintf(stderr, "mrt_render: --denoise-variance is single rank only (a sharded renderer keeps no moments)\n");
    return -1;
  }
  if (o->refine_set) {
    if (o->gpus > 1) {
      fprintf(stderr, "mrt_render: --refine-passes is single rank only (a sharded renderer keeps no moments)\n");
      return -1;
    }
    if (!o->refine_passes) o->refine_passes = 1;
    if (!o->refine_frames) o->refine_frames = 1;
    if (!o->refine_tiles) {
      const uint32_t tiles = ((o->width + 63) / 64) * ((o->height + 63) / 64);
      o->refine_tiles = tiles / 4 ? tiles / 4 : 1;
    }
  }
  if (o->converge_set && !o->target_set) {
    fprintf(stderr, "mrt_render: --converge-frames, --converge-max-passes and --converge-budget need --target-error E\n");
    return -1;
  }
  if (o->target_set) {
    if (o->gpus > 1) {
      fprintf(stderr, "mrt_render: --target-error is single rank only (a sharded renderer keeps no moments)\n");
      return -1;
    }
    if (o->refine_set) {
      fprintf(stderr, "mrt_render: --target-error and --refine-passes exclude each other\n");
      return -1;
    }
    if (o->denoise) {
      fprintf(stderr, "mrt_render: --target-error and --denoise exclude each other\n");
      return -1;
    }
    o->denoise_variance = 1;   /* the image it saves */
  }
  if (o->firefly && !o->denoise_variance) {
    fprintf(stderr, "mrt_render: --firefly needs --denoise-variance or --target-error\n");
    usage();
    return -1;
  }
  if (o->denoise_variance || o->refine_set) o->flags |= MRT_FLAG_MOMENTS;
  return 0;
}

/* the camera of the options, seen from `eye`; look_at == 0 (only a lens was
 * given): the reference's pose, bit for bit */
static int make_camera(const options* o, const float eye[3], int look_at, mrt_camera* cam) {
  if (!look_at) {
    if (mrt_camera_default(cam)) return die("mrt_camera_default");
  } else if (mrt_camera_look_at(eye, o->target, o->up, o->fov, cam)) {
    return die("mrt_camera_look_at");
  }
  cam->lens_radius = o->aperture;
  if (o->focus_set) {
    cam->focus_distance = o->focus;
  } else if (o->aperture > 0.0f) {   /* focused on the target */
    float d = 0.0f;
    for (int k = 0; k < 3; ++k) d += (o->target[k] - eye[k]) * cam->forward[k];
    cam->focus_distance = d;
  }
  return 0;
}

static int write_all(int fd, const void* p, size_t n) {
  const char* c = p;
  while (n) {
    const ssize_t k = write(fd, c, n);
    if (k < 0 && errno == EINTR) continue;
    if (k <= 0) return -1;
    c += k;
    n -= (size_t)k;
  }
  return 0;
}

static int read_all(int fd, void* p, size_t n) {
  char* c = p;
  while (n) {
    const ssize_t k = read(fd, c, n);
    if (k < 0 && errno == EINTR) continue;
    if (k <= 0) return -1;
    c += k;
    n -= (size_t)k;
  }
  return 0;
}

/* One rank of the job.  id_fd: rank 0 writes the RCCL id to the N-1 write
 * ends it owns (to_peer[k]); rank k > 0 reads it from from_root.  tiles:
 * host exchange, rank k > 0 writes its packed tiles to tiles_w, rank 0 reads
 * rank k's from tiles_r[k]. */
static int run_rank(const options* o, uint32_t rank, const int* to_peer, int from_root, const int* tiles_r,
                    int tiles_w) {
  const uint32_t N = o->gpus;
  char obj[PATH_MAX];
  if (resolve_scene(o->scene, obj, sizeof obj)) {
    fprintf(stderr, "mrt_render: cannot resolve scene %s\n", o->scene);
    return 1;
  }
  const int ndev = mrt_device_count();
  if (ndev <= 0) {
    fprintf(stderr, "mrt_render: no HIP device visible\n");
    return 1;
  }
  const int device = N > 1 ? (int)(rank % (uint32_t)ndev) : o->device;
  const int rccl = N > 1 && strcmp(o->exchange, "rccl") == 0;
  mrt_comm* comm = NULL;
  if (rccl) {   /* the communicator first: every rank blocks in it until all have joined */
    unsigned char id[MRT_COMM_ID_BYTES];
    if (rank == 0) {
      if (mrt_comm_unique_id(id, sizeof id)) return die("mrt_comm_unique_id");
      for (uint32_t k = 1; k < N; ++k)
        if (write_all(to_peer[k], id, sizeof id)) return die("send comm id");
    } else if (read_all(from_root, id, sizeof id)) {
      fprintf(stderr, "mrt_render: rank %u: no comm id from rank 0\n", rank);
      return 1;
    }
    if (mrt_comm_create(id, N, rank, device, &comm)) return die("mrt_comm_create");
  }
  mrt_scene_desc sd = {0};
  sd.obj_path = obj;
  sd.mtl_override = o->mtl;
  sd.procedural_triangles = o->procedural;
  sd.procedural_seed = 1;
  sd.device = device;
  mrt_scene* scene = NULL;
  if (mrt_scene_create(&sd, &scene)) return die("mrt_scene_create");
  mrt_renderer_desc rd = {0};
  rd.scene = scene;
  rd.width = o->width;
  rd.height = o->height;
  rd.max_path_length = o->max_path_length;
  rd.seed = o->seed;
  rd.shard_rank = rank;
  rd.shard_count = N;
  rd.flags = o->flags;
  mrt_renderer* r = NULL;
  if (mrt_renderer_create(&rd, &r)) return die("mrt_renderer_create");
  if (o->camera_set) {   /* every rank sets the same camera */
    mrt_camera cam;
    if (make_camera(o, o->eye, o->pose_set, &cam)) return 1;
    if (mrt_renderer_set_camera(r, &cam)) return die("mrt_renderer_set_camera");
  }
  if (o->firefly) {
    mrt_firefly_params fp;
    if (mrt_firefly_params_default(&fp)) return die("mrt_firefly_params_default");
    if (o->firefly_k_set) fp.k = o->firefly_k;
    if (mrt_renderer_set_firefly(r, &fp)) return die("mrt_renderer_set_firefly");
  }
  struct timespec t0, t1;
  clock_gettime(CLOCK_MONOTONIC, &t0);
  if (mrt_renderer_draw_n(r, o->spp)) return die("mrt_renderer_draw_n");
  for (uint32_t k = 1; k <= o->orbit_steps; ++k) {   /* nothing here waits for the GPU */
    const double a = (double)o->orbit_degrees * (double)k * (3.14159265358979323846 / 180.0);
    const double dx = (double)o->eye[0] - (double)o->target[0], dz = (double)o->eye[2] - (double)o->target[2];
    const float eye[3] = {(float)((double)o->target[0] + dx * cos(a) + dz * sin(a)), o->eye[1],
                          (float)((double)o->target[2] - dx * sin(a) + dz * cos(a))};
    mrt_camera cam;
    if (make_camera(o, eye, 1, &cam)) return 1;
    if (mrt_renderer_move_camera(r, &cam, NULL)) return die("mrt_renderer_move_camera");
    if (mrt_renderer_draw_n(r, o->spp)) return die("mrt_renderer_draw_n");
  }
  mrt_scene* first_scene = NULL;
  if (o->then_scene) {   /* (single rank) waits for the GPU once, inside the move */
    char obj2[PATH_MAX];
    if (resolve_scene(o->then_scene, obj2, sizeof obj2)) {
      fprintf(stderr, "mrt_render: cannot resolve scene %s\n", o->then_scene);
      return 1;
    }
    mrt_scene_desc sd2 = sd;
    sd2.obj_path = obj2;
    sd2.mtl_override = o->then_mtl;
    mrt_scene* next = NULL;
    if (mrt_scene_create(&sd2, &next)) return die("mrt_scene_create (--then-scene)");
    if (mrt_renderer_move_scene(r, next, NULL, NULL)) return die("mrt_renderer_move_scene");
    first_scene = scene;   /* read by the motion pass until the renderer has synchronised */
    scene = next;
    if (mrt_renderer_draw_n(r, o->spp)) return die("mrt_renderer_draw_n");
  }
  for (uint32_t k = 0; k < o->refine_passes; ++k)   /* (single rank) nor does this */
    if (mrt_renderer_refine(r, o->refine_frames, o->refine_tiles, NULL)) return die("mrt_renderer_refine");
  if (o->target_set) {   /* (single rank) this waits for the GPU once per estimate */
    mrt_converge_params cp;
    mrt_converge_result cr;
    if (mrt_converge_params_default(&cp)) return die("mrt_converge_params_default");
    cp.target_error = o->target_error;
    if (o->converge_frames) cp.frames_per_pass = o->converge_frames;
    if (o->converge_max_passes) cp.max_passes = o->converge_max_passes;
    cp.max_tile_frames = o->converge_budget;
    if (mrt_renderer_converge(r, &cp, &cr)) return die("mrt_renderer_converge");
    printf("{\"converge_passes\": %u, \"tile_frames\": %" PRIu64 ", \"first_frame_error\": %.9g, "
           "\"last_frame_error\": %.9g, \"converged\": %u}\n",
           cr.passes, cr.tile_frames, (double)cr.first.frame_error, (double)cr.last.frame_error, cr.converged);
  }
  if (rccl) {
    if (mrt_renderer_exchange(r, comm, MRT_EXCHANGE_GATHER)) return die("mrt_renderer_exchange");
  } else if (N > 1) {
    uint64_t floats = 0;
    if (rank > 0) {
      if (mrt_tiles_packed_floats(o->width, o->height, rank, N, &floats)) return die("mrt_tiles_packed_floats");
      float* buf = malloc(floats * sizeof(float) + 1);
      if (!buf || mrt_renderer_tiles_read(r, buf, floats)) return die("mrt_renderer_tiles_read");
      if (write_all(tiles_w, buf, floats * sizeof(float))) return die("send tiles");
      free(buf);
    } else {
      for (uint32_t k = 1; k < N; ++k) {
        if (mrt_tiles_packed_floats(o->width, o->height, k, N, &floats)) return die("mrt_tiles_packed_floats");
        float* buf = malloc(floats * sizeof(float) + 1);
        if (!buf || read_all(tiles_r[k], buf, floats * sizeof(float))) {
          fprintf(stderr, "mrt_render: no tiles from rank %u\n", k);
          return 1;
        }
        if (mrt_renderer_tiles_write(r, k, buf, floats)) return die("mrt_renderer_tiles_write");
        free(buf);
      }
    }
  }
  if (mrt_renderer_sync(r)) return die("mrt_renderer_sync");
  clock_gettime(CLOCK_MONOTONIC, &t1);
  mrt_stats st;
  if (mrt_renderer_stats(r, &st)) return die("mrt_renderer_stats");
  if (rank == 0) {
    if (o->denoise_variance) {
      mrt_svgf_params vp;
      if (mrt_svgf_params_default(&vp)) return die("mrt_svgf_params_default");
      if (o->svgf_iterations_set) vp.iterations = o->svgf_iterations;
      if (o->svgf_sigma_set) vp.sigma_luminance = o->svgf_sigma_luminance;
      if (mrt_renderer_denoise_variance(r, &vp)) return die("mrt_renderer_denoise_variance");
      if (mrt_renderer_save_denoised(r, o->out)) return die("mrt_renderer_save_denoised");
    } else if (o->denoise) {
      mrt_denoise_params dp;
      if (mrt_denoise_params_default(st.frame_index, &dp)) return die("mrt_denoise_params_default");
      if (o->denoise_iterations_set) dp.iterations = o->denoise_iterations;
      if (o->denoise_sigma_set) dp.sigma_color = o->denoise_sigma_color;
      if (o->orbit_steps || o->refine_set || o->then_scene) {
        if (mrt_renderer_denoise_resolved(r, &dp)) return die("mrt_renderer_denoise_resolved");
      } else if (mrt_renderer_denoise(r, &dp)) {
        return die("mrt_renderer_denoise");
      }
      if (mrt_renderer_save_denoised(r, o->out)) return die("mrt_renderer_save_denoised");
    } else if (o->orbit_steps || o->refine_set || o->then_scene) {
      if (mrt_renderer_resolve(r)) return die("mrt_renderer_resolve");
      if (mrt_renderer_save_resolved(r, o->out)) return die("mrt_renderer_save_resolved");
    } else if (mrt_renderer_save_image(r, o->out)) {
      return die("mrt_renderer_save_image");
    }
    const double s = (double)(t1.tv_sec - t0.tv_sec) + 1e-9 * (double)(t1.tv_nsec - t0.tv_nsec);
    const double paths = (double)o->width * o->height * o->spp;
    printf("{\"out\": \"%s\", \"width\": %u, \"height\": %u, \"spp\": %u, \"max_path_length\": %u, \"gpus\": %u, "
           "\"exchange\": \"%s\", \"frames\": %" PRIu64 ", \"rank0_paths\": %" PRIu64
           ", \"active_ray_bounces_rank0\": %" PRIu64 ", \"seconds\": %.4f, \"mpaths_per_s\": %.2f}\n",
           o->out, o->width, o->height, o->spp, o->max_path_length, N, N > 1 ? o->exchange : "none",
           st.frame_index, st.paths, st.active_ray_bounces, s, paths / s / 1e6);
    fflush(stdout);
  }
  mrt_renderer_destroy(r);
  mrt_scene_destroy(scene);
  if (first_scene) mrt_scene_destroy(first_scene);
  if (comm) mrt_comm_destroy(comm);
  return 0;
}

int main(int argc, char** argv) {
  options o;
  if (parse(argc, argv, &o)) return 2;
  if (mrt_abi_version() != MRT_ABI_VERSION) {
    fprintf(stderr, "mrt_render: libmrt ABI %d, header %d\n", mrt_abi_version(), MRT_ABI_VERSION);
    return 1;
  }
  const uint32_t N = o.gpus;
  if (N == 1) return run_rank(&o, 0, NULL, -1, NULL, -1);
  /* fork the ranks before any HIP call in this process */
  int* id_pipe = calloc(2 * N, sizeof(int));
  int* tile_pipe = calloc(2 * N, sizeof(int));
  pid_t* pid = calloc(N, sizeof(pid_t));
  if (!id_pipe || !tile_pipe || !pid) return 1;
  for (uint32_t k = 1; k < N; ++k)
    if (pipe(id_pipe + 2 * k) || pipe(tile_pipe + 2 * k)) {
      perror("pipe");
      return 1;
    }
  for (uint32_t k = 0; k < N; ++k) {
    pid[k] = fork();
    if (pid[k] < 0) {
      perror("fork");
      return 1;
    }
    if (pid[k] == 0) {
      int* to_peer = calloc(N, sizeof(int));
      int* tiles_r = calloc(N, sizeof(int));
      for (uint32_t j = 1; j < N; ++j) {   /* keep only this rank's pipe ends, so a dead peer reads as EOF */
        to_peer[j] = id_pipe[2 * j + 1];
        tiles_r[j] = tile_pipe[2 * j];
        if (k == 0) {
          close(id_pipe[2 * j]);
          close(tile_pipe[2 * j + 1]);
        } else {
          close(id_pipe[2 * j + 1]);
          close(tile_pipe[2 * j]);
          if (j != k) {
            close(id_pipe[2 * j]);
            close(tile_pipe[2 * j + 1]);
          }
        }
      }
      const int rc = run_rank(&o, k, to_peer, k ? id_pipe[2 * k] : -1, tiles_r, k ? tile_pipe[2 * k + 1] : -1);
      fflush(NULL);
      _exit(rc);
    }
  }
  for (uint32_t k = 1; k < N; ++k) {   /* the parent keeps no pipe ends: a dead rank yields EOF, not a hang */
    close(id_pipe[2 * k]);
    close(id_pipe[2 * k + 1]);
    close(tile_pipe[2 * k]);
    close(tile_pipe[2 * k + 1]);
  }
  int failed = 0;
  for (uint32_t k = 0; k < N; ++k) {
    int status = 0;
    if (waitpid(pid[k], &status, 0) < 0 || !WIFEXITED(status) || WEXITSTATUS(status) != 0) {
      fprintf(stderr, "mrt_render: rank %u failed\n", k);
      failed = 1;
    }
  }
  return failed;
}
