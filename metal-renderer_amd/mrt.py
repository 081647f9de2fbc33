"""Python mirror of the reference's Renderer interface over libmrt.so (C ABI).

The reference API (renderer/Renderer.h:3-8, Renderer.mm) maps to:

    -initWithMetalKitView:            -> Renderer(scene, width, height, ...)
    -mtkView:drawableSizeWillChange:  -> Renderer.resize(width, height)
    -drawInMTKView:                   -> Renderer.draw()          (1 spp frame)
    -saveCurrentImage                 -> Renderer.save_current_image(path)
    title-bar "Mrays/s, ms/frame"     -> Renderer.stats()

and the per-stage dispatches of performRaytracing: (Renderer.mm:500-585) map to
the module functions raygen / intersect / shade / resolve_shadow / accumulate,
which take device pointers (ints) to reference-layout AoS buffers.

This module only binds the native library: every call runs the HIP kernels in
libmrt.so.  There is no CPU fallback; if the library is missing the import
fails loudly.

include/mrt.h is restated here in three places and nowhere else: the block of
constants, the Structure classes, and the table _ABI of every entry point's
argument types.  tests/test_abi_host.py holds all three against the header.

Interop note: PyTorch-ROCm wheels bundle their own HIP runtime, HSA runtime
and RCCL under the same sonames as ROCm's (libamdhip64.so.7, librccl.so.1), so
a process holds ONE copy of each — whichever was loaded first (checked in
/proc/self/maps: with torch imported first, libmrt binds to torch/lib's
copies).  Device pointers (torch tensors) can therefore be handed to libmrt;
the tests import torch first (the order that is exercised), and synchronise
libmrt's work with Renderer.sync() / synchronize() rather than torch streams.
"""
from __future__ import annotations

import ctypes
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("MRT_LIB") or os.path.join(HERE, "lib", "libmrt.so")   # MRT_LIB: diagnostic builds
INCLUDE_H = os.path.join(os.path.dirname(HERE), "include", "mrt.h")
SCENES_DIR = os.path.join(HERE, "scenes")   # renderer/Media scene data, rendered unchanged

# ---- the constants of include/mrt.h: NAME here is MRT_NAME there ---------------------
FLAG_PRECISE = 1            # MRT_FLAG_PRECISE
FLAG_PROFILE = 2            # MRT_FLAG_PROFILE
# the reference's compile-time switches (renderer/Raytracing.h:14,20; Shaders.metal:7)
FLAG_STATIC_NOISE = 4       # MRT_FLAG_STATIC_NOISE: ANIMATE_NOISE 0
FLAG_NO_ACCUMULATE = 8      # MRT_FLAG_NO_ACCUMULATE: ACCUMULATE_IMAGE false
FLAG_DEBUG_MATERIAL = 16    # MRT_FLAG_DEBUG_MATERIAL: DEBUG_MATERIAL 1
FLAG_MOMENTS = 32           # MRT_FLAG_MOMENTS: luminance moments accumulated beside the image (variance-guided denoising)
BVH_HOST_SAH, BVH_DEVICE_LBVH, BVH_DEVICE_PLOC = 1, 2, 3   # MRT_BVH_HOST_SAH, MRT_BVH_DEVICE_LBVH, MRT_BVH_DEVICE_PLOC
REFINE_SEED_XOR = 0x9E3779B97F4A7C15   # MRT_REFINE_SEED_XOR: the refine draws' noise seed is seed ^ this
DISPLAY_TONEMAP, DISPLAY_SRGB = 1, 2   # MRT_DISPLAY_TONEMAP, MRT_DISPLAY_SRGB
DISPLAY_DENOISED = 4   # MRT_DISPLAY_DENOISED: Renderer.display / display_enqueue blit the denoised buffer instead of the image
DISPLAY_RESOLVED = 8   # MRT_DISPLAY_RESOLVED: ... the resolved buffer (Renderer.resolve); not together with DISPLAY_DENOISED
COMM_ID_BYTES = 128    # MRT_COMM_ID_BYTES
EXCHANGE_GATHER, EXCHANGE_REDUCE, EXCHANGE_OVERLAP = 1, 2, 0x100   # MRT_EXCHANGE_GATHER, _REDUCE, _OVERLAP
ERR_COMM = -6   # MRT_ERR_COMM (mrt_status): a collective failed or timed out; the communicator is aborted

# ---- values the header has no macro for ----------------------------------------------
TILE = 64                   # csrc/mrt_layout.h kTile: the unit of adaptive sampling (and of sharding), 64x64 pixels
RAY_BYTES, SHADOW_RAY_BYTES, ISECT_BYTES = 80, 48, 16   # csrc/mrt_layout.h RefRay, RefShadowRay, RefIntersection
DEFAULT_SEED = 0x6D6574616C2D7274  # "metal-rt", cli/render.c's default seed


class MrtError(RuntimeError):
    pass


_vp, _u32, _u64, _f32, _f64 = ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint64, ctypes.c_float, ctypes.c_double
_i64, _int, _size, _str, _P = ctypes.c_int64, ctypes.c_int, ctypes.c_size_t, ctypes.c_char_p, ctypes.POINTER


# ---- the structs of include/mrt.h: class CamelCase mirrors mrt_camel_case -------------
def _plain(v):
    """A field's value for as_dict: ctypes arrays (nested) to lists, a nested
    struct to its dict; scalars unchanged."""
    if isinstance(v, ctypes.Array):
        return [_plain(x) for x in v]
    return v.as_dict() if isinstance(v, _Struct) else v


class _Struct(ctypes.Structure):
    @classmethod
    def _c_name(cls) -> str:
        return "mrt" + "".join("_" + c.lower() if c.isupper() else c for c in cls.__name__)

    def as_dict(self) -> dict:
        return {k: _plain(getattr(self, k)) for k, _ in self._fields_ if k != "reserved"}


class _Params(_Struct):
    """A struct the library fills (mrt_<name>_default) and validates
    (mrt_<name>_check).  A subclass without a default() of its own gets the
    plain one, annotated with its own name."""

    def __init_subclass__(cls):
        if "default" not in vars(cls):
            def default(cls):
                return cls._default()
            default.__annotations__["return"] = repr(cls.__name__)
            default.__qualname__ = cls.__qualname__ + ".default"
            cls.default = classmethod(default)

    @classmethod
    def _default(cls, *args):
        return _get(cls, cls._c_name() + "_default", *args)

    def check(self) -> None:
        _call(self._c_name() + "_check", ctypes.byref(self))


class SceneDesc(_Struct):
    _fields_ = [
        ("obj_path", _str),
        ("mtl_override", _str),
        ("procedural_triangles", _u32),
        ("procedural_seed", _u64),
        ("max_leaf_size", _u32),
        ("lds_nodes", _u32),
        ("device", _int),
        ("bvh_width", _u32),
        ("bvh_builder", _u32),
        ("no_occluder_tree", _u32),
    ]


class AccelDesc(_Struct):
    _fields_ = [
        ("vertices", _vp), ("vertex_stride", _u32),
        ("indices", _vp), ("triangle_count", _u32),
        ("device", _int), ("builder", _u32), ("max_leaf_size", _u32),
        ("stream", _vp),
    ]


class AccelInfo(_Struct):
    _fields_ = [
        ("triangles", _u32), ("bvh_nodes", _u32), ("bvh_leaves", _u32),
        ("bvh_levels", _u32), ("bvh_max_stack", _u32), ("builder", _u32),
        ("build_ms", _f64), ("device_bytes", _u64),
    ]


class SceneInfo(_Struct):
    _fields_ = [
        ("vertices", _u32), ("triangles", _u32), ("materials", _u32),
        ("light_triangles", _u32), ("bvh_nodes", _u32), ("bvh_leaves", _u32),
        ("bvh_depth", _u32), ("bvh_lds_nodes", _u32), ("bvh_width", _u32),
        ("bvh_max_stack", _u32), ("bvh_sah_cost", _f64),
        ("build_ms", _f64), ("device_bytes", _u64),
        ("occluder_planes", _u32), ("occluder_culled", _u32),
        ("occluder_nodes", _u32), ("occluder_margin", _f32),
        ("occluder_max_stack", _u32), ("occluder_cos_min", _f32),
        ("occluder_plane", (_f32 * 4) * 8),
        ("convex_solids", _u32), ("convex_delta", _f32),
        ("convex_obb", (_f32 * 16) * 4), ("convex_face_tris", (_u32 * 8) * 4),
    ]


class RendererDesc(_Struct):
    _fields_ = [
        ("scene", _vp),
        ("width", _u32), ("height", _u32),
        ("max_path_length", _u32),
        ("seed", _u64),
        ("shard_rank", _u32), ("shard_count", _u32),
        ("flags", _u32),
        ("stream", _vp),
        ("image", _vp),
    ]


class Stats(_Struct):
    _fields_ = [
        ("frame_index", _u64), ("paths", _u64), ("active_ray_bounces", _u64),
        ("last_draw_ms", _f64), ("mpaths_per_s", _f64),
        ("kernel_launches", _u64), ("kernel_ms", _f64), ("owned_pixels", _u64),
        ("timed_launches", _u64), ("kernel", _u32), ("inflight", _u32),
        ("span_ms", _f64), ("spans", _u64),
        ("primary_blocks", _u32), ("primary_mean", _f32),
        ("noise_ms", _f64), ("noise_tables", _u64),
        ("draws", _u64), ("draws_overlapped", _u64), ("inflight_waits", _u64),
        ("noise_waits", _u64), ("noise_prefetched", _u64),
    ]


class Camera(_Params):
    """mrt_camera (include/mrt.h): pose, field of view and thin lens.  Build one
    with Camera.default() (the reference's fixed camera) or Camera.look_at()."""
    _fields_ = [
        ("origin", _f32 * 3),
        ("right", _f32 * 3), ("up", _f32 * 3), ("forward", _f32 * 3),
        ("tan_half_fov", _f32), ("lens_radius", _f32), ("focus_distance", _f32),
    ]

    @classmethod
    def look_at(cls, eye, target, up, fov_x_degrees: float, lens_radius: float = 0.0,
                focus_distance: float = 0.0) -> "Camera":
        """A camera at `eye` looking at `target`; fov_x_degrees is the full
        horizontal field of view.  lens_radius > 0 makes it a thin lens focused
        at depth focus_distance along the view direction."""
        v3 = _f32 * 3
        c = _get(cls, "mrt_camera_look_at", v3(*eye), v3(*target), v3(*up), fov_x_degrees)
        c.lens_radius, c.focus_distance = lens_radius, focus_distance
        c.check()
        return c


class DenoiseParams(_Params):
    """mrt_denoise_params (include/mrt.h): the A-Trous filter's parameters."""
    _fields_ = [
        ("iterations", _u32), ("sigma_color", _f32), ("sigma_plane", _f32),
        ("normal_log2_power", _u32),
    ]

    @classmethod
    def default(cls, frames: int) -> "DenoiseParams":
        """The library's defaults for an image of `frames` accumulated frames."""
        return cls._default(frames)


class ReprojectParams(_Params):
    """mrt_reproject_params (include/mrt.h): the history reprojection's tests."""
    _fields_ = [
        ("plane_tolerance", _f32), ("normal_cos_min", _f32), ("max_history", _f32),
    ]


class SvgfParams(_Params):
    """mrt_svgf_params (include/mrt.h): the variance estimate's and the
    variance-guided filter's parameters."""
    _fields_ = [
        ("iterations", _u32), ("sigma_luminance", _f32), ("sigma_plane", _f32),
        ("normal_log2_power", _u32), ("min_frames", _u32),
    ]


class FireflyParams(_Params):
    """mrt_firefly_params (include/mrt.h): the outlier clamp ahead of the
    variance-guided filter."""
    _fields_ = [
        ("radius", _u32), ("k", _f32), ("min_taps", _u32),
        ("normal_cos_min", _f32), ("plane_tolerance", _f32),
    ]


class AdaptiveParams(_Params):
    """mrt_adaptive_params (include/mrt.h): the tile priority's parameters."""
    _fields_ = [("luminance_floor", _f32)]


class RefineStats(_Struct):
    """mrt_refine_stats (include/mrt.h)."""
    _fields_ = [("passes", _u64), ("extra_frames", _u64), ("tile_frames", _u64),
                ("paths", _u64)]


class ErrorSummary(_Struct):
    """mrt_error_summary (include/mrt.h): what mrt_tile_threshold found."""
    _fields_ = [("frame_error", _f32), ("max_tile_error", _f32), ("tiles_above", _u32),
                ("tiles_listed", _u32), ("tiles_counted", _u32), ("pixels", _u32),
                ("reserved", _u32 * 2)]


class ConvergeParams(_Params):
    """mrt_converge_params (include/mrt.h): the stop rule of Renderer.converge."""
    _fields_ = [("target_error", _f32), ("frames_per_pass", _u32), ("max_passes", _u32),
                ("max_tiles", _u32), ("max_tile_frames", _u64), ("luminance_floor", _f32)]

    @classmethod
    def default(cls, **fields) -> "ConvergeParams":
        p = cls._default()
        for k, v in fields.items():
            if k not in dict(cls._fields_):
                raise TypeError(f"ConvergeParams has no field {k}")
            setattr(p, k, v)
        return p


class ConvergeResult(_Struct):
    """mrt_converge_result (include/mrt.h)."""
    _fields_ = [("converged", _u32), ("passes", _u32), ("tile_frames", _u64),
                ("first", ErrorSummary), ("last", ErrorSummary)]


# ---- the entry points of include/mrt.h: name -> argtypes -----------------------------
# Every one returns int (0 or a negative mrt_status) except mrt_last_error.  A
# handle, a stream and a device pointer are c_void_p; what the host reads or
# writes through a pointer is POINTER(its mirror).
_ABI = {
    "mrt_scene_create": [_P(SceneDesc), _P(_vp)],
    "mrt_scene_info_get": [_vp, _P(SceneInfo)],
    "mrt_scene_export": [_vp, _vp, _vp, _vp, _vp, _vp],
    "mrt_scene_destroy": [_vp],
    "mrt_scene_check_bvh": [_vp],
    "mrt_raygen": [_vp, _u32, _u32, _vp, _vp, _u32, _vp],
    "mrt_intersect": [_vp, _vp, _u32, _u32, _vp, _u32, _vp],
    "mrt_shade": [_vp, _u32, _u32, _u32, _u32, _vp, _vp, _vp, _vp, _u32, _vp],
    "mrt_resolve_shadow": [_vp, _u32, _vp, _vp, _vp, _u32, _vp],
    "mrt_accumulate": [_vp, _u32, _u32, _u32, _vp, _vp, _u32, _vp],
    "mrt_renderer_create": [_P(RendererDesc), _P(_vp)],
    "mrt_renderer_resize": [_vp, _u32, _u32],
    "mrt_renderer_reset": [_vp],
    "mrt_renderer_prepare": [_vp, _u32],
    "mrt_renderer_draw": [_vp],
    "mrt_renderer_draw_n": [_vp, _u32],
    "mrt_renderer_sync": [_vp],
    "mrt_renderer_image": [_vp, _P(_vp)],
    "mrt_renderer_stream": [_vp, _P(_vp)],
    "mrt_renderer_read_image": [_vp, _vp, _size],
    "mrt_renderer_save_image": [_vp, _str],
    "mrt_renderer_stats": [_vp, _P(Stats)],
    "mrt_renderer_destroy": [_vp],
    "mrt_last_error": [],
    "mrt_abi_version": [],
    "mrt_noise_table": [_u64, _i64, _vp],
    "mrt_device_count": [],
    "mrt_synchronize": [_vp],
    "mrt_event_record": [_vp, _P(_vp)],
    "mrt_event_synchronize": [_vp],
    "mrt_event_destroy": [_vp],
    "mrt_debug_stamps": [_vp, _int],
    "mrt_debug_wave_times": [_vp, _size],
    "mrt_debug_lanes": [_vp, _size, _int],
    "mrt_debug_sweep_list": [_vp, _vp, _u32, _vp, _vp],
    "mrt_debug_sweep_pairs": [_vp, _vp, _vp, _u32, _vp],
    "mrt_debug_sweep_phase1": [_vp, _vp, _u32, _vp],
    "mrt_debug_sweep_cap": [_vp, _vp],
    "mrt_debug_bvh_nodes": [_vp, _vp, _u32, _vp],
    "mrt_debug_exchange_unpack": [_vp, _u32, _vp, _size],
    "mrt_debug_box_margin": [_vp, _vp, _u32, _u32, _vp, _vp],
    "mrt_debug_magic_div": [_u32, _vp, _u32, _vp],
    "mrt_comm_set_timeout": [_vp, _u32],
    "mrt_comm_check": [_vp],
    "mrt_debug_comm_fail": [_vp, _u32],
    "mrt_shard_mask": [_u32, _u32, _u32, _u32, _vp, _vp],
    "mrt_tiles_packed_floats": [_u32, _u32, _u32, _u32, _P(_u64)],
    "mrt_display": [_vp, _vp, _vp, _u32, _u32, _u32, _f32, _vp],
    "mrt_renderer_set_max_frames": [_vp, _u32],
    "mrt_tiles_pack": [_vp, _u32, _u32, _u32, _u32, _vp, _vp],
    "mrt_tiles_unpack": [_vp, _u32, _u32, _u32, _u32, _vp, _vp],
    "mrt_accel_create": [_P(AccelDesc), _P(_vp)],
    "mrt_accel_rebuild": [_vp],
    "mrt_accel_intersect": [_vp, _vp, _u32, _u32, _vp, _u32, _vp],
    "mrt_accel_info_get": [_vp, _P(AccelInfo)],
    "mrt_accel_destroy": [_vp],
    "mrt_comm_unique_id": [_vp, _size],
    "mrt_comm_create": [_vp, _u32, _u32, _int, _P(_vp)],
    "mrt_comm_destroy": [_vp],
    "mrt_renderer_exchange": [_vp, _vp, _u32],
    "mrt_renderer_exchange_flush": [_vp],
    "mrt_renderer_tiles_read": [_vp, _vp, _size],
    "mrt_renderer_tiles_write": [_vp, _u32, _vp, _size],
    "mrt_image_load_exr": [_str, _vp, _size, _P(_u32), _P(_u32)],
    "mrt_renderer_load_reference": [_vp, _str],
    "mrt_renderer_display": [_vp, _u32, _f32, _vp, _size],
    "mrt_renderer_display_enqueue": [_vp, _u32, _f32, _u32],
    "mrt_renderer_display_map": [_vp, _u32, _P(_vp), _P(_size)],
    "mrt_camera_default": [_P(Camera)],
    "mrt_camera_look_at": [_f32 * 3, _f32 * 3, _f32 * 3, _f32, _P(Camera)],
    "mrt_camera_check": [_P(Camera)],
    "mrt_raygen_camera": [_vp, _P(Camera), _u32, _u32, _vp, _vp, _u32, _vp],
    "mrt_renderer_set_camera": [_vp, _P(Camera)],
    "mrt_renderer_get_camera": [_vp, _P(Camera)],
    "mrt_guides": [_vp, _P(Camera), _u32, _u32, _vp, _vp, _u32, _vp],
    "mrt_denoise_params_default": [_u64, _P(DenoiseParams)],
    "mrt_denoise_params_check": [_P(DenoiseParams)],
    "mrt_denoise": [_vp, _vp, _vp, _vp, _vp, _u32, _u32, _P(DenoiseParams), _vp],
    "mrt_renderer_denoise": [_vp, _P(DenoiseParams)],
    "mrt_renderer_read_denoised": [_vp, _vp, _size],
    "mrt_renderer_save_denoised": [_vp, _str],
    "mrt_debug_denoise_path": [_u32],
    "mrt_debug_denoise_step": [_vp, _vp, _vp, _vp, _vp, _u32, _u32, _P(DenoiseParams), _u32, _u32, _vp],
    "mrt_reproject_params_default": [_P(ReprojectParams)],
    "mrt_reproject_params_check": [_P(ReprojectParams)],
    "mrt_temporal_resolve": [_vp, _u64, _vp, _vp, _u32, _u32, _vp],
    "mrt_reproject": [_vp, _vp, _vp, _P(Camera), _vp, _vp, _vp, _u32, _u32, _P(ReprojectParams), _vp],
    "mrt_renderer_move_camera": [_vp, _P(Camera), _P(ReprojectParams)],
    "mrt_renderer_resolve": [_vp],
    "mrt_renderer_read_resolved": [_vp, _vp, _size],
    "mrt_renderer_save_resolved": [_vp, _str],
    "mrt_renderer_denoise_resolved": [_vp, _P(DenoiseParams)],
    "mrt_moments": [_vp, _u32, _u32, _u32, _vp, _vp, _u32, _vp],
    "mrt_svgf_params_default": [_P(SvgfParams)],
    "mrt_svgf_params_check": [_P(SvgfParams)],
    "mrt_variance": [_vp, _vp, _vp, _vp, _u32, _u32, _P(SvgfParams), _vp],
    "mrt_denoise_variance": [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _u32, _u32, _P(SvgfParams), _vp],
    "mrt_renderer_read_moments": [_vp, _vp, _size],
    "mrt_renderer_moments": [_vp, _P(_vp)],
    "mrt_renderer_denoise_variance": [_vp, _P(SvgfParams)],
    "mrt_renderer_read_variance": [_vp, _vp, _size],
    "mrt_debug_denoise_variance_step": [_vp, _vp, _vp, _vp, _vp, _u32, _u32, _P(SvgfParams), _u32, _u32, _vp],
    "mrt_adaptive_params_default": [_P(AdaptiveParams)],
    "mrt_adaptive_params_check": [_P(AdaptiveParams)],
    "mrt_counted_merge": [_vp, _vp, _vp, _u32, _u32, _u32, _vp],
    "mrt_tile_priority": [_vp, _vp, _vp, _vp, _u32, _u32, _P(AdaptiveParams), _u32, _vp],
    "mrt_tile_select": [_vp, _u32, _u32, _vp, _vp],
    "mrt_renderer_draw_tiles": [_vp, _vp, _u32, _u32],
    "mrt_renderer_refine": [_vp, _u32, _u32, _P(AdaptiveParams)],
    "mrt_renderer_read_extra": [_vp, _vp, _size],
    "mrt_renderer_read_extra_moments": [_vp, _vp, _size],
    "mrt_renderer_read_tile_priority": [_vp, _vp, _size],
    "mrt_renderer_read_tile_list": [_vp, _vp, _size, _P(_u32)],
    "mrt_renderer_refine_stats": [_vp, _P(RefineStats)],
    "mrt_tile_error": [_vp, _vp, _vp, _vp, _vp, _u32, _u32, _P(AdaptiveParams), _u32, _vp],
    "mrt_tile_threshold": [_vp, _vp, _u32, _f32, _u32, _vp, _vp, _vp],
    "mrt_converge_params_default": [_P(ConvergeParams)],
    "mrt_converge_params_check": [_P(ConvergeParams)],
    "mrt_renderer_error": [_vp, _P(SvgfParams), _f32, _f32, _P(ErrorSummary)],
    "mrt_renderer_read_tile_error": [_vp, _vp, _vp, _size],
    "mrt_renderer_converge": [_vp, _P(ConvergeParams), _P(ConvergeResult)],
    "mrt_firefly_params_default": [_P(FireflyParams)],
    "mrt_firefly_params_check": [_P(FireflyParams)],
    "mrt_firefly_clamp": [_vp, _vp, _vp, _vp, _vp, _u32, _u32, _P(FireflyParams), _vp],
    "mrt_renderer_set_firefly": [_vp, _P(FireflyParams)],
    "mrt_renderer_get_firefly": [_vp, _P(FireflyParams), _P(_u32)],
    "mrt_renderer_read_clamped": [_vp, _vp, _size, _P(_u32)],
    "mrt_scene_motion_compatible": [_vp, _vp],
    "mrt_guides_motion": [_vp, _vp, _P(Camera), _u32, _u32, _vp, _vp, _vp, _vp, _u32, _vp],
    "mrt_renderer_set_scene": [_vp, _vp],
    "mrt_renderer_move_scene": [_vp, _vp, _P(Camera), _P(ReprojectParams)],
}
EXPORTED = list(_ABI)

_lib = None


def build(jobs: int = 4) -> None:
    """Compile libmrt.so for gfx950 in-tree (hipcc cross-compiles without a GPU)."""
    subprocess.run(["make", "-s", f"-j{jobs}", "-C", HERE], check=True)


def lib() -> ctypes.CDLL:
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise MrtError(f"native library missing: {LIB_PATH} (run __graft_entry__.build())")
    L = ctypes.CDLL(LIB_PATH)
    for name, args in _ABI.items():
        fn = getattr(L, name, None)
        if fn is None and os.environ.get("MRT_LIB"):   # an older diagnostic build (A/B): entries it lacks
            continue
        fn = getattr(L, name)
        fn.argtypes = args
        fn.restype = _int
    L.mrt_last_error.restype = _str
    _lib = L
    return L


def _call(name: str, *args) -> None:
    """Call the entry point `name`; a status other than 0 raises MrtError."""
    rc = getattr(lib(), name)(*args)
    if rc != 0:
        e = MrtError(f"{name} failed ({rc}): {lib().mrt_last_error().decode()}")
        e.status = rc
        raise e


def _get(ctype, name: str, *args):
    """A new `ctype` that the entry point `name` fills through its last argument."""
    out = ctype()
    _call(name, *args, ctypes.byref(out))
    return out


def _launch(name: str, *args, stream, sync) -> None:
    """A stage-level entry point: `stream` is its last argument, and sync waits for it."""
    _call(name, *args, stream)
    if sync:
        synchronize(stream)


def _opt(struct):
    """An optional struct argument: its address, or NULL for None."""
    return ctypes.byref(struct) if struct is not None else None


def _ptr(array):
    """The address of a numpy array's data."""
    return ctypes.c_void_p(array.ctypes.data)


class _Handle:
    """An object of the library's that this one owns: _destroy names the entry
    point that frees it."""
    _destroy = None
    _h = None

    @property
    def handle(self):
        return self._h

    def close(self):
        if self._h:
            getattr(lib(), self._destroy)(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def scene_path(name: str) -> str:
    """Path of a scene shipped with the package (metal-renderer_amd/scenes: the
    reference's renderer/Media OBJ/MTL data files, unchanged)."""
    return name if os.path.sep in name else os.path.join(SCENES_DIR, name if name.endswith(".obj") else name + ".obj")


class Scene(_Handle):
    """Flattened scene + BVH on the device (initRaytracing, Renderer.mm:255-470)."""
    _destroy = "mrt_scene_destroy"

    def __init__(self, obj: str, mtl_override: str | None = None, *, procedural_triangles: int = 0,
                 procedural_seed: int = 1, max_leaf_size: int = 0, lds_nodes: int = 0, device: int = 0,
                 bvh_width: int = 0, bvh_builder: int = 0, occluder_tree: bool = True):
        d = SceneDesc(scene_path(obj).encode(), (mtl_override or "").encode(), procedural_triangles,
                      procedural_seed, max_leaf_size, lds_nodes, device, bvh_width, bvh_builder,
                      0 if occluder_tree else 1)
        self._h = _get(_vp, "mrt_scene_create", ctypes.byref(d))
        self.info = _get(SceneInfo, "mrt_scene_info_get", self._h).as_dict()

    def export(self):
        """Flattened reference-layout buffers as numpy structured arrays."""
        import numpy as np
        n = self.info
        vt = np.dtype({"names": ["v", "n"], "formats": [("<f4", 3), ("<f4", 3)], "offsets": [0, 12], "itemsize": 24})
        mt = np.dtype({"names": ["diffuse", "emissive", "ior", "materialType"],
                       "formats": [("<f4", 3), ("<f4", 3), "<f4", "<u4"], "offsets": [0, 12, 24, 28], "itemsize": 32})
        rt = np.dtype({"names": ["tri", "materialIndex", "lightTriangleIndex"],
                       "formats": [("<u4", 3), "<u4", "<u4"], "offsets": [0, 12, 16], "itemsize": 20})
        lt = np.dtype({"names": ["emissive", "v1", "v2", "v3", "area", "pdf", "cdf", "index"],
                       "formats": [("<f4", 3), vt, vt, vt, "<f4", "<f4", "<f4", "<u4"],
                       "offsets": [0, 12, 36, 60, 84, 88, 92, 96], "itemsize": 100})
        V = np.zeros(n["vertices"], vt)
        I = np.zeros(3 * n["triangles"], np.uint32)
        M = np.zeros(n["materials"], mt)
        R = np.zeros(n["triangles"], rt)
        Lt = np.zeros(n["light_triangles"] + 1, lt)
        _call("mrt_scene_export", self._h, _ptr(V), _ptr(I), _ptr(M), _ptr(R), _ptr(Lt))
        return {"vertices": V, "indices": I, "materials": M, "references": R, "lights": Lt}

    def check_bvh(self) -> None:
        _call("mrt_scene_check_bvh", self._h)

    def box_margin(self, rays, intersections):
        """Host-only test entry mrt_debug_box_margin: per ray (numpy records,
        reference layout) and its nearest hit, the culling slack the hit needs
        in the main tree, as (precise, fast) slab arithmetic, then the same for
        the hit's near ties (mrt.h): float32 [n, 4]."""
        import numpy as np
        rays = np.ascontiguousarray(rays)
        intersections = np.ascontiguousarray(intersections)
        assert len(rays) == len(intersections) and intersections.dtype.itemsize == 16
        out = np.zeros((len(rays), 4), np.float32)
        _call("mrt_debug_box_margin", self._h, _ptr(rays), rays.dtype.itemsize, len(rays), _ptr(intersections),
              _ptr(out))
        return out


class Accel(_Handle):
    """MPSTriangleAccelerationStructure + MPSRayIntersector over caller-owned
    device buffers (renderer/Renderer.mm:456-469): positions at `vertex_stride`
    (24 = sizeof(Vertex)), uint32 indices, nearest-hit queries."""
    _destroy = "mrt_accel_destroy"

    def __init__(self, vertices_ptr: int, vertex_stride: int, indices_ptr: int, triangle_count: int, *,
                 device: int = 0, builder: int = 0, max_leaf_size: int = 0, stream: int | None = None):
        d = AccelDesc(vertices_ptr, vertex_stride, indices_ptr, triangle_count, device, builder, max_leaf_size,
                      stream)
        self._h = _get(_vp, "mrt_accel_create", ctypes.byref(d))

    def rebuild(self) -> None:
        _call("mrt_accel_rebuild", self._h)

    def info(self) -> dict:
        return _get(AccelInfo, "mrt_accel_info_get", self._h).as_dict()

    def intersect(self, rays_ptr: int, stride: int, count: int, isect_ptr: int, precise=True, stream=None,
                  sync=True) -> None:
        _launch("mrt_accel_intersect", self._h, rays_ptr, stride, count, isect_ptr, _flags(precise),
                stream=stream, sync=sync)


class Renderer(_Handle):
    """One accumulating renderer on one device (the reference's `Renderer`)."""
    _destroy = "mrt_renderer_destroy"

    def __init__(self, scene: Scene, width: int, height: int, max_path_length: int = 8, *,
                 seed: int = DEFAULT_SEED, shard_rank: int = 0, shard_count: int = 1, precise: bool = False,
                 profile: bool = False, stream: int | None = None, image_ptr: int | None = None,
                 animate_noise: bool = True, accumulate_image: bool = True, debug_material: bool = False,
                 moments: bool = False):
        """animate_noise / accumulate_image / debug_material: the reference's
        ANIMATE_NOISE, ACCUMULATE_IMAGE and DEBUG_MATERIAL switches (defaults =
        the reference's defaults).  moments: accumulate the luminance moments
        beside the image (FLAG_MOMENTS), for denoise_variance."""
        self.scene = scene  # keep alive
        flags = ((FLAG_PRECISE if precise else 0) | (FLAG_PROFILE if profile else 0) |
                 (0 if animate_noise else FLAG_STATIC_NOISE) | (0 if accumulate_image else FLAG_NO_ACCUMULATE) |
                 (FLAG_DEBUG_MATERIAL if debug_material else 0) | (FLAG_MOMENTS if moments else 0))
        d = RendererDesc(scene.handle, width, height, max_path_length, seed, shard_rank, shard_count, flags,
                         stream, image_ptr)
        self._h = _get(_vp, "mrt_renderer_create", ctypes.byref(d))
        self.width, self.height = width, height
        self._prev_scene = None   # the scene a move_scene left, until the renderer has synchronised
        self._pinned = []         # scenes of move_scene calls that failed on the device (move_scene)

    # -mtkView:drawableSizeWillChange:
    def resize(self, width: int, height: int) -> None:
        _call("mrt_renderer_resize", self._h, width, height)
        self.width, self.height = width, height
        self._prev_scene = None

    def set_scene(self, scene: Scene) -> None:
        """resize() to the same size with another scene: waits for the queued
        work, plans the kernel again, restarts at frame 0; camera, flags and
        noise schedules persist (mrt_renderer_set_scene)."""
        _call("mrt_renderer_set_scene", self._h, scene.handle)
        self.scene = scene
        self._prev_scene = None

    def reset(self) -> None:
        _call("mrt_renderer_reset", self._h)

    def set_camera(self, camera: Camera) -> None:
        """reset() plus a new camera; draws already enqueued keep theirs, and
        the call does not wait for the GPU (mrt_renderer_set_camera)."""
        _call("mrt_renderer_set_camera", self._h, ctypes.byref(camera))

    @property
    def camera(self) -> Camera:
        return _get(Camera, "mrt_renderer_get_camera", self._h)

    def prepare(self, frames: int) -> None:
        _call("mrt_renderer_prepare", self._h, frames)

    # -drawInMTKView:
    def draw(self, frames: int = 1) -> None:
        _call("mrt_renderer_draw_n", self._h, frames)

    def draw_frame(self) -> None:
        """One drawInMTKView: frame (mrt_renderer_draw, 1 spp): enqueued
        without waiting for the GPU (at most 3 draws in flight, the
        reference's MaxBuffersInFlight)."""
        _call("mrt_renderer_draw", self._h)

    def set_max_frames(self, n: int) -> None:
        """MAX_FRAMES (Renderer.mm:589-590): draws past frame n are no-ops (0 = unlimited)."""
        _call("mrt_renderer_set_max_frames", self._h, n)

    def sync(self) -> None:
        _call("mrt_renderer_sync", self._h)
        self._prev_scene = None

    def image_ptr(self) -> int:
        return _get(_vp, "mrt_renderer_image", self._h).value

    def stream(self) -> int:
        """The renderer's main stream (libmrt's HIP runtime)."""
        return _get(_vp, "mrt_renderer_stream", self._h).value

    def _read(self, what, shape=None, dtype="float32", *more):
        """A new array ([H, W, 4] unless `shape` is given) filled by the reader
        `what`, which takes the renderer, the array, its size and then `more`."""
        import numpy as np
        a = np.zeros((self.height, self.width, 4) if shape is None else shape, dtype)
        _call(what, self._h, _ptr(a), a.size, *more)
        self._prev_scene = None   # (every reader synchronises)
        return a

    def read_image(self):
        """[H, W, 4] float32, row 0 = bottom (the reference texture orientation)."""
        return self._read("mrt_renderer_read_image")

    # -saveCurrentImage
    def save_current_image(self, path: str) -> None:
        _call("mrt_renderer_save_image", self._h, path.encode())

    # ---- denoised output (include/mrt.h: mrt_renderer_denoise) ----
    def denoise(self, params: "DenoiseParams | None" = None) -> None:
        """Filter the accumulation image into the renderer's denoised buffer,
        enqueued behind the draws queued so far (no host wait); params None =
        DenoiseParams.default(frames accumulated).  The image is not written."""
        _call("mrt_renderer_denoise", self._h, _opt(params))

    def read_denoised(self):
        """[H, W, 4] float32 denoised image, row 0 = bottom."""
        return self._read("mrt_renderer_read_denoised")

    def save_denoised(self, path: str) -> None:
        _call("mrt_renderer_save_denoised", self._h, path.encode())

    # ---- temporal history (include/mrt.h: mrt_renderer_move_camera) ----
    def move_camera(self, camera: Camera, params: "ReprojectParams | None" = None) -> None:
        """set_camera() that carries what has been accumulated into the new
        view, as a counted history beside the image (no host wait); params
        None = ReprojectParams.default()."""
        _call("mrt_renderer_move_camera", self._h, ctypes.byref(camera), _opt(params))

    def move_scene(self, scene: Scene, camera: "Camera | None" = None,
                   params: "ReprojectParams | None" = None) -> None:
        """move_camera() across a scene change: `scene` is another pose of the
        scene in force (scene_motion_compatible); camera None keeps the camera.
        The scene it replaces is kept alive here until the next sync or read
        (mrt_renderer_move_scene)."""
        try:
            _call("mrt_renderer_move_scene", self._h, scene.handle, _opt(camera), _opt(params))
        except MrtError as e:
            # A failed check (INVALID, STATE) changed nothing.  A device error may have struck before or behind
            # the swap, and the library has no call that tells which scene is in force: both stay alive with the
            # renderer, and self.scene goes on naming the one it was created or last moved with
            if e.status not in (-1, -5):   # MRT_ERR_INVALID, MRT_ERR_STATE
                self._pinned.append(scene)
            raise
        self._prev_scene, self.scene = self.scene, scene

    def resolve(self) -> None:
        """Merge the image with the history into the renderer's resolved
        buffer, enqueued behind the draws queued so far (no host wait)."""
        _call("mrt_renderer_resolve", self._h)

    def read_resolved(self):
        """[H, W, 4] float32 resolved image, row 0 = bottom; the fourth channel
        is the sample count behind the pixel."""
        return self._read("mrt_renderer_read_resolved")

    def save_resolved(self, path: str) -> None:
        _call("mrt_renderer_save_resolved", self._h, path.encode())

    def denoise_resolved(self, params: "DenoiseParams | None" = None) -> None:
        """resolve(), then the A-Trous filter of the resolved buffer into the
        denoised buffer; params None = DenoiseParams.default(max(frames, 1))."""
        _call("mrt_renderer_denoise_resolved", self._h, _opt(params))

    # ---- variance-guided denoising (include/mrt.h: mrt_renderer_denoise_variance) ----
    def read_moments(self):
        """[H, W, 4] float32 moments image (mean l, mean l*l, 0, 1), row 0 = bottom."""
        return self._read("mrt_renderer_read_moments")

    def moments_ptr(self) -> int:
        return _get(_vp, "mrt_renderer_moments", self._h).value

    def denoise_variance(self, params: "SvgfParams | None" = None) -> None:
        """resolve(), the variance estimate from the resolved moments, then the
        variance-guided filter of the resolved buffer into the denoised buffer
        (no host wait); params None = SvgfParams.default()."""
        _call("mrt_renderer_denoise_variance", self._h, _opt(params))

    def read_variance(self):
        """[H, W] float32: the variance plane the last denoise_variance fed to the filter."""
        return self._read("mrt_renderer_read_variance", (self.height, self.width))

    # ---- firefly suppression (include/mrt.h: mrt_renderer_set_firefly) ----
    def set_firefly(self, params: "FireflyParams | None") -> None:
        """Clamp outliers of the resolved buffer ahead of denoise_variance's
        filter (and so of error_estimate and converge); None switches it off.
        Biased: energy is removed, not redistributed."""
        _call("mrt_renderer_set_firefly", self._h, _opt(params))

    @property
    def firefly(self) -> "FireflyParams | None":
        """The clamp's parameters while it is on, else None."""
        p = FireflyParams()
        on = _get(_u32, "mrt_renderer_get_firefly", self._h, ctypes.byref(p))
        return p if on.value else None

    def read_clamped(self):
        """([H, W, 4] float32, pixels changed): what the last clamp fed to the filter."""
        n = _u32()
        return self._read("mrt_renderer_read_clamped", None, "float32", ctypes.byref(n)), n.value

    # ---- adaptive sampling (include/mrt.h: mrt_renderer_refine) ----
    def tile_count(self) -> int:
        return ((self.width + TILE - 1) // TILE) * ((self.height + TILE - 1) // TILE)

    def draw_tiles(self, tiles, frames: int = 1) -> None:
        """`frames` extra frames of the listed 64x64 tiles (row-major tile
        indices, distinct) into the counted extra images; the image, the
        moments and stats()['frame_index'] are not touched (no host wait)."""
        import numpy as np
        t = np.ascontiguousarray(tiles, np.uint32).reshape(-1)
        _call("mrt_renderer_draw_tiles", self._h, _ptr(t), t.size, frames)

    def refine(self, frames: int, tiles: int, params: "AdaptiveParams | None" = None) -> None:
        """One adaptive pass: the variance plane of what has been accumulated,
        a priority per tile, the `tiles` tiles of highest priority chosen on
        the device, and `frames` extra frames of them (no host wait); params
        None = AdaptiveParams.default()."""
        _call("mrt_renderer_refine", self._h, frames, tiles, _opt(params))

    def read_extra(self):
        """[H, W, 4] float32 extra image E: (r, g, b, extra samples), row 0 = bottom."""
        return self._read("mrt_renderer_read_extra")

    def read_extra_moments(self):
        """[H, W, 4] float32 extra moments EM: (mean l, mean l*l, 0, extra samples)."""
        return self._read("mrt_renderer_read_extra_moments")

    def read_tile_priority(self):
        """float32 priorities of the last refine, one per tile (row-major)."""
        return self._read("mrt_renderer_read_tile_priority", self.tile_count())

    def read_tile_list(self):
        """uint32 tile indices the last refine or draw_tiles drew, in rank order."""
        n = _u32()
        return self._read("mrt_renderer_read_tile_list", self.tile_count(), "uint32", ctypes.byref(n))[:n.value].copy()

    def refine_stats(self) -> dict:
        return _get(RefineStats, "mrt_renderer_refine_stats", self._h).as_dict()

    # ---- sampling to a target error (include/mrt.h: mrt_renderer_converge) ----
    def error_estimate(self, threshold: float = 0.0, svgf: "SvgfParams | None" = None,
                       luminance_floor: float = 0.0) -> dict:
        """denoise_variance(svgf), then the mean relative squared error per tile
        with the denoised image below the variance, and the tiles above
        `threshold` into the tile list; draws nothing.  Returns the summary
        (ErrorSummary.as_dict()).  Waits for the device once."""
        return _get(ErrorSummary, "mrt_renderer_error", self._h, _opt(svgf), luminance_floor, threshold).as_dict()

    def read_tile_error(self):
        """(float32 mean error, uint32 counted pixels) per tile of the last error_estimate or converge."""
        import numpy as np
        e, n = np.zeros(self.tile_count(), np.float32), np.zeros(self.tile_count(), np.uint32)
        _call("mrt_renderer_read_tile_error", self._h, _ptr(e), _ptr(n), e.size)
        return e, n

    def converge(self, params: "ConvergeParams | None" = None, **fields) -> dict:
        """Estimate, draw params.frames_per_pass extra frames of the tiles
        above params.target_error, and repeat until none is above it or a limit
        ends the loop; always ends on an estimate, so read_denoised() is the
        finished picture.  params None = ConvergeParams.default(**fields).
        Returns ConvergeResult.as_dict()."""
        if params is None:
            params = ConvergeParams.default(**fields)
        elif fields:
            raise TypeError("pass either params or fields")
        return _get(ConvergeResult, "mrt_renderer_converge", self._h, ctypes.byref(params)).as_dict()

    # ---- multi-GPU exchange (include/mrt.h: mrt_renderer_exchange) ----
    def exchange(self, comm: "Comm", mode: int = EXCHANGE_GATHER) -> None:
        """Enqueue the image exchange of this shard renderer on its stream:
        RCCL gather of the packed owned tiles to rank 0 (or SUM reduce)."""
        _call("mrt_renderer_exchange", self._h, comm.handle, mode)

    def exchange_flush(self) -> None:
        _call("mrt_renderer_exchange_flush", self._h)

    def tiles_read(self, rank: int, count: int):
        """This shard's owned tiles packed into host memory (float32)."""
        import numpy as np
        out = np.zeros(tiles_packed_floats(self.width, self.height, rank, count), np.float32)
        _call("mrt_renderer_tiles_read", self._h, _ptr(out), out.size)
        return out

    def tiles_write(self, shard_rank: int, packed) -> None:
        """Write another shard's packed tiles (host float32) into the image."""
        import numpy as np
        packed = np.ascontiguousarray(packed, np.float32)
        _call("mrt_renderer_tiles_write", self._h, shard_rank, _ptr(packed), packed.size)

    def debug_exchange_unpack(self, nranks: int, gathered) -> None:
        """Test entry: rank 0's unpack of an nranks-way gather whose received
        buffer is `gathered` (host float32, nranks slabs of
        tiles_packed_floats(W, H, 0, nranks) floats) — the RCCL path's unpack
        of slabs 1..N-1 without a communicator."""
        import numpy as np
        g = np.ascontiguousarray(gathered, np.float32)
        _call("mrt_debug_exchange_unpack", self._h, nranks, _ptr(g), g.size)

    # ---- golden comparison (loadReferenceImage + blitFragment) ----
    def load_reference(self, path: str) -> None:
        _call("mrt_renderer_load_reference", self._h, path.encode())

    def display(self, flags: int = 0, compare_scale: float = 10.0):
        """[H, W, 4] float32 blit of the image (row 0 = bottom)."""
        import numpy as np
        img = np.zeros((self.height, self.width, 4), np.float32)
        _call("mrt_renderer_display", self._h, flags, compare_scale, _ptr(img), img.size)
        return img

    def display_enqueue(self, slot: int, flags: int = 0, compare_scale: float = 10.0) -> None:
        """Queue the blit of the image into display slot `slot` (no host wait)."""
        _call("mrt_renderer_display_enqueue", self._h, flags, compare_scale, slot)

    def display_map(self, slot: int):
        """[H, W, 4] float32 copy of display slot `slot` (waits for its blit)."""
        import numpy as np
        p = _vp()
        n = _get(_size, "mrt_renderer_display_map", self._h, slot, ctypes.byref(p))
        buf = (_f32 * n.value).from_address(p.value)
        return np.frombuffer(buf, np.float32).reshape(self.height, self.width, 4).copy()

    def stats(self) -> dict:
        return _get(Stats, "mrt_renderer_stats", self._h).as_dict()


# ---- stage-level ABI (device pointers, reference AoS layouts) -------------
# Each call launches on `stream` (None = libmrt's default stream) and, unless
# sync=False, waits for it with mrt_synchronize (torch.cuda.synchronize() does
# not see libmrt's runtime copy).
def synchronize(stream=None) -> None:
    _call("mrt_synchronize", stream)


def _flags(precise):
    return FLAG_PRECISE if precise else 0


def raygen(scene: Scene, width: int, height: int, noise_ptr: int, rays_ptr: int, precise=True, stream=None,
           sync=True, camera: Camera | None = None):
    if camera is None:
        _launch("mrt_raygen", scene.handle, width, height, noise_ptr, rays_ptr, _flags(precise),
                stream=stream, sync=sync)
    else:
        _launch("mrt_raygen_camera", scene.handle, ctypes.byref(camera), width, height, noise_ptr, rays_ptr,
                _flags(precise), stream=stream, sync=sync)


def intersect(scene: Scene, rays_ptr: int, stride: int, count: int, isect_ptr: int, precise=True, stream=None,
              sync=True):
    _launch("mrt_intersect", scene.handle, rays_ptr, stride, count, isect_ptr, _flags(precise),
            stream=stream, sync=sync)


def shade(scene: Scene, width, height, frame_index, max_path_length, noise_ptr, isect_ptr, rays_ptr, srays_ptr,
          precise=True, stream=None, sync=True, debug_material=False):
    flags = _flags(precise) | (FLAG_DEBUG_MATERIAL if debug_material else 0)
    _launch("mrt_shade", scene.handle, width, height, frame_index, max_path_length, noise_ptr, isect_ptr, rays_ptr,
            srays_ptr, flags, stream=stream, sync=sync)


def resolve_shadow(scene: Scene, count, isect_ptr, rays_ptr, srays_ptr, precise=True, stream=None, sync=True):
    _launch("mrt_resolve_shadow", scene.handle, count, isect_ptr, rays_ptr, srays_ptr, _flags(precise),
            stream=stream, sync=sync)


def accumulate(scene: Scene, width, height, frame_index, rays_ptr, image_ptr, precise=True, stream=None, sync=True,
               accumulate_image=True):
    flags = _flags(precise) | (0 if accumulate_image else FLAG_NO_ACCUMULATE)
    _launch("mrt_accumulate", scene.handle, width, height, frame_index, rays_ptr, image_ptr, flags,
            stream=stream, sync=sync)


def moments(scene: Scene, width, height, frame_index, rays_ptr, moments_ptr, precise=True, stream=None, sync=True):
    """accumulate's counterpart for the luminance moments (mrt_moments)."""
    _launch("mrt_moments", scene.handle, width, height, frame_index, rays_ptr, moments_ptr, _flags(precise),
            stream=stream, sync=sync)


def variance(moments_ptr: int, n_ptr: int, p_ptr: int, variance_ptr: int, width: int, height: int,
             params: "SvgfParams | None", stream=None, sync=True) -> None:
    """The per-pixel variance estimate from counted moments (mrt_variance): W*H floats."""
    _launch("mrt_variance", moments_ptr, n_ptr, p_ptr, variance_ptr, width, height, _opt(params),
            stream=stream, sync=sync)


def denoise_variance(image_ptr: int, variance_ptr: int, n_ptr: int, p_ptr: int, out_ptr: int, scratch_ptr: int,
                     variance_out_ptr: "int | None", width: int, height: int, params: "SvgfParams | None", stream=None,
                     sync=True) -> None:
    """The variance-guided A-Trous filter (mrt_denoise_variance) on device buffers."""
    _launch("mrt_denoise_variance", image_ptr, variance_ptr, n_ptr, p_ptr, out_ptr, scratch_ptr, variance_out_ptr,
            width, height, _opt(params), stream=stream, sync=sync)


def firefly_clamp(image_ptr: int, n_ptr: int, p_ptr: int, out_ptr: int, clamped_ptr: "int | None", width: int,
                  height: int, params: "FireflyParams | None", stream=None, sync=True) -> None:
    """The outlier clamp (mrt_firefly_clamp) on device buffers; clamped_ptr: one uint32 or None."""
    _launch("mrt_firefly_clamp", image_ptr, n_ptr, p_ptr, out_ptr, clamped_ptr, width, height, _opt(params),
            stream=stream, sync=sync)


def debug_denoise_variance_step(image_ptr: int, variance_ptr: int, n_ptr: int, p_ptr: int, out_ptr: int, width: int,
                                height: int, params: SvgfParams, step_log2: int, path: int, stream=None,
                                sync=True) -> None:
    """Measurement entry: one iteration at step 2^step_log2 with implementation `path`."""
    _launch("mrt_debug_denoise_variance_step", image_ptr, variance_ptr, n_ptr, p_ptr, out_ptr, width, height,
            ctypes.byref(params), step_log2, path, stream=stream, sync=sync)


def counted_merge(a_ptr: int, b_ptr: int, out_ptr: int, width: int, height: int, precise=True, stream=None,
                  sync=True) -> None:
    """Merge two counted images (mrt_counted_merge); out_ptr may be a_ptr."""
    _launch("mrt_counted_merge", a_ptr, b_ptr, out_ptr, width, height, _flags(precise), stream=stream, sync=sync)


def tile_priority(image_ptr: int, variance_ptr: int, n_ptr: int, priority_ptr: int, width: int, height: int,
                  params: "AdaptiveParams | None", precise=True, stream=None, sync=True) -> None:
    """One float per 64x64 tile: the relative squared error a further sample buys (mrt_tile_priority)."""
    _launch("mrt_tile_priority", image_ptr, variance_ptr, n_ptr, priority_ptr, width, height, _opt(params),
            _flags(precise), stream=stream, sync=sync)


def tile_error(image_ptr: int, variance_ptr: int, n_ptr: int, mean_ptr: int, pixels_ptr: int, width: int, height: int,
               params: "AdaptiveParams | None", precise=True, stream=None, sync=True) -> None:
    """Per 64x64 tile: the mean of v / (l^2 + eps^2) over the counted pixels, and their number (mrt_tile_error)."""
    _launch("mrt_tile_error", image_ptr, variance_ptr, n_ptr, mean_ptr, pixels_ptr, width, height, _opt(params),
            _flags(precise), stream=stream, sync=sync)


def tile_threshold(mean_ptr: int, pixels_ptr: int, tiles: int, threshold: float, max_count: int, list_ptr: int,
                   summary_ptr: int, stream=None, sync=True) -> None:
    """The tiles whose mean error exceeds `threshold`, worst first, and an
    ErrorSummary in device memory (mrt_tile_threshold)."""
    _launch("mrt_tile_threshold", mean_ptr, pixels_ptr, tiles, threshold, max_count, list_ptr, summary_ptr,
            stream=stream, sync=sync)


def tile_select(priority_ptr: int, tiles: int, count: int, list_ptr: int, stream=None, sync=True) -> None:
    """The `count` tiles of highest priority, uint32, in rank order (mrt_tile_select)."""
    _launch("mrt_tile_select", priority_ptr, tiles, count, list_ptr, stream=stream, sync=sync)


def guides(scene: Scene, width: int, height: int, n_ptr: int, p_ptr: int, camera: Camera | None = None, precise=True,
           stream=None, sync=True):
    """First-hit guide planes of the denoiser (mrt_guides): (normal, bits(word))
    and (position, t), W*H float4 each on the device."""
    _launch("mrt_guides", scene.handle, _opt(camera), width, height, n_ptr, p_ptr, _flags(precise),
            stream=stream, sync=sync)


def scene_motion_compatible(a: Scene, b: Scene) -> None:
    """Raises MrtError (status -1, naming the first difference) unless the two
    scenes are poses of one mesh (mrt_scene_motion_compatible; host only)."""
    _call("mrt_scene_motion_compatible", a.handle, b.handle)


def guides_motion(scene: Scene, prev_scene: Scene, width: int, height: int, n_ptr: int, p_ptr: int, motion_n_ptr: int,
                  motion_p_ptr: int, camera: Camera | None = None, precise=True, stream=None, sync=True):
    """guides() of `scene` and the motion planes: each pixel's surface point as
    it lies in prev_scene (mrt_guides_motion).  With sync=False both scenes must
    outlive the stream's work."""
    _launch("mrt_guides_motion", scene.handle, prev_scene.handle, _opt(camera), width, height, n_ptr, p_ptr,
            motion_n_ptr, motion_p_ptr, _flags(precise), stream=stream, sync=sync)


def denoise(image_ptr: int, n_ptr: int, p_ptr: int, out_ptr: int, scratch_ptr: int, width: int, height: int,
            params: DenoiseParams, stream=None, sync=True):
    """The edge-avoiding A-Trous filter (mrt_denoise) on device buffers."""
    _launch("mrt_denoise", image_ptr, n_ptr, p_ptr, out_ptr, scratch_ptr, width, height, _opt(params),
            stream=stream, sync=sync)


def temporal_resolve(image_ptr: int, frames: int, history_ptr: "int | None", out_ptr: int, width: int, height: int,
                     stream=None, sync=True) -> None:
    """Merge an accumulation image of `frames` frames with a counted history
    (None = no history) into a counted image (mrt_temporal_resolve)."""
    _launch("mrt_temporal_resolve", image_ptr, frames, history_ptr, out_ptr, width, height, stream=stream, sync=sync)


def reproject(prev_ptr: int, prev_n_ptr: int, prev_p_ptr: int, prev_camera: "Camera | None", cur_n_ptr: int,
              cur_p_ptr: int, out_ptr: int, width: int, height: int, params: "ReprojectParams | None", stream=None,
              sync=True) -> None:
    """Reproject a counted image through the guide planes of the previous and
    the current camera (mrt_reproject)."""
    _launch("mrt_reproject", prev_ptr, prev_n_ptr, prev_p_ptr, _opt(prev_camera), cur_n_ptr, cur_p_ptr, out_ptr,
            width, height, _opt(params), stream=stream, sync=sync)


def debug_denoise_path(path: int) -> None:
    """Test entry: 0 = the shipped choice per step, 1 = direct, 2 = LDS-staged where supported."""
    _call("mrt_debug_denoise_path", path)


def debug_denoise_step(image_ptr: int, n_ptr: int, p_ptr: int, out_ptr: int, scratch_ptr: int, width: int, height: int,
                       params: DenoiseParams, step_log2: int, path: int, stream=None, sync=True) -> None:
    """Measurement entry: one iteration at step 2^step_log2 with implementation `path`."""
    _launch("mrt_debug_denoise_step", image_ptr, n_ptr, p_ptr, out_ptr, scratch_ptr, width, height,
            ctypes.byref(params), step_log2, path, stream=stream, sync=sync)


def noise_table(seed: int, frame: int):
    import numpy as np
    out = np.zeros(64 * 64 * 4, np.float32)
    _call("mrt_noise_table", seed, frame, _ptr(out))
    return out


def shard_mask(width: int, height: int, rank: int, count: int):
    """[H, W] uint8 ownership mask of a shard (row 0 = bottom) and its pixel count."""
    import numpy as np
    m = np.zeros((height, width), np.uint8)
    n = np.zeros(1, np.uint64)
    _call("mrt_shard_mask", width, height, rank, count, _ptr(m), _ptr(n))
    return m, int(n[0])


def display_compare(mode: int) -> int:
    return mode << 8


def display(image_ptr: int, out_ptr: int, width: int, height: int, flags: int = 0, reference_ptr: int | None = None,
            compare_scale: float = 10.0, stream=None, sync=True) -> None:
    """blitFragment (Shaders.metal:33-70): tone map / sRGB / golden comparison on the device."""
    _launch("mrt_display", image_ptr, reference_ptr, out_ptr, width, height, flags, compare_scale,
            stream=stream, sync=sync)


def tiles_packed_floats(width: int, height: int, rank: int, count: int) -> int:
    return _get(_u64, "mrt_tiles_packed_floats", width, height, rank, count).value


def tiles_pack(image_ptr: int, width: int, height: int, rank: int, count: int, packed_ptr: int, stream=None,
               sync=True) -> None:
    """A shard's owned tiles of a device image -> dense [tile][64*64] RGBA32F (multi-GPU exchange)."""
    _launch("mrt_tiles_pack", image_ptr, width, height, rank, count, packed_ptr, stream=stream, sync=sync)


def tiles_unpack(packed_ptr: int, width: int, height: int, rank: int, count: int, image_ptr: int, stream=None,
                 sync=True) -> None:
    _launch("mrt_tiles_unpack", packed_ptr, width, height, rank, count, image_ptr, stream=stream, sync=sync)


def tiles_pack_host(image, rank: int, count: int):
    """numpy restatement of mrt_tiles_pack (host rehearsal of the exchange; image is H x W x 4)."""
    import numpy as np
    H, W = image.shape[:2]
    tx_n, ty_n = (W + 63) // 64, (H + 63) // 64
    tiles = list(range(rank, tx_n * ty_n, count))
    out = np.zeros((len(tiles), 64, 64, 4), np.float32)
    for k, t in enumerate(tiles):
        ty, tx = divmod(t, tx_n)
        blk = image[ty * 64:(ty + 1) * 64, tx * 64:(tx + 1) * 64]
        out[k, :blk.shape[0], :blk.shape[1]] = blk
    return out


def tiles_unpack_host(packed, image, rank: int, count: int) -> None:
    H, W = image.shape[:2]
    tx_n, ty_n = (W + 63) // 64, (H + 63) // 64
    for k, t in enumerate(range(rank, tx_n * ty_n, count)):
        ty, tx = divmod(t, tx_n)
        h, w = min(64, H - ty * 64), min(64, W - tx * 64)
        image[ty * 64:ty * 64 + h, tx * 64:tx * 64 + w] = packed[k, :h, :w]


def debug_magic_div(d: int, n):
    """n // d through libmrt's exact launch-divisor division (test entry)."""
    import numpy as np
    n = np.ascontiguousarray(n, np.uint32)
    q = np.zeros(len(n), np.uint32)
    _call("mrt_debug_magic_div", d, _ptr(n), len(n), _ptr(q))
    return q


def debug_stamps(reset: bool = True):
    import numpy as np
    out = np.zeros(8, np.uint64)
    _call("mrt_debug_stamps", _ptr(out), int(reset))
    return out


def debug_lanes(reset: bool = True):
    """Lane-occupancy counters of the lane-statistics library (zeros in the
    product library); tools/lane_stats.py names the slots."""
    import numpy as np
    out = np.zeros(64, np.uint64)
    _call("mrt_debug_lanes", _ptr(out), out.size, int(reset))
    return out


def debug_sweep_list(scene: "Scene"):
    """(enabled, records) of the scene's leaf-box sweep list (test entry):
    records is an (n, 8) uint32 view of the float records (lo.xyz, leaf ref,
    hi.xyz, 0), empty for a tree the sweep cannot take; enabled tells whether
    nearest queries sweep it instead of walking the tree."""
    import numpy as np
    out = np.zeros((32, 8), np.uint32)
    count = _u32()
    enabled = _get(_u32, "mrt_debug_sweep_list", scene.handle, _ptr(out), len(out), ctypes.byref(count))
    return bool(enabled.value), out[:min(count.value, len(out))].copy()


def debug_sweep_pairs(scene: "Scene"):
    """(records, prims) of the list the sweep kernels get, derived from the
    per-leaf list (test entry): records is an (n, 8) uint32 view of the float
    records (lo.xyz, ka | kb << 16, hi.xyz, 0), one per group of at most two
    triangles (leaf-ordered indices; kb == ka: one); prims is (n, 2), the two
    triangles' primitive ids.  Empty for a tree the sweep cannot take."""
    import numpy as np
    out, prims = np.zeros((32, 8), np.uint32), np.zeros((32, 2), np.uint32)
    count = _get(_u32, "mrt_debug_sweep_pairs", scene.handle, _ptr(out), _ptr(prims), len(out))
    n = min(count.value, len(out))
    return out[:n].copy(), prims[:n].copy()


def debug_sweep_phase1(scene: "Scene"):
    """Phase 1's list of a scene that sweeps (test entry): an (n, 8) uint32
    view of the float records (c.xyz, id, e.xyz, 1 << id), one per record of
    debug_sweep_pairs in its order; empty for a scene whose queries walk."""
    import numpy as np
    out = np.zeros((32, 8), np.uint32)
    count = _get(_u32, "mrt_debug_sweep_phase1", scene.handle, _ptr(out), len(out))
    return out[:min(count.value, len(out))].copy()


def debug_sweep_cap(scene: "Scene") -> int:
    """Rest pops per pass of the stream kernel's queue levels before a ray
    with leaves left is recycled (test entry; 32: never)."""
    return _get(_u32, "mrt_debug_sweep_cap", scene.handle).value


def debug_bvh_nodes(scene: "Scene"):
    """The main tree's BVH4 nodes as an (n, 32) uint32 array (test entry)."""
    import numpy as np
    out = np.zeros((scene.info["bvh_nodes"], 32), np.uint32)
    count = _get(_u32, "mrt_debug_bvh_nodes", scene.handle, _ptr(out), len(out))
    return out[:count.value]


def debug_wave_times():
    """Per-wave timeline of the last launch of each bounce index % 4 (stamp
    library only), shape (4, 8192, 16), 100 MHz ticks: {start, exit,
    iterations | exit reason << 32, last grab, end of the last grab's work,
    summed grab latency, max grab latency, last grab's latency, phase
    cycles 0..4, 0, 0, 0}."""
    import numpy as np
    out = np.zeros((4, 8192, 16), np.uint64)
    _call("mrt_debug_wave_times", _ptr(out), out.size)
    return out


class Event:
    """A completion marker on a libmrt stream (host-side ordering against
    another runtime's work, e.g. torch/RCCL in the multi-GPU exchange)."""

    def __init__(self):
        self._e = _vp()

    def record(self, stream=None) -> None:
        _call("mrt_event_record", stream, ctypes.byref(self._e))

    def synchronize(self) -> None:
        _call("mrt_event_synchronize", self._e)

    def close(self) -> None:
        if self._e.value:
            _call("mrt_event_destroy", self._e)
            self._e = _vp()


def load_exr(path: str):
    """Decode a scanline OpenEXR file (libmrt's reader): [H, W, 4] float32,
    row 0 = BOTTOM."""
    import numpy as np
    w, h = _u32(), _u32()
    _call("mrt_image_load_exr", path.encode(), None, 0, ctypes.byref(w), ctypes.byref(h))
    img = np.zeros((h.value, w.value, 4), np.float32)
    _call("mrt_image_load_exr", path.encode(), _ptr(img), img.size, ctypes.byref(w), ctypes.byref(h))
    return img


def comm_unique_id() -> bytes:
    """ncclGetUniqueId on rank 0; distribute the bytes to every rank."""
    buf = ctypes.create_string_buffer(COMM_ID_BYTES)
    _call("mrt_comm_unique_id", buf, COMM_ID_BYTES)
    return buf.raw


class Comm(_Handle):
    """RCCL communicator of one rank (one process per GPU)."""
    _destroy = "mrt_comm_destroy"

    def __init__(self, unique_id: bytes, nranks: int, rank: int, device: int = 0):
        if len(unique_id) != COMM_ID_BYTES:
            raise MrtError("unique id must be 128 bytes")
        self._h = _get(_vp, "mrt_comm_create", ctypes.create_string_buffer(unique_id, COMM_ID_BYTES), nranks, rank,
                       device)
        self.nranks, self.rank = nranks, rank

    def set_timeout(self, ms: int) -> None:
        """Bound of the renderer's waits for this communicator's collectives (0 = 120 s)."""
        _call("mrt_comm_set_timeout", self._h, ms)

    def check(self) -> None:
        """Non-blocking health check: raises MrtError once the communicator is aborted."""
        _call("mrt_comm_check", self._h)

    def debug_fail(self, mode: int) -> None:
        """Test entry: 1 = report an asynchronous error, 2 = collectives never complete."""
        _call("mrt_debug_comm_fail", self._h, mode)


def device_count() -> int:
    return int(lib().mrt_device_count())
