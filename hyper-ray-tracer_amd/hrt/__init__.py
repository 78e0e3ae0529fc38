"""hrt — Python binding of libhrt.so, the MI355X path-tracing inner loop.

Host side of the drop-in boundary (include/hrt/hrt.h) for tests, bench and scripts.  Names follow
the reference (SkillerRaptor/hyper-ray-tracer): Scene presets mirror `arguments::Scene`
(src/arguments.rs:9-19), `render()` replaces `Application::render` (src/application.rs:393-475).

The library is the HIP build in hyper-ray-tracer_amd/lib/libhrt.so; importing this module never
falls back to anything else: a missing library raises.
"""
from __future__ import annotations

import ctypes
import os
from dataclasses import dataclass, field
from typing import List, Optional, Sequence, Tuple

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
PKG_ROOT = os.path.dirname(_HERE)
LIB_PATH = os.environ.get("HRT_LIB") or os.path.join(PKG_ROOT, "lib", "libhrt.so")  # HRT_LIB: A/B against another build

# ---------------------------------------------------------------------------------------- enums
OK = 0
ERR_INVALID_ARG, ERR_EMPTY, ERR_NO_BBOX, ERR_NAN, ERR_STATE, ERR_HIP, ERR_OOM, ERR_UNSUPPORTED = range(1, 9)
PLANE_XY, PLANE_YZ, PLANE_ZX = 0, 1, 2
AXIS_X, AXIS_Y, AXIS_Z = 0, 1, 2

PRESETS = {
    "random": 0,
    "two_spheres": 1,
    "two_perlin_spheres": 2,
    "earth": 3,
    "simple_light": 4,
    "cornell": 5,
    "cornell_smoke": 6,
    "final": 7,
    "earth_perlin": 8,
    "random_10k": 9,
    "features": 10,
    "random_40k": 11,  # build-defined: 39.9k leaves, the device-built walk hierarchy by default
    "motion": 12,  # build-defined: moving spheres with their own shutter intervals (no scene-wide factor)
}


class HrtError(RuntimeError):
    def __init__(self, status: int, msg: str):
        super().__init__(f"hrt status {status}: {msg}")
        self.status = status


# ---------------------------------------------------------------------------------------- structs
class Camera(ctypes.Structure):
    _fields_ = [
        ("origin", ctypes.c_float * 3),
        ("lower_left_corner", ctypes.c_float * 3),
        ("horizontal", ctypes.c_float * 3),
        ("vertical", ctypes.c_float * 3),
        ("u", ctypes.c_float * 3),
        ("v", ctypes.c_float * 3),
        ("w", ctypes.c_float * 3),
        ("lens_radius", ctypes.c_float),
        ("time0", ctypes.c_float),
        ("time1", ctypes.c_float),
    ]


class RenderParams(ctypes.Structure):
    _fields_ = [
        ("width", ctypes.c_uint32),
        ("height", ctypes.c_uint32),
        ("samples", ctypes.c_uint32),
        ("max_depth", ctypes.c_uint32),
        ("sample_offset", ctypes.c_uint32),
        ("flags", ctypes.c_uint32),
        ("t_min", ctypes.c_float),
        ("background", ctypes.c_float * 3),
        ("seed", ctypes.c_uint64),
    ]


class Tile(ctypes.Structure):
    _fields_ = [("x", ctypes.c_uint32), ("y", ctypes.c_uint32), ("w", ctypes.c_uint32), ("h", ctypes.c_uint32)]


class RenderStats(ctypes.Structure):
    _fields_ = [(n, ctypes.c_uint64) for n in ("segments", "samples", "pixels", "node_visits", "prim_tests", "tex_evals",
                                                      "walk_slots", "shade_slots", "prim_slots")] + \
        [("phase_cycles", ctypes.c_uint64 * 3), ("park_slots", ctypes.c_uint64), ("wait_slots", ctypes.c_uint64),
         ("leaf_cycles", ctypes.c_uint64), ("walk_steps", ctypes.c_uint64)]


class TilePixels(ctypes.Structure):
    """hrt_tile_pixels (include/hrt/hrt.h)."""
    _fields_ = [("x", ctypes.c_uint32), ("y", ctypes.c_uint32), ("width", ctypes.c_uint32),
                ("height", ctypes.c_uint32), ("pixels", ctypes.POINTER(ctypes.c_float))]


TILE_FN = ctypes.CFUNCTYPE(None, ctypes.POINTER(TilePixels), ctypes.c_void_p)


class BlobInfo(ctypes.Structure):
    """hrt_blob_info (include/hrt/hrt.h)."""
    _fields_ = [(n, ctypes.c_uint64) for n in ("off_nodes", "off_prims", "off_insts", "off_media", "off_mats", "off_texs",
                                                "off_perlin", "off_images")] + \
        [(n, ctypes.c_uint32) for n in ("n_nodes", "main_end", "n_prims", "feature_mask", "cull_mode", "motion_uniform")] + \
        [("motion_t0", ctypes.c_float), ("motion_span", ctypes.c_float), ("ln_e", ctypes.c_float),
         ("media_nested", ctypes.c_uint32), ("box_t0", ctypes.c_float), ("box_t1", ctypes.c_float),
         ("off_walk", ctypes.c_uint64), ("walk_bytes", ctypes.c_uint32), ("walk_regrouped", ctypes.c_uint32),
         ("bvh_tied_sorts", ctypes.c_uint32), ("walk_hot", ctypes.c_uint32),
                ("walk_general", ctypes.c_uint32), ("off_chains", ctypes.c_uint64),
        ("walk_half", ctypes.c_uint32), ("walk_c16", ctypes.c_uint32), ("walk_nodes", ctypes.c_uint32),
        ("walk_pbase", ctypes.c_uint32)]


class PresetInfo(ctypes.Structure):
    _fields_ = [
        ("look_from", ctypes.c_float * 3),
        ("look_at", ctypes.c_float * 3),
        ("fov", ctypes.c_float),
        ("aperture", ctypes.c_float),
        ("focus_dist", ctypes.c_float),
        ("time0", ctypes.c_float),
        ("time1", ctypes.c_float),
        ("background", ctypes.c_float * 3),
        ("root", ctypes.c_uint32),
    ]


class SceneInfo(ctypes.Structure):
    _fields_ = [
        (n, ctypes.c_uint32)
        for n in ("nodes", "prims", "materials", "textures", "instances", "media", "feature_mask", "blob_bytes", "in_lds",
                  "cull_mode", "sah_stream_len", "bvh_tied_sorts", "walk_regrouped", "walk_device_built", "walk_build_us")
    ]


class LaunchInfo(ctypes.Structure):
    """hrt_launch_info: the last render launch of the calling thread (hrt_last_launch)."""
    _fields_ = [("kernel", ctypes.c_char * 160)] + [
        (n, ctypes.c_uint32) for n in ("grid", "block", "blocks_per_cu", "cus", "waves_per_simd", "vgprs", "scratch_bytes",
                                       "lds_bytes")
    ] + [("knobs", ctypes.c_char * 256)]


class TileNoise(ctypes.Structure):
    """hrt_tile_noise: a tile's mean and max per-pixel error, and the samples and chunks it holds."""
    _fields_ = [("mean", ctypes.c_float), ("max", ctypes.c_float), ("samples", ctypes.c_uint64), ("chunks", ctypes.c_uint64)]


class FilterParams(ctypes.Structure):
    """hrt_filter_params: the a-trous filter's iterations (1..5) and luminance tolerance in standard errors."""
    _fields_ = [("iterations", ctypes.c_uint32), ("sigma", ctypes.c_float)]


class GuidedParams(ctypes.Structure):
    """hrt_guided_params: the a-trous filter's iterations and sigma, and the tolerances of the normal, albedo and depth
    terms (0: the term is off)."""
    _fields_ = [("iterations", ctypes.c_uint32), ("sigma", ctypes.c_float), ("normal", ctypes.c_float),
                ("albedo", ctypes.c_float), ("depth", ctypes.c_float)]


class GuidedExParams(ctypes.Structure):
    """hrt_guided_ex_params: hrt_guided_params, then the HRT_GUIDED_* flags, the albedo floor of GUIDED_DEMODULATE (> 0)
    and a reserved word (0)."""
    _fields_ = GuidedParams._fields_ + [("flags", ctypes.c_uint32), ("albedo_floor", ctypes.c_float),
                                        ("reserved", ctypes.c_uint32)]


class SnapshotInfo(ctypes.Structure):
    """hrt_snapshot_info: what an accumulator must be created with to take a snapshot blob."""
    _fields_ = [(n, ctypes.c_uint32) for n in ("version", "flags", "width", "height", "n_tiles", "uniform")] + \
        [("n_pixels", ctypes.c_uint64), ("bytes", ctypes.c_uint64)]


class SceneOptions(ctypes.Structure):
    """hrt_scene_options: the explicit configuration that can change an image's bits (all-zero = default)."""
    _fields_ = [(n, ctypes.c_uint32) for n in ("bvh_ties", "walk_tree", "chunk_min", "chunk_max", "chunk_uniform")]


class QueryParams(ctypes.Structure):
    """hrt_query_params (24 bytes): flags, the interval the rays' times lie in, the seed of the media's draws."""
    _fields_ = [("flags", ctypes.c_uint32), ("reserved", ctypes.c_uint32), ("time0", ctypes.c_float), ("time1", ctypes.c_float),
                ("seed", ctypes.c_uint64)]


# hrt_ray / hrt_hit (48 bytes each) as numpy structured types
RAY_DTYPE = np.dtype([("origin", np.float32, 3), ("t_min", np.float32), ("direction", np.float32, 3), ("t_max", np.float32),
                      ("time", np.float32), ("pixel", np.uint32), ("sample", np.uint32), ("segment", np.uint32)])
HIT_DTYPE = np.dtype([("t", np.float32), ("prim", np.uint32), ("material", np.uint32), ("flags", np.uint32),
                      ("point", np.float32, 3), ("u", np.float32), ("normal", np.float32, 3), ("v", np.float32)])
HIT_HIT, HIT_FRONT, HIT_MEDIUM, HIT_INVALID = 1, 2, 4, 8
QUERY_SKIP_MEDIA, QUERY_NO_LDS, QUERY_REFERENCE_CULL = 1, 2, 4


class ScatterParams(ctypes.Structure):
    """hrt_scatter_params (24 bytes): flags (none defined), the background a miss gathers, two reserved words."""
    _fields_ = [("flags", ctypes.c_uint32), ("reserved", ctypes.c_uint32), ("background", ctypes.c_float * 3),
                ("reserved2", ctypes.c_uint32)]


# hrt_path (48 bytes): a caller-held path between hrt_scene_intersect and hrt_scene_scatter
PATH_DTYPE = np.dtype([("rng", np.uint32, 4), ("throughput", np.float32, 3), ("depth_left", np.uint32),
                       ("radiance", np.float32, 3), ("flags", np.uint32)])
PATH_DONE, PATH_MISSED, PATH_ABSORBED, PATH_DEPTH, PATH_INVALID = 1, 2, 4, 8, 16


class StepParams(ctypes.Structure):
    """hrt_step_params (40 bytes): STEP_* flags (the QUERY_* ones), the rounds a live path makes inside the call, the
    interval the rays' times lie in, the seed of the media's draws, the background a miss gathers."""
    _fields_ = [("flags", ctypes.c_uint32), ("steps", ctypes.c_uint32), ("time0", ctypes.c_float), ("time1", ctypes.c_float),
                ("seed", ctypes.c_uint64), ("background", ctypes.c_float * 3), ("reserved", ctypes.c_uint32)]


class PathList(ctypes.Structure):
    """hrt_path_list (24 bytes): a host struct of device pointers, `capacity` u32 indices and one u32 count."""
    _fields_ = [("d_index", ctypes.c_void_p), ("d_count", ctypes.c_void_p), ("capacity", ctypes.c_uint32),
                ("reserved", ctypes.c_uint32)]


STEP_SKIP_MEDIA, STEP_NO_LDS, STEP_REFERENCE_CULL = 1, 2, 4


# Diagnostics an older build may lack; only tolerated when HRT_LIB points at another build (A/B runs)
OPTIONAL = {"hrt_abi_version", "hrt_last_launch", "hrt_debug_box_test", "hrt_scene_set_options", "hrt_scene_get_options",
            "hrt_debug_sample_chunks", "hrt_scene_set_view",
            "hrt_accum_create", "hrt_accum_destroy", "hrt_accum_reset", "hrt_accum_add", "hrt_accum_add_resolve",
            "hrt_accum_samples", "hrt_accum_resolve", "hrt_accum_resolve_host", "hrt_accum_merge", "hrt_accum_download",
            "hrt_accum_upload", "hrt_debug_accumulate", "hrt_debug_walk_regroup",
            "hrt_accum_create_ex", "hrt_accum_add_tiles", "hrt_accum_noise", "hrt_accum_tile_samples", "hrt_debug_noise",
            "hrt_debug_accum_moments",
            "hrt_accum_resolve_filtered", "hrt_accum_resolve_filtered_host", "hrt_debug_filter",
        "hrt_accum_add_features", "hrt_accum_feature_samples", "hrt_accum_features", "hrt_accum_features_host",
            "hrt_accum_resolve_guided", "hrt_accum_resolve_guided_host", "hrt_debug_guided", "hrt_debug_accum_features",
            "hrt_accum_snapshot", "hrt_accum_restore", "hrt_accum_snapshot_info", "hrt_accum_merge_tiles",
            "hrt_accum_resolve_guided_ex", "hrt_accum_resolve_guided_ex_host", "hrt_debug_guided_ex",
            "hrt_accum_noise_filtered", "hrt_debug_noise_filtered",
            "hrt_scene_intersect", "hrt_scene_intersect_host", "hrt_camera_rays", "hrt_camera_rays_host",
            "hrt_scene_scatter", "hrt_scene_scatter_host", "hrt_camera_paths", "hrt_camera_paths_host",
            "hrt_scene_step", "hrt_scene_step_host",
            "hrt_accum_add_paths", "hrt_accum_add_paths_host", "hrt_debug_accum_paths"}
HRT_LIB_OVERRIDE = bool(os.environ.get("HRT_LIB"))

# Every entry point of include/hrt/hrt.h (tests/test_abi.py checks the header against this list).
EXPORTS = [
    "hrt_last_error", "hrt_version", "hrt_abi_version", "hrt_scene_create", "hrt_scene_destroy",
    "hrt_tex_solid", "hrt_tex_checker", "hrt_tex_noise", "hrt_tex_image",
    "hrt_mat_lambertian", "hrt_mat_metal", "hrt_mat_dielectric", "hrt_mat_diffuse_light", "hrt_mat_isotropic",
    "hrt_node_sphere", "hrt_node_moving_sphere", "hrt_node_rect", "hrt_node_cuboid", "hrt_node_translate",
    "hrt_node_rotate", "hrt_node_constant_medium", "hrt_node_list", "hrt_node_bvh", "hrt_node_count",
    "hrt_node_bounding_box", "hrt_scene_set_root", "hrt_scene_commit", "hrt_preset_build", "hrt_camera_init",
    "hrt_render_tiles_device", "hrt_render_device", "hrt_render", "hrt_tile_grid", "hrt_scene_get_info", "hrt_last_launch", "hrt_debug_box_test",
    "hrt_debug_device_math", "hrt_debug_trace_path", "hrt_debug_scene_blob", "hrt_image_write", "hrt_render_progressive", "hrt_debug_prim_record",
    "hrt_scene_synchronize", "hrt_debug_poke_blob", "hrt_scene_set_options", "hrt_scene_get_options",
    "hrt_debug_sample_chunks", "hrt_scene_set_view",
    "hrt_accum_create", "hrt_accum_destroy", "hrt_accum_reset", "hrt_accum_add", "hrt_accum_add_resolve", "hrt_accum_samples",
    "hrt_accum_resolve", "hrt_accum_resolve_host", "hrt_accum_merge", "hrt_accum_download", "hrt_accum_upload",
    "hrt_debug_accumulate", "hrt_debug_walk_regroup",
    "hrt_accum_create_ex", "hrt_accum_add_tiles", "hrt_accum_noise", "hrt_accum_tile_samples", "hrt_debug_noise",
    "hrt_debug_accum_moments",
    "hrt_accum_resolve_filtered", "hrt_accum_resolve_filtered_host", "hrt_debug_filter",
    "hrt_accum_add_features", "hrt_accum_feature_samples", "hrt_accum_features", "hrt_accum_features_host",
    "hrt_accum_resolve_guided", "hrt_accum_resolve_guided_host", "hrt_debug_guided", "hrt_debug_accum_features",
    "hrt_accum_snapshot", "hrt_accum_restore", "hrt_accum_snapshot_info", "hrt_accum_merge_tiles",
    "hrt_accum_resolve_guided_ex", "hrt_accum_resolve_guided_ex_host", "hrt_debug_guided_ex",
    "hrt_accum_noise_filtered", "hrt_debug_noise_filtered",
    "hrt_scene_intersect", "hrt_scene_intersect_host", "hrt_camera_rays", "hrt_camera_rays_host",
    "hrt_scene_scatter", "hrt_scene_scatter_host", "hrt_camera_paths", "hrt_camera_paths_host",
    "hrt_scene_step", "hrt_scene_step_host",
    "hrt_accum_add_paths", "hrt_accum_add_paths_host", "hrt_debug_accum_paths",
]

ABI_VERSION = 6  # include/hrt/hrt.h HRT_ABI_VERSION: the struct layouts below
_lib = None
_U32P = ctypes.POINTER(ctypes.c_uint32)
_F3 = ctypes.c_float * 3


def load(path: str = LIB_PATH) -> ctypes.CDLL:
    """Load libhrt.so (raises if it has not been built: there is no fallback path)."""
    global _lib
    if _lib is not None:
        return _lib
    # torch ships its own libamdhip64 (same soname libamdhip64.so.7 as /opt/rocm's).  Loading torch
    # first makes libhrt bind to that already-loaded runtime: ONE HIP runtime per process, so torch
    # device pointers and hipStream_t handles are valid in libhrt.  (Loaded the other way round,
    # torch would map a second runtime by file name and fail to find the device.)
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    if not os.path.exists(path):
        raise FileNotFoundError(f"{path} missing: build it with `make -C hyper-ray-tracer_amd` (or __graft_entry__.build())")
    L = ctypes.CDLL(path)
    S = ctypes.c_int32
    vp = ctypes.c_void_p
    f, u32, i32, u64 = ctypes.c_float, ctypes.c_uint32, ctypes.c_int32, ctypes.c_uint64
    sig = {
        "hrt_last_error": (ctypes.c_char_p, []),
        "hrt_version": (ctypes.c_char_p, []),
        "hrt_abi_version": (ctypes.c_uint32, []),
        "hrt_scene_create": (S, [ctypes.POINTER(vp)]),
        "hrt_scene_destroy": (None, [vp]),
        "hrt_tex_solid": (S, [vp, f, f, f, _U32P]),
        "hrt_tex_checker": (S, [vp, u32, u32, _U32P]),
        "hrt_tex_noise": (S, [vp, f, vp, vp, _U32P]),
        "hrt_tex_image": (S, [vp, vp, u32, u32, u32, _U32P]),
        "hrt_mat_lambertian": (S, [vp, u32, _U32P]),
        "hrt_mat_metal": (S, [vp, f, f, f, f, _U32P]),
        "hrt_mat_dielectric": (S, [vp, f, _U32P]),
        "hrt_mat_diffuse_light": (S, [vp, u32, _U32P]),
        "hrt_mat_isotropic": (S, [vp, u32, _U32P]),
        "hrt_node_sphere": (S, [vp, _F3, f, u32, _U32P]),
        "hrt_node_moving_sphere": (S, [vp, _F3, _F3, f, f, f, u32, _U32P]),
        "hrt_node_rect": (S, [vp, i32, f, f, f, f, f, u32, _U32P]),
        "hrt_node_cuboid": (S, [vp, _F3, _F3, u32, _U32P]),
        "hrt_node_translate": (S, [vp, u32, _F3, _U32P]),
        "hrt_node_rotate": (S, [vp, i32, u32, f, _U32P]),
        "hrt_node_constant_medium": (S, [vp, u32, f, u32, _U32P]),
        "hrt_node_list": (S, [vp, vp, u32, _U32P]),
        "hrt_node_bvh": (S, [vp, vp, u32, f, f, _U32P]),
        "hrt_node_count": (S, [vp, u32, _U32P]),
        "hrt_node_bounding_box": (S, [vp, u32, f, f, ctypes.POINTER(i32), _F3, _F3]),
        "hrt_scene_set_root": (S, [vp, u32]),
        "hrt_scene_commit": (S, [vp, i32]),
        "hrt_preset_build": (S, [vp, i32, u64, vp, u32, u32, u32, ctypes.POINTER(PresetInfo)]),
        "hrt_camera_init": (S, [ctypes.POINTER(Camera), _F3, _F3, f, f, f, f, f, i32, i32]),
        "hrt_render_tiles_device": (S, [vp, ctypes.POINTER(Camera), ctypes.POINTER(RenderParams), vp, u32, vp, vp, ctypes.POINTER(RenderStats)]),
        "hrt_render_device": (S, [vp, ctypes.POINTER(Camera), ctypes.POINTER(RenderParams), u32, u32, u32, u32, vp, vp, ctypes.POINTER(RenderStats)]),
        "hrt_render": (S, [vp, ctypes.POINTER(Camera), ctypes.POINTER(RenderParams), u32, u32, u32, u32, vp, ctypes.POINTER(RenderStats)]),
        "hrt_tile_grid": (S, [u32, u32, u32, u32, u32, vp, u32, _U32P]),
        "hrt_scene_get_info": (S, [vp, ctypes.POINTER(SceneInfo)]),
        "hrt_last_launch": (S, [ctypes.POINTER(LaunchInfo)]),
        "hrt_debug_box_test": (S, [ctypes.c_int32, ctypes.c_int32, vp, ctypes.c_uint32, vp, ctypes.c_uint32, ctypes.c_float,
                                   ctypes.c_float, vp]),
        "hrt_debug_device_math": (S, [i32, vp, vp, vp, u32]),
        "hrt_debug_scene_blob": (S, [vp, vp, ctypes.c_uint64, ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(BlobInfo)]),
        "hrt_debug_prim_record": (S, [vp, i32, u32, vp]),
        "hrt_image_write": (S, [ctypes.c_char_p, vp, u32, u32, i32]),
        "hrt_render_progressive": (S, [vp, ctypes.POINTER(Camera), ctypes.POINTER(RenderParams), u32, u32, u32, u32,
                                       TILE_FN, vp, ctypes.POINTER(RenderStats)]),
        "hrt_debug_trace_path": (S, [vp, ctypes.POINTER(Camera), ctypes.POINTER(RenderParams), u32, u32, u32, u32, vp, _U32P]),
        "hrt_scene_synchronize": (S, [vp]),
        "hrt_debug_poke_blob": (S, [vp, u64, vp, u64]),
        "hrt_scene_set_options": (S, [vp, ctypes.POINTER(SceneOptions)]),
        "hrt_scene_get_options": (S, [vp, ctypes.POINTER(SceneOptions)]),
        "hrt_scene_set_view": (S, [vp, ctypes.POINTER(Camera)]),
        "hrt_debug_sample_chunks": (S, [vp, ctypes.POINTER(RenderParams), _U32P]),
        "hrt_accum_create": (S, [vp, u32, u32, vp, u32, ctypes.POINTER(vp)]),
        "hrt_accum_destroy": (None, [vp]),
        "hrt_accum_reset": (S, [vp, vp]),
        "hrt_accum_add": (S, [vp, ctypes.POINTER(Camera), ctypes.POINTER(RenderParams), vp, ctypes.POINTER(RenderStats)]),
        "hrt_accum_add_resolve": (S, [vp, ctypes.POINTER(Camera), ctypes.POINTER(RenderParams), i32, vp, vp,
                                      ctypes.POINTER(RenderStats)]),
        "hrt_accum_samples": (S, [vp, ctypes.POINTER(u64)]),
        "hrt_accum_resolve": (S, [vp, i32, vp, vp]),
        "hrt_accum_resolve_host": (S, [vp, i32, vp]),
        "hrt_accum_merge": (S, [vp, vp, vp]),
        "hrt_accum_download": (S, [vp, vp, vp, u32, _U32P]),
        "hrt_accum_upload": (S, [vp, ctypes.POINTER(Camera), ctypes.POINTER(RenderParams), vp, vp, u32]),
        "hrt_debug_accumulate": (S, [i32, vp, u32, u32, vp, u64, i32, vp]),
        "hrt_debug_walk_regroup": (S, [i32, vp, u32, u32, vp, vp, vp, vp]),
        "hrt_accum_create_ex": (S, [vp, u32, u32, vp, u32, u32, ctypes.POINTER(vp)]),
        "hrt_accum_add_tiles": (S, [vp, ctypes.POINTER(Camera), ctypes.POINTER(RenderParams), vp, u32, vp,
                                    ctypes.POINTER(RenderStats)]),
        "hrt_accum_noise": (S, [vp, f, vp, vp, vp]),
        "hrt_accum_tile_samples": (S, [vp, vp]),
        "hrt_debug_noise": (S, [i32, vp, vp, u32, u32, vp, vp, u64, u64, f, vp, vp]),
        "hrt_debug_accum_moments": (S, [vp, vp]),
        "hrt_accum_resolve_filtered": (S, [vp, ctypes.POINTER(FilterParams), i32, vp, vp]),
        "hrt_accum_resolve_filtered_host": (S, [vp, ctypes.POINTER(FilterParams), i32, vp]),
        "hrt_debug_filter": (S, [i32, vp, u32, u32, u32, f, vp]),
        "hrt_accum_add_features": (S, [vp, ctypes.POINTER(Camera), ctypes.POINTER(RenderParams), vp]),
        "hrt_accum_feature_samples": (S, [vp, ctypes.POINTER(u64)]),
        "hrt_accum_features": (S, [vp, vp, vp, vp]),
        "hrt_accum_features_host": (S, [vp, vp, vp]),
        "hrt_accum_resolve_guided": (S, [vp, ctypes.POINTER(GuidedParams), i32, vp, vp]),
        "hrt_accum_resolve_guided_host": (S, [vp, ctypes.POINTER(GuidedParams), i32, vp]),
        "hrt_debug_guided": (S, [i32, vp, vp, vp, u32, u32, u32, f, f, f, f, vp]),
        "hrt_debug_accum_features": (S, [vp, vp, vp]),
        "hrt_accum_snapshot": (S, [vp, vp, u64, ctypes.POINTER(u64)]),
        "hrt_accum_restore": (S, [vp, vp, u64]),
        "hrt_accum_snapshot_info": (S, [vp, u64, ctypes.POINTER(SnapshotInfo), vp, u32]),
        "hrt_accum_merge_tiles": (S, [vp, vp, vp]),
        "hrt_accum_resolve_guided_ex": (S, [vp, ctypes.POINTER(GuidedExParams), i32, vp, vp]),
        "hrt_accum_resolve_guided_ex_host": (S, [vp, ctypes.POINTER(GuidedExParams), i32, vp]),
        "hrt_debug_guided_ex": (S, [i32, vp, vp, vp, u32, u32, u32, f, f, f, f, u32, f, vp]),
        "hrt_accum_noise_filtered": (S, [vp, ctypes.POINTER(GuidedExParams), f, vp, vp, vp]),
        "hrt_debug_noise_filtered": (S, [i32, vp, vp, vp, u32, u32, u32, f, f, f, f, u32, f, f, vp, u32, vp, vp]),
        "hrt_scene_intersect": (S, [vp, ctypes.POINTER(QueryParams), vp, u64, vp, vp]),
        "hrt_scene_intersect_host": (S, [vp, ctypes.POINTER(QueryParams), vp, u64, vp]),
        "hrt_camera_rays": (S, [vp, ctypes.POINTER(Camera), ctypes.POINTER(RenderParams), vp, u32, vp, vp]),
        "hrt_camera_rays_host": (S, [vp, ctypes.POINTER(Camera), ctypes.POINTER(RenderParams), vp, u32, vp]),
        "hrt_scene_scatter": (S, [vp, ctypes.POINTER(ScatterParams), vp, vp, vp, u64, vp]),
        "hrt_scene_scatter_host": (S, [vp, ctypes.POINTER(ScatterParams), vp, vp, vp, u64]),
        "hrt_camera_paths": (S, [vp, ctypes.POINTER(Camera), ctypes.POINTER(RenderParams), vp, u32, vp, vp, vp]),
        "hrt_camera_paths_host": (S, [vp, ctypes.POINTER(Camera), ctypes.POINTER(RenderParams), vp, u32, vp, vp]),
        "hrt_scene_step": (S, [vp, ctypes.POINTER(StepParams), vp, vp, u64, vp, ctypes.POINTER(PathList), ctypes.POINTER(PathList), vp, vp]),
        "hrt_scene_step_host": (S, [vp, ctypes.POINTER(StepParams), vp, vp, u64, vp, ctypes.POINTER(u64)]),
        "hrt_accum_add_paths": (S, [vp, ctypes.POINTER(Camera), ctypes.POINTER(RenderParams), vp, u32, vp, u64, i32, vp, vp, vp]),
        "hrt_accum_add_paths_host": (S, [vp, ctypes.POINTER(Camera), ctypes.POINTER(RenderParams), vp, u32, vp, u64, _U32P]),
        "hrt_debug_accum_paths": (S, [i32, vp, u32, u32, vp, vp, vp, u64, i32, vp, _U32P]),
    }
    for name, (res, args) in sig.items():
        if name in OPTIONAL and HRT_LIB_OVERRIDE and not hasattr(L, name):
            continue  # an older build loaded for an A/B run (HRT_LIB): diagnostics it lacks stay unbound
        fn = getattr(L, name)
        fn.restype = res
        fn.argtypes = args
    if hasattr(L, "hrt_abi_version") and L.hrt_abi_version() != ABI_VERSION and not HRT_LIB_OVERRIDE:
        raise RuntimeError(f"{path}: ABI version {L.hrt_abi_version()}, this binding is written for {ABI_VERSION} "
                           "(include/hrt/hrt.h HRT_ABI_VERSION): rebuild the library")
    _lib = L
    return L


def _check(st: int) -> None:
    if st != OK:
        raise HrtError(st, load().hrt_last_error().decode())


def f3(v: Sequence[float]):
    return _F3(*[float(x) for x in v])


# ---------------------------------------------------------------------------------------- scene
class Scene:
    """A hrt_scene handle: constructors mirror the reference's Hittable/Material/Texture types."""

    def __init__(self):
        L = load()
        h = ctypes.c_void_p()
        _check(L.hrt_scene_create(ctypes.byref(h)))
        self.h = h
        self.info: Optional[PresetInfo] = None
        self.device = -1
        self._keep: list = []

    def close(self):
        if self.h:
            load().hrt_scene_destroy(self.h)
            self.h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _id(self, fn, *args) -> int:
        out = ctypes.c_uint32()
        _check(fn(self.h, *args, ctypes.byref(out)))
        return out.value

    # textures
    def solid(self, r, g, b):
        return self._id(load().hrt_tex_solid, r, g, b)

    def checker(self, odd, even):
        return self._id(load().hrt_tex_checker, odd, even)

    def noise(self, scale, ranvec, perm):
        rv = np.ascontiguousarray(ranvec, np.float32).reshape(-1)
        pm = np.ascontiguousarray(perm, np.uint32).reshape(-1)
        assert rv.size == 768 and pm.size == 768
        return self._id(load().hrt_tex_noise, scale, rv.ctypes.data, pm.ctypes.data)

    def image(self, data: Optional[np.ndarray]):
        if data is None:
            return self._id(load().hrt_tex_image, None, 0, 0, 0)
        d = np.ascontiguousarray(data, np.uint8)
        h, w, c = d.shape
        return self._id(load().hrt_tex_image, d.ctypes.data, w, h, c)

    # materials
    def lambertian(self, tex):
        return self._id(load().hrt_mat_lambertian, tex)

    def metal(self, albedo, fuzz):
        return self._id(load().hrt_mat_metal, *[float(a) for a in albedo], fuzz)

    def dielectric(self, ior):
        return self._id(load().hrt_mat_dielectric, ior)

    def diffuse_light(self, tex):
        return self._id(load().hrt_mat_diffuse_light, tex)

    def isotropic(self, tex):
        return self._id(load().hrt_mat_isotropic, tex)

    # hittables
    def sphere(self, center, radius, mat):
        return self._id(load().hrt_node_sphere, f3(center), radius, mat)

    def moving_sphere(self, c0, c1, t0, t1, radius, mat):
        return self._id(load().hrt_node_moving_sphere, f3(c0), f3(c1), t0, t1, radius, mat)

    def rect(self, plane, a0, a1, b0, b1, k, mat):
        return self._id(load().hrt_node_rect, plane, a0, a1, b0, b1, k, mat)

    def cuboid(self, p0, p1, mat):
        return self._id(load().hrt_node_cuboid, f3(p0), f3(p1), mat)

    def translate(self, child, d):
        return self._id(load().hrt_node_translate, child, f3(d))

    def rotate(self, axis, child, angle):
        return self._id(load().hrt_node_rotate, axis, child, angle)

    def constant_medium(self, boundary, density, tex):
        return self._id(load().hrt_node_constant_medium, boundary, density, tex)

    def list(self, children: Sequence[int]):
        arr = (ctypes.c_uint32 * max(1, len(children)))(*children)
        return self._id(load().hrt_node_list, ctypes.cast(arr, ctypes.c_void_p), len(children))

    def bvh(self, children: Sequence[int], t0=0.0, t1=1.0):
        arr = (ctypes.c_uint32 * max(1, len(children)))(*children)
        return self._id(load().hrt_node_bvh, ctypes.cast(arr, ctypes.c_void_p), len(children), t0, t1)

    def count(self, node) -> int:
        out = ctypes.c_uint32()
        _check(load().hrt_node_count(self.h, node, ctypes.byref(out)))
        return out.value

    def bounding_box(self, node, t0=0.0, t1=1.0):
        has = ctypes.c_int32()
        mn, mx = _F3(), _F3()
        _check(load().hrt_node_bounding_box(self.h, node, t0, t1, ctypes.byref(has), mn, mx))
        return (tuple(mn), tuple(mx)) if has.value else None

    def set_options(self, **kw):
        """hrt_scene_set_options: bvh_ties (0 stable / 1 reversed), walk_tree (0 re-grouped / 1 the reference tree),
        chunk_min, chunk_max, chunk_uniform (sample chunks); unnamed fields keep their current values."""
        o = self.options()
        for k, v in kw.items():
            if k not in dict(SceneOptions._fields_):
                raise TypeError(f"unknown scene option {k!r}")
            setattr(o, k, int(v))
        _check(load().hrt_scene_set_options(self.h, ctypes.byref(o)))

    def set_view(self, cam: Optional["Camera"]):
        """hrt_scene_set_view: the camera most renders will use (None: no hint).  Placement only: which node parts
        of a walk stream too large for LDS are staged there; the image is the same bit for bit."""
        if cam is not None:
            self._keep.append(cam)
        _check(load().hrt_scene_set_view(self.h, ctypes.byref(cam) if cam is not None else None))

    def options(self) -> SceneOptions:
        o = SceneOptions()
        _check(load().hrt_scene_get_options(self.h, ctypes.byref(o)))
        return o

    def set_root(self, node):
        _check(load().hrt_scene_set_root(self.h, node))

    def commit(self, device: int = -1):
        _check(load().hrt_scene_commit(self.h, device))
        self.device = device  # -1: the device that was current at the commit

    def synchronize(self):
        """Wait for every render launched on this scene; raises HrtError(ERR_STATE) if one of them
        was stopped by the walk watchdog (hrt_scene_synchronize)."""
        _check(load().hrt_scene_synchronize(self.h))

    def poke_blob(self, offset: int, data: bytes):
        """Fault injection: overwrite bytes of the committed device blob (hrt_debug_poke_blob)."""
        buf = ctypes.create_string_buffer(bytes(data), len(data))
        _check(load().hrt_debug_poke_blob(self.h, offset, buf, len(data)))

    def intersect(self, rays, flags: int = 0, seed: int = 0, shutter=(0.0, 1.0), out=None, stream: int = 0):
        """The closest hit of every ray (hrt_scene_intersect).  A numpy array of RAY_DTYPE goes through the host variant
        and returns an array of HIT_DTYPE; a CUDA torch tensor (n x 12 float32 words, or n x 48 bytes) goes through the
        device variant on `stream` and returns an (n, 12) float32 tensor of hit records (view it as int32 for the ids).
        shutter: the interval the rays' times lie in; seed: the key of the media's draws (with each ray's pixel, sample
        and segment)."""
        q = query_params(flags, seed, shutter)
        if isinstance(rays, np.ndarray):
            rays = np.ascontiguousarray(rays, RAY_DTYPE)
            hits = np.empty(rays.shape, HIT_DTYPE) if out is None else out
            if hits.dtype != HIT_DTYPE or hits.shape != rays.shape or not hits.flags.c_contiguous:
                raise ValueError("out: a contiguous HIT_DTYPE array of the rays' shape")
            _check(load().hrt_scene_intersect_host(self.h, ctypes.byref(q), rays.ctypes.data, rays.size, hits.ctypes.data))
            return hits
        import torch

        if not (isinstance(rays, torch.Tensor) and rays.is_cuda and rays.is_contiguous() and
                rays.numel() * rays.element_size() % 48 == 0):
            raise ValueError("rays: a numpy RAY_DTYPE array or a contiguous CUDA tensor of 48-byte records")
        n = rays.numel() * rays.element_size() // 48
        hits = torch.empty((n, 12), dtype=torch.float32, device=rays.device) if out is None else out
        if not (hits.is_cuda and hits.is_contiguous() and hits.numel() * hits.element_size() == 48 * n):
            raise ValueError("out: a contiguous CUDA tensor of n 48-byte records")
        _check(load().hrt_scene_intersect(self.h, ctypes.byref(q), rays.data_ptr(), n, hits.data_ptr(), stream or None))
        return hits

    def scatter(self, rays, hits, paths, background, stream: int = 0):
        """One scatter step of every path that is not DONE (hrt_scene_scatter): the miss's background or the hit's
        emission, scatter and texture, drawn from the path's own stream.  numpy arrays (RAY_DTYPE, HIT_DTYPE, PATH_DTYPE)
        go through the host variant and NEW (rays, paths) arrays come back; contiguous CUDA tensors of 48-byte records go
        through the device variant on `stream`, which updates rays and paths IN PLACE and returns them."""
        sp = scatter_params(background)
        if isinstance(rays, np.ndarray):
            rays, paths = np.array(rays, RAY_DTYPE, order="C"), np.array(paths, PATH_DTYPE, order="C")  # copies
            hits = np.ascontiguousarray(hits, HIT_DTYPE)
            if not (rays.shape == hits.shape == paths.shape):
                raise ValueError("rays, hits and paths: arrays of one shape")
            _check(load().hrt_scene_scatter_host(self.h, ctypes.byref(sp), rays.ctypes.data, hits.ctypes.data, paths.ctypes.data,
                                                 rays.size))
            return rays, paths
        import torch

        def records(t):
            ok = isinstance(t, torch.Tensor) and t.is_cuda and t.is_contiguous() and t.numel() * t.element_size() % 48 == 0
            return t.numel() * t.element_size() // 48 if ok else -1

        n = records(rays)
        if n < 0 or records(hits) != n or records(paths) != n:
            raise ValueError("rays, hits, paths: numpy record arrays, or contiguous CUDA tensors of n 48-byte records each")
        _check(load().hrt_scene_scatter(self.h, ctypes.byref(sp), rays.data_ptr(), hits.data_ptr(), paths.data_ptr(), n, stream or None))
        return rays, paths

    def step(self, rays, paths, *, steps: int = 1, seed: int = 0, shutter=(0.0, 1.0), background=(0.0, 0.0, 0.0), flags: int = 0,
             hits=None, live=None, live_out=None, n_rays=None, stream: int = 0):
        """`steps` rounds of intersect and scatter for every path of the domain that is not DONE, fused, with no hit
        records in between (hrt_scene_step).  numpy arrays (RAY_DTYPE, PATH_DTYPE) go through the host variant and NEW
        (rays, paths) arrays come back; `hits` (a HIT_DTYPE array) and `n_rays` (a one-element uint64 / int64 array, added
        to) are then filled in place.  Contiguous CUDA tensors of 48-byte records go through the device variant on
        `stream`, which updates rays and paths IN PLACE and returns them; hits: a tensor of n hit records to fill (the last
        intersect's hit of each stepped path); live: the domain as an (index tensor int32, count tensor int32[1]) pair
        (default: every path); live_out: such a pair that takes the paths still live, the next call's `live`; n_rays: an
        int64 tensor of one element the call adds the rays it walked to."""
        sp = step_params(steps, seed, shutter, background, flags)
        L = load()
        if isinstance(rays, np.ndarray):
            if live is not None or live_out is not None:
                raise ValueError("live lists are device memory: use CUDA tensors")
            rays, paths = np.array(rays, RAY_DTYPE, order="C"), np.array(paths, PATH_DTYPE, order="C")  # copies
            if rays.shape != paths.shape:
                raise ValueError("rays and paths: arrays of one shape")
            if hits is not None and (hits.dtype != HIT_DTYPE or hits.shape != rays.shape or not hits.flags.c_contiguous):
                raise ValueError("hits: a contiguous HIT_DTYPE array of the rays' shape")
            count = ctypes.c_uint64(0)
            _check(L.hrt_scene_step_host(self.h, ctypes.byref(sp), rays.ctypes.data, paths.ctypes.data, rays.size,
                                         None if hits is None else hits.ctypes.data, None if n_rays is None else ctypes.byref(count)))
            if n_rays is not None:
                n_rays[0] += count.value
            return rays, paths
        import torch

        def records(t):
            ok = isinstance(t, torch.Tensor) and t.is_cuda and t.is_contiguous() and t.numel() * t.element_size() % 48 == 0
            return t.numel() * t.element_size() // 48 if ok else -1

        def path_list(pair, what):
            if pair is None:
                return None
            index, count = pair
            for t in (index, count):
                if not (isinstance(t, torch.Tensor) and t.is_cuda and t.is_contiguous() and t.dtype == torch.int32):
                    raise ValueError(what + ": an (index, count) pair of contiguous int32 CUDA tensors")
            if count.numel() != 1:
                raise ValueError(what + ": the count is one int32")
            return PathList(index.data_ptr(), count.data_ptr(), index.numel(), 0)

        n = records(rays)
        if n < 0 or records(paths) != n or (hits is not None and records(hits) != n):
            raise ValueError("rays, paths (and hits): numpy record arrays, or contiguous CUDA tensors of n 48-byte records each")
        if n_rays is not None and not (isinstance(n_rays, torch.Tensor) and n_rays.is_cuda and n_rays.dtype == torch.int64 and
                                       n_rays.numel() == 1):
            raise ValueError("n_rays: an int64 CUDA tensor of one element")
        lin, lout = path_list(live, "live"), path_list(live_out, "live_out")
        _check(L.hrt_scene_step(self.h, ctypes.byref(sp), rays.data_ptr(), paths.data_ptr(), n, None if hits is None else hits.data_ptr(),
                                None if lin is None else ctypes.byref(lin), None if lout is None else ctypes.byref(lout),
                                None if n_rays is None else n_rays.data_ptr(), stream or None))
        return rays, paths

    def scene_info(self) -> SceneInfo:
        si = SceneInfo()
        _check(load().hrt_scene_get_info(self.h, ctypes.byref(si)))
        return si


def synthetic_earth(width: int = 1024, height: int = 512) -> np.ndarray:
    """Deterministic stand-in for assets/earthmap.jpg (same shape, RGB8): the asset is not shipped,
    so Earth-textured scenes use this image on both sides of every parity test."""
    y, x = np.mgrid[0:height, 0:width].astype(np.float64)
    lon = x / width * 2 * np.pi
    lat = (y / height - 0.5) * np.pi
    land = (np.sin(3 * lon) * np.cos(2 * lat) + 0.5 * np.sin(7 * lon + 1.3) * np.sin(5 * lat)) > 0.2
    r = np.where(land, 90 + 60 * np.cos(lat), 20)
    g = np.where(land, 120 + 50 * np.sin(2 * lon) ** 2, 60 + 40 * np.cos(lat))
    b = np.where(land, 50, 140 + 80 * np.cos(lat))
    ice = np.abs(lat) > 1.25
    img = np.stack([np.where(ice, 240, r), np.where(ice, 245, g), np.where(ice, 250, b)], -1)
    return np.clip(img, 0, 255).astype(np.uint8)


def load_image(path: str) -> np.ndarray:
    """Decode an image file to the bytes hrt_tex_image takes (H x W x C uint8), as ImageTexture::new
    does with `image::open` (image_texture.rs:19-33).  Decoding is host plumbing (Pillow here; the
    Rust host keeps `image`): the ABI itself takes decoded bytes."""
    from PIL import Image

    im = Image.open(path)
    if im.mode not in ("L", "LA", "RGB", "RGBA"):
        im = im.convert("RGB")
    a = np.asarray(im, dtype=np.uint8)
    return np.ascontiguousarray(a[..., None] if a.ndim == 2 else a)


def preset(name_or_id, scene_seed: int = 1, image: Optional[np.ndarray] = None, options: Optional[dict] = None) -> Scene:
    """Build one of the reference scenes (application.rs:497-935) with a seeded builder stream; `options` are
    hrt_scene_options fields, set before the builder runs (bvh_ties applies to its BvhNode::new calls)."""
    pid = PRESETS[name_or_id] if isinstance(name_or_id, str) else int(name_or_id)
    img = synthetic_earth() if image is None else np.ascontiguousarray(image, np.uint8)
    s = Scene()
    if options:
        s.set_options(**options)
    info = PresetInfo()
    h, w, c = img.shape
    _check(load().hrt_preset_build(s.h, pid, scene_seed, img.ctypes.data, w, h, c, ctypes.byref(info)))
    s.info = info
    s._keep.append(img)
    return s


def camera(look_from, look_at, fov, aperture, focus_dist, time0, time1, width, height) -> Camera:
    cam = Camera()
    _check(load().hrt_camera_init(ctypes.byref(cam), f3(look_from), f3(look_at), fov, aperture, focus_dist, time0, time1, width, height))
    return cam


def preset_camera(info: PresetInfo, width: int, height: int) -> Camera:
    return camera(info.look_from, info.look_at, info.fov, info.aperture, info.focus_dist, info.time0, info.time1, width, height)


RENDER_COUNT_WORK = 1
RENDER_NO_LDS = 2
RENDER_REFERENCE_CULL = 8
RENDER_FAST_CULL = 16
RENDER_SAH = 32


def params(width, height, samples, max_depth=50, seed=1, background=(0.7, 0.8, 1.0), t_min=0.001, sample_offset=0, flags=0) -> RenderParams:
    p = RenderParams()
    p.width, p.height, p.samples, p.max_depth = width, height, samples, max_depth
    p.sample_offset, p.flags, p.t_min, p.seed = sample_offset, flags, t_min, seed
    for i in range(3):
        p.background[i] = float(background[i])
    return p


def query_params(flags: int = 0, seed: int = 0, shutter=(0.0, 1.0)) -> QueryParams:
    """hrt_query_params: QUERY_* flags, the seed of the media's draws, the interval the rays' times lie in."""
    return QueryParams(flags, 0, float(shutter[0]), float(shutter[1]), seed)


def camera_rays(scene: "Scene", cam: Camera, p: RenderParams, tiles=None, device: bool = False, stream: int = 0):
    """The camera rays of samples [p.sample_offset, + p.samples) of every pixel of `tiles` (default: the frame as one
    tile), ray (packed pixel) * p.samples + k (hrt_camera_rays): a RAY_DTYPE array, or with device=True an (n, 12)
    float32 CUDA tensor on the current torch device (which must be the scene's)."""
    tiles = [(0, 0, p.width, p.height)] if tiles is None else list(tiles)
    arr = (Tile * len(tiles))(*[Tile(*t) for t in tiles])
    n = sum(t[2] * t[3] for t in tiles) * p.samples
    if not device:
        rays = np.empty(n, RAY_DTYPE)
        _check(load().hrt_camera_rays_host(scene.h, ctypes.byref(cam), ctypes.byref(p), arr, len(tiles), rays.ctypes.data))
        return rays
    import torch

    rays = torch.empty((n, 12), dtype=torch.float32, device="cuda")
    _check(load().hrt_camera_rays(scene.h, ctypes.byref(cam), ctypes.byref(p), arr, len(tiles), rays.data_ptr(), stream or None))
    return rays


def scatter_params(background, flags: int = 0) -> ScatterParams:
    """hrt_scatter_params: the background a miss gathers (a render's p.background); no flag is defined yet."""
    return ScatterParams(flags, 0, _F3(*[float(x) for x in background]), 0)


def camera_paths(scene: "Scene", cam: Camera, p: RenderParams, tiles=None, device: bool = False, stream: int = 0):
    """hrt.camera_rays' rays and, for each, the path a render's sample starts with (hrt_camera_paths): (rays, paths) as
    RAY_DTYPE and PATH_DTYPE arrays, or with device=True as two (n, 12) float32 CUDA tensors (view the paths as int32 for
    rng, depth_left and flags: words 0..3, 7 and 11)."""
    tiles = [(0, 0, p.width, p.height)] if tiles is None else list(tiles)
    arr = (Tile * len(tiles))(*[Tile(*t) for t in tiles])
    n = sum(t[2] * t[3] for t in tiles) * p.samples
    if not device:
        rays, paths = np.empty(n, RAY_DTYPE), np.empty(n, PATH_DTYPE)
        _check(load().hrt_camera_paths_host(scene.h, ctypes.byref(cam), ctypes.byref(p), arr, len(tiles), rays.ctypes.data,
                                            paths.ctypes.data))
        return rays, paths
    import torch

    rays = torch.empty((n, 12), dtype=torch.float32, device="cuda")
    paths = torch.empty((n, 12), dtype=torch.float32, device="cuda")
    _check(load().hrt_camera_paths(scene.h, ctypes.byref(cam), ctypes.byref(p), arr, len(tiles), rays.data_ptr(), paths.data_ptr(),
                                   stream or None))
    return rays, paths


def trace_paths(scene: "Scene", cam: Camera, p: RenderParams, tiles=None, device: bool = False):
    """Your own integrator in a dozen lines: the render's paths through the query calls, on the device.  Camera paths,
    then intersect and scatter in turn until every path is DONE (at most p.max_depth rounds).  Returns the per-sample
    radiance (n, 3) float32, path (packed pixel) * p.samples + k, bit for bit what hrt.render gathers for sample
    p.sample_offset + k of that pixel, and the number of rays traced, which is the render's RenderStats.segments.
    device=True: the finished paths stay on the device, an (n, 12) float32 CUDA tensor of hrt_path records (radiance:
    columns 8..10), instead of the downloaded radiance."""
    import torch

    rays, paths = camera_paths(scene, cam, p, tiles, device=True)
    path_flags = paths.view(torch.int32)[:, 11]
    hits = torch.empty_like(rays)
    hit_flags = hits.view(torch.int32)[:, 3]
    n_rays = 0
    for _ in range(p.max_depth):
        if not bool((path_flags & PATH_DONE == 0).any()):
            break
        scene.intersect(rays, seed=p.seed, shutter=(cam.time0, cam.time1), out=hits)
        n_rays += int((hit_flags & HIT_INVALID == 0).sum())  # a finished path's ray is invalid and was not traced
        scene.scatter(rays, hits, paths, tuple(p.background))
    return (paths if device else paths[:, 8:11].cpu().numpy()), n_rays


def step_params(steps: int = 1, seed: int = 0, shutter=(0.0, 1.0), background=(0.0, 0.0, 0.0), flags: int = 0) -> StepParams:
    """hrt_step_params: the rounds per call, query_params' seed and shutter, scatter_params' background, STEP_* flags."""
    return StepParams(flags, steps, float(shutter[0]), float(shutter[1]), seed, _F3(*[float(x) for x in background]), 0)


def trace_paths_fused(scene: "Scene", cam: Camera, p: RenderParams, tiles=None, device: bool = False, steps: int = 2,
                      check_every: int = 4):
    """trace_paths through the fused call: camera paths, then Scene.step over two ping-pong live lists that stay on the
    device, `steps` rounds per call.  The live count is read back every `check_every` calls only (0: never, the loop then
    makes all ceil(p.max_depth / steps) calls, the late ones over an empty list), the ray count once at the end.  Returns
    what trace_paths returns, bit for bit."""
    rays, paths = camera_paths(scene, cam, p, tiles, device=True)
    n_rays = _step_to_completion(scene, cam, p, rays, paths, steps, check_every)
    return (paths if device else paths[:, 8:11].cpu().numpy()), n_rays


def _step_to_completion(scene: "Scene", cam: Camera, p: RenderParams, rays, paths, steps: int, check_every: int) -> int:
    """trace_paths_fused's loop on device tensors of rays and paths, in place; returns the rays traced."""
    import torch

    n = rays.shape[0]
    lists = [(torch.empty(n, dtype=torch.int32, device=rays.device), torch.zeros(1, dtype=torch.int32, device=rays.device))
             for _ in range(2)]
    n_rays = torch.zeros(1, dtype=torch.int64, device=rays.device)
    live = None
    for call in range((p.max_depth + steps - 1) // steps):
        out = lists[call & 1]
        scene.step(rays, paths, steps=steps, seed=p.seed, shutter=(cam.time0, cam.time1), background=tuple(p.background),
                   live=live, live_out=out, n_rays=n_rays)
        live = out
        if check_every and (call + 1) % check_every == 0 and int(out[1]) == 0:
            break
    return int(n_rays)


def tile_grid(width: int, height: int, tile_size: int = 80, rank: int = 0, world: int = 1) -> List[Tuple[int, int, int, int]]:
    """Reference tile grid (application.rs:363-364, 404-430) split round-robin over `world` ranks."""
    L = load()
    n = ctypes.c_uint32()
    _check(L.hrt_tile_grid(width, height, tile_size, rank, world, None, 0, ctypes.byref(n)))
    arr = (Tile * max(1, n.value))()
    _check(L.hrt_tile_grid(width, height, tile_size, rank, world, ctypes.cast(arr, ctypes.c_void_p), n.value, ctypes.byref(n)))
    return [(t.x, t.y, t.w, t.h) for t in arr[: n.value]]


def render(scene: Scene, cam: Camera, p: RenderParams, region=None, stats: bool = False):
    """Render a region into host memory (synchronous); returns (h, w, 4) float32 [, RenderStats]."""
    x0, y0, w, h = region if region is not None else (0, 0, p.width, p.height)
    out = np.zeros((h, w, 4), np.float32)
    st = RenderStats()
    _check(load().hrt_render(scene.h, ctypes.byref(cam), ctypes.byref(p), x0, y0, w, h, out.ctypes.data, ctypes.byref(st)))
    return (out, st) if stats else out


def render_tiles_device(scene: Scene, cam: Camera, p: RenderParams, tiles, d_out_ptr: int, stream_ptr: int = 0, want_stats: bool = False):
    """Asynchronous render of a tile list into device memory (tiles packed back to back)."""
    arr = (Tile * len(tiles))(*[Tile(*t) for t in tiles])
    st = RenderStats()
    _check(load().hrt_render_tiles_device(scene.h, ctypes.byref(cam), ctypes.byref(p), ctypes.cast(arr, ctypes.c_void_p), len(tiles),
                                          ctypes.c_void_p(d_out_ptr), ctypes.c_void_p(stream_ptr), ctypes.byref(st) if want_stats else None))
    return st if want_stats else None


ACCUM_F32, ACCUM_RGBA8 = 0, 1
ACCUM_NOISE, ACCUM_FEATURES = 1, 4  # hrt_accum_create_ex flags
_ACCUM_FORMATS = {"f32": ACCUM_F32, "rgba8": ACCUM_RGBA8}


def filter_params(iterations: int = 3, sigma: float = 4.0) -> FilterParams:
    """hrt_filter_params with the defaults of Accumulator.resolve(denoise=True)."""
    return FilterParams(int(iterations), float(sigma))


# the guided filter's default tolerances (the sweep over both test inputs; a normal term this
# tight is what keeps geometry smaller than the footprint)
GUIDED_DEFAULTS = dict(normal=0.1, albedo=0.1, depth=0.1)


def guided_params(iterations: int = 3, sigma: float = 4.0, normal: Optional[float] = None, albedo: Optional[float] = None,
                  depth: Optional[float] = None) -> GuidedParams:
    """hrt_guided_params with the defaults of Accumulator.resolve(guide=True); a tolerance of 0 switches its term off."""
    t = [GUIDED_DEFAULTS[k] if v is None else v for k, v in (("normal", normal), ("albedo", albedo), ("depth", depth))]
    return GuidedParams(int(iterations), float(sigma), float(t[0]), float(t[1]), float(t[2]))


GUIDED_DEMODULATE = 1  # hrt_guided_ex_params.flags
# demodulate=True: the albedo floor and the tolerances under demodulation (the sweep and the rule
# of GUIDED_DEFAULTS; the remodulated texture carries the albedo plane's own sampling noise, so the normal term is tighter)
DEMOD_FLOOR = 0.01
DEMOD_DEFAULTS = dict(normal=0.05, albedo=0.2, depth=0.2)


def _demod_floor(demodulate) -> float:
    return DEMOD_FLOOR if demodulate is True else float(demodulate)


def guided_ex_params(iterations: int = 3, sigma: float = 4.0, normal: Optional[float] = None, albedo: Optional[float] = None,
                     depth: Optional[float] = None, demodulate=True) -> GuidedExParams:
    """hrt_guided_ex_params.  demodulate: True means DEMOD_FLOOR, a float is the albedo floor; the tolerances default to
    DEMOD_DEFAULTS.  False: flags 0 and GUIDED_DEFAULTS, which is hrt_guided_params' frame."""
    on = demodulate is not False and demodulate is not None
    dflt = DEMOD_DEFAULTS if on else GUIDED_DEFAULTS
    t = [dflt[k] if v is None else v for k, v in (("normal", normal), ("albedo", albedo), ("depth", depth))]
    return GuidedExParams(int(iterations), float(sigma), float(t[0]), float(t[1]), float(t[2]), GUIDED_DEMODULATE if on else 0,
                          _demod_floor(demodulate) if on else 0.0, 0)


class Accumulator:
    """hrt_accum: device-resident raw per-pixel sums of a tile set (the whole frame when `tiles` is None).  Passes
    add sample ranges (`add` with params.sample_offset / params.samples), and `resolve` gives the frame of the
    samples held so far.  The frame's bits depend on the pass schedule alone (include/hrt/hrt.h).  noise=True
    (HRT_ACCUM_NOISE) also keeps the noise plane that `noise` and `refine` read; features=True (HRT_ACCUM_FEATURES) the
    two first-hit feature planes that `add_features` fills and `features` and `resolve(guide=...)` read."""

    def __init__(self, scene: Scene, width: int, height: int, tiles=None, noise: bool = False, features: bool = False):
        self.scene, self.width, self.height = scene, int(width), int(height)  # the scene must outlive the accumulator
        self.tiles = [tuple(int(v) for v in t) for t in tiles] if tiles is not None else [(0, 0, self.width, self.height)]
        self.n_pixels = sum(t[2] * t[3] for t in self.tiles)
        self.h = ctypes.c_void_p()
        arr = (Tile * max(1, len(self.tiles)))(*[Tile(*t) for t in self.tiles])
        self.has_noise, self.has_features = bool(noise), bool(features)
        if noise or features:
            flags = (ACCUM_NOISE if noise else 0) | (ACCUM_FEATURES if features else 0)
            _check(load().hrt_accum_create_ex(scene.h, self.width, self.height, ctypes.cast(arr, ctypes.c_void_p),
                                              len(self.tiles), flags, ctypes.byref(self.h)))
        else:
            _check(load().hrt_accum_create(scene.h, self.width, self.height, ctypes.cast(arr, ctypes.c_void_p),
                                           len(self.tiles), ctypes.byref(self.h)))

    def close(self):
        if self.h:
            load().hrt_accum_destroy(self.h)
            self.h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _shaped(self, flat: np.ndarray) -> np.ndarray:
        """(h, w, 4) for one tile (as hrt.render), else the packed (n_pixels, 4)."""
        if len(self.tiles) == 1:
            return flat.reshape(self.tiles[0][3], self.tiles[0][2], 4)
        return flat.reshape(self.n_pixels, 4)

    def _device_buffer(self, n: int, dtype):
        """(buffer, stream): an empty torch buffer of n elements on the scene's device, and that device's current stream."""
        import torch

        dev = torch.device("cuda", self.scene.device if self.scene.device >= 0 else torch.cuda.current_device())
        return torch.empty(n, dtype=dtype, device=dev), torch.cuda.current_stream(dev)

    def _tile_noise(self, call, error_map: bool):
        """The tail `noise` and `noise_filtered` share: call(d_err, stream, records), with a device error map if asked for."""
        rec = (TileNoise * len(self.tiles))()
        if not error_map:
            _check(call(None, None, ctypes.cast(rec, ctypes.c_void_p)))
            return list(rec)
        import torch

        buf, stream = self._device_buffer(self.n_pixels, torch.float32)
        _check(call(ctypes.c_void_p(buf.data_ptr()), ctypes.c_void_p(stream.cuda_stream), ctypes.cast(rec, ctypes.c_void_p)))
        return list(rec), buf.cpu().numpy()

    def add(self, cam: Camera, p: RenderParams, stats: bool = False, preview=None, tiles=None):
        """Render samples [p.sample_offset, p.sample_offset + p.samples) of every pixel and add them.  preview
        ("f32" / "rgba8", or True for "f32"): also return the frame after this pass, resolved by the kernel that adds
        the pass (hrt_accum_add_resolve).  tiles: indices into self.tiles; the pass then goes to those tiles alone
        (hrt_accum_add_tiles; no preview).  Returns None, RenderStats, the preview, or (preview, RenderStats)."""
        st = RenderStats()
        sp = ctypes.byref(st) if stats else None
        if tiles is not None:
            if preview is not None and preview is not False:
                raise ValueError("a pass over a subset of the tiles has no preview")
            idx = np.ascontiguousarray(list(tiles), np.uint32)
            _check(load().hrt_accum_add_tiles(self.h, ctypes.byref(cam), ctypes.byref(p), idx.ctypes.data if idx.size else None,
                                              idx.size, None, sp))
            return st if stats else None
        if preview is None or preview is False:
            _check(load().hrt_accum_add(self.h, ctypes.byref(cam), ctypes.byref(p), None, sp))
            return st if stats else None
        import torch

        fmt = "f32" if preview is True else preview
        buf, stream = self._device_buffer(self.n_pixels * 4, torch.float32 if fmt == "f32" else torch.uint8)
        _check(load().hrt_accum_add_resolve(self.h, ctypes.byref(cam), ctypes.byref(p), _ACCUM_FORMATS[fmt],
                                            ctypes.c_void_p(buf.data_ptr()), ctypes.c_void_p(stream.cuda_stream), sp))
        stream.synchronize()
        img = self._shaped(buf.cpu().numpy())
        return (img, st) if stats else img

    def add_paths(self, paths, cam: Camera, p: RenderParams, tiles=None, preview=None, live: bool = False):
        """Add the radiance of caller-traced paths as ONE pass, bit for bit what `add` with the same arguments adds when
        the paths are the render's (hrt_accum_add_paths): samples [p.sample_offset, + p.samples) of every pixel, or of
        the tiles `tiles` indexes into self.tiles.  paths: the batch hrt.camera_paths(scene, cam, p, those tiles in that
        order) starts, stepped by the caller: an (n, 12) float32 CUDA tensor, or a PATH_DTYPE numpy array, which takes
        the host variant (no preview).  A record's radiance is added whatever its flags; live=True also returns how many
        records were not DONE.  Returns what `add` returns (None or the preview), with live=True (that, count)."""
        idx = None if tiles is None else np.ascontiguousarray(list(tiles), np.uint32)
        ip, ni = (None, 0) if idx is None else (idx.ctypes.data if idx.size else None, idx.size)
        want = preview is not None and preview is not False
        if isinstance(paths, np.ndarray):
            if want:
                raise ValueError("the host variant has no preview: pass a CUDA tensor")
            if paths.dtype != PATH_DTYPE or not paths.flags.c_contiguous:
                raise ValueError("paths: a contiguous PATH_DTYPE array")
            count = ctypes.c_uint32(0)
            _check(load().hrt_accum_add_paths_host(self.h, ctypes.byref(cam), ctypes.byref(p), ip, ni, paths.ctypes.data, paths.size,
                                                   ctypes.byref(count) if live else None))
            return (None, count.value) if live else None
        import torch

        if not (isinstance(paths, torch.Tensor) and paths.is_cuda and paths.is_contiguous() and
                paths.numel() * paths.element_size() % 48 == 0):
            raise ValueError("paths: a PATH_DTYPE array, or a contiguous CUDA tensor of 48-byte records")
        n = paths.numel() * paths.element_size() // 48
        count = torch.zeros(1, dtype=torch.int32, device=paths.device) if live else None
        fmt = "f32" if preview is True else preview
        buf = torch.empty(self.n_pixels * 4, dtype=torch.float32 if fmt == "f32" else torch.uint8, device=paths.device) if want else None
        _check(load().hrt_accum_add_paths(self.h, ctypes.byref(cam), ctypes.byref(p), ip, ni, paths.data_ptr(), n,
                                          _ACCUM_FORMATS[fmt] if want else -1, buf.data_ptr() if want else None,
                                          count.data_ptr() if live else None, None))
        img = self._shaped(buf.cpu().numpy()) if want else None
        return (img, int(count)) if live else img

    def add_wavefront(self, cam: Camera, p: RenderParams, tiles=None, steps: int = 2, check_every: int = 4, preview=None) -> int:
        """`add` by another route, and the template of a caller's own integrator: hrt.camera_paths on the tiles, then
        hrt.trace_paths_fused's loop (Scene.step over two device-side live lists), then `add_paths`.  The accumulator
        ends bit for bit where add(cam, p, tiles=tiles) leaves it.  Returns the rays traced (the render's
        RenderStats.segments); with a preview, (preview, rays).
        Memory: the batch holds a 48-byte ray and a 48-byte path per sample of the pass, 96 bytes per path, plus two
        4-byte live-list entries.  How many samples go into one pass is the caller's choice and part of the result:
        splitting a pass changes the pass schedule (hrt.sample_chunks) and so the frame's bits, exactly as it does for `add`."""
        sub = None if tiles is None else [self.tiles[i] for i in tiles]
        rays, paths = camera_paths(self.scene, cam, p, self.tiles if sub is None else sub, device=True)
        n_rays = _step_to_completion(self.scene, cam, p, rays, paths, steps, check_every)
        img = self.add_paths(paths, cam, p, tiles=tiles, preview=preview)
        return n_rays if img is None else (img, n_rays)

    @property
    def samples(self) -> int:
        n = ctypes.c_uint64()
        _check(load().hrt_accum_samples(self.h, ctypes.byref(n)))
        return n.value

    @property
    def tile_samples(self) -> List[int]:
        """The samples each tile holds (hrt_accum_tile_samples)."""
        n = np.zeros(len(self.tiles), np.uint64)
        _check(load().hrt_accum_tile_samples(self.h, n.ctypes.data))
        return [int(v) for v in n]

    def noise(self, floor: float = 0.05, error_map: bool = False):
        """hrt_accum_noise: one TileNoise per tile (mean and max of the per-pixel relative standard error, samples,
        chunks); with error_map also the per-pixel errors as float32 (n_pixels,), packed as the tiles are."""
        return self._tile_noise(lambda d_err, stream, rec: load().hrt_accum_noise(self.h, float(floor), d_err, stream, rec), error_map)

    def moments(self) -> np.ndarray:
        """The noise plane m2 as float32 (n_pixels,) (hrt_debug_accum_moments)."""
        out = np.zeros(self.n_pixels, np.float32)
        _check(load().hrt_debug_accum_moments(self.h, out.ctypes.data))
        return out

    def refine(self, cam: Camera, p: RenderParams, target: float, pass_spp: int, max_spp: int, floor: float = 0.05,
               min_spp: int = 0, on_pass=None, resume: bool = False):
        """Noise-driven passes of pass_spp samples (p's samples and sample_offset are ignored): one pass over every
        tile, then passes over the tiles whose mean error exceeds `target` (or that hold fewer than min_spp samples)
        and whose samples have not reached max_spp, until no such tile is left.  A tile's k-th pass is always samples
        [k * pass_spp, (k + 1) * pass_spp), so its pixels depend on its pass count alone.  on_pass(tile indices,
        records) is called after every pass.  Returns the per-tile records (noise(floor)).
        resume=True goes on from whatever the tiles hold (an interrupted refine, restored from a snapshot) instead of
        raising: the selection rule is applied to noise(floor) first, and every round sends one pass per distinct
        sample count held among the selected tiles, in ascending order, at sample_offset = that count; so a tile's
        k-th pass is the same samples and the resumed frame equals the uninterrupted one."""
        q = RenderParams.from_buffer_copy(p)
        q.samples = int(pass_spp)
        if resume and any(self.tile_samples):
            def keep(rec, among):
                return [t for t in among if (rec[t].mean > target or rec[t].samples < min_spp) and rec[t].samples < max_spp]

            rec = self.noise(floor)
            todo = keep(rec, range(len(self.tiles)))
            while todo:
                held = self.tile_samples
                for count in sorted({held[t] for t in todo}):
                    group = [t for t in todo if held[t] == count]
                    q.sample_offset = count
                    self.add(cam, q, tiles=group)
                    rec = self.noise(floor)
                    if on_pass is not None:
                        on_pass(group, rec)
                todo = keep(rec, todo)
            return rec
        todo = list(range(len(self.tiles)))
        first = True
        while True:
            held = self.tile_samples
            if first:
                if len(set(held)) != 1:
                    raise ValueError("refine starts from an accumulator whose tiles hold the same passes")
                q.sample_offset = held[0]
                self.add(cam, q)
                first = False
            else:
                # tiles in `todo` are those that took every pass so far, so they all hold the same samples
                q.sample_offset = held[todo[0]]
                self.add(cam, q, tiles=todo)
            rec = self.noise(floor)
            if on_pass is not None:
                on_pass(todo, rec)
            todo = [t for t in todo if (rec[t].mean > target or rec[t].samples < min_spp) and rec[t].samples < max_spp]
            if not todo:
                return rec

    def _noise_filtered_params(self, denoise, guide, demodulate) -> GuidedExParams:
        kw = {} if denoise is None or denoise is True else dict(denoise)
        demod = demodulate is not False and demodulate is not None
        if guide is False or guide is None:
            terms = dict(normal=0.0, albedo=0.0, depth=0.0)
        else:
            terms = {} if guide is True else dict(guide)
        return guided_ex_params(**kw, **terms, demodulate=demodulate if demod else False)

    def noise_filtered(self, floor: float = 0.05, denoise=True, guide=False, demodulate=False, error_map: bool = False):
        """hrt_accum_noise_filtered: `noise` for the frame a filtered resolve shows, from the variance the filter itself
        propagates (the variance of the filtered frame, not its blur: a lower bound on the shown frame's error).
        denoise, guide, demodulate: resolve_guided's conventions, naming the resolve whose frame is estimated;
        guide=False (the default) switches every feature term off, which with demodulate=False is resolve(denoise=...)'s
        frame and needs no feature planes.  Returns what `noise` returns."""
        g = self._noise_filtered_params(denoise, guide, demodulate)
        return self._tile_noise(
            lambda d_err, stream, rec: load().hrt_accum_noise_filtered(self.h, ctypes.byref(g), float(floor), d_err, stream, rec), error_map)

    def refine_filtered(self, cam: Camera, p: RenderParams, target: float, pass_spp: int, max_spp: int, floor: float = 0.05,
                        denoise=True, guide=False, demodulate=False, min_spp: int = 0, on_pass=None, resume: bool = False):
        """refine, with the tiles selected on noise_filtered(floor, denoise, guide, demodulate): the passes stop when the
        FILTERED preview's estimated error meets the target.  The loop and the pass-numbering rule are refine's (a tile's
        k-th pass is samples [k * pass_spp, (k + 1) * pass_spp); resume=True goes on from whatever the tiles hold), except
        that a tile which met the target may be selected again when its neighbours' passes move its estimate.  While
        any tile holds fewer than 2 chunks the filtered estimate does not exist (HRT_ERR_STATE); that round uses
        noise(floor), whose +inf keeps those tiles selected.  With guide or demodulate the feature samples must be held
        already (add_features): it raises otherwise, before any pass."""
        needs_features = (guide is not False and guide is not None) or (demodulate is not False and demodulate is not None)
        if needs_features and (not self.has_features or self.feature_samples == 0):
            raise ValueError("refine_filtered with guide or demodulate needs feature samples (add_features) before the first pass")

        def estimate():
            try:
                return self.noise_filtered(floor, denoise, guide, demodulate)
            except HrtError as e:
                if e.status != ERR_STATE:
                    raise
                return self.noise(floor)  # a tile with fewer than 2 chunks: its +inf keeps it selected

        q = RenderParams.from_buffer_copy(p)
        q.samples = int(pass_spp)
        held = self.tile_samples
        rec = None
        if not (resume and any(held)):
            if len(set(held)) != 1:
                raise ValueError("refine_filtered starts from an accumulator whose tiles hold the same passes")
            q.sample_offset = held[0]
            self.add(cam, q)
            rec = estimate()
            if on_pass is not None:
                on_pass(list(range(len(self.tiles))), rec)
        while True:
            # A tile's filtered record moves with its neighbours' passes, so the selection is made among ALL tiles after
            # every pass, and the next pass goes to the selected tiles that hold the fewest samples: what happens next is a
            # function of what the tiles hold, which is what makes an interrupted run resumable.
            if rec is None:
                rec = estimate()
            todo = [t for t in range(len(self.tiles)) if (rec[t].mean > target or rec[t].samples < min_spp) and rec[t].samples < max_spp]
            if not todo:
                return rec
            count = min(rec[t].samples for t in todo)
            group = [t for t in todo if rec[t].samples == count]
            q.sample_offset = count
            self.add(cam, q, tiles=group)
            rec = estimate()
            if on_pass is not None:
                on_pass(group, rec)

    def add_features(self, cam: Camera, p: RenderParams):
        """The first-hit features of samples [p.sample_offset, p.sample_offset + p.samples) of every pixel, added to the
        feature planes (hrt_accum_add_features): one launch, no radiance."""
        _check(load().hrt_accum_add_features(self.h, ctypes.byref(cam), ctypes.byref(p), None))

    @property
    def feature_samples(self) -> int:
        n = ctypes.c_uint64()
        _check(load().hrt_accum_feature_samples(self.h, ctypes.byref(n)))
        return n.value

    def features(self):
        """(albedo, normal): the mean feature planes as float32 shaped like `resolve`'s frame: albedo (a.xyz, the hit
        fraction) and normal (n.xyz, the mean depth of the hits) (hrt_accum_features_host)."""
        al, no = np.zeros(self.n_pixels * 4, np.float32), np.zeros(self.n_pixels * 4, np.float32)
        _check(load().hrt_accum_features_host(self.h, al.ctypes.data, no.ctypes.data))
        return self._shaped(al), self._shaped(no)

    def debug_features(self):
        """(fa, fn): the raw feature sums as (n_pixels, 4) float32 each (hrt_debug_accum_features)."""
        fa, fn = np.zeros((self.n_pixels, 4), np.float32), np.zeros((self.n_pixels, 4), np.float32)
        _check(load().hrt_debug_accum_features(self.h, fa.ctypes.data, fn.ctypes.data))
        return fa, fn

    def resolve(self, fmt: str = "f32", denoise=None) -> np.ndarray:
        """The frame of the samples held: float32 sqrt(sum / samples) with alpha 1 shaped like hrt.render's result,
        or uint8 (the PPM rule, alpha 255); several tiles: packed (n_pixels, 4).  denoise (a noise=True accumulator):
        the frame through the variance-guided a-trous filter instead (hrt_accum_resolve_filtered_host); True means
        dict(iterations=3, sigma=4.0), a dict overrides either value.  A preview for noisy scenes, never a default.
        With the feature terms: resolve_guided."""
        out = np.zeros(self.n_pixels * 4, np.float32 if fmt == "f32" else np.uint8)
        if denoise is None or denoise is False:
            _check(load().hrt_accum_resolve_host(self.h, _ACCUM_FORMATS[fmt], out.ctypes.data))
            return self._shaped(out)
        f = filter_params(**({} if denoise is True else dict(denoise)))
        _check(load().hrt_accum_resolve_filtered_host(self.h, ctypes.byref(f), _ACCUM_FORMATS[fmt], out.ctypes.data))
        return self._shaped(out)

    def resolve_guided(self, fmt: str = "f32", denoise=None, guide=True, demodulate=False) -> np.ndarray:
        """resolve(fmt, denoise) through the filter WITH the feature terms (hrt_accum_resolve_guided_host), for a
        noise=True, features=True accumulator that holds feature samples.  denoise: as resolve's, None meaning True.
        guide: True means GUIDED_DEFAULTS, a dict(normal=, albedo=, depth=) overrides a tolerance (0: that term off).
        demodulate (opt-in, hrt_accum_resolve_guided_ex_host with HRT_GUIDED_DEMODULATE): filter the radiance divided
        by the first-hit albedo and multiply it back; True means the floor DEMOD_FLOOR, a float is the albedo floor,
        and guide=True then means DEMOD_DEFAULTS."""
        out = np.zeros(self.n_pixels * 4, np.float32 if fmt == "f32" else np.uint8)
        kw = {} if denoise is None or denoise is True else dict(denoise)
        if demodulate is not False and demodulate is not None:
            g = guided_ex_params(**kw, **({} if guide is True else dict(guide)), demodulate=demodulate)
            _check(load().hrt_accum_resolve_guided_ex_host(self.h, ctypes.byref(g), _ACCUM_FORMATS[fmt], out.ctypes.data))
            return self._shaped(out)
        g = guided_params(**kw, **({} if guide is True else dict(guide)))
        _check(load().hrt_accum_resolve_guided_host(self.h, ctypes.byref(g), _ACCUM_FORMATS[fmt], out.ctypes.data))
        return self._shaped(out)

    def merge(self, other: "Accumulator"):
        """self += other (same scene device, tiles and frame identity; disjoint sample ranges)."""
        _check(load().hrt_accum_merge(self.h, other.h, None))

    def merge_tiles(self, other: "Accumulator"):
        """merge for accumulators whose tiles may hold different passes (hrt_accum_merge_tiles): every tile for which
        `other` holds samples takes them (its ranges must be disjoint from this one's for that tile); the others are not
        touched."""
        _check(load().hrt_accum_merge_tiles(self.h, other.h, None))

    def snapshot_size(self) -> int:
        n = ctypes.c_uint64()
        _check(load().hrt_accum_snapshot(self.h, None, 0, ctypes.byref(n)))
        return n.value

    def snapshot_into(self, buf: np.ndarray) -> int:
        """hrt_accum_snapshot into a caller-owned contiguous uint8 array; returns the snapshot's bytes."""
        if buf.dtype != np.uint8 or not buf.flags.c_contiguous or not buf.flags.writeable:
            raise ValueError("a writable contiguous uint8 array")
        n = ctypes.c_uint64()
        _check(load().hrt_accum_snapshot(self.h, buf.ctypes.data, buf.size, ctypes.byref(n)))
        return n.value

    def snapshot(self) -> bytes:
        """The whole state (sums, noise plane, feature planes, per-tile ranges and chunk counts, frame identity) as one
        self-describing blob (hrt_accum_snapshot; include/hrt/hrt.h states the layout).  Waits for the device."""
        buf = np.empty(self.snapshot_size(), np.uint8)
        n = self.snapshot_into(buf)
        return buf[:n].tobytes()

    def restore(self, blob):
        """Put a snapshot into this accumulator, which must hold no samples and have the snapshot's width, height, tiles
        and flags (hrt_accum_restore); every later call then answers as on the snapshotted accumulator, bit for bit."""
        b = np.frombuffer(blob, np.uint8)
        _check(load().hrt_accum_restore(self.h, b.ctypes.data if b.size else None, b.size))

    def save(self, path):
        """The snapshot to a file (straight from the buffer the library filled, without snapshot()'s bytes object)."""
        buf = np.empty(self.snapshot_size(), np.uint8)
        n = self.snapshot_into(buf)
        with open(path, "wb") as f:
            f.write(memoryview(buf[:n]))

    @classmethod
    def load(cls, scene: Scene, path) -> "Accumulator":
        """An accumulator on `scene` (the committed scene the snapshot was rendered on) from a file written by save:
        created with the blob's size, tiles and flags (hrt_accum_snapshot_info), then restored."""
        with open(path, "rb") as f:
            blob = f.read()
        info, tiles = snapshot_info(blob)
        acc = cls(scene, info.width, info.height, tiles, noise=bool(info.flags & ACCUM_NOISE), features=bool(info.flags & ACCUM_FEATURES))
        try:
            acc.restore(blob)
        except Exception:
            acc.close()
            raise
        return acc

    def download(self):
        """(sums, ranges): the raw sums as (n_pixels, 4) float32 (w = 0) and the [(begin, end), ...] held."""
        n = ctypes.c_uint32()
        _check(load().hrt_accum_download(self.h, None, None, 0, ctypes.byref(n)))
        sums = np.zeros((self.n_pixels, 4), np.float32)
        rng = np.zeros(2 * max(1, n.value), np.uint32)
        _check(load().hrt_accum_download(self.h, sums.ctypes.data, rng.ctypes.data, n.value, ctypes.byref(n)))
        return sums, [(int(rng[2 * i]), int(rng[2 * i + 1]) or 1 << 32) for i in range(n.value)]

    def upload(self, cam: Camera, p: RenderParams, sums: np.ndarray, ranges):
        """Put downloaded sums and their ranges into this accumulator under the frame identity of (cam, p)."""
        s = np.ascontiguousarray(sums, np.float32)
        if s.size != self.n_pixels * 4:
            raise ValueError("sums must hold n_pixels x 4 float32")
        rng = np.array([[b, e & 0xFFFFFFFF] for b, e in ranges], np.uint32).reshape(-1)
        _check(load().hrt_accum_upload(self.h, ctypes.byref(cam), ctypes.byref(p), s.ctypes.data,
                                       rng.ctypes.data if rng.size else None, len(ranges)))

    def reset(self):
        _check(load().hrt_accum_reset(self.h, None))


def snapshot_info(blob):
    """hrt_accum_snapshot_info: (SnapshotInfo, [(x, y, w, h), ...]) of a snapshot blob, validated as a restore
    validates it; no device involved."""
    b = np.frombuffer(blob, np.uint8)
    ptr = b.ctypes.data if b.size else None
    info = SnapshotInfo()
    cap = 4096  # most tile lists fit: one validation (and one checksum pass over the blob), not two
    arr = (Tile * cap)()
    _check(load().hrt_accum_snapshot_info(ptr, b.size, ctypes.byref(info), ctypes.cast(arr, ctypes.c_void_p), cap))
    if info.n_tiles > cap:
        arr = (Tile * info.n_tiles)()
        _check(load().hrt_accum_snapshot_info(ptr, b.size, ctypes.byref(info), ctypes.cast(arr, ctypes.c_void_p), info.n_tiles))
    return info, [(t.x, t.y, t.w, t.h) for t in arr[: info.n_tiles]]


def debug_accumulate(partial: np.ndarray, acc: np.ndarray, samples: int = 0, fmt: Optional[str] = None, on_device: bool = False):
    """hrt_debug_accumulate: csrc/accum.h on the host, or the real kernels on the current device.  partial:
    (n_chunks, n, 4) float32 chunk sums of one pass, acc: (n, 4) float32 sums before it.  Returns (acc after the pass,
    the frame of `samples` samples in `fmt`: (n, 4) float32 / uint8, or None without fmt)."""
    pa = np.ascontiguousarray(partial, np.float32)
    n_chunks, n = pa.shape[0], pa.shape[1]
    a = np.array(acc, np.float32).reshape(n, 4).copy()
    out = None if fmt is None else np.zeros((n, 4), np.float32 if fmt == "f32" else np.uint8)
    _check(load().hrt_debug_accumulate(1 if on_device else 0, pa.ctypes.data, n_chunks, n, a.ctypes.data, int(samples),
                                       -1 if fmt is None else _ACCUM_FORMATS[fmt], None if out is None else out.ctypes.data))
    return a, out


def debug_accum_paths(paths: np.ndarray, samples: int, schedule, acc: np.ndarray, m2=None, total_samples: int = 0,
                      fmt: Optional[str] = None, on_device: bool = False):
    """hrt_debug_accum_paths: csrc/accum_paths.h on the host, or the real kernel on the current device.  paths: a
    PATH_DTYPE array of n_px x samples records, a pixel's consecutive; schedule: hrt.sample_chunks' dict or its
    (chunk, head, first); acc (n_px, 4) / m2 (n_px,) or None: the sums and moments before the pass.  Returns (acc, m2 or
    None after the pass, the frame of total_samples samples in `fmt` or None, the records that are not DONE)."""
    pa = np.ascontiguousarray(paths, PATH_DTYPE).reshape(-1)
    n_px = pa.size // samples
    if n_px * samples != pa.size:
        raise ValueError("paths: n_px x samples records")
    if isinstance(schedule, dict):
        schedule = (schedule["chunk"], schedule["head"], schedule["first"])
    sch = np.array(schedule, np.uint32)[:3].copy()
    a = np.array(acc, np.float32).reshape(n_px, 4).copy()
    m = None if m2 is None else np.array(m2, np.float32).reshape(n_px).copy()
    out = None if fmt is None else np.zeros((n_px, 4), np.float32 if fmt == "f32" else np.uint8)
    live = ctypes.c_uint32(0)
    _check(load().hrt_debug_accum_paths(1 if on_device else 0, pa.ctypes.data if pa.size else None, n_px, int(samples), sch.ctypes.data,
                                        a.ctypes.data if a.size else None, None if m is None else m.ctypes.data, int(total_samples),
                                        -1 if fmt is None else _ACCUM_FORMATS[fmt], None if out is None else out.ctypes.data,
                                        ctypes.byref(live)))
    return a, m, out, live.value


def debug_noise(partial: np.ndarray, sizes, acc: np.ndarray, m2: np.ndarray, samples: int, chunks: int, floor: float = 0.05,
                on_device: bool = False):
    """hrt_debug_noise: the noise estimate of csrc/accum.h for one tile of n pixels on the host, or through the real
    kernels on the current device.  partial: (n_chunks, n, 4) float32 chunk sums of one pass with `sizes` samples
    each, acc (n, 4) / m2 (n,) the sums and moments before it, samples / chunks: N and K held after it.  Returns
    (acc, m2 after the pass, err (n,), mean, max) as float32."""
    pa = np.ascontiguousarray(partial, np.float32)
    n_chunks, n = pa.shape[0], pa.shape[1]
    sz = np.ascontiguousarray(sizes, np.uint32)
    if sz.shape != (n_chunks,):
        raise ValueError("one size per chunk")
    a = np.array(acc, np.float32).reshape(n, 4).copy()
    m = np.array(m2, np.float32).reshape(n).copy()
    err, mm = np.zeros(n, np.float32), np.zeros(2, np.float32)
    _check(load().hrt_debug_noise(1 if on_device else 0, pa.ctypes.data, sz.ctypes.data, n_chunks, n, a.ctypes.data, m.ctypes.data,
                                  int(samples), int(chunks), float(floor), err.ctypes.data, mm.ctypes.data))
    return a, m, err, mm[0], mm[1]


def debug_filter(raster: np.ndarray, iterations: int, sigma: float, on_device: bool = False) -> np.ndarray:
    """hrt_debug_filter: the a-trous filter's iterations (csrc/filter.h) on the host, or through the real kernel on
    the current device.  raster: (height, width, 4) float32 (c.xyz, v; v < 0: an absent pixel).  Returns the same
    shape: (c'.xyz before the sqrt, v'); absent pixels come out as they went in."""
    r = np.ascontiguousarray(raster, np.float32)
    if r.ndim != 3 or r.shape[2] != 4:
        raise ValueError("raster must be (height, width, 4) float32")
    out = np.zeros_like(r)
    _check(load().hrt_debug_filter(1 if on_device else 0, r.ctypes.data, r.shape[1], r.shape[0], int(iterations), float(sigma),
                                   out.ctypes.data))
    return out


def debug_guided(raster: np.ndarray, albedo: np.ndarray, normal: np.ndarray, iterations: int, sigma: float, kn: float = 0.0,
                 ka: float = 0.0, kz: float = 0.0, on_device: bool = False, demodulate=False) -> np.ndarray:
    """hrt_debug_guided: debug_filter for the guided filter (csrc/filter.h).  albedo, normal: the feature rasters,
    (height, width, 4) float32 ((a.xyz, -), (n.xyz, z)); kn, ka, kz: 1 / tolerance of each term, 0: off.
    demodulate (hrt_debug_guided_ex with HRT_GUIDED_DEMODULATE; True: DEMOD_FLOOR, a float: the albedo floor): the
    raster is gather's (c, v), and (c'' before the sqrt, v' in demodulated units) comes back."""
    r = np.ascontiguousarray(raster, np.float32)
    a, n = np.ascontiguousarray(albedo, np.float32), np.ascontiguousarray(normal, np.float32)
    if r.ndim != 3 or r.shape[2] != 4 or a.shape != r.shape or n.shape != r.shape:
        raise ValueError("raster, albedo and normal must be (height, width, 4) float32 of one shape")
    out = np.zeros_like(r)
    if demodulate is not False and demodulate is not None:
        _check(load().hrt_debug_guided_ex(1 if on_device else 0, r.ctypes.data, a.ctypes.data, n.ctypes.data, r.shape[1], r.shape[0],
                                          int(iterations), float(sigma), float(kn), float(ka), float(kz), GUIDED_DEMODULATE,
                                          _demod_floor(demodulate), out.ctypes.data))
        return out
    _check(load().hrt_debug_guided(1 if on_device else 0, r.ctypes.data, a.ctypes.data, n.ctypes.data, r.shape[1], r.shape[0],
                                   int(iterations), float(sigma), float(kn), float(ka), float(kz), out.ctypes.data))
    return out


def debug_noise_filtered(raster: np.ndarray, albedo, normal, iterations: int, sigma: float, tiles, kn: float = 0.0, ka: float = 0.0,
                         kz: float = 0.0, demodulate=False, floor: float = 0.05, on_device: bool = False):
    """hrt_debug_noise_filtered: hrt_accum_noise_filtered's arithmetic (csrc/filter.h) on a raster cut into `tiles`
    ((x, y, w, h) inside the raster, disjoint, present pixels only).  albedo, normal: the feature rasters, or None when
    no term and no demodulation is on.  Returns (err, mean_max): the errs packed as the tiles are and (n_tiles, 2)."""
    r = np.ascontiguousarray(raster, np.float32)
    a = None if albedo is None else np.ascontiguousarray(albedo, np.float32)
    n = None if normal is None else np.ascontiguousarray(normal, np.float32)
    tl = [tuple(int(v) for v in t) for t in tiles]
    arr = (Tile * max(1, len(tl)))(*[Tile(*t) for t in tl])
    err = np.zeros(sum(t[2] * t[3] for t in tl), np.float32)
    mm = np.zeros((len(tl), 2), np.float32)
    on = demodulate is not False and demodulate is not None
    _check(load().hrt_debug_noise_filtered(1 if on_device else 0, r.ctypes.data, None if a is None else a.ctypes.data,
                                           None if n is None else n.ctypes.data, r.shape[1], r.shape[0], int(iterations), float(sigma),
                                           float(kn), float(ka), float(kz), GUIDED_DEMODULATE if on else 0,
                                           _demod_floor(demodulate) if on else 0.0, float(floor), ctypes.cast(arr, ctypes.c_void_p),
                                           len(tl), err.ctypes.data, mm.ctypes.data))
    return err, mm


def debug_accum_features(acc: "Accumulator"):
    """hrt_debug_accum_features: the raw feature sums (fa, fn) of an accumulator."""
    return acc.debug_features()


WALK_GREEDY, WALK_DP_AREA, WALK_DP_LEAVES, WALK_GREEDY_SUB, WALK_DEVICE = range(5)


def walk_regroup(boxes: np.ndarray, builder: int, dp_sub: int = 0, out=None):
    """hrt_debug_walk_regroup: one builder of the walk hierarchy (WALK_*) on (n, 6) float32 leaf boxes (min xyz,
    max xyz).  Returns the 2n - 1 pre-order nodes as (leaf int32, end uint32, depth uint32, boxes (2n - 1, 6)
    float32); `out`: such a tuple of arrays to write into."""
    b = np.ascontiguousarray(boxes, np.float32).reshape(-1, 6)
    m = max(2 * len(b) - 1, 1)
    leaf, end, depth, nb = out if out is not None else (np.zeros(m, np.int32), np.zeros(m, np.uint32),
                                                        np.zeros(m, np.uint32), np.zeros((m, 6), np.float32))
    _check(load().hrt_debug_walk_regroup(int(builder), b.ctypes.data, len(b), int(dp_sub), leaf.ctypes.data, end.ctypes.data,
                                         depth.ctypes.data, nb.ctypes.data))
    return leaf, end, depth, nb


def last_launch() -> Optional[dict]:
    """The calling thread's last render launch (hrt_last_launch): kernel, grid, occupancy, VGPRs, scratch, LDS, and
    the library's A/B environment knobs set in this process.  None with an older build that lacks the entry
    point (an A/B run through HRT_LIB)."""
    L = load()
    if not hasattr(L, "hrt_last_launch"):
        return None
    li = LaunchInfo()
    _check(L.hrt_last_launch(ctypes.byref(li)))
    d = {n: getattr(li, n) for n, _ in LaunchInfo._fields_[1:-1]}
    d["kernel"] = li.kernel.decode()
    d["knobs"] = li.knobs.decode()
    d["waves"] = li.grid * li.block // 64
    return d


def box_test(form: int, boxes: np.ndarray, rays: np.ndarray, tmin: float, tmax: float, on_device: bool = True) -> np.ndarray:
    """hrt_debug_box_test: (n_boxes, n_rays) uint8 pass flags of the walk's inflated box test (form 0 / 1)."""
    b = np.ascontiguousarray(boxes, np.float32).reshape(-1, 8)
    r = np.ascontiguousarray(rays, np.float32).reshape(-1, 6)
    out = np.zeros((len(b), len(r)), np.uint8)
    _check(load().hrt_debug_box_test(form, 1 if on_device else 0, b.ctypes.data, len(b), r.ctypes.data, len(r), tmin, tmax,
                                     out.ctypes.data))
    return out


def device_math(op: int, x: np.ndarray, y: Optional[np.ndarray] = None) -> np.ndarray:
    x = np.ascontiguousarray(x, np.float32)
    out = np.zeros_like(x)
    yy = None if y is None else np.ascontiguousarray(y, np.float32)
    _check(load().hrt_debug_device_math(op, x.ctypes.data, None if yy is None else yy.ctypes.data, out.ctypes.data, x.size))
    return out


def trace_path(scene: Scene, cam: Camera, p: RenderParams, x: int, y: int, sample: int, max_segments: int = 64):
    """Device trace of one path: list of (origin, direction, time, t, winner) per segment, radiance."""
    out = np.zeros(9 * max_segments + 3, np.float32)
    n = ctypes.c_uint32()
    _check(load().hrt_debug_trace_path(scene.h, ctypes.byref(cam), ctypes.byref(p), x, y, sample, max_segments, out.ctypes.data, ctypes.byref(n)))
    segs = []
    for i in range(min(n.value, max_segments)):
        r = out[9 * i:9 * i + 9]
        segs.append((r[0:3].copy(), r[3:6].copy(), float(r[6]), float(r[7]), int(r[8:9].view(np.uint32)[0])))
    return segs, out[9 * max_segments:9 * max_segments + 3].copy()


IMAGE_PFM, IMAGE_PPM = 0, 1


def write_image(path: str, rgba: np.ndarray, fmt: Optional[int] = None) -> None:
    """Write a render result ((h, w, 4) f32, row 0 = bottom) as PFM (exact floats) or 8-bit PPM;
    the format follows the extension unless given."""
    img = np.ascontiguousarray(rgba, np.float32)
    if img.ndim != 3 or img.shape[2] != 4:
        raise ValueError("expected an (h, w, 4) float32 frame")
    if fmt is None:
        fmt = IMAGE_PPM if str(path).lower().endswith(".ppm") else IMAGE_PFM
    _check(load().hrt_image_write(str(path).encode(), img.ctypes.data, img.shape[1], img.shape[0], fmt))


def read_pfm(path: str) -> np.ndarray:
    """Read a PFM written by write_image back into an (h, w, 3) float32 array (row 0 = bottom)."""
    with open(path, "rb") as f:
        assert f.readline().strip() == b"PF"
        w, h = (int(v) for v in f.readline().split())
        scale = float(f.readline())
        data = np.frombuffer(f.read(), "<f4" if scale < 0 else ">f4")
    return data.reshape(h, w, 3).astype(np.float32)


class TileMessage:
    """application.rs:45-52 Tile (the mpsc message): tile-grid position, size, and (height, width, 4)
    RGBA pixels (row 0 = bottom)."""

    def __init__(self, x, y, width, height, pixels):
        self.x, self.y, self.width, self.height, self.pixels = x, y, width, height, pixels


def render_progressive(scene: "Scene", cam: Camera, p: RenderParams, on_tile, tile_size: int = 80, rank: int = 0,
                       world: int = 1, batch: int = 64, stats: bool = False):
    """Application::render with progressive delivery: on_tile(TileMessage) is called for every tile of this
    rank's share of the grid, batch by batch, while the next batch renders (hrt_render_progressive)."""
    err = []

    def cb(tp, _user):
        try:
            t = tp.contents
            px = np.ctypeslib.as_array(t.pixels, shape=(t.height * t.width * 4,)).reshape(t.height, t.width, 4).copy()
            on_tile(TileMessage(t.x, t.y, t.width, t.height, px))
        except BaseException as e:  # noqa: BLE001 - re-raised after the C call returns
            err.append(e)

    fn = TILE_FN(cb)
    st = RenderStats()
    _check(load().hrt_render_progressive(scene.h, ctypes.byref(cam), ctypes.byref(p), tile_size, rank, world, batch,
                                         fn, None, ctypes.byref(st) if stats else None))
    if err:
        raise err[0]
    return st if stats else None


def sample_chunks(scene: "Scene", p: RenderParams) -> dict:
    """hrt_debug_sample_chunks: the chunk schedule a render of `p` would sum each pixel's samples in."""
    out = (ctypes.c_uint32 * 4)()
    _check(load().hrt_debug_sample_chunks(scene.h, ctypes.byref(p), out))
    return {"chunk": out[0], "head": out[1], "first": out[2], "tail": out[3]}


def scene_blob(scene: "Scene"):
    """The flattened scene (layout.h) as the kernels see it, without a device: (bytes, BlobInfo)."""
    size = ctypes.c_uint64()
    info = BlobInfo()
    _check(load().hrt_debug_scene_blob(scene.h, None, 0, ctypes.byref(size), ctypes.byref(info)))
    buf = ctypes.create_string_buffer(size.value)
    _check(load().hrt_debug_scene_blob(scene.h, buf, size.value, ctypes.byref(size), ctypes.byref(info)))
    return buf, info


def prim_record(scene: Scene, index: int, order: int = 0) -> np.ndarray:
    out = np.zeros(12, np.float32)
    _check(load().hrt_debug_prim_record(scene.h, order, index, out.ctypes.data))
    return out
