"""ctypes binding of include/ptmi.h (libptmi.so).  No fallbacks: if the library is missing or a call
fails, this raises — there is no CPU path in the product."""
import ctypes
import os

import numpy as np

from . import _build

_HERE = os.path.dirname(os.path.abspath(__file__))

BUF = {"spheres": 1, "quads": 2, "triangles": 5, "meshes": 6, "transforms": 7, "materials": 8, "bvh": 9}

# every symbol include/ptmi.h declares
SYMBOLS = [
    "ptmi_version", "ptmi_status_string", "ptmi_last_error", "ptmi_create", "ptmi_create_multi", "ptmi_destroy", "ptmi_default_params",
    "ptmi_set_params", "ptmi_get_params", "ptmi_upload", "ptmi_resize", "ptmi_clear_framebuffer", "ptmi_set_shard",
    "ptmi_render_frame", "ptmi_render", "ptmi_synchronize", "ptmi_prepare", "ptmi_read_framebuffer", "ptmi_write_framebuffer", "ptmi_reduce_framebuffer",
    "ptmi_framebuffer_device_ptr", "ptmi_bind_framebuffer", "ptmi_stream", "ptmi_resolve_rgba8", "ptmi_set_counters", "ptmi_set_onb_table",
    "ptmi_set_timing", "ptmi_get_stats", "ptmi_reset_stats", "ptmi_trace", "ptmi_math_eval", "ptmi_selftest", "ptmi_build_bvh",
    "ptmi_build_bvh_sah", "ptmi_build_bvh_device", "ptmi_build_scene_bvh", "ptmi_read_scene_buffer", "ptmi_obj_parse", "ptmi_free",
    "ptmi_device_count", "ptmi_reduce_info", "ptmi_reload_tuning", "ptmi_build_scene_bvh_sah", "ptmi_scene_bvh_info", "ptmi_build_bvh_sah_device",
    "ptmi_render_views", "ptmi_read_view", "ptmi_resolve_view_rgba8", "ptmi_views_device_ptr", "ptmi_release_views",
    "ptmi_render_aov", "ptmi_read_aov", "ptmi_aov_device_ptr", "ptmi_release_aov", "ptmi_camera_rays",
    "ptmi_default_denoise_params", "ptmi_denoise_views", "ptmi_read_denoised", "ptmi_resolve_denoised_rgba8", "ptmi_denoised_device_ptr", "ptmi_release_denoised",
    "ptmi_denoise_images", "ptmi_denoise_reference",
    "ptmi_default_guided_params", "ptmi_denoise_views_guided", "ptmi_denoise_images_guided", "ptmi_denoise_guided_reference",
    "ptmi_default_fuse_params", "ptmi_fuse_views", "ptmi_read_fused", "ptmi_resolve_fused_rgba8", "ptmi_fused_device_ptr", "ptmi_release_fused",
    "ptmi_fuse_images", "ptmi_fuse_reference",
    "ptmi_default_accumulate_params", "ptmi_accumulate_views", "ptmi_read_accumulated", "ptmi_resolve_accumulated_rgba8", "ptmi_accumulated_device_ptr",
    "ptmi_release_accumulated", "ptmi_accumulate_images", "ptmi_accumulate_reference",
    "ptmi_denoise_views_accumulated", "ptmi_denoise_images_accumulated", "ptmi_denoise_accumulated_reference",
    "ptmi_set_view_moments", "ptmi_read_moments", "ptmi_moments_device_ptr", "ptmi_release_moments",
    "ptmi_default_noise_params", "ptmi_view_noise_stats", "ptmi_noise_images", "ptmi_noise_reference", "ptmi_render_views_until",
    "ptmi_render_views_frames", "ptmi_render_aov_frames", "ptmi_render_views_until_each", "ptmi_view_slot_plan",
    "ptmi_check_bvh_boxes",
    "ptmi_denoise_views_frames", "ptmi_denoise_views_guided_frames", "ptmi_fuse_views_frames", "ptmi_accumulate_views_frames",
    "ptmi_denoise_images_frames", "ptmi_denoise_images_guided_frames", "ptmi_fuse_images_frames", "ptmi_accumulate_images_frames",
    "ptmi_denoise_reference_frames", "ptmi_denoise_guided_reference_frames", "ptmi_fuse_reference_frames", "ptmi_accumulate_reference_frames",
    "ptmi_denoise_views_counts", "ptmi_denoise_views_guided_counts", "ptmi_fuse_views_counts", "ptmi_accumulate_views_counts",
    "ptmi_denoise_images_counts", "ptmi_denoise_images_guided_counts", "ptmi_fuse_images_counts", "ptmi_accumulate_images_counts",
    "ptmi_denoise_reference_counts", "ptmi_denoise_guided_reference_counts", "ptmi_fuse_reference_counts", "ptmi_accumulate_reference_counts",
    "ptmi_refit_bvh", "ptmi_refit_scene_bvh",
    "ptmi_accumulate_views_motion", "ptmi_accumulate_images_motion", "ptmi_accumulate_reference_motion", "ptmi_object_ids_reference", "ptmi_motions_from_transforms",
    "ptmi_fuse_views_motion", "ptmi_fuse_images_motion", "ptmi_fuse_reference_motion", "ptmi_compose_motions",
    "ptmi_accumulate_images_deform", "ptmi_accumulate_reference_deform", "ptmi_deform_records",
    "ptmi_capture_view_geometry", "ptmi_read_view_geometry", "ptmi_geometry_device_ptr", "ptmi_release_geometry", "ptmi_accumulate_views_deform",
    "ptmi_fuse_views_deform", "ptmi_fuse_images_deform", "ptmi_fuse_reference_deform", "ptmi_fuse_deform_records",
    "ptmi_render_view_runs", "ptmi_view_run_noise", "ptmi_run_noise_images", "ptmi_run_noise_reference", "ptmi_render_views_until_runs",
    "ptmi_read_view_mean", "ptmi_resolve_view_mean_rgba8",
    "ptmi_render_views_runs", "ptmi_run_refs_reference", "ptmi_run_refs_images",
]

RUN_PIXELS = 64  # a run: 64 consecutive pixels of an image in row-major order (include/ptmi.h, "RENDERING TO A NOISE TARGET BY RUNS")

MOTION_MAX_RECORDS = 1 << 20  # PTMI_MOTION_MAX_RECORDS

VIEW_SLOT_TABLE_MAX_WORDS = 1 << 24  # PTMI_VIEW_SLOT_TABLE_MAX_WORDS


class Params(ctypes.Structure):
    _fields_ = [
        ("num_samples", ctypes.c_int32), ("max_bounces", ctypes.c_int32), ("stratify", ctypes.c_int32),
        ("importance_sampling", ctypes.c_int32), ("stack_size", ctypes.c_int32), ("background", ctypes.c_float * 3),
        ("fov_degrees", ctypes.c_float), ("frames_in_flight", ctypes.c_int32), ("tmin", ctypes.c_float), ("light_mix", ctypes.c_float), ("reserved", ctypes.c_int32 * 3),
    ]


class DenoiseParams(ctypes.Structure):
    _fields_ = [
        ("levels", ctypes.c_int32), ("sigma_normal", ctypes.c_float), ("sigma_depth", ctypes.c_float), ("sigma_colour", ctypes.c_float),
        ("albedo_floor", ctypes.c_float), ("reserved", ctypes.c_int32 * 3),
    ]


class GuidedParams(ctypes.Structure):
    _fields_ = [
        ("levels", ctypes.c_int32), ("sigma_normal", ctypes.c_float), ("sigma_depth", ctypes.c_float), ("sigma_luma", ctypes.c_float),
        ("albedo_floor", ctypes.c_float), ("min_frames", ctypes.c_int32), ("var_eps", ctypes.c_float), ("reserved", ctypes.c_int32 * 1),
    ]


class FuseParams(ctypes.Structure):
    _fields_ = [
        ("radius", ctypes.c_int32), ("sigma_normal", ctypes.c_float), ("sigma_depth", ctypes.c_float), ("albedo_floor", ctypes.c_float), ("reserved", ctypes.c_int32 * 4),
    ]


class AccumulateParams(ctypes.Structure):
    _fields_ = [
        ("max_history", ctypes.c_float), ("min_frames", ctypes.c_int32), ("sigma_normal", ctypes.c_float), ("sigma_depth", ctypes.c_float),
        ("albedo_floor", ctypes.c_float), ("reserved", ctypes.c_int32 * 3),
    ]


class NoiseParams(ctypes.Structure):
    _fields_ = [("floor", ctypes.c_float), ("threshold", ctypes.c_float), ("reserved", ctypes.c_int32 * 6)]


class ViewNoise(ctypes.Structure):
    _fields_ = [("counted", ctypes.c_uint64), ("sum_q", ctypes.c_uint64), ("above", ctypes.c_uint64), ("max_q", ctypes.c_uint32), ("reserved", ctypes.c_uint32)]


VIEW_NOISE_DTYPE = np.dtype([("counted", "<u8"), ("sum_q", "<u8"), ("above", "<u8"), ("max_q", "<u4"), ("reserved", "<u4")])
RUN_NOISE_DTYPE = np.dtype([("counted", "<u4"), ("sum_q", "<u4"), ("max_q", "<u4"), ("open", "<u4")])  # ptmi_run_noise


class Stats(ctypes.Structure):
    _fields_ = [(n, ctypes.c_uint64) for n in (
        "rays", "paths", "node_visits", "tri_tests", "sphere_tests", "quad_tests", "mat_fetches", "frames",
        "intersect_launches", "shade_launches", "bvh_node_visits", "bvh_mat_fetches")] + [
        (n, ctypes.c_double) for n in ("render_ms", "intersect_ms", "shade_ms", "other_ms", "prims_ms", "bvh_ms", "generate_ms", "accumulate_ms")] + [
        (n, ctypes.c_uint64) for n in ("generate_launches", "accumulate_launches", "devices")] + [("tail_ms", ctypes.c_double), ("tail_launches", ctypes.c_uint64)] + [
        (n, ctypes.c_uint64) for n in ("reduce_mode", "peer_links", "placement_sets")] + [("placement_ms", ctypes.c_double)]

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_}


HIT_DTYPE = np.dtype([("hit", "<i4"), ("t", "<f4"), ("p", "<f4", 3), ("normal", "<f4", 3), ("front_face", "<i4"), ("material", "<f4", 16)])


class PtmiError(RuntimeError):
    def __init__(self, status, message):
        super().__init__("ptmi status %d: %s" % (status, message))
        self.status = status


_lib = None
_libs = {}


def lib_path():
    return _build.LIB


def load_library(build=False, path=None):
    """dlopen libptmi.so (optionally building it first).  Raises if it is not there.  `path`: another build of the library next to the default
    one (the tests' fault-injection build, _build.build_testhooks) — pass the result to Context(..., lib=...)."""
    global _lib
    if path is None and _lib is not None:
        return _lib
    if path is not None and path in _libs:
        return _libs[path]
    if build:
        _build.build_lib()
    explicit = path is not None
    path = path or os.environ.get("PTMI_LIB") or _build.LIB  # PTMI_LIB: an A/B build (_build.build_variant), as for the N-API addon
    if not os.path.exists(path):
        raise OSError("%s not built: run `python -c 'import __graft_entry__ as g; g.build()'` (needs hipcc)" % os.path.basename(path))
    L = ctypes.CDLL(path)
    vp, i32, u32, sz, fp = ctypes.c_void_p, ctypes.c_int, ctypes.c_uint32, ctypes.c_size_t, ctypes.c_void_p
    L.ptmi_version.restype = i32
    L.ptmi_status_string.restype = ctypes.c_char_p
    L.ptmi_status_string.argtypes = [i32]
    L.ptmi_last_error.restype = ctypes.c_char_p
    L.ptmi_last_error.argtypes = [vp]
    L.ptmi_create.argtypes = [ctypes.POINTER(vp), i32]
    L.ptmi_create_multi.argtypes = [ctypes.POINTER(vp), ctypes.POINTER(ctypes.c_int), i32]
    L.ptmi_prepare.argtypes = [vp]
    L.ptmi_destroy.argtypes = [vp]
    L.ptmi_destroy.restype = None
    L.ptmi_default_params.argtypes = [ctypes.POINTER(Params)]
    L.ptmi_default_params.restype = None
    L.ptmi_set_params.argtypes = [vp, ctypes.POINTER(Params)]
    L.ptmi_get_params.argtypes = [vp, ctypes.POINTER(Params)]
    L.ptmi_upload.argtypes = [vp, i32, fp, sz]
    L.ptmi_resize.argtypes = [vp, i32, i32]
    L.ptmi_clear_framebuffer.argtypes = [vp]
    L.ptmi_set_shard.argtypes = [vp, i32, i32, i32]
    L.ptmi_render_frame.argtypes = [vp, fp]
    L.ptmi_render.argtypes = [vp, fp, u32, u32]
    L.ptmi_synchronize.argtypes = [vp]
    L.ptmi_read_framebuffer.argtypes = [vp, fp, sz]
    L.ptmi_write_framebuffer.argtypes = [vp, fp, sz]
    L.ptmi_reduce_framebuffer.argtypes = [vp]
    L.ptmi_framebuffer_device_ptr.argtypes = [vp, ctypes.POINTER(vp), ctypes.POINTER(sz)]
    L.ptmi_bind_framebuffer.argtypes = [vp, vp, sz]
    L.ptmi_stream.argtypes = [vp, ctypes.POINTER(vp)]
    L.ptmi_resolve_rgba8.argtypes = [vp, ctypes.c_float, fp, sz]
    L.ptmi_set_counters.argtypes = [vp, i32]
    if hasattr(L, "ptmi_set_onb_table"):  # (an older A/B build loaded through PTMI_LIB lacks it)
        L.ptmi_set_onb_table.argtypes = [vp, i32]
    L.ptmi_set_timing.argtypes = [vp, i32]
    L.ptmi_get_stats.argtypes = [vp, ctypes.POINTER(Stats)]
    L.ptmi_reset_stats.argtypes = [vp]
    L.ptmi_trace.argtypes = [vp, sz, fp, fp, fp]
    L.ptmi_math_eval.argtypes = [vp, i32, sz, fp, fp, fp]
    if hasattr(L, "ptmi_selftest"):  # (an older A/B build loaded through PTMI_LIB may lack the newest test hooks)
        L.ptmi_selftest.argtypes = [vp, i32, ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(ctypes.c_uint32)]
    L.ptmi_build_bvh.argtypes = [sz, fp, fp, i32, fp, fp]
    L.ptmi_build_bvh_sah.argtypes = [sz, fp, fp, i32, fp, fp, ctypes.POINTER(sz)]
    L.ptmi_build_bvh_device.argtypes = [vp, sz, fp, fp, i32, fp, fp]
    if hasattr(L, "ptmi_check_bvh_boxes"):  # (an older A/B build loaded through PTMI_LIB has no stated domain)
        L.ptmi_check_bvh_boxes.argtypes = [sz, fp, fp, i32, ctypes.c_char_p, sz]
    L.ptmi_build_scene_bvh.argtypes = [vp]
    L.ptmi_build_scene_bvh_sah.argtypes = [vp]
    L.ptmi_scene_bvh_info.argtypes = [vp, ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_int32)]
    L.ptmi_build_bvh_sah_device.argtypes = [vp, sz, fp, fp, i32, fp, fp, ctypes.POINTER(sz)]
    L.ptmi_read_scene_buffer.argtypes = [vp, i32, fp, sz]
    L.ptmi_obj_parse.argtypes = [ctypes.c_char_p, sz, ctypes.POINTER(vp), ctypes.POINTER(sz), ctypes.POINTER(vp), ctypes.POINTER(sz)]
    L.ptmi_free.argtypes = [vp]
    L.ptmi_free.restype = None
    L.ptmi_device_count.restype = i32
    L.ptmi_reduce_info.restype = ctypes.c_char_p
    L.ptmi_reduce_info.argtypes = [vp]
    L.ptmi_reload_tuning.argtypes = [vp]
    if hasattr(L, "ptmi_render_views"):  # (an older A/B build loaded through PTMI_LIB renders one view per call)
        L.ptmi_render_views.argtypes = [vp, fp, u32, u32, u32, i32]
        L.ptmi_read_view.argtypes = [vp, u32, fp, sz]
        L.ptmi_resolve_view_rgba8.argtypes = [vp, u32, ctypes.c_float, fp, sz]
        L.ptmi_views_device_ptr.argtypes = [vp, ctypes.POINTER(vp), ctypes.POINTER(sz), ctypes.POINTER(u32)]
        L.ptmi_release_views.argtypes = [vp]
    if hasattr(L, "ptmi_render_aov"):  # (an older A/B build loaded through PTMI_LIB has no feature pass)
        L.ptmi_render_aov.argtypes = [vp, fp, u32, u32, u32, i32]
        L.ptmi_read_aov.argtypes = [vp, u32, i32, fp, sz]
        L.ptmi_aov_device_ptr.argtypes = [vp, ctypes.POINTER(vp), ctypes.POINTER(sz), ctypes.POINTER(u32)]
        L.ptmi_release_aov.argtypes = [vp]
        L.ptmi_camera_rays.argtypes = [vp, fp, u32, fp, fp]
    if hasattr(L, "ptmi_denoise_views"):  # (an older A/B build loaded through PTMI_LIB has no denoiser)
        dp = ctypes.POINTER(DenoiseParams)
        L.ptmi_default_denoise_params.argtypes = [dp]
        L.ptmi_default_denoise_params.restype = None
        L.ptmi_denoise_views.argtypes = [vp, dp, ctypes.c_float, u32, u32]
        L.ptmi_read_denoised.argtypes = [vp, u32, fp, sz]
        L.ptmi_resolve_denoised_rgba8.argtypes = [vp, u32, fp, sz]
        L.ptmi_denoised_device_ptr.argtypes = [vp, ctypes.POINTER(vp), ctypes.POINTER(sz), ctypes.POINTER(u32)]
        L.ptmi_release_denoised.argtypes = [vp]
        L.ptmi_denoise_images.argtypes = [vp, fp, fp, i32, i32, u32, ctypes.c_float, dp, fp]
        L.ptmi_denoise_reference.argtypes = [fp, fp, i32, i32, u32, ctypes.c_float, dp, fp]
    if hasattr(L, "ptmi_denoise_views_guided"):  # (an older A/B build loaded through PTMI_LIB has no variance-guided filter)
        gp = ctypes.POINTER(GuidedParams)
        L.ptmi_default_guided_params.argtypes = [gp]
        L.ptmi_default_guided_params.restype = None
        L.ptmi_denoise_views_guided.argtypes = [vp, gp, ctypes.c_float, u32, u32]
        L.ptmi_denoise_images_guided.argtypes = [vp, fp, fp, fp, i32, i32, u32, ctypes.c_float, gp, fp, fp]
        L.ptmi_denoise_guided_reference.argtypes = [fp, fp, fp, i32, i32, u32, ctypes.c_float, gp, fp, fp]
    if hasattr(L, "ptmi_fuse_views"):  # (an older A/B build loaded through PTMI_LIB has no cross-view fusion)
        up = ctypes.POINTER(FuseParams)
        L.ptmi_default_fuse_params.argtypes = [up]
        L.ptmi_default_fuse_params.restype = None
        L.ptmi_fuse_views.argtypes = [vp, up, fp, ctypes.c_float, i32, u32, u32]
        L.ptmi_read_fused.argtypes = [vp, u32, fp, sz]
        L.ptmi_resolve_fused_rgba8.argtypes = [vp, u32, fp, sz]
        L.ptmi_fused_device_ptr.argtypes = [vp, ctypes.POINTER(vp), ctypes.POINTER(sz), ctypes.POINTER(u32)]
        L.ptmi_release_fused.argtypes = [vp]
        L.ptmi_fuse_images.argtypes = [vp, fp, fp, fp, i32, i32, u32, ctypes.c_float, ctypes.c_float, fp, u32, up, fp]
        L.ptmi_fuse_reference.argtypes = [fp, fp, fp, i32, i32, u32, ctypes.c_float, ctypes.c_float, fp, u32, up, fp]
    if hasattr(L, "ptmi_accumulate_views"):  # (an older A/B build loaded through PTMI_LIB has no temporal accumulation)
        ap, gp = ctypes.POINTER(AccumulateParams), ctypes.POINTER(GuidedParams)
        L.ptmi_default_accumulate_params.argtypes = [ap]
        L.ptmi_default_accumulate_params.restype = None
        L.ptmi_accumulate_views.argtypes = [vp, ap, fp, ctypes.c_float, u32, u32, i32]
        L.ptmi_read_accumulated.argtypes = [vp, u32, i32, fp, sz]
        L.ptmi_resolve_accumulated_rgba8.argtypes = [vp, u32, fp, sz]
        L.ptmi_accumulated_device_ptr.argtypes = [vp, ctypes.POINTER(vp), ctypes.POINTER(sz), ctypes.POINTER(u32)]
        L.ptmi_release_accumulated.argtypes = [vp]
        L.ptmi_accumulate_images.argtypes = [vp, fp, fp, fp, fp, i32, i32, u32, ctypes.c_float, ctypes.c_float, fp, u32, ap, fp, fp]
        L.ptmi_accumulate_reference.argtypes = [fp, fp, fp, fp, i32, i32, u32, ctypes.c_float, ctypes.c_float, fp, u32, ap, fp, fp, i32]
        L.ptmi_denoise_views_accumulated.argtypes = [vp, gp, u32, u32]
        L.ptmi_denoise_images_accumulated.argtypes = [vp, fp, fp, fp, i32, i32, u32, gp, fp, fp]
        L.ptmi_denoise_accumulated_reference.argtypes = [fp, fp, fp, i32, i32, u32, gp, fp, fp, i32]
    if hasattr(L, "ptmi_set_view_moments"):  # (an older A/B build loaded through PTMI_LIB keeps no second moments)
        qp = ctypes.POINTER(NoiseParams)
        L.ptmi_set_view_moments.argtypes = [vp, i32]
        L.ptmi_read_moments.argtypes = [vp, u32, fp, sz]
        L.ptmi_moments_device_ptr.argtypes = [vp, ctypes.POINTER(vp), ctypes.POINTER(sz), ctypes.POINTER(u32)]
        L.ptmi_release_moments.argtypes = [vp]
        L.ptmi_default_noise_params.argtypes = [qp]
        L.ptmi_default_noise_params.restype = None
        L.ptmi_view_noise_stats.argtypes = [vp, qp, u32, u32, fp]
        L.ptmi_noise_images.argtypes = [vp, fp, fp, i32, i32, u32, qp, fp, fp]
        L.ptmi_noise_reference.argtypes = [fp, fp, i32, i32, u32, qp, fp, fp]
        L.ptmi_render_views_until.argtypes = [vp, fp, u32, u32, u32, u32, qp, ctypes.c_float, ctypes.POINTER(u32), fp]
    if hasattr(L, "ptmi_render_views_frames"):  # (an older A/B build loaded through PTMI_LIB gives every view the same frame numbers)
        up = ctypes.POINTER(u32)
        L.ptmi_render_views_frames.argtypes = [vp, fp, u32, fp, fp, i32]
        L.ptmi_render_aov_frames.argtypes = [vp, fp, u32, fp, fp, i32]
        L.ptmi_render_views_until_each.argtypes = [vp, fp, u32, fp, u32, u32, ctypes.POINTER(NoiseParams), ctypes.c_float, fp, fp]
        L.ptmi_view_slot_plan.argtypes = [u32, fp, fp, fp, sz, up]
    if hasattr(L, "ptmi_denoise_views_frames"):  # (an older A/B build loaded through PTMI_LIB takes one frame_num per call)
        dp, gp, up, ap = ctypes.POINTER(DenoiseParams), ctypes.POINTER(GuidedParams), ctypes.POINTER(FuseParams), ctypes.POINTER(AccumulateParams)
        L.ptmi_denoise_views_frames.argtypes = [vp, dp, fp, u32, u32]
        L.ptmi_denoise_views_guided_frames.argtypes = [vp, gp, fp, u32, u32]
        L.ptmi_fuse_views_frames.argtypes = [vp, up, fp, fp, u32, u32]
        L.ptmi_accumulate_views_frames.argtypes = [vp, ap, fp, fp, u32, u32, i32]
        L.ptmi_denoise_images_frames.argtypes = [vp, fp, fp, i32, i32, u32, fp, dp, fp]
        L.ptmi_denoise_images_guided_frames.argtypes = [vp, fp, fp, fp, i32, i32, u32, fp, gp, fp, fp]
        L.ptmi_fuse_images_frames.argtypes = [vp, fp, fp, fp, i32, i32, u32, fp, ctypes.c_float, fp, u32, up, fp]
        L.ptmi_accumulate_images_frames.argtypes = [vp, fp, fp, fp, fp, i32, i32, u32, fp, ctypes.c_float, fp, u32, ap, fp, fp]
        L.ptmi_denoise_reference_frames.argtypes = [fp, fp, i32, i32, u32, fp, dp, fp]
        L.ptmi_denoise_guided_reference_frames.argtypes = [fp, fp, fp, i32, i32, u32, fp, gp, fp, fp]
        L.ptmi_fuse_reference_frames.argtypes = [fp, fp, fp, i32, i32, u32, fp, ctypes.c_float, fp, u32, up, fp]
        L.ptmi_accumulate_reference_frames.argtypes = [fp, fp, fp, fp, i32, i32, u32, fp, ctypes.c_float, fp, u32, ap, fp, fp, i32]
    if hasattr(L, "ptmi_denoise_views_counts"):  # (an older A/B build loaded through PTMI_LIB takes one divisor per call or per view)
        dp, gp, up, ap = ctypes.POINTER(DenoiseParams), ctypes.POINTER(GuidedParams), ctypes.POINTER(FuseParams), ctypes.POINTER(AccumulateParams)
        L.ptmi_denoise_views_counts.argtypes = [vp, dp, u32, u32]
        L.ptmi_denoise_views_guided_counts.argtypes = [vp, gp, u32, u32]
        L.ptmi_fuse_views_counts.argtypes = [vp, up, fp, u32, u32]
        L.ptmi_accumulate_views_counts.argtypes = [vp, ap, fp, u32, u32, i32]
        L.ptmi_denoise_images_counts.argtypes = [vp, fp, fp, i32, i32, u32, fp, dp, fp]
        L.ptmi_denoise_images_guided_counts.argtypes = [vp, fp, fp, fp, i32, i32, u32, gp, fp, fp]
        L.ptmi_fuse_images_counts.argtypes = [vp, fp, fp, fp, i32, i32, u32, fp, ctypes.c_float, fp, u32, up, fp]
        L.ptmi_accumulate_images_counts.argtypes = [vp, fp, fp, fp, fp, i32, i32, u32, ctypes.c_float, fp, u32, ap, fp, fp]
        L.ptmi_denoise_reference_counts.argtypes = [fp, fp, i32, i32, u32, fp, dp, fp]
        L.ptmi_denoise_guided_reference_counts.argtypes = [fp, fp, fp, i32, i32, u32, gp, fp, fp]
        L.ptmi_fuse_reference_counts.argtypes = [fp, fp, fp, i32, i32, u32, fp, ctypes.c_float, fp, u32, up, fp]
        L.ptmi_accumulate_reference_counts.argtypes = [fp, fp, fp, fp, i32, i32, u32, ctypes.c_float, fp, u32, ap, fp, fp, i32]
    if hasattr(L, "ptmi_refit_scene_bvh"):  # (an older A/B build loaded through PTMI_LIB rebuilds a stale tree)
        L.ptmi_refit_bvh.argtypes = [sz, fp, fp, fp, sz]
        L.ptmi_refit_scene_bvh.argtypes = [vp]
    if hasattr(L, "ptmi_accumulate_views_motion"):  # (an older A/B build loaded through PTMI_LIB accumulates through a static world)
        ap = ctypes.POINTER(AccumulateParams)
        L.ptmi_accumulate_views_motion.argtypes = [vp, ap, fp, fp, fp, u32, u32, u32, i32]
        L.ptmi_accumulate_images_motion.argtypes = [vp, fp, fp, fp, fp, i32, i32, u32, fp, fp, u32, fp, ctypes.c_float, fp, u32, ap, fp, fp]
        L.ptmi_accumulate_reference_motion.argtypes = [fp, fp, fp, fp, i32, i32, u32, fp, fp, u32, fp, ctypes.c_float, fp, u32, ap, fp, fp, i32]
        L.ptmi_object_ids_reference.argtypes = [fp, i32, i32, u32, fp, u32, fp, u32, fp, u32, fp, u32, fp]
        L.ptmi_motions_from_transforms.argtypes = [fp, fp, u32, fp]
    if hasattr(L, "ptmi_fuse_views_motion"):  # (an older A/B build loaded through PTMI_LIB fuses through a static world)
        up = ctypes.POINTER(FuseParams)
        L.ptmi_fuse_views_motion.argtypes = [vp, up, fp, fp, fp, u32, i32, u32, u32]
        L.ptmi_fuse_images_motion.argtypes = [vp, fp, fp, fp, i32, i32, u32, fp, fp, u32, fp, ctypes.c_float, fp, u32, up, fp]
        L.ptmi_fuse_reference_motion.argtypes = [fp, fp, fp, i32, i32, u32, fp, fp, u32, fp, ctypes.c_float, fp, u32, up, fp, fp]
        L.ptmi_compose_motions.argtypes = [fp, u32, u32, u32, u32, fp]
    if hasattr(L, "ptmi_fuse_views_deform"):  # (an older A/B build loaded through PTMI_LIB fuses no deforming mesh)
        up = ctypes.POINTER(FuseParams)
        L.ptmi_fuse_views_deform.argtypes = [vp, up, fp, fp, fp, u32, i32, u32, u32]
        L.ptmi_fuse_images_deform.argtypes = [vp, fp, fp, fp, i32, i32, u32, fp, fp, u32, fp, u32, fp, u32, fp, u32, fp, ctypes.c_float, fp, u32, up, fp]
        L.ptmi_fuse_reference_deform.argtypes = [fp, fp, fp, i32, i32, u32, fp, fp, u32, fp, u32, fp, u32, fp, u32, fp, ctypes.c_float, fp, u32, up, fp, fp, i32]
        L.ptmi_fuse_deform_records.argtypes = [fp, u32, fp, fp]
    if hasattr(L, "ptmi_accumulate_images_deform"):  # (an older A/B build loaded through PTMI_LIB knows rigid motions alone)
        ap = ctypes.POINTER(AccumulateParams)
        L.ptmi_accumulate_images_deform.argtypes = [vp, fp, fp, fp, fp, i32, i32, u32, fp, fp, u32, fp, u32, fp, u32, fp, u32, fp, ctypes.c_float, fp, u32, ap, fp, fp]
        L.ptmi_accumulate_reference_deform.argtypes = [fp, fp, fp, fp, i32, i32, u32, fp, fp, u32, fp, u32, fp, u32, fp, u32, fp, ctypes.c_float, fp, u32, ap, fp, fp, i32]
        L.ptmi_deform_records.argtypes = [fp, fp, u32, fp, fp]
        L.ptmi_capture_view_geometry.argtypes = [vp, u32, u32]
        L.ptmi_read_view_geometry.argtypes = [vp, u32, fp, sz, fp, sz]
        L.ptmi_geometry_device_ptr.argtypes = [vp, ctypes.POINTER(ctypes.c_void_p), ctypes.POINTER(ctypes.c_void_p), ctypes.POINTER(ctypes.c_uint32),
                                               ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(ctypes.c_uint64)]
        L.ptmi_release_geometry.argtypes = [vp]
        L.ptmi_accumulate_views_deform.argtypes = [vp, ap, fp, fp, fp, u32, u32, u32, i32]
    if hasattr(L, "ptmi_render_view_runs"):  # (an older A/B build loaded through PTMI_LIB renders whole views)
        qp = ctypes.POINTER(NoiseParams)
        L.ptmi_render_view_runs.argtypes = [vp, fp, u32, u32, u32, fp, u32]
        L.ptmi_view_run_noise.argtypes = [vp, qp, ctypes.c_float, u32, u32, fp, fp, fp]
        L.ptmi_run_noise_images.argtypes = [vp, fp, fp, i32, i32, u32, qp, ctypes.c_float, fp, fp, fp]
        L.ptmi_run_noise_reference.argtypes = [fp, fp, i32, i32, u32, qp, ctypes.c_float, fp, fp, fp]
        L.ptmi_render_views_until_runs.argtypes = [vp, fp, u32, fp, u32, u32, u32, qp, ctypes.c_float, fp, fp, ctypes.POINTER(ctypes.c_uint64)]
        L.ptmi_read_view_mean.argtypes = [vp, u32, fp, sz]
        L.ptmi_resolve_view_mean_rgba8.argtypes = [vp, u32, fp, sz]
    if hasattr(L, "ptmi_render_views_runs"):  # (an older A/B build loaded through PTMI_LIB renders one view's runs per batch)
        qp = ctypes.POINTER(NoiseParams)
        L.ptmi_render_views_runs.argtypes = [vp, fp, u32, fp, u32, fp, fp, u32]
        L.ptmi_run_refs_reference.argtypes = [u32, u32, fp, fp, fp, fp]
        L.ptmi_run_refs_images.argtypes = [vp, fp, fp, i32, i32, u32, qp, ctypes.c_float, fp, fp]
    if explicit:
        _libs[path] = L
    else:
        _lib = L
    return L


def _ptr(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def _frame_arrays(n_views, first_frames, frame_counts):
    """The per-view u32 arrays of the calls with per-view frame ranges; a scalar stands for every view."""
    f = np.ascontiguousarray(np.broadcast_to(np.asarray(first_frames, np.uint32), (n_views,)))
    k = np.ascontiguousarray(np.broadcast_to(np.asarray(frame_counts, np.uint32), (n_views,)))
    return f, k


def _frame_nums(frame_nums, n):
    """The per-view f32 divisors of the *_frames consumers: any sequence of n numbers — render_views_until_each's frames_done as it is; None stays a null pointer,
    which the library refuses."""
    if frame_nums is None:
        return None
    f = np.ascontiguousarray(frame_nums, np.float32).reshape(-1)
    assert f.size == n, "frame_nums: one count per view, %d of them" % n
    return f


def _optr(a):
    return None if a is None else _ptr(a)


def _pixel_counts(counts, shape):
    """The per-pixel f32 divisors of the plain and fuse *_counts forms, (n, H, W) — a moment stack's [..., 3] as it is; None stays a null pointer, which the library
    refuses."""
    if counts is None:
        return None
    k = np.ascontiguousarray(counts, np.float32)
    assert k.size == int(np.prod(shape)), "counts: one count per pixel, (n, H, W) = %r" % (tuple(shape),)
    return k.reshape(shape)


def view_slot_plan(first_frames, frame_counts):
    """Test hook, no GPU (ptmi_view_slot_plan): the slot table render_views_frames uploads for these per-view first frame numbers and frame counts, as
    (records (V, 4) uint32 — first slot, count, first frame, next view with a frame —, view_of_slot (n_slots,) uint32).  Raises PtmiError where the call would."""
    lib = load_library()
    k = np.ascontiguousarray(frame_counts, np.uint32)
    f = np.ascontiguousarray(first_frames, np.uint32)
    assert f.shape == k.shape and f.ndim == 1
    n = ctypes.c_uint32()
    st = lib.ptmi_view_slot_plan(k.size, _ptr(f), _ptr(k), None, 0, ctypes.byref(n))
    if st:
        raise PtmiError(st, "ptmi_view_slot_plan")
    table = np.zeros(4 * k.size + n.value, np.uint32)
    st = lib.ptmi_view_slot_plan(k.size, _ptr(f), _ptr(k), _ptr(table), table.size, None)
    if st:
        raise PtmiError(st, "ptmi_view_slot_plan")
    return table[:4 * k.size].reshape(-1, 4), table[4 * k.size:]


def default_params(**kw):
    p = Params()
    load_library().ptmi_default_params(ctypes.byref(p))
    for k, v in kw.items():
        if k == "background":
            p.background[:] = list(v)
        else:
            setattr(p, k, v)
    return p


def default_denoise_params(lib=None, **kw):
    """ptmi_default_denoise_params (levels 5, sigma_normal 0.25, sigma_depth 0.1, sigma_colour 0 = off, albedo_floor 1e-3) with fields replaced by keyword."""
    p = DenoiseParams()
    (lib or load_library()).ptmi_default_denoise_params(ctypes.byref(p))
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def _denoise_arrays(colour_sums, layers):
    c = np.ascontiguousarray(colour_sums, np.float32)
    if c.ndim == 3:
        c = c[None]
    n, h, w = c.shape[:3]
    l = np.ascontiguousarray(layers, np.float32).reshape(n, 3, h, w, 4)
    assert c.shape == (n, h, w, 4), "colour_sums: (n, H, W, 4) float32, layers: (n, 3, H, W, 4)"
    return c, l, np.empty((n, h, w, 4), np.float32)


def denoise_reference(colour_sums, layers, frame_num, params=None, lib=None):
    """ptmi_denoise_reference: the denoising filter of Context.denoise_views on host arrays, on the CPU (no GPU needed) — colour_sums (n, H, W, 4) RGBA sums,
    layers (n, 3, H, W, 4) as Context.read_aov gives them; returns (n, H, W, 4) mean radiance, the kernels' bits."""
    c, l, out = _denoise_arrays(colour_sums, layers)
    st = (lib or load_library()).ptmi_denoise_reference(_ptr(c), _ptr(l), c.shape[2], c.shape[1], c.shape[0], float(frame_num), None if params is None else ctypes.byref(params), _ptr(out))
    if st != 0:
        raise PtmiError(st, "ptmi_denoise_reference failed")
    return out


def denoise_reference_frames(colour_sums, layers, frame_nums, params=None, lib=None):
    """ptmi_denoise_reference_frames: denoise_reference with one frame count per image, frame_nums (n,): image v's sums are divided by frame_nums[v]."""
    c, l, out = _denoise_arrays(colour_sums, layers)
    f = _frame_nums(frame_nums, c.shape[0])
    st = (lib or load_library()).ptmi_denoise_reference_frames(_ptr(c), _ptr(l), c.shape[2], c.shape[1], c.shape[0], _optr(f), None if params is None else ctypes.byref(params), _ptr(out))
    if st != 0:
        raise PtmiError(st, "ptmi_denoise_reference_frames failed")
    return out


def denoise_reference_counts(colour_sums, layers, counts, params=None, lib=None):
    """ptmi_denoise_reference_counts: denoise_reference with one frame count per PIXEL, counts (n, H, W): every pixel's sums are divided by its own count (a moment
    stack's M.w).  A count of 0 is no special case: the division's NaN or inf makes the pixel invalid."""
    c, l, out = _denoise_arrays(colour_sums, layers)
    k = _pixel_counts(counts, c.shape[:3])
    st = (lib or load_library()).ptmi_denoise_reference_counts(_ptr(c), _ptr(l), c.shape[2], c.shape[1], c.shape[0], _optr(k), None if params is None else ctypes.byref(params), _ptr(out))
    if st != 0:
        raise PtmiError(st, "ptmi_denoise_reference_counts failed")
    return out


def default_guided_params(lib=None, **kw):
    """ptmi_default_guided_params (levels 5, sigma_normal 0.25, sigma_depth 0.1, sigma_luma 4, albedo_floor 1e-3, min_frames 4, var_eps 1e-10) with fields replaced
    by keyword."""
    p = GuidedParams()
    (lib or load_library()).ptmi_default_guided_params(ctypes.byref(p))
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def _guided_arrays(colour_sums, moments, layers, want_var):
    c, l, out = _denoise_arrays(colour_sums, layers)
    m = np.ascontiguousarray(moments, np.float32).reshape(c.shape)
    return c, m, l, out, (np.empty(c.shape[:3], np.float32) if want_var else None)


def denoise_guided_reference(colour_sums, moments, layers, frame_num, params=None, want_var=False, lib=None):
    """ptmi_denoise_guided_reference: the variance-guided filter of Context.denoise_views_guided on host arrays, on the CPU (no GPU needed) — colour_sums and moments
    (n, H, W, 4) as Context.read_view and Context.read_moments give them, layers (n, 3, H, W, 4) as Context.read_aov gives them; returns (n, H, W, 4) mean radiance,
    the kernels' bits — and, with want_var, (radiance, var): var (n, H, W) float32, the final filtered variance, NaN on invalid pixels."""
    c, m, l, out, var = _guided_arrays(colour_sums, moments, layers, want_var)
    st = (lib or load_library()).ptmi_denoise_guided_reference(_ptr(c), _ptr(m), _ptr(l), c.shape[2], c.shape[1], c.shape[0], float(frame_num),
                                                               None if params is None else ctypes.byref(params), _ptr(out), None if var is None else _ptr(var))
    if st != 0:
        raise PtmiError(st, "ptmi_denoise_guided_reference failed")
    return (out, var) if want_var else out


def denoise_guided_reference_frames(colour_sums, moments, layers, frame_nums, params=None, want_var=False, lib=None):
    """ptmi_denoise_guided_reference_frames: denoise_guided_reference with one frame count per image, frame_nums (n,)."""
    c, m, l, out, var = _guided_arrays(colour_sums, moments, layers, want_var)
    f = _frame_nums(frame_nums, c.shape[0])
    st = (lib or load_library()).ptmi_denoise_guided_reference_frames(_ptr(c), _ptr(m), _ptr(l), c.shape[2], c.shape[1], c.shape[0], _optr(f),
                                                                      None if params is None else ctypes.byref(params), _ptr(out), _optr(var))
    if st != 0:
        raise PtmiError(st, "ptmi_denoise_guided_reference_frames failed")
    return (out, var) if want_var else out


def denoise_guided_reference_counts(colour_sums, moments, layers, params=None, want_var=False, lib=None):
    """ptmi_denoise_guided_reference_counts: denoise_guided_reference with every pixel's own frame count, the w of its moments."""
    c, m, l, out, var = _guided_arrays(colour_sums, moments, layers, want_var)
    st = (lib or load_library()).ptmi_denoise_guided_reference_counts(_ptr(c), _ptr(m), _ptr(l), c.shape[2], c.shape[1], c.shape[0],
                                                                      None if params is None else ctypes.byref(params), _ptr(out), _optr(var))
    if st != 0:
        raise PtmiError(st, "ptmi_denoise_guided_reference_counts failed")
    return (out, var) if want_var else out


def default_fuse_params(lib=None, **kw):
    """ptmi_default_fuse_params (radius 4, sigma_normal 0.25, sigma_depth 0.1, albedo_floor 1e-3) with fields replaced by keyword."""
    p = FuseParams()
    (lib or load_library()).ptmi_default_fuse_params(ctypes.byref(p))
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def _fuse_arrays(colour, layers, views, lambertian):
    c, l, out = _denoise_arrays(colour, layers)
    v = np.ascontiguousarray(views, np.float32).reshape(-1, 16)
    assert v.shape[0] == c.shape[0], "views: one (16,) column-major matrix per image"
    t = None if lambertian is None else np.ascontiguousarray(np.asarray(lambertian) != 0, np.uint8).reshape(-1)
    return c, l, v, t, out


def fuse_reference(colour, layers, views, frame_num, fov_degrees=60.0, lambertian=None, params=None, lib=None):
    """ptmi_fuse_reference: the cross-view fusion of Context.fuse_views on host arrays, on the CPU (no GPU needed) — colour (n, H, W, 4) RGBA sums of `frame_num`
    frames, layers (n, 3, H, W, 4) as Context.read_aov gives them, views (n, 16); lambertian: one truth value per material index (None: every material fuses).
    Returns (n, H, W, 4) mean radiance, the kernel's bits."""
    c, l, v, t, out = _fuse_arrays(colour, layers, views, lambertian)
    st = (lib or load_library()).ptmi_fuse_reference(_ptr(c), _ptr(l), _ptr(v), c.shape[2], c.shape[1], c.shape[0], float(frame_num), float(fov_degrees),
                                                     None if t is None else _ptr(t), 0 if t is None else t.size, None if params is None else ctypes.byref(params), _ptr(out))
    if st != 0:
        raise PtmiError(st, "ptmi_fuse_reference failed")
    return out


def fuse_reference_frames(colour, layers, views, frame_nums, fov_degrees=60.0, lambertian=None, params=None, lib=None):
    """ptmi_fuse_reference_frames: fuse_reference with one frame count per image, frame_nums (n,): the output view's own count divides its pixel and the output, a
    neighbour view's count the pixel looked up in it."""
    c, l, v, t, out = _fuse_arrays(colour, layers, views, lambertian)
    f = _frame_nums(frame_nums, c.shape[0])
    st = (lib or load_library()).ptmi_fuse_reference_frames(_ptr(c), _ptr(l), _ptr(v), c.shape[2], c.shape[1], c.shape[0], _optr(f), float(fov_degrees),
                                                            _optr(t), 0 if t is None else t.size, None if params is None else ctypes.byref(params), _ptr(out))
    if st != 0:
        raise PtmiError(st, "ptmi_fuse_reference_frames failed")
    return out


def fuse_reference_counts(colour, layers, views, counts, fov_degrees=60.0, lambertian=None, params=None, lib=None):
    """ptmi_fuse_reference_counts: fuse_reference with one frame count per PIXEL, counts (n, H, W): the output pixel takes its own count, the pixel sampled in a
    neighbour view that pixel's."""
    c, l, v, t, out = _fuse_arrays(colour, layers, views, lambertian)
    k = _pixel_counts(counts, c.shape[:3])
    st = (lib or load_library()).ptmi_fuse_reference_counts(_ptr(c), _ptr(l), _ptr(v), c.shape[2], c.shape[1], c.shape[0], _optr(k), float(fov_degrees),
                                                            _optr(t), 0 if t is None else t.size, None if params is None else ctypes.byref(params), _ptr(out))
    if st != 0:
        raise PtmiError(st, "ptmi_fuse_reference_counts failed")
    return out


def default_accumulate_params(lib=None, **kw):
    """ptmi_default_accumulate_params (max_history 32, min_frames 4, sigma_normal 0.25, sigma_depth 0.1, albedo_floor 1e-3) with fields replaced by keyword."""
    p = AccumulateParams()
    (lib or load_library()).ptmi_default_accumulate_params(ctypes.byref(p))
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def _accumulate_arrays(colour_sums, moments, layers, views, lambertian, history):
    c, l, v, t, _ = _fuse_arrays(colour_sums, layers, views, lambertian)
    m = np.ascontiguousarray(moments, np.float32).reshape(c.shape)
    hist = None if history is None else np.ascontiguousarray(history, np.float32).reshape((2,) + c.shape[1:])
    return c, m, l, v, t, hist, np.empty((3,) + c.shape, np.float32)


def accumulate_reference(colour_sums, moments, layers, views, frame_num, fov_degrees=60.0, lambertian=None, params=None, history=None, threads=1, lib=None):
    """ptmi_accumulate_reference: the temporal accumulation of Context.accumulate_views on host arrays, on the CPU (no GPU needed) — colour_sums and moments
    (n, H, W, 4) as Context.read_view and Context.read_moments give them, layers (n, 3, H, W, 4), views (n, 16); lambertian: one truth value per material index
    (None: every material accumulates).  history (2, H, W, 4): planes 1 and 2 that image 0 is taken to hold — image 0 is then the view before the first accumulated
    one (see ptmi_accumulate_images).  Returns (3, n, H, W, 4): the planes of the accumulated stack, the kernel's bits."""
    c, m, l, v, t, hist, out = _accumulate_arrays(colour_sums, moments, layers, views, lambertian, history)
    st = (lib or load_library()).ptmi_accumulate_reference(_ptr(c), _ptr(m), _ptr(l), _ptr(v), c.shape[2], c.shape[1], c.shape[0], float(frame_num), float(fov_degrees),
                                                           None if t is None else _ptr(t), 0 if t is None else t.size, None if params is None else ctypes.byref(params),
                                                           None if hist is None else _ptr(hist), _ptr(out), int(threads))
    if st != 0:
        raise PtmiError(st, "ptmi_accumulate_reference failed")
    return out


def accumulate_reference_frames(colour_sums, moments, layers, views, frame_nums, fov_degrees=60.0, lambertian=None, params=None, history=None, threads=1, lib=None):
    """ptmi_accumulate_reference_frames: accumulate_reference with one frame count per image, frame_nums (n,): view v's own count divides its sums, view v-1's the
    pixel looked up there (with `history`, image 0's entry serves that lookup)."""
    c, m, l, v, t, hist, out = _accumulate_arrays(colour_sums, moments, layers, views, lambertian, history)
    f = _frame_nums(frame_nums, c.shape[0])
    st = (lib or load_library()).ptmi_accumulate_reference_frames(_ptr(c), _ptr(m), _ptr(l), _ptr(v), c.shape[2], c.shape[1], c.shape[0], _optr(f), float(fov_degrees),
                                                                  _optr(t), 0 if t is None else t.size, None if params is None else ctypes.byref(params),
                                                                  _optr(hist), _ptr(out), int(threads))
    if st != 0:
        raise PtmiError(st, "ptmi_accumulate_reference_frames failed")
    return out


def accumulate_reference_counts(colour_sums, moments, layers, views, fov_degrees=60.0, lambertian=None, params=None, history=None, threads=1, lib=None):
    """ptmi_accumulate_reference_counts: accumulate_reference with every pixel's own frame count, the w of its moments: pixel p of view v divides by M.w of (v, p),
    the pixel q looked up in view v-1 by M.w of (v-1, q)."""
    c, m, l, v, t, hist, out = _accumulate_arrays(colour_sums, moments, layers, views, lambertian, history)
    st = (lib or load_library()).ptmi_accumulate_reference_counts(_ptr(c), _ptr(m), _ptr(l), _ptr(v), c.shape[2], c.shape[1], c.shape[0], float(fov_degrees),
                                                                  _optr(t), 0 if t is None else t.size, None if params is None else ctypes.byref(params),
                                                                  _optr(hist), _ptr(out), int(threads))
    if st != 0:
        raise PtmiError(st, "ptmi_accumulate_reference_counts failed")
    return out


def _motion_arrays(motions, object_ids, n, image_shape=None):
    """The motions (n, n_objects, 16) and, where the call takes them, the id images (n, H, W) of the *_motion calls; None stays a null pointer, which the library
    refuses.  Returns (motions, n_objects, object_ids)."""
    g = None if motions is None else np.ascontiguousarray(motions, np.float32).reshape(n, -1, 16)
    ids = None if object_ids is None else np.ascontiguousarray(object_ids, np.int32).reshape((n,) + tuple(image_shape))
    return g, 0 if g is None else g.shape[1], ids


def accumulate_reference_motion(colour_sums, moments, layers, views, frame_nums, motions, object_ids, fov_degrees=60.0, lambertian=None, params=None, history=None,
                                threads=1, n_objects=None, lib=None):
    """ptmi_accumulate_reference_motion: accumulate_reference_frames through a world whose objects move — motions (n, n_objects, 16): per image and object the
    column-major matrix that carries a world point of the object at the time of image v to the same material point at the time of image v-1 (image 0's are not
    read); object_ids (n, H, W) int32: every pixel's object, -1 = static (object_ids_reference).  n_objects: for a call with no motions array (tests)."""
    c, m, l, v, t, hist, out = _accumulate_arrays(colour_sums, moments, layers, views, lambertian, history)
    f = _frame_nums(frame_nums, c.shape[0])
    g, n_obj, ids = _motion_arrays(motions, object_ids, c.shape[0], c.shape[1:3])
    st = (lib or load_library()).ptmi_accumulate_reference_motion(_ptr(c), _ptr(m), _ptr(l), _ptr(v), c.shape[2], c.shape[1], c.shape[0], _optr(f), _optr(g),
                                                                  n_obj if n_objects is None else n_objects, _optr(ids), float(fov_degrees), _optr(t),
                                                                  0 if t is None else t.size, None if params is None else ctypes.byref(params), _optr(hist), _ptr(out),
                                                                  int(threads))
    if st != 0:
        raise PtmiError(st, "ptmi_accumulate_reference_motion failed")
    return out


def _deform_arrays(triangles_seq, transforms_seq, meshes, n):
    """The geometry of the *_deform calls: triangles (n, n_triangles, 24) and transforms (n, n_transforms, 32) float32, meshes (n_meshes, 4) int32; an empty transform
    or mesh table stays a null pointer.  Returns the argument run (triangles, n_triangles, transforms, n_transforms, meshes, n_meshes) and the arrays, to keep alive."""
    tr = np.ascontiguousarray(triangles_seq, np.float32).reshape(n, -1, 24)
    tf = None if transforms_seq is None or np.size(transforms_seq) == 0 else np.ascontiguousarray(transforms_seq, np.float32).reshape(n, -1, 32)
    me = None if meshes is None or np.size(meshes) == 0 else np.ascontiguousarray(meshes, np.int32).reshape(-1, 4)
    return [_ptr(tr), tr.shape[1], _optr(tf), 0 if tf is None else tf.shape[1], _optr(me), 0 if me is None else me.shape[0]], (tr, tf, me)


def accumulate_reference_deform(colour_sums, moments, layers, views, frame_nums, triangles_seq, transforms_seq, meshes, motions=None, object_ids=None, fov_degrees=60.0,
                                lambertian=None, params=None, history=None, threads=1, n_objects=None, lib=None):
    """ptmi_accumulate_reference_deform: accumulate_reference_motion through a world whose meshes DEFORM — triangles_seq (n, n_triangles, 24): every image's triangles
    in the order its layers were rendered in, the same order in all; transforms_seq (n, n_transforms, 32): every image's transform table; meshes (n_meshes, 4) int32.
    A triangle pixel whose indices count is carried from its triangle in image v to the same triangle in image v-1; every other pixel goes through motions /
    object_ids as accumulate_reference_motion's do (both None: a static world).  Image 0's geometry is read only as image 1's predecessor."""
    c, m, l, v, t, hist, out = _accumulate_arrays(colour_sums, moments, layers, views, lambertian, history)
    f = _frame_nums(frame_nums, c.shape[0])
    g, n_obj, ids = _motion_arrays(motions, object_ids, c.shape[0], c.shape[1:3])
    geo, keep = _deform_arrays(triangles_seq, transforms_seq, meshes, c.shape[0])
    st = (lib or load_library()).ptmi_accumulate_reference_deform(_ptr(c), _ptr(m), _ptr(l), _ptr(v), c.shape[2], c.shape[1], c.shape[0], _optr(f), *geo, _optr(g),
                                                                  n_obj if n_objects is None else n_objects, _optr(ids), float(fov_degrees), _optr(t),
                                                                  0 if t is None else t.size, None if params is None else ctypes.byref(params), _optr(hist), _ptr(out),
                                                                  int(threads))
    if st != 0:
        raise PtmiError(st, "ptmi_accumulate_reference_deform failed")
    return out


def deform_records(prev, cur, lib=None):
    """ptmi_deform_records: the records the *_deform calls make for one view, (n_transforms, 36) uint32 words (include/ptmi_deform.h, ptmdf_record), from the
    transform tables (n_transforms, 32) of the earlier view (prev) and the later one (cur).  PtmiError naming the object where an element read is not finite."""
    p = np.ascontiguousarray(prev, np.float32).reshape(-1, 32)
    c = np.ascontiguousarray(cur, np.float32).reshape(-1, 32)
    assert p.shape == c.shape, "prev and cur: the same number of transforms"
    out = np.zeros((p.shape[0], 36), np.uint32)
    bad = np.zeros(1, np.uint32)
    st = (lib or load_library()).ptmi_deform_records(_ptr(p), _ptr(c), p.shape[0], _ptr(out), _ptr(bad))
    if st != 0:
        raise PtmiError(st, "ptmi_deform_records failed: object %d" % int(bad[0]))
    return out


def object_ids_reference(layers, spheres=None, quads=None, triangles=None, meshes=None, lib=None):
    """ptmi_object_ids_reference: every pixel's object (global_id) from layer 2 of layers (n, 3, H, W, 4) and host copies of the scene buffers in their reference
    layouts — spheres (., 8), quads (., 20), triangles (., 24) float32 IN THE ORDER THE LAYERS WERE RENDERED IN (Context.read_scene_buffer(5, n)), meshes (., 4)
    int32; None: none of that kind.  Returns (n, H, W) int32, -1 where a pixel has no object."""
    l = np.ascontiguousarray(layers, np.float32)
    assert l.ndim == 5 and l.shape[1] == 3 and l.shape[4] == 4, "layers: (n, 3, H, W, 4)"
    arrs = [None if a is None or np.size(a) == 0 else np.ascontiguousarray(a, ty).reshape(-1, k)
            for a, ty, k in ((spheres, np.float32, 8), (quads, np.float32, 20), (triangles, np.float32, 24), (meshes, np.int32, 4))]
    out = np.empty((l.shape[0], l.shape[2], l.shape[3]), np.int32)
    args = []
    for a in arrs:
        args += [_optr(a), 0 if a is None else a.shape[0]]
    st = (lib or load_library()).ptmi_object_ids_reference(_ptr(l), l.shape[3], l.shape[2], l.shape[0], *args, _ptr(out))
    if st != 0:
        raise PtmiError(st, "ptmi_object_ids_reference failed")
    return out


def motions_from_transforms(prev, cur, lib=None):
    """ptmi_motions_from_transforms: the motions of one step, (n_objects, 16) float32, from the transform tables (n_objects, 32) of the earlier view (prev) and the
    later one (cur): model_prev . invModel_cur, the exact identity for an object whose two records are bytewise equal."""
    p = np.ascontiguousarray(prev, np.float32).reshape(-1, 32)
    c = np.ascontiguousarray(cur, np.float32).reshape(-1, 32)
    assert p.shape == c.shape, "prev and cur: the same number of objects"
    out = np.empty((p.shape[0], 16), np.float32)
    st = (lib or load_library()).ptmi_motions_from_transforms(_ptr(p), _ptr(c), p.shape[0], _ptr(out))
    if st != 0:
        raise PtmiError(st, "ptmi_motions_from_transforms failed")
    return out


def fuse_reference_motion(colour, layers, views, frame_nums, motions, object_ids, fov_degrees=60.0, lambertian=None, params=None, want_weight=False, n_objects=None,
                          lib=None):
    """ptmi_fuse_reference_motion: fuse_reference_frames through a world whose objects move — motions (n, n_objects, 16) as accumulate_reference_motion takes them
    (per image and object the matrix from the time of image v to the time of image v-1; composed across the window by the library); object_ids (n, H, W) int32,
    -1 = static.  want_weight: also return (n, H, W) float32, the summed weight (den) of every fused pixel, 0 where the pixel passes through."""
    c, l, v, t, out = _fuse_arrays(colour, layers, views, lambertian)
    f = _frame_nums(frame_nums, c.shape[0])
    g, n_obj, ids = _motion_arrays(motions, object_ids, c.shape[0], c.shape[1:3])
    wgt = np.empty(c.shape[:3], np.float32) if want_weight else None
    st = (lib or load_library()).ptmi_fuse_reference_motion(_ptr(c), _ptr(l), _ptr(v), c.shape[2], c.shape[1], c.shape[0], _optr(f), _optr(g),
                                                            n_obj if n_objects is None else n_objects, _optr(ids), float(fov_degrees), _optr(t), 0 if t is None else t.size,
                                                            None if params is None else ctypes.byref(params), _ptr(out), _optr(wgt))
    if st != 0:
        raise PtmiError(st, "ptmi_fuse_reference_motion failed")
    return (out, wgt) if want_weight else out


def fuse_reference_deform(colour, layers, views, frame_nums, triangles_seq, transforms_seq, meshes, motions=None, object_ids=None, fov_degrees=60.0, lambertian=None,
                          params=None, want_weight=False, threads=1, n_objects=None, lib=None):
    """ptmi_fuse_reference_deform: fuse_reference_motion through a world whose meshes DEFORM — triangles_seq (n, n_triangles, 24), transforms_seq (n, n_transforms, 32)
    and meshes (n_meshes, 4) int32 as accumulate_reference_deform takes them.  A triangle pixel whose indices count is carried from its triangle in image v to the
    same triangle in every image of its window; every other pixel goes through motions / object_ids as fuse_reference_motion's do (both None: a static world).
    want_weight: also return (n, H, W) float32, the summed weight of every fused pixel.  threads > 1 share a view's rows and change no bit."""
    c, l, v, t, out = _fuse_arrays(colour, layers, views, lambertian)
    f = _frame_nums(frame_nums, c.shape[0])
    g, n_obj, ids = _motion_arrays(motions, object_ids, c.shape[0], c.shape[1:3])
    geo, keep = _deform_arrays(triangles_seq, transforms_seq, meshes, c.shape[0])
    wgt = np.empty(c.shape[:3], np.float32) if want_weight else None
    st = (lib or load_library()).ptmi_fuse_reference_deform(_ptr(c), _ptr(l), _ptr(v), c.shape[2], c.shape[1], c.shape[0], _optr(f), *geo, _optr(g),
                                                            n_obj if n_objects is None else n_objects, _optr(ids), float(fov_degrees), _optr(t), 0 if t is None else t.size,
                                                            None if params is None else ctypes.byref(params), _ptr(out), _optr(wgt), int(threads))
    if st != 0:
        raise PtmiError(st, "ptmi_fuse_reference_deform failed")
    return (out, wgt) if want_weight else out


def fuse_deform_records(transforms, lib=None):
    """ptmi_fuse_deform_records: the records the fusion *_deform calls make for ONE view, (n_transforms, 24) uint32 words (include/ptmi_fuse_deform.h, ptmfd_record),
    from that view's transform table (n_transforms, 32).  PtmiError naming the object where an element read is not finite."""
    t = np.ascontiguousarray(transforms, np.float32).reshape(-1, 32)
    out = np.zeros((t.shape[0], 24), np.uint32)
    bad = np.zeros(1, np.uint32)
    st = (lib or load_library()).ptmi_fuse_deform_records(_ptr(t), t.shape[0], _ptr(out), _ptr(bad))
    if st != 0:
        raise PtmiError(st, "ptmi_fuse_deform_records failed: object %d" % int(bad[0]))
    return out


def compose_motions(motions, from_view, to_view, lib=None):
    """ptmi_compose_motions: the composed motion of every object from the time of view from_view to the time of view to_view, (n_objects, 16) float32, out of the
    per-step motions (n_views, n_objects, 16): what the *_motion fusion calls make their records from for that pair."""
    g = np.ascontiguousarray(motions, np.float32)
    assert g.ndim == 3 and g.shape[2] == 16, "motions: (n_views, n_objects, 16)"
    out = np.empty((g.shape[1], 16), np.float32)
    st = (lib or load_library()).ptmi_compose_motions(_ptr(g), g.shape[0], g.shape[1], int(from_view), int(to_view), _ptr(out))
    if st != 0:
        raise PtmiError(st, "ptmi_compose_motions failed")
    return out


def denoise_accumulated_reference(means, plane2, layers, params=None, want_var=False, threads=1, lib=None):
    """ptmi_denoise_accumulated_reference: the guided filter of Context.denoise_views_accumulated on host arrays, on the CPU (no GPU needed) — means and plane2
    (n, H, W, 4): planes 0 and 2 of an accumulated stack; layers (n, 3, H, W, 4).  Returns what denoise_guided_reference returns."""
    c, p2, l, out, var = _guided_arrays(means, plane2, layers, want_var)
    st = (lib or load_library()).ptmi_denoise_accumulated_reference(_ptr(c), _ptr(p2), _ptr(l), c.shape[2], c.shape[1], c.shape[0], None if params is None else ctypes.byref(params),
                                                                    _ptr(out), None if var is None else _ptr(var), int(threads))
    if st != 0:
        raise PtmiError(st, "ptmi_denoise_accumulated_reference failed")
    return (out, var) if want_var else out


def default_noise_params(lib=None, **kw):
    """ptmi_default_noise_params (floor 1e-2, threshold 0.05) with fields replaced by keyword."""
    p = NoiseParams()
    (lib or load_library()).ptmi_default_noise_params(ctypes.byref(p))
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def _noise_arrays(colour_sums, moments, want_map):
    c = np.ascontiguousarray(colour_sums, np.float32)
    if c.ndim == 3:
        c = c[None]
    n, h, w = c.shape[:3]
    m = np.ascontiguousarray(moments, np.float32).reshape(n, h, w, 4)
    assert c.shape == (n, h, w, 4), "colour_sums and moments: (n, H, W, 4) float32"
    return c, m, np.zeros(n, VIEW_NOISE_DTYPE), (np.empty((n, h, w), np.float32) if want_map else None)


def noise_reference(colour_sums, moments, params=None, want_map=False, lib=None):
    """ptmi_noise_reference: the noise statistic of Context.view_noise on host arrays, on the CPU (no GPU needed) — colour_sums (n, H, W, 4) as Context.read_view and
    moments (n, H, W, 4) as Context.read_moments give them.  Returns one VIEW_NOISE_DTYPE record per image (counted, sum_q, above, max_q: the kernel's integers) — and,
    with want_map, (records, map): map (n, H, W) float32, the relative standard error per pixel, NaN where the pixel is not counted."""
    c, m, out, emap = _noise_arrays(colour_sums, moments, want_map)
    st = (lib or load_library()).ptmi_noise_reference(_ptr(c), _ptr(m), c.shape[2], c.shape[1], c.shape[0], None if params is None else ctypes.byref(params), _ptr(out),
                                                      None if emap is None else _ptr(emap))
    if st != 0:
        raise PtmiError(st, "ptmi_noise_reference failed")
    return (out, emap) if want_map else out


def _run_noise_arrays(colour_sums, moments):
    c, m, _, _ = _noise_arrays(colour_sums, moments, False)
    n, n_runs = c.shape[0], (c.shape[1] * c.shape[2] + RUN_PIXELS - 1) // RUN_PIXELS
    return c, m, np.zeros((n, n_runs), RUN_NOISE_DTYPE), np.zeros(n, np.uint32), np.zeros((n, n_runs), np.uint32)


def _run_noise_result(records, n_open, open_runs):
    """(records (n, n_runs) RUN_NOISE_DTYPE, n_open (n,) uint32, the n ascending lists of open runs as uint32 arrays)"""
    return records, n_open, [open_runs[v, :int(k)].copy() for v, k in enumerate(n_open)]


def run_noise_reference(colour_sums, moments, target, params=None, lib=None):
    """ptmi_run_noise_reference: the noise statistic per RUN of 64 consecutive pixels, on the CPU (no GPU needed) — colour_sums and moments (n, H, W, 4) as for
    noise_reference.  Returns (records (n, n_runs) RUN_NOISE_DTYPE — counted, sum_q, max_q, open —, n_open (n,) uint32, [per image the ascending uint32 array of its
    open runs]): a run is open until it has counted > 0 and sum_q <= target * 65536 * counted."""
    c, m, rec, n_open, runs = _run_noise_arrays(colour_sums, moments)
    st = (lib or load_library()).ptmi_run_noise_reference(_ptr(c), _ptr(m), c.shape[2], c.shape[1], c.shape[0], None if params is None else ctypes.byref(params), float(target),
                                                          _ptr(rec), _ptr(n_open), _ptr(runs))
    if st != 0:
        raise PtmiError(st, "ptmi_run_noise_reference failed")
    return _run_noise_result(rec, n_open, runs)


def _run_refs_result(refs, header):
    """(refs (n_listed, 2) uint32 — {view, run}, the full runs' section and then the partial runs' —, (n_full, n_part, n_local))"""
    n_full, n_part, n_local = (int(x) for x in header)
    return refs[:n_full + n_part].copy(), (n_full, n_part, n_local)


def run_refs_reference(n_open, open_runs, npix, lib=None):
    """ptmi_run_refs_reference: the two-section list of a run batch across views, on the CPU (no GPU needed) — THE DEFINITION of its order.  n_open: (V,) uint32;
    open_runs: per view its ascending open runs — the list of arrays run_noise_reference / view_run_noise return, or a (V, n_runs) array whose rows begin with them.
    Returns (refs (n_full + n_part, 2) uint32 {view, run}: the full runs ascending by (view, run), then the partial runs ascending by view; (n_full, n_part, n_local))."""
    n = np.ascontiguousarray(n_open, np.uint32).reshape(-1)
    n_runs = (int(npix) + RUN_PIXELS - 1) // RUN_PIXELS
    rows = np.full((n.size, max(n_runs, 1)), 0xFFFFFFFF, np.uint32)
    for v in range(n.size):
        l = np.asarray(open_runs[v], np.uint32).reshape(-1)[:min(int(n[v]), n_runs)]
        rows[v, :l.size] = l
    refs, header = np.full((max(int(n.sum()), 1), 2), 0xFFFFFFFF, np.uint32), np.zeros(3, np.uint32)
    st = (lib or load_library()).ptmi_run_refs_reference(n.size, int(npix), _ptr(n), _ptr(rows), _ptr(refs), _ptr(header))
    if st != 0:
        raise PtmiError(st, "ptmi_run_refs_reference failed")
    return _run_refs_result(refs, header)


class NativeHost:
    """Host-side natives (no GPU): plug into host.scene.build_bvh(native=...)."""

    def __init__(self):
        self.lib = load_library()

    def _why(self, bmin, bmax, sah):
        """The sentence of ptmi_check_bvh_boxes for boxes a host builder refused (these have no context to leave it in)."""
        msg = ctypes.create_string_buffer(256)
        self.lib.ptmi_check_bvh_boxes(bmin.shape[0], _ptr(bmin), _ptr(bmax), 1 if sah else 0, msg, len(msg))
        return msg.value.decode()

    def build_bvh(self, bmin, bmax, prim_type=2):
        bmin = np.ascontiguousarray(bmin, np.float64)
        bmax = np.ascontiguousarray(bmax, np.float64)
        n = bmin.shape[0]
        nodes = np.zeros((max(2 * n - 1, 0), 12), np.float32)
        order = np.zeros(n, np.int64)
        st = self.lib.ptmi_build_bvh(n, _ptr(bmin), _ptr(bmax), prim_type, _ptr(nodes), _ptr(order))
        if st != 0:
            raise PtmiError(st, self._why(bmin, bmax, False) or "ptmi_build_bvh failed")
        return nodes, order


    def build_bvh_sah(self, bmin, bmax, prim_type=2):
        """The reference's binned-SAH builder (lib/BVH/bvhNode.js:108-283, dead code there), opt-in."""
        bmin = np.ascontiguousarray(bmin, np.float64)
        bmax = np.ascontiguousarray(bmax, np.float64)
        n = bmin.shape[0]
        nodes = np.zeros((max(2 * n - 1, 0), 12), np.float32)
        order = np.zeros(n, np.int64)
        count = ctypes.c_size_t()
        st = self.lib.ptmi_build_bvh_sah(n, _ptr(bmin), _ptr(bmax), prim_type, _ptr(nodes), _ptr(order), ctypes.byref(count))
        if st != 0:
            raise PtmiError(st, self._why(bmin, bmax, True) or "ptmi_build_bvh_sah failed")
        return nodes[: count.value].copy(), order

    def refit_bvh(self, bmin, bmax, rows):
        """ptmi_refit_bvh: `rows` (n_nodes, 12) with their boxes recomputed bottom-up over the primitive boxes bmin / bmax (n, 3), which are given in the tree's leaf
        order (indexed by row[8]); topology, links and leaf ranges stay.  Returns a new array; `rows` is not written."""
        bmin = np.ascontiguousarray(bmin, np.float64)
        bmax = np.ascontiguousarray(bmax, np.float64)
        out = np.array(rows, np.float32, order="C", copy=True).reshape(-1, 12)
        assert bmin.shape == bmax.shape and bmin.ndim == 2 and bmin.shape[1] == 3
        st = self.lib.ptmi_refit_bvh(bmin.shape[0], _ptr(bmin), _ptr(bmax), _ptr(out), out.shape[0])
        if st != 0:
            raise PtmiError(st, self._why(bmin, bmax, False) or "ptmi_refit_bvh: the rows are not a pre-order tree over these primitives")
        return out

    def parse_obj(self, text):
        """ObjReader.parse in native code: {vertices, normals} float32 arrays (lib/primitives/objReader.js grammar)."""
        data = text.encode("utf-8") if isinstance(text, str) else bytes(text)
        pv, pn, nv, nn = ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_size_t(), ctypes.c_size_t()
        st = self.lib.ptmi_obj_parse(data, len(data), ctypes.byref(pv), ctypes.byref(nv), ctypes.byref(pn), ctypes.byref(nn))
        if st != 0:
            raise PtmiError(st, "ptmi_obj_parse failed")
        try:
            v = np.ctypeslib.as_array(ctypes.cast(pv, ctypes.POINTER(ctypes.c_float)), (nv.value,)).copy() if nv.value else np.zeros(0, np.float32)
            n = np.ctypeslib.as_array(ctypes.cast(pn, ctypes.POINTER(ctypes.c_float)), (nn.value,)).copy() if nn.value else np.zeros(0, np.float32)
        finally:
            self.lib.ptmi_free(pv)
            self.lib.ptmi_free(pn)
        return {"vertices": v, "normals": n}

    def load_obj(self, path):
        with open(path, "rb") as f:
            return self.parse_obj(f.read())


class Context:
    """One integrator context (mirrors the reference's Renderer+WebGPU pair for the hot path).  `device` is a GPU index, or a
    list of them for a multi-device context (ptmi_create_multi: tiles sharded across the GPUs, one RCCL reduce on read-back)."""

    def __init__(self, device=0, lib=None):
        self.lib = lib if lib is not None else load_library()
        h = ctypes.c_void_p()
        if isinstance(device, (list, tuple)):
            ids = (ctypes.c_int * len(device))(*[int(d) for d in device])
            st = self.lib.ptmi_create_multi(ctypes.byref(h), ids, len(device))
        else:
            st = self.lib.ptmi_create(ctypes.byref(h), device)
        if st != 0:
            raise PtmiError(st, self.lib.ptmi_last_error(None).decode())
        self.h = h
        self.width = self.height = 0

    def close(self):
        if getattr(self, "h", None):
            self.lib.ptmi_destroy(self.h)
            self.h = None

    __del__ = close

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def _ck(self, st):
        if st != 0:
            raise PtmiError(st, self.lib.ptmi_last_error(self.h).decode())

    def _read_image(self, fn, *which):
        """an (H, W, 4) float32 image through fn(ctx, *which, dst, bytes)"""
        out = np.empty((self.height, self.width, 4), np.float32)
        self._ck(fn(self.h, *which, _ptr(out), out.nbytes))
        return out

    def _resolve_image(self, fn, *which):
        """an (H, W, 4) uint8 image through fn(ctx, *which, dst, bytes)"""
        out = np.empty((self.height, self.width, 4), np.uint8)
        self._ck(fn(self.h, *which, _ptr(out), out.nbytes))
        return out

    def _device_ptr(self, fn):
        """(device pointer, bytes, n_views) of a stack through fn"""
        p, n, v = ctypes.c_void_p(), ctypes.c_size_t(), ctypes.c_uint32()
        self._ck(fn(self.h, ctypes.byref(p), ctypes.byref(n), ctypes.byref(v)))
        return p.value, n.value, v.value

    def set_params(self, params=None, **kw):
        p = params if params is not None else default_params(**kw)
        self._ck(self.lib.ptmi_set_params(self.h, ctypes.byref(p)))
        return p

    def get_params(self):
        p = Params()
        self._ck(self.lib.ptmi_get_params(self.h, ctypes.byref(p)))
        return p

    def upload(self, which, array):
        a = np.ascontiguousarray(array)
        if a.dtype not in (np.float32, np.int32):
            raise TypeError("buffers are float32 (int32 for meshes)")
        self._ck(self.lib.ptmi_upload(self.h, BUF[which] if isinstance(which, str) else which, _ptr(a), a.nbytes))

    def upload_scene(self, buffers):
        for k in ("spheres", "quads", "triangles", "meshes", "transforms", "materials", "bvh"):
            a = buffers[k]
            self.upload(k, np.asarray(a, np.int32 if k == "meshes" else np.float32))

    def resize(self, w, h):
        self._ck(self.lib.ptmi_resize(self.h, w, h))
        self.width, self.height = w, h

    def clear(self):
        self._ck(self.lib.ptmi_clear_framebuffer(self.h))

    def set_shard(self, rank, world, tile=64):
        self._ck(self.lib.ptmi_set_shard(self.h, rank, world, tile))

    def render_frame(self, uniforms20):
        u = np.ascontiguousarray(uniforms20, np.float32)
        assert u.size == 20
        self._ck(self.lib.ptmi_render_frame(self.h, _ptr(u)))

    def render(self, view16, first_frame, n_frames):
        v = np.ascontiguousarray(view16, np.float32)
        assert v.size == 16
        self._ck(self.lib.ptmi_render(self.h, _ptr(v), first_frame, n_frames))

    def render_views(self, views, first_frame, frames_per_view, reset=True):
        """A camera path in one pass (ptmi_render_views): `views` is (V, 16) float32, one column-major view matrix per row; image v of the context's
        view stack receives frames first_frame .. first_frame + frames_per_view - 1 of view v.  Asynchronous."""
        v = np.ascontiguousarray(views, np.float32)
        assert v.ndim == 2 and v.shape[1] == 16, "views: (V, 16) float32"
        self._ck(self.lib.ptmi_render_views(self.h, _ptr(v), v.shape[0], first_frame, frames_per_view, 1 if reset else 0))

    def render_views_frames(self, views, first_frames, frame_counts, reset=True):
        """ptmi_render_views_frames: render_views with a frame range of its own per view — image v receives frames first_frames[v] .. first_frames[v] +
        frame_counts[v] - 1 of view v; a view with count 0 is left alone.  first_frames / frame_counts: (V,) uint32 (a scalar stands for every view).  Asynchronous."""
        v = np.ascontiguousarray(views, np.float32)
        assert v.ndim == 2 and v.shape[1] == 16, "views: (V, 16) float32"
        f, k = _frame_arrays(v.shape[0], first_frames, frame_counts)
        self._ck(self.lib.ptmi_render_views_frames(self.h, _ptr(v), v.shape[0], _ptr(f), _ptr(k), 1 if reset else 0))

    def read_view(self, view):
        return self._read_image(self.lib.ptmi_read_view, view)

    def resolve_view_rgba8(self, view, frame_num):
        return self._resolve_image(self.lib.ptmi_resolve_view_rgba8, view, float(frame_num))

    def views_device_ptr(self):
        """(device pointer, bytes, n_views) of the view stack: one contiguous [n_views][H][W][4] float32 array (single-device contexts)."""
        return self._device_ptr(self.lib.ptmi_views_device_ptr)

    def release_views(self):
        self._ck(self.lib.ptmi_release_views(self.h))

    def render_aov(self, views, first_frame, frames_per_view, reset=True):
        """The feature pass (ptmi_render_aov): `views` is (V, 16) float32 as for render_views; view v's three layers of the context's feature stack receive
        the first hits of frames first_frame .. first_frame + frames_per_view - 1.  Asynchronous."""
        v = np.ascontiguousarray(views, np.float32).reshape(-1, 16)
        self._ck(self.lib.ptmi_render_aov(self.h, _ptr(v), v.shape[0], first_frame, frames_per_view, 1 if reset else 0))

    def render_aov_frames(self, views, first_frames, frame_counts, reset=True):
        """ptmi_render_aov_frames: render_aov with render_views_frames' per-view frame ranges.  Asynchronous."""
        v = np.ascontiguousarray(views, np.float32).reshape(-1, 16)
        f, k = _frame_arrays(v.shape[0], first_frames, frame_counts)
        self._ck(self.lib.ptmi_render_aov_frames(self.h, _ptr(v), v.shape[0], _ptr(f), _ptr(k), 1 if reset else 0))

    def read_aov(self, view, layer=None):
        """Layer `layer` of view `view` of the feature stack as (H, W, 4) float32 — 0: normal sum + depth sum, 1: albedo sum + hit count, 2: kind, primitive
        index, material index, front_face — or, with layer=None, all three as (3, H, W, 4)."""
        if layer is not None:
            return self._read_image(self.lib.ptmi_read_aov, view, layer)
        return np.stack([self._read_image(self.lib.ptmi_read_aov, view, l) for l in range(3)])

    def aov_device_ptr(self):
        """(device pointer, bytes, n_views) of the feature stack: one contiguous [n_views][3][H][W][4] float32 array (single-device contexts)."""
        return self._device_ptr(self.lib.ptmi_aov_device_ptr)

    def release_aov(self):
        self._ck(self.lib.ptmi_release_aov(self.h))

    def denoise_views(self, frame_num, first_view=0, n_views=None, params=None):
        """ptmi_denoise_views: filters images [first_view, first_view + n_views) of the view stack (render_views) under the same images of the feature stack
        (render_aov) into the context's denoised stack; `frame_num` = the frames each view-stack image sums.  params: DenoiseParams (default_denoise_params).
        n_views=None: up to the end of the stack.  Asynchronous."""
        if n_views is None:
            n_views = self.views_device_ptr()[2] - first_view
        self._ck(self.lib.ptmi_denoise_views(self.h, None if params is None else ctypes.byref(params), float(frame_num), first_view, n_views))

    def read_denoised(self, view):
        return self._read_image(self.lib.ptmi_read_denoised, view)

    def resolve_denoised_rgba8(self, view):
        return self._resolve_image(self.lib.ptmi_resolve_denoised_rgba8, view)

    def denoised_device_ptr(self):
        """(device pointer, bytes, n_views) of the denoised stack: one contiguous [n_views][H][W][4] float32 array of mean radiance."""
        return self._device_ptr(self.lib.ptmi_denoised_device_ptr)

    def release_denoised(self):
        self._ck(self.lib.ptmi_release_denoised(self.h))

    def denoise_images(self, colour_sums, layers, frame_num, params=None):
        """ptmi_denoise_images: the kernels of denoise_views on host arrays of any size (see denoise_reference for the shapes); synchronous."""
        c, l, out = _denoise_arrays(colour_sums, layers)
        self._ck(self.lib.ptmi_denoise_images(self.h, _ptr(c), _ptr(l), c.shape[2], c.shape[1], c.shape[0], float(frame_num), None if params is None else ctypes.byref(params), _ptr(out)))
        return out

    def denoise_views_guided(self, frame_num, first_view=0, n_views=None, params=None):
        """ptmi_denoise_views_guided: denoise_views with the variance-guided filter — reads the same images of the moment stack too (set_view_moments) and writes the
        same denoised stack.  params: GuidedParams (default_guided_params).  n_views=None: up to the end of the stack.  Asynchronous."""
        if n_views is None:
            n_views = self.views_device_ptr()[2] - first_view
        self._ck(self.lib.ptmi_denoise_views_guided(self.h, None if params is None else ctypes.byref(params), float(frame_num), first_view, n_views))

    def denoise_images_guided(self, colour_sums, moments, layers, frame_num, params=None, want_var=False):
        """ptmi_denoise_images_guided: the kernels of denoise_views_guided on host arrays of any size (see denoise_guided_reference for the shapes and the result);
        synchronous."""
        c, m, l, out, var = _guided_arrays(colour_sums, moments, layers, want_var)
        self._ck(self.lib.ptmi_denoise_images_guided(self.h, _ptr(c), _ptr(m), _ptr(l), c.shape[2], c.shape[1], c.shape[0], float(frame_num),
                                                     None if params is None else ctypes.byref(params), _ptr(out), None if var is None else _ptr(var)))
        return (out, var) if want_var else out

    def fuse_views(self, views, frame_num=1.0, source=0, first_view=0, n_views=None, params=None):
        """ptmi_fuse_views: fuses output views [first_view, first_view + n_views) across their neighbours in the stack by reprojection into the context's fused
        stack.  `views`: (V, 16), the matrices of ALL views of the stack; source 0: the view stack, whose images sum `frame_num` frames; source 1: the denoised
        stack.  params: FuseParams (default_fuse_params).  n_views=None: up to the end of the stack.  Asynchronous."""
        v = np.ascontiguousarray(views, np.float32).reshape(-1, 16)
        n_stack = self.views_device_ptr()[2]
        assert v.shape[0] == n_stack, "views: the matrices of all %d views of the stack" % n_stack
        if n_views is None:
            n_views = n_stack - first_view
        self._ck(self.lib.ptmi_fuse_views(self.h, None if params is None else ctypes.byref(params), _ptr(v), float(frame_num), int(source), first_view, n_views))

    def read_fused(self, view):
        return self._read_image(self.lib.ptmi_read_fused, view)

    def resolve_fused_rgba8(self, view):
        return self._resolve_image(self.lib.ptmi_resolve_fused_rgba8, view)

    def fused_device_ptr(self):
        """(device pointer, bytes, n_views) of the fused stack: one contiguous [n_views][H][W][4] float32 array of mean radiance."""
        return self._device_ptr(self.lib.ptmi_fused_device_ptr)

    def release_fused(self):
        self._ck(self.lib.ptmi_release_fused(self.h))

    def fuse_images(self, colour, layers, views, frame_num, fov_degrees=60.0, lambertian=None, params=None):
        """ptmi_fuse_images: the kernel of fuse_views on host arrays of any size (see fuse_reference for the shapes); synchronous."""
        c, l, v, t, out = _fuse_arrays(colour, layers, views, lambertian)
        self._ck(self.lib.ptmi_fuse_images(self.h, _ptr(c), _ptr(l), _ptr(v), c.shape[2], c.shape[1], c.shape[0], float(frame_num), float(fov_degrees),
                                           None if t is None else _ptr(t), 0 if t is None else t.size, None if params is None else ctypes.byref(params), _ptr(out)))
        return out

    def accumulate_views(self, views, frame_num=1.0, first_view=0, n_views=None, resume=False, params=None):
        """ptmi_accumulate_views: accumulates views [first_view, first_view + n_views) of the camera path, each on its predecessor, into the context's accumulated
        stack.  `views`: (V, 16), the matrices of ALL views of the stack, whose images sum `frame_num` frames; resume: view first_view takes its history from view
        first_view - 1 of the stack as it is.  params: AccumulateParams (default_accumulate_params).  n_views=None: up to the end of the stack.  Asynchronous."""
        v = np.ascontiguousarray(views, np.float32).reshape(-1, 16)
        n_stack = self.views_device_ptr()[2]
        assert v.shape[0] == n_stack, "views: the matrices of all %d views of the stack" % n_stack
        if n_views is None:
            n_views = n_stack - first_view
        self._ck(self.lib.ptmi_accumulate_views(self.h, None if params is None else ctypes.byref(params), _ptr(v), float(frame_num), first_view, n_views, 1 if resume else 0))

    def read_accumulated(self, view, plane=None):
        """Plane `plane` of view `view` of the accumulated stack as (H, W, 4) float32 — 0: mean radiance, 1: (D, n), 2: (Q, v0) — or, with plane=None, all three as
        (3, H, W, 4)."""
        if plane is not None:
            return self._read_image(self.lib.ptmi_read_accumulated, view, plane)
        return np.stack([self._read_image(self.lib.ptmi_read_accumulated, view, p) for p in range(3)])

    def resolve_accumulated_rgba8(self, view):
        return self._resolve_image(self.lib.ptmi_resolve_accumulated_rgba8, view)

    def accumulated_device_ptr(self):
        """(device pointer, bytes, n_views) of the accumulated stack: one contiguous [3][n_views][H][W][4] float32 array."""
        return self._device_ptr(self.lib.ptmi_accumulated_device_ptr)

    def release_accumulated(self):
        self._ck(self.lib.ptmi_release_accumulated(self.h))

    def accumulate_images(self, colour_sums, moments, layers, views, frame_num, fov_degrees=60.0, lambertian=None, params=None, history=None):
        """ptmi_accumulate_images: the kernel of accumulate_views on host arrays of any size (see accumulate_reference for the shapes); synchronous."""
        c, m, l, v, t, hist, out = _accumulate_arrays(colour_sums, moments, layers, views, lambertian, history)
        self._ck(self.lib.ptmi_accumulate_images(self.h, _ptr(c), _ptr(m), _ptr(l), _ptr(v), c.shape[2], c.shape[1], c.shape[0], float(frame_num), float(fov_degrees),
                                                 None if t is None else _ptr(t), 0 if t is None else t.size, None if params is None else ctypes.byref(params),
                                                 None if hist is None else _ptr(hist), _ptr(out)))
        return out

    def denoise_views_accumulated(self, first_view=0, n_views=None, params=None):
        """ptmi_denoise_views_accumulated: the variance-guided filter on images [first_view, first_view + n_views) of the accumulated stack, whose plane 2 brings the
        initial variance; writes the denoised stack.  params: GuidedParams.  n_views=None: up to the end of the stack.  Asynchronous."""
        if n_views is None:
            n_views = self.accumulated_device_ptr()[2] - first_view
        self._ck(self.lib.ptmi_denoise_views_accumulated(self.h, None if params is None else ctypes.byref(params), first_view, n_views))

    def denoise_images_accumulated(self, means, plane2, layers, params=None, want_var=False):
        """ptmi_denoise_images_accumulated: the kernels of denoise_views_accumulated on host arrays of any size (see denoise_accumulated_reference); synchronous."""
        c, p2, l, out, var = _guided_arrays(means, plane2, layers, want_var)
        self._ck(self.lib.ptmi_denoise_images_accumulated(self.h, _ptr(c), _ptr(p2), _ptr(l), c.shape[2], c.shape[1], c.shape[0], None if params is None else ctypes.byref(params),
                                                          _ptr(out), None if var is None else _ptr(var)))
        return (out, var) if want_var else out

    # ---- the consumers with one frame count per view (include/ptmi.h, "CONSUMERS WITH PER-VIEW FRAME COUNTS") ----
    def _stack_frame_nums(self, frame_nums):
        return _frame_nums(frame_nums, self.views_device_ptr()[2])

    def denoise_views_frames(self, frame_nums, first_view=0, n_views=None, params=None):
        """ptmi_denoise_views_frames: denoise_views for a stack whose views sum different numbers of frames.  frame_nums: one count per view OF THE STACK, any
        sequence — render_views_until_each's frames_done as it is; only the entries of the range are read.  Asynchronous."""
        f = self._stack_frame_nums(frame_nums)
        if n_views is None:
            n_views = self.views_device_ptr()[2] - first_view
        self._ck(self.lib.ptmi_denoise_views_frames(self.h, None if params is None else ctypes.byref(params), _optr(f), first_view, n_views))

    def denoise_views_guided_frames(self, frame_nums, first_view=0, n_views=None, params=None):
        """ptmi_denoise_views_guided_frames: denoise_views_guided with one frame count per view of the stack (see denoise_views_frames).  Asynchronous."""
        f = self._stack_frame_nums(frame_nums)
        if n_views is None:
            n_views = self.views_device_ptr()[2] - first_view
        self._ck(self.lib.ptmi_denoise_views_guided_frames(self.h, None if params is None else ctypes.byref(params), _optr(f), first_view, n_views))

    def fuse_views_frames(self, views, frame_nums, first_view=0, n_views=None, params=None):
        """ptmi_fuse_views_frames: fuse_views on the view stack (source 0) with one frame count per view of the stack; the entries of the range widened by the radius
        are read.  Asynchronous."""
        v = np.ascontiguousarray(views, np.float32).reshape(-1, 16)
        n_stack = self.views_device_ptr()[2]
        assert v.shape[0] == n_stack, "views: the matrices of all %d views of the stack" % n_stack
        f = _frame_nums(frame_nums, n_stack)
        if n_views is None:
            n_views = n_stack - first_view
        self._ck(self.lib.ptmi_fuse_views_frames(self.h, None if params is None else ctypes.byref(params), _ptr(v), _optr(f), first_view, n_views))

    def accumulate_views_frames(self, views, frame_nums, first_view=0, n_views=None, resume=False, params=None):
        """ptmi_accumulate_views_frames: accumulate_views with one frame count per view of the stack; the entries of the range are read, and with resume the one
        before it.  Asynchronous."""
        v = np.ascontiguousarray(views, np.float32).reshape(-1, 16)
        n_stack = self.views_device_ptr()[2]
        assert v.shape[0] == n_stack, "views: the matrices of all %d views of the stack" % n_stack
        f = _frame_nums(frame_nums, n_stack)
        if n_views is None:
            n_views = n_stack - first_view
        self._ck(self.lib.ptmi_accumulate_views_frames(self.h, None if params is None else ctypes.byref(params), _ptr(v), _optr(f), first_view, n_views, 1 if resume else 0))

    def denoise_images_frames(self, colour_sums, layers, frame_nums, params=None):
        """ptmi_denoise_images_frames: denoise_images with one frame count per image; synchronous."""
        c, l, out = _denoise_arrays(colour_sums, layers)
        f = _frame_nums(frame_nums, c.shape[0])
        self._ck(self.lib.ptmi_denoise_images_frames(self.h, _ptr(c), _ptr(l), c.shape[2], c.shape[1], c.shape[0], _optr(f), None if params is None else ctypes.byref(params), _ptr(out)))
        return out

    def denoise_images_guided_frames(self, colour_sums, moments, layers, frame_nums, params=None, want_var=False):
        """ptmi_denoise_images_guided_frames: denoise_images_guided with one frame count per image; synchronous."""
        c, m, l, out, var = _guided_arrays(colour_sums, moments, layers, want_var)
        f = _frame_nums(frame_nums, c.shape[0])
        self._ck(self.lib.ptmi_denoise_images_guided_frames(self.h, _ptr(c), _ptr(m), _ptr(l), c.shape[2], c.shape[1], c.shape[0], _optr(f),
                                                            None if params is None else ctypes.byref(params), _ptr(out), _optr(var)))
        return (out, var) if want_var else out

    def fuse_images_frames(self, colour, layers, views, frame_nums, fov_degrees=60.0, lambertian=None, params=None):
        """ptmi_fuse_images_frames: fuse_images with one frame count per image; synchronous."""
        c, l, v, t, out = _fuse_arrays(colour, layers, views, lambertian)
        f = _frame_nums(frame_nums, c.shape[0])
        self._ck(self.lib.ptmi_fuse_images_frames(self.h, _ptr(c), _ptr(l), _ptr(v), c.shape[2], c.shape[1], c.shape[0], _optr(f), float(fov_degrees),
                                                  _optr(t), 0 if t is None else t.size, None if params is None else ctypes.byref(params), _ptr(out)))
        return out

    def accumulate_images_frames(self, colour_sums, moments, layers, views, frame_nums, fov_degrees=60.0, lambertian=None, params=None, history=None):
        """ptmi_accumulate_images_frames: accumulate_images with one frame count per image; synchronous."""
        c, m, l, v, t, hist, out = _accumulate_arrays(colour_sums, moments, layers, views, lambertian, history)
        f = _frame_nums(frame_nums, c.shape[0])
        self._ck(self.lib.ptmi_accumulate_images_frames(self.h, _ptr(c), _ptr(m), _ptr(l), _ptr(v), c.shape[2], c.shape[1], c.shape[0], _optr(f), float(fov_degrees),
                                                        _optr(t), 0 if t is None else t.size, None if params is None else ctypes.byref(params), _optr(hist), _ptr(out)))
        return out

    # ---- the consumers with every pixel's own frame count (include/ptmi.h, "CONSUMERS WITH PER-PIXEL FRAME COUNTS") ----
    def denoise_views_counts(self, first_view=0, n_views=None, params=None):
        """ptmi_denoise_views_counts: denoise_views for a stack whose PIXELS sum different numbers of frames (render_views_until_runs): every pixel's divisor is its
        M.w in the moment stack, read on the device.  Needs set_view_moments.  Asynchronous."""
        if n_views is None:
            n_views = self.views_device_ptr()[2] - first_view
        self._ck(self.lib.ptmi_denoise_views_counts(self.h, None if params is None else ctypes.byref(params), first_view, n_views))

    def denoise_views_guided_counts(self, first_view=0, n_views=None, params=None):
        """ptmi_denoise_views_guided_counts: denoise_views_guided with every pixel's own frame count (see denoise_views_counts).  Asynchronous."""
        if n_views is None:
            n_views = self.views_device_ptr()[2] - first_view
        self._ck(self.lib.ptmi_denoise_views_guided_counts(self.h, None if params is None else ctypes.byref(params), first_view, n_views))

    def fuse_views_counts(self, views, first_view=0, n_views=None, params=None):
        """ptmi_fuse_views_counts: fuse_views on the view stack (source 0) with every pixel's own frame count: the output pixel's M.w and, for a sample in a
        neighbour view, that pixel's.  views: (n_views of the stack, 16).  Asynchronous."""
        v = np.ascontiguousarray(views, np.float32).reshape(-1, 16)
        if n_views is None:
            n_views = v.shape[0] - first_view
        self._ck(self.lib.ptmi_fuse_views_counts(self.h, None if params is None else ctypes.byref(params), _ptr(v), first_view, n_views))

    def accumulate_views_counts(self, views, first_view=0, n_views=None, resume=False, params=None):
        """ptmi_accumulate_views_counts: accumulate_views with every pixel's own frame count: M.w of the pixel, and M.w of the pixel looked up in the view before.
        views: (n_views of the stack, 16).  Asynchronous."""
        v = np.ascontiguousarray(views, np.float32).reshape(-1, 16)
        if n_views is None:
            n_views = v.shape[0] - first_view
        self._ck(self.lib.ptmi_accumulate_views_counts(self.h, None if params is None else ctypes.byref(params), _ptr(v), first_view, n_views, 1 if resume else 0))

    def denoise_images_counts(self, colour_sums, layers, counts, params=None):
        """ptmi_denoise_images_counts: denoise_images with one frame count per pixel, counts (n, H, W); synchronous."""
        c, l, out = _denoise_arrays(colour_sums, layers)
        k = _pixel_counts(counts, c.shape[:3])
        self._ck(self.lib.ptmi_denoise_images_counts(self.h, _ptr(c), _ptr(l), c.shape[2], c.shape[1], c.shape[0], _optr(k), None if params is None else ctypes.byref(params), _ptr(out)))
        return out

    def denoise_images_guided_counts(self, colour_sums, moments, layers, params=None, want_var=False):
        """ptmi_denoise_images_guided_counts: denoise_images_guided with every pixel's own frame count, the w of its moments; synchronous."""
        c, m, l, out, var = _guided_arrays(colour_sums, moments, layers, want_var)
        self._ck(self.lib.ptmi_denoise_images_guided_counts(self.h, _ptr(c), _ptr(m), _ptr(l), c.shape[2], c.shape[1], c.shape[0],
                                                            None if params is None else ctypes.byref(params), _ptr(out), _optr(var)))
        return (out, var) if want_var else out

    def fuse_images_counts(self, colour, layers, views, counts, fov_degrees=60.0, lambertian=None, params=None):
        """ptmi_fuse_images_counts: fuse_images with one frame count per pixel, counts (n, H, W); synchronous."""
        c, l, v, t, out = _fuse_arrays(colour, layers, views, lambertian)
        k = _pixel_counts(counts, c.shape[:3])
        self._ck(self.lib.ptmi_fuse_images_counts(self.h, _ptr(c), _ptr(l), _ptr(v), c.shape[2], c.shape[1], c.shape[0], _optr(k), float(fov_degrees),
                                                  _optr(t), 0 if t is None else t.size, None if params is None else ctypes.byref(params), _ptr(out)))
        return out

    def accumulate_images_counts(self, colour_sums, moments, layers, views, fov_degrees=60.0, lambertian=None, params=None, history=None):
        """ptmi_accumulate_images_counts: accumulate_images with every pixel's own frame count, the w of its moments; synchronous."""
        c, m, l, v, t, hist, out = _accumulate_arrays(colour_sums, moments, layers, views, lambertian, history)
        self._ck(self.lib.ptmi_accumulate_images_counts(self.h, _ptr(c), _ptr(m), _ptr(l), _ptr(v), c.shape[2], c.shape[1], c.shape[0], float(fov_degrees),
                                                        _optr(t), 0 if t is None else t.size, None if params is None else ctypes.byref(params), _optr(hist), _ptr(out)))
        return out

    # ---- accumulation through a world whose objects move (include/ptmi.h, "ACCUMULATION WITH PER-OBJECT MOTION") ----
    def accumulate_views_motion(self, views, frame_nums, motions, first_view=0, n_views=None, resume=False, params=None, n_objects=None):
        """ptmi_accumulate_views_motion: accumulate_views_frames with motions (n_views of the stack, n_objects, 16) — per view and object (global_id) the column-major
        matrix that carries a world point of the object at the time of view v to the same material point at the time of view v-1 (render_moving_path returns them);
        the entries of views first_view + 1 .. are read, and first_view's with resume.  The pixel's object is found in the scene AS IT IS UPLOADED NOW: it has
        to be the one the feature stack was rendered from, its triangles in the order they lay in then.  refit_scene_bvh keeps that order; build_scene_bvh or an
        upload of triangles between render_moving_path and this call changes it, and the call then takes wrong ids — every index is checked, so nothing worse.
        Asynchronous."""
        v = np.ascontiguousarray(views, np.float32).reshape(-1, 16)
        n_stack = self.views_device_ptr()[2]
        assert v.shape[0] == n_stack, "views: the matrices of all %d views of the stack" % n_stack
        f = _frame_nums(frame_nums, n_stack)
        g, n_obj, _ = _motion_arrays(motions, None, n_stack)
        if n_views is None:
            n_views = n_stack - first_view
        self._ck(self.lib.ptmi_accumulate_views_motion(self.h, None if params is None else ctypes.byref(params), _ptr(v), _optr(f), _optr(g),
                                                       n_obj if n_objects is None else n_objects, first_view, n_views, 1 if resume else 0))

    def accumulate_images_motion(self, colour_sums, moments, layers, views, frame_nums, motions, object_ids, fov_degrees=60.0, lambertian=None, params=None, history=None,
                                 n_objects=None):
        """ptmi_accumulate_images_motion: the kernel of accumulate_views_motion on host arrays of any size (see accumulate_reference_motion); synchronous."""
        c, m, l, v, t, hist, out = _accumulate_arrays(colour_sums, moments, layers, views, lambertian, history)
        f = _frame_nums(frame_nums, c.shape[0])
        g, n_obj, ids = _motion_arrays(motions, object_ids, c.shape[0], c.shape[1:3])
        self._ck(self.lib.ptmi_accumulate_images_motion(self.h, _ptr(c), _ptr(m), _ptr(l), _ptr(v), c.shape[2], c.shape[1], c.shape[0], _optr(f), _optr(g),
                                                        n_obj if n_objects is None else n_objects, _optr(ids), float(fov_degrees), _optr(t), 0 if t is None else t.size,
                                                        None if params is None else ctypes.byref(params), _optr(hist), _ptr(out)))
        return out

    # ---- accumulation through deforming meshes (include/ptmi.h, "ACCUMULATION THROUGH DEFORMING MESHES") ----
    def accumulate_images_deform(self, colour_sums, moments, layers, views, frame_nums, triangles_seq, transforms_seq, meshes, motions=None, object_ids=None,
                                 fov_degrees=60.0, lambertian=None, params=None, history=None, n_objects=None):
        """ptmi_accumulate_images_deform: k_accumulate_view_deform on host arrays of any size (see accumulate_reference_deform); synchronous."""
        c, m, l, v, t, hist, out = _accumulate_arrays(colour_sums, moments, layers, views, lambertian, history)
        f = _frame_nums(frame_nums, c.shape[0])
        g, n_obj, ids = _motion_arrays(motions, object_ids, c.shape[0], c.shape[1:3])
        geo, keep = _deform_arrays(triangles_seq, transforms_seq, meshes, c.shape[0])
        self._ck(self.lib.ptmi_accumulate_images_deform(self.h, _ptr(c), _ptr(m), _ptr(l), _ptr(v), c.shape[2], c.shape[1], c.shape[0], _optr(f), *geo, _optr(g),
                                                        n_obj if n_objects is None else n_objects, _optr(ids), float(fov_degrees), _optr(t), 0 if t is None else t.size,
                                                        None if params is None else ctypes.byref(params), _optr(hist), _ptr(out)))
        return out

    def capture_view_geometry(self, view, n_views):
        """ptmi_capture_view_geometry: the device triangles in the order they lie in now and the transform table as uploaded now, into slot `view` of the context's
        geometry stack of n_views slots.  Asynchronous."""
        self._ck(self.lib.ptmi_capture_view_geometry(self.h, int(view), int(n_views)))

    def geometry_device_ptr(self):
        """ptmi_geometry_device_ptr: (triangles pointer, transforms pointer or None, n_views, n_triangles, n_transforms) of the geometry stack."""
        t, x, n, nt, nx = ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_uint32(), ctypes.c_uint64(), ctypes.c_uint64()
        self._ck(self.lib.ptmi_geometry_device_ptr(self.h, ctypes.byref(t), ctypes.byref(x), ctypes.byref(n), ctypes.byref(nt), ctypes.byref(nx)))
        return t.value, x.value, n.value, nt.value, nx.value

    def read_view_geometry(self, view):
        """ptmi_read_view_geometry: slot `view` of the geometry stack as (triangles (n_triangles, 24), transforms (n_transforms, 32)) float32."""
        _, _, _, nt, nx = self.geometry_device_ptr()
        tr, tf = np.empty((nt, 24), np.float32), np.empty((nx, 32), np.float32)
        self._ck(self.lib.ptmi_read_view_geometry(self.h, int(view), _ptr(tr), tr.nbytes, _ptr(tf), tf.nbytes))
        return tr, tf

    def release_geometry(self):
        self._ck(self.lib.ptmi_release_geometry(self.h))

    def accumulate_views_deform(self, views, frame_nums, motions=None, first_view=0, n_views=None, resume=False, params=None, n_objects=None):
        """ptmi_accumulate_views_deform: accumulate_views_motion through the geometry stack (capture_view_geometry; render_deforming_path fills it) — a triangle pixel
        is carried from its triangle in view v to the same triangle in view v-1; every other pixel goes through motions as accumulate_views_motion's do (None: a
        static world).  Asynchronous."""
        v = np.ascontiguousarray(views, np.float32).reshape(-1, 16)
        n_stack = self.views_device_ptr()[2]
        assert v.shape[0] == n_stack, "views: the matrices of all %d views of the stack" % n_stack
        f = _frame_nums(frame_nums, n_stack)
        g, n_obj, _ = _motion_arrays(motions, None, n_stack)
        if n_views is None:
            n_views = n_stack - first_view
        self._ck(self.lib.ptmi_accumulate_views_deform(self.h, None if params is None else ctypes.byref(params), _ptr(v), _optr(f), _optr(g),
                                                       n_obj if n_objects is None else n_objects, first_view, n_views, 1 if resume else 0))

    def render_deforming_path(self, views, triangles_seq, transforms_seq, first_frames, frame_counts):
        """A camera path through a scene whose meshes deform, a host loop over existing calls: for every view v it uploads triangles_seq[v] ((n_triangles, 24) float32
        IN THE CALLER'S ORIGINAL ORDER, the one the tree was built over) and transforms_seq[v] ((n_objects, 32)), refits the scene's device-resident tree
        (refit_scene_bvh), renders that view alone as render_moving_path does, and captures its geometry (capture_view_geometry).  The view moments must be on."""
        v = np.ascontiguousarray(views, np.float32).reshape(-1, 16)
        tr = np.ascontiguousarray(triangles_seq, np.float32).reshape(v.shape[0], -1, 24)
        t = np.ascontiguousarray(transforms_seq, np.float32).reshape(v.shape[0], -1, 32)
        f, k = _frame_arrays(v.shape[0], first_frames, frame_counts)
        for i in range(v.shape[0]):
            self.upload("triangles", tr[i])
            self.upload("transforms", t[i])
            self.refit_scene_bvh()
            only = np.where(np.arange(v.shape[0]) == i, k, 0).astype(np.uint32)
            self.render_views_frames(v, f, only, reset=True)
            self.moments_device_ptr()  # (PTMI_ERR_STATE while the view moments are off: say so after the first view, not after the last)
            self.render_aov_frames(v, f, only, reset=True)
            self.capture_view_geometry(i, v.shape[0])

    # ---- fusion through a world whose objects move (include/ptmi.h, "FUSION WITH PER-OBJECT MOTION") ----
    def fuse_views_motion(self, views, frame_nums, motions, source=0, first_view=0, n_views=None, params=None, n_objects=None):
        """ptmi_fuse_views_motion: fuse_views_frames with motions (n_views of the stack, n_objects, 16), the array accumulate_views_motion takes (render_moving_path
        returns it), composed across each output view's window; source 1 reads the denoised stack, frame_nums may then be None.  The pixel's object is found in the
        scene AS IT IS UPLOADED NOW, as accumulate_views_motion finds it.  Asynchronous."""
        v = np.ascontiguousarray(views, np.float32).reshape(-1, 16)
        n_stack = self.views_device_ptr()[2]
        assert v.shape[0] == n_stack, "views: the matrices of all %d views of the stack" % n_stack
        f = _frame_nums(frame_nums, n_stack)
        g, n_obj, _ = _motion_arrays(motions, None, n_stack)
        if n_views is None:
            n_views = n_stack - first_view
        self._ck(self.lib.ptmi_fuse_views_motion(self.h, None if params is None else ctypes.byref(params), _ptr(v), _optr(f), _optr(g),
                                                 n_obj if n_objects is None else n_objects, int(source), first_view, n_views))

    def fuse_images_motion(self, colour, layers, views, frame_nums, motions, object_ids, fov_degrees=60.0, lambertian=None, params=None, n_objects=None):
        """ptmi_fuse_images_motion: the kernel of fuse_views_motion on host arrays of any size (see fuse_reference_motion); synchronous."""
        c, l, v, t, out = _fuse_arrays(colour, layers, views, lambertian)
        f = _frame_nums(frame_nums, c.shape[0])
        g, n_obj, ids = _motion_arrays(motions, object_ids, c.shape[0], c.shape[1:3])
        self._ck(self.lib.ptmi_fuse_images_motion(self.h, _ptr(c), _ptr(l), _ptr(v), c.shape[2], c.shape[1], c.shape[0], _optr(f), _optr(g),
                                                  n_obj if n_objects is None else n_objects, _optr(ids), float(fov_degrees), _optr(t), 0 if t is None else t.size,
                                                  None if params is None else ctypes.byref(params), _ptr(out)))
        return out

    # ---- fusion through deforming meshes (include/ptmi.h, "FUSION THROUGH DEFORMING MESHES") ----
    def fuse_views_deform(self, views, frame_nums, motions=None, source=0, first_view=0, n_views=None, params=None, n_objects=None):
        """ptmi_fuse_views_deform: fuse_views_motion through the geometry stack (capture_view_geometry; render_deforming_path fills it) — a triangle pixel is carried
        from its triangle in view v to the same triangle in every view of its window; every other pixel goes through motions as fuse_views_motion's do (None: a
        static world).  source 1 reads the denoised stack, frame_nums may then be None.  Asynchronous."""
        v = np.ascontiguousarray(views, np.float32).reshape(-1, 16)
        n_stack = self.views_device_ptr()[2]
        assert v.shape[0] == n_stack, "views: the matrices of all %d views of the stack" % n_stack
        f = _frame_nums(frame_nums, n_stack)
        g, n_obj, _ = _motion_arrays(motions, None, n_stack)
        if n_views is None:
            n_views = n_stack - first_view
        self._ck(self.lib.ptmi_fuse_views_deform(self.h, None if params is None else ctypes.byref(params), _ptr(v), _optr(f), _optr(g),
                                                 n_obj if n_objects is None else n_objects, int(source), first_view, n_views))

    def fuse_images_deform(self, colour, layers, views, frame_nums, triangles_seq, transforms_seq, meshes, motions=None, object_ids=None, fov_degrees=60.0,
                           lambertian=None, params=None, n_objects=None):
        """ptmi_fuse_images_deform: k_fuse_deform on host arrays of any size (see fuse_reference_deform); synchronous."""
        c, l, v, t, out = _fuse_arrays(colour, layers, views, lambertian)
        f = _frame_nums(frame_nums, c.shape[0])
        g, n_obj, ids = _motion_arrays(motions, object_ids, c.shape[0], c.shape[1:3])
        geo, keep = _deform_arrays(triangles_seq, transforms_seq, meshes, c.shape[0])
        self._ck(self.lib.ptmi_fuse_images_deform(self.h, _ptr(c), _ptr(l), _ptr(v), c.shape[2], c.shape[1], c.shape[0], _optr(f), *geo, _optr(g),
                                                  n_obj if n_objects is None else n_objects, _optr(ids), float(fov_degrees), _optr(t), 0 if t is None else t.size,
                                                  None if params is None else ctypes.byref(params), _ptr(out)))
        return out

    def render_moving_path(self, views, transforms_seq, first_frames, frame_counts):
        """A camera path through a scene whose objects move, a host loop over existing calls: for every view v it uploads transforms_seq[v] ((n_objects, 32) float32,
        binding 7's layout), refits the scene's device-resident tree (refit_scene_bvh) and renders that view alone — render_views_frames and render_aov_frames with
        every other view's count 0, reset as those calls define it per view.  The view moments must be on (set_view_moments), so that the stacks are the ones
        accumulate_views_motion needs.  Returns the motions it takes, (V, n_objects, 16): motions_from_transforms over the sequence, view 0's the identity."""
        v = np.ascontiguousarray(views, np.float32).reshape(-1, 16)
        t = np.ascontiguousarray(transforms_seq, np.float32).reshape(v.shape[0], -1, 32)
        f, k = _frame_arrays(v.shape[0], first_frames, frame_counts)
        motions = np.empty((v.shape[0], t.shape[1], 16), np.float32)
        for i in range(v.shape[0]):
            self.upload("transforms", t[i])
            self.refit_scene_bvh()
            only = np.where(np.arange(v.shape[0]) == i, k, 0).astype(np.uint32)
            self.render_views_frames(v, f, only, reset=True)
            self.moments_device_ptr()  # (PTMI_ERR_STATE while the view moments are off: say so after the first view, not after the last)
            self.render_aov_frames(v, f, only, reset=True)
            motions[i] = motions_from_transforms(t[i - 1] if i else t[i], t[i], lib=self.lib)
        return motions

    def set_view_moments(self, on=True):
        """ptmi_set_view_moments: while on, render_views also folds the frames' squared colours into the context's moment stack (read_moments); off frees it."""
        self._ck(self.lib.ptmi_set_view_moments(self.h, 1 if on else 0))

    def read_moments(self, view):
        """Image `view` of the moment stack as (H, W, 4) float32: xyz the sums of the frames' squared colours, w the number of frames."""
        return self._read_image(self.lib.ptmi_read_moments, view)

    def moments_device_ptr(self):
        """(device pointer, bytes, n_views) of the moment stack: one contiguous [n_views][H][W][4] float32 array (single-device contexts)."""
        return self._device_ptr(self.lib.ptmi_moments_device_ptr)

    def release_moments(self):
        self._ck(self.lib.ptmi_release_moments(self.h))

    def view_noise(self, first_view=0, n_views=None, params=None):
        """ptmi_view_noise_stats: one VIEW_NOISE_DTYPE record (counted, sum_q, above, max_q) per view of [first_view, first_view + n_views) from the view and moment
        stacks; the mean noise of a view is sum_q / counted / 65536.  params: NoiseParams (default_noise_params).  n_views=None: up to the end of the stack (single-device contexts).  Synchronises."""
        if n_views is None:
            n_views = self.moments_device_ptr()[2] - first_view
        out = np.zeros(n_views, VIEW_NOISE_DTYPE)
        self._ck(self.lib.ptmi_view_noise_stats(self.h, None if params is None else ctypes.byref(params), first_view, n_views, _ptr(out) if out.size else None))
        return out

    def noise_images(self, colour_sums, moments, params=None, want_map=False):
        """ptmi_noise_images: the kernel of view_noise on host arrays of any size (see noise_reference for the shapes and the result); synchronous."""
        c, m, out, emap = _noise_arrays(colour_sums, moments, want_map)
        self._ck(self.lib.ptmi_noise_images(self.h, _ptr(c), _ptr(m), c.shape[2], c.shape[1], c.shape[0], None if params is None else ctypes.byref(params), _ptr(out),
                                            None if emap is None else _ptr(emap)))
        return (out, emap) if want_map else out

    def render_views_until(self, views, first_frame, frames_per_round, max_frames, target, params=None):
        """ptmi_render_views_until: render_views in rounds of frames_per_round frames per view until every view's mean noise is at most `target` or max_frames are
        done.  Needs set_view_moments.  Returns (frames_done, records): the frames every view then sums and the last round's VIEW_NOISE_DTYPE records."""
        v = np.ascontiguousarray(views, np.float32)
        assert v.ndim == 2 and v.shape[1] == 16, "views: (V, 16) float32"
        done = ctypes.c_uint32()
        out = np.zeros(v.shape[0], VIEW_NOISE_DTYPE)
        self._ck(self.lib.ptmi_render_views_until(self.h, _ptr(v), v.shape[0], first_frame, frames_per_round, max_frames, None if params is None else ctypes.byref(params),
                                                  float(target), ctypes.byref(done), _ptr(out)))
        return done.value, out

    def render_views_until_each(self, views, first_frames, frames_per_round, max_frames, target, params=None):
        """ptmi_render_views_until_each: render_views_until view by view — a view stops getting frames once ITS mean noise is at most `target`.  first_frames: (V,)
        uint32, a scalar, or None for 0.  Needs set_view_moments.  Returns (frames_done (V,) uint32, records): the frames each view then sums and the VIEW_NOISE_DTYPE
        records last taken."""
        v = np.ascontiguousarray(views, np.float32)
        assert v.ndim == 2 and v.shape[1] == 16, "views: (V, 16) float32"
        f = None if first_frames is None else _frame_arrays(v.shape[0], first_frames, 0)[0]
        done = np.zeros(v.shape[0], np.uint32)
        out = np.zeros(v.shape[0], VIEW_NOISE_DTYPE)
        self._ck(self.lib.ptmi_render_views_until_each(self.h, _ptr(v), v.shape[0], None if f is None else _ptr(f), frames_per_round, max_frames,
                                                       None if params is None else ctypes.byref(params), float(target), _ptr(done), _ptr(out)))
        return done, out

    def render_view_runs(self, view16, view, first_frame, n_frames, runs):
        """ptmi_render_view_runs: adds frames first_frame .. first_frame + n_frames - 1 of view16 to image `view` of the view and moment stacks, for the pixels of the
        listed runs alone (run r = pixels [64 r, 64 r + 64) in row-major order).  runs: strictly ascending uint32.  Needs set_view_moments and both stacks.  Asynchronous."""
        v = np.ascontiguousarray(view16, np.float32)
        assert v.size == 16
        r = np.ascontiguousarray(runs, np.uint32).reshape(-1)
        self._ck(self.lib.ptmi_render_view_runs(self.h, _ptr(v), view, first_frame, n_frames, _ptr(r) if r.size else None, r.size))

    def view_run_noise(self, target, first_view=0, n_views=None, params=None):
        """ptmi_view_run_noise: run_noise_reference's result for views [first_view, first_view + n_views) of the view and moment stacks.  n_views=None: up to the end
        of the stack.  Synchronises."""
        if n_views is None:
            n_views = self.moments_device_ptr()[2] - first_view
        n_runs = (self.width * self.height + RUN_PIXELS - 1) // RUN_PIXELS
        rec, n_open, runs = np.zeros((n_views, n_runs), RUN_NOISE_DTYPE), np.zeros(n_views, np.uint32), np.zeros((n_views, n_runs), np.uint32)
        self._ck(self.lib.ptmi_view_run_noise(self.h, None if params is None else ctypes.byref(params), float(target), first_view, n_views, _ptr(rec), _ptr(n_open), _ptr(runs)))
        return _run_noise_result(rec, n_open, runs)

    def run_noise_images(self, colour_sums, moments, target, params=None):
        """ptmi_run_noise_images: the kernels of view_run_noise on host arrays of any size (see run_noise_reference for the shapes and the result); synchronous."""
        c, m, rec, n_open, runs = _run_noise_arrays(colour_sums, moments)
        self._ck(self.lib.ptmi_run_noise_images(self.h, _ptr(c), _ptr(m), c.shape[2], c.shape[1], c.shape[0], None if params is None else ctypes.byref(params), float(target),
                                                _ptr(rec), _ptr(n_open), _ptr(runs)))
        return _run_noise_result(rec, n_open, runs)

    def render_views_until_runs(self, views, first_frames, frames_per_round, min_frames, max_frames, target, params=None):
        """ptmi_render_views_until_runs: min(min_frames, max_frames) frames of every view in one batched call, then rounds of frames_per_round frames for the RUNS of
        each view that have not met `target`, until none is open below max_frames.  first_frames: (V,) uint32, a scalar, or None for 0.  Needs set_view_moments.
        Returns (frames_done (V,) uint32 — the most any run of the view got; a pixel's own count is read_moments' w —, records: view_noise of all views at the end,
        paths_traced)."""
        v = np.ascontiguousarray(views, np.float32)
        assert v.ndim == 2 and v.shape[1] == 16, "views: (V, 16) float32"
        f = None if first_frames is None else _frame_arrays(v.shape[0], first_frames, 0)[0]
        done = np.zeros(v.shape[0], np.uint32)
        out = np.zeros(v.shape[0], VIEW_NOISE_DTYPE)
        paths = ctypes.c_uint64()
        self._ck(self.lib.ptmi_render_views_until_runs(self.h, _ptr(v), v.shape[0], _optr(f), frames_per_round, min_frames, max_frames,
                                                       None if params is None else ctypes.byref(params), float(target), _ptr(done), _ptr(out), ctypes.byref(paths)))
        return done, out, paths.value

    def render_views_runs(self, views, first_frames, n_frames, run_views, runs):
        """ptmi_render_views_runs: ONE wavefront batch for the listed runs of many views — adds frames first_frames[v] .. first_frames[v] + n_frames - 1 of views[v] to
        the listed runs of image v of the view and moment stacks, for every listed view; every other pixel keeps its bits.  views: (V, 16); first_frames: (V,) uint32 or
        a scalar; (run_views[i], runs[i]): strictly ascending by (view, run).  Needs set_view_moments and both stacks.  Asynchronous."""
        v = np.ascontiguousarray(views, np.float32)
        assert v.ndim == 2 and v.shape[1] == 16, "views: (V, 16) float32"
        f = _frame_arrays(v.shape[0], first_frames, 0)[0]
        rv = np.ascontiguousarray(run_views, np.uint32).reshape(-1)
        r = np.ascontiguousarray(runs, np.uint32).reshape(-1)
        assert rv.size == r.size, "one view per listed run"
        self._ck(self.lib.ptmi_render_views_runs(self.h, _ptr(v), v.shape[0], _ptr(f), n_frames, _ptr(rv) if rv.size else None, _ptr(r) if r.size else None, r.size))

    def run_refs_images(self, colour_sums, moments, target, params=None):
        """ptmi_run_refs_images: the kernels of a round of render_views_until_runs (k_run_noise, k_run_list, k_run_refs) on host arrays of any size — the device's
        two-section list, in run_refs_reference's form; synchronous."""
        c, m, _, _, runs = _run_noise_arrays(colour_sums, moments)
        refs, header = np.zeros((max(runs.size, 1), 2), np.uint32), np.zeros(3, np.uint32)
        self._ck(self.lib.ptmi_run_refs_images(self.h, _ptr(c), _ptr(m), c.shape[2], c.shape[1], c.shape[0], None if params is None else ctypes.byref(params), float(target),
                                               _ptr(refs), _ptr(header)))
        full = _run_refs_result(refs, header)
        assert (refs[full[0].shape[0]:runs.size] == 0xFFFFFFFF).all(), "behind the list the device block keeps its fill"
        return full

    def read_view_mean(self, view):
        """ptmi_read_view_mean: image `view` as (H, W, 4) float32 with every pixel's own divisor — rgb = S.rgb / M.w, 0 where M.w == 0; w = M.w."""
        return self._read_image(self.lib.ptmi_read_view_mean, view)

    def resolve_view_mean_rgba8(self, view):
        """ptmi_resolve_view_mean_rgba8: resolve_view_rgba8 with every pixel's own frame count (read_moments' w) in place of frame_num."""
        return self._resolve_image(self.lib.ptmi_resolve_view_mean_rgba8, view)

    def camera_rays(self, view16, frame):
        """Test hook (ptmi_camera_rays): (rays (W*H, 6) float32, rng (W*H,) uint32) — the first camera ray of `frame` for every pixel and the RNG state its
        hitScene starts with."""
        v = np.ascontiguousarray(view16, np.float32)
        assert v.size == 16
        n = self.width * self.height
        rays, rng = np.empty((n, 6), np.float32), np.empty(n, np.uint32)
        self._ck(self.lib.ptmi_camera_rays(self.h, _ptr(v), frame, _ptr(rays), _ptr(rng)))
        return rays, rng

    def synchronize(self):
        self._ck(self.lib.ptmi_synchronize(self.h))

    def prepare(self):
        """Validate the uploaded scene and build the device-side digests now (otherwise the first render does it)."""
        self._ck(self.lib.ptmi_prepare(self.h))

    def read_framebuffer(self):
        return self._read_image(self.lib.ptmi_read_framebuffer)

    def reduce_info(self):
        """One line about how this context sums its devices' buffers (RCCL, add kernel, or the FALLBACK after an RCCL failure)."""
        return self.lib.ptmi_reduce_info(self.h).decode()

    def reload_tuning(self):
        """Re-read the PTMI_* tuning variables (they are read once, at creation)."""
        self._ck(self.lib.ptmi_reload_tuning(self.h))

    def reduce_framebuffer(self):
        """The one collective of a multi-device render (sum of the per-device buffers on the first device); a sync on one device."""
        self._ck(self.lib.ptmi_reduce_framebuffer(self.h))

    def write_framebuffer(self, fb):
        a = np.ascontiguousarray(fb, np.float32)
        self._ck(self.lib.ptmi_write_framebuffer(self.h, _ptr(a), a.nbytes))

    def framebuffer_device_ptr(self):
        p, n = ctypes.c_void_p(), ctypes.c_size_t()
        self._ck(self.lib.ptmi_framebuffer_device_ptr(self.h, ctypes.byref(p), ctypes.byref(n)))
        return p.value, n.value

    def bind_framebuffer(self, dev_ptr, nbytes):
        self._ck(self.lib.ptmi_bind_framebuffer(self.h, ctypes.c_void_p(dev_ptr), nbytes))

    def stream(self):
        p = ctypes.c_void_p()
        self._ck(self.lib.ptmi_stream(self.h, ctypes.byref(p)))
        return p.value

    def resolve_rgba8(self, frame_num):
        return self._resolve_image(self.lib.ptmi_resolve_rgba8, float(frame_num))

    def set_counters(self, on):
        self._ck(self.lib.ptmi_set_counters(self.h, int(on)))

    def set_onb_table(self, on):
        """k_shade's LDS table of quad records (ptmi_set_onb_table): on by default, the same bits either way."""
        self._ck(self.lib.ptmi_set_onb_table(self.h, int(on)))

    def set_timing(self, mode):
        """0/False off, 1/True every kernel, 2 / 3 / 4 / 5 only k_bvh / k_shade / k_generate / k_accumulate."""
        self._ck(self.lib.ptmi_set_timing(self.h, int(mode)))

    def stats(self):
        s = Stats()
        self._ck(self.lib.ptmi_get_stats(self.h, ctypes.byref(s)))
        return s.as_dict()

    def reset_stats(self):
        self._ck(self.lib.ptmi_reset_stats(self.h))

    def build_bvh(self, bmin, bmax, prim_type=2):
        """ptmi_build_bvh_device: the median-split build on this context's GPU; same result as NativeHost.build_bvh."""
        bmin = np.ascontiguousarray(bmin, np.float64)
        bmax = np.ascontiguousarray(bmax, np.float64)
        n = bmin.shape[0]
        nodes = np.zeros((max(2 * n - 1, 0), 12), np.float32)
        order = np.zeros(n, np.int64)
        self._ck(self.lib.ptmi_build_bvh_device(self.h, n, _ptr(bmin), _ptr(bmax), prim_type, _ptr(nodes), _ptr(order)))
        return nodes, order

    def build_scene_bvh(self, sah=False):
        """ptmi_build_scene_bvh: Scene.create_bvh() on the GPU over the uploaded (unordered) triangles, meshes and transforms; nothing comes back.
        sah=True: the reference's other builder (lib/BVH/bvhNode.js:108-283), the opt-in."""
        self._ck((self.lib.ptmi_build_scene_bvh_sah if sah else self.lib.ptmi_build_scene_bvh)(self.h))

    def refit_scene_bvh(self):
        """ptmi_refit_scene_bvh: the device-resident tree's boxes recomputed over the triangles, meshes and transforms uploaded now, its topology kept."""
        self._ck(self.lib.ptmi_refit_scene_bvh(self.h))

    def scene_bvh_info(self):
        """{nodes, depth, on_device} of the scene's BVH (ptmi_scene_bvh_info)."""
        n, d, o = ctypes.c_uint64(), ctypes.c_int32(), ctypes.c_int32()
        self._ck(self.lib.ptmi_scene_bvh_info(self.h, ctypes.byref(n), ctypes.byref(d), ctypes.byref(o)))
        return {"nodes": n.value, "depth": d.value, "on_device": bool(o.value)}

    def build_bvh_sah(self, bmin, bmax, prim_type=2):
        """ptmi_build_bvh_sah_device: the binned-SAH build on this context's GPU; same result as NativeHost.build_bvh_sah."""
        bmin = np.ascontiguousarray(bmin, np.float64)
        bmax = np.ascontiguousarray(bmax, np.float64)
        n = bmin.shape[0]
        nodes = np.zeros((max(2 * n - 1, 0), 12), np.float32)
        order = np.zeros(n, np.int64)
        count = ctypes.c_size_t()
        self._ck(self.lib.ptmi_build_bvh_sah_device(self.h, n, _ptr(bmin), _ptr(bmax), prim_type, _ptr(nodes), _ptr(order), ctypes.byref(count)))
        return nodes[: count.value].copy(), order

    def read_scene_buffer(self, which, count):
        """Test hook: the context's triangles ('triangles', count = number of triangles) or BVH rows ('bvh', count = number of nodes) as an array."""
        out = np.empty((count, 24 if which == "triangles" else 12), np.float32)
        self._ck(self.lib.ptmi_read_scene_buffer(self.h, BUF[which], _ptr(out), out.nbytes))
        return out

    def trace(self, rays6, rng=None):
        r = np.ascontiguousarray(rays6, np.float32).reshape(-1, 6)
        n = r.shape[0]
        out = np.zeros(n, HIT_DTYPE)
        g = None if rng is None else np.ascontiguousarray(rng, np.uint32).copy()
        self._ck(self.lib.ptmi_trace(self.h, n, _ptr(r), None if g is None else _ptr(g), _ptr(out)))
        return out, g

    def selftest(self, which):
        """Exhaustive device-side check of a unary shortcut against the IEEE operation: (mismatches, first bad argument bits).
        which = 8: the uploaded scene's quad records: (records that differ from the bounce's own evaluation, quads whose back-side frame is not the record's negated)."""
        n, first = ctypes.c_uint64(), ctypes.c_uint32()
        self._ck(self.lib.ptmi_selftest(self.h, which, ctypes.byref(n), ctypes.byref(first)))
        return n.value, first.value

    def math_eval(self, fn, x, y=None):
        x = np.ascontiguousarray(x, np.float32)
        out = np.empty_like(x)
        yy = None if y is None else np.ascontiguousarray(y, np.float32)
        self._ck(self.lib.ptmi_math_eval(self.h, fn, x.size, _ptr(x), None if yy is None else _ptr(yy), _ptr(out)))
        return out
