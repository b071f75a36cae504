"""rtmi — Python binding of librtmi.so (the MI355X path-tracing hot path).

This package is plumbing over the C ABI declared in include/rtmi.h: ctypes calls
for the scene recorder / RNG / render entry points and PyTorch tensors for device
memory, streams and ``torch.distributed``.  There is no CPU rendering path: every
compute call raises ``RtmiError`` when librtmi.so or a GPU is missing.
"""
import collections
import ctypes as C
import os

import numpy as np

_PKG_DIR = os.path.dirname(os.path.abspath(__file__))
_ROOT = os.path.dirname(_PKG_DIR)  # ray-tracing-cuda_amd/
# RTMI_LIB_PATH: diagnostic builds of the same library (tools/mesh_stats.sh); never a different implementation
LIB_PATH = os.environ.get("RTMI_LIB_PATH") or os.path.join(_ROOT, "lib", "librtmi.so")

TILE = 8
STATE_WORDS = 6
MAX_DEPTH = 64
TRACE_WORK_WORDS = 256  # RTMI_TRACE_WORK_WORDS: the device words of one rtmi_trace call
BUDGET_WORK_WORDS = TRACE_WORK_WORDS  # RTMI_BUDGET_WORK_WORDS: the device words of one rtmi_render_budget call
PATH_COMPACT_ITEMS = 1024  # RTMI_PATH_COMPACT_ITEMS: list entries per workgroup (and per scratch word) of rtmi_path_compact
MODE_FIELDS = 9  # RTMI_MODE_FIELDS: the words of rtmi_render_mode_ex
FAST_PATH_FACTS = 14  # RTMI_FAST_PATH_FACTS: the words rtmi_fast_path_kernel reads
MAX_MATERIALS = 1 << 24  # RTMI_MAX_MATERIALS: a larger scene is refused by commit (RTMI_ERR_CAPACITY)
# what trace_steps(compact, direct=True, shadow=None) means: "all" (rtmi_occluded over all N shadow rays) or "list"
# (rtmi_occluded_list on the step's list).  The outputs are the same; DESIGN.md 2.14 has the cost that decides it: on an
# MI355X the "list" loop is not slower than the "all" loop on any of the four measured scenes.
SHADOW_DEFAULT = "list"

# rtmi_hit.kind (include/rtmi.h)
RTMI_HIT_NONE = 0
RTMI_HIT_SPHERE = 1
RTMI_HIT_TRIANGLE = 2
RTMI_HIT_PARALLELOGRAM = 3
RTMI_HIT_PARALLELEPIPED = 4
RTMI_HIT_MESH = 5
RTMI_HIT_SKY = 6
HIT_WORDS = 12  # sizeof(rtmi_hit) / 4


class RtmiError(RuntimeError):
    pass


class Frame(C.Structure):
    """rtmi_frame of include/rtmi.h."""
    _fields_ = [("height", C.c_int32), ("width", C.c_int32), ("spp", C.c_int32), ("max_depth", C.c_int32),
                ("post_process", C.c_int32), ("rank", C.c_int32), ("world_size", C.c_int32)]


class RenderOpts(C.Structure):
    """rtmi_render_opts of include/rtmi.h (per-call scheduling options)."""
    _fields_ = [("size", C.c_int32), ("schedule", C.c_int32), ("blocks_per_cu", C.c_int32),
                ("threads_per_block", C.c_int32), ("sparse_stride", C.c_int32), ("exclusive", C.c_int32),
                ("outlier_x10", C.c_int32), ("probe_spp", C.c_int32), ("head_pct", C.c_int32 * 3),
                ("plan", C.c_int32), ("wave_priority", C.c_int32), ("lane_stride", C.c_int32),
                ("promote_after", C.c_int32), ("cost_probe", C.c_int32), ("first_pass", C.c_int32), ("fast_path", C.c_int32),
                ("d_scratch", C.c_void_p), ("scratch_bytes", C.c_size_t)]


def render_opts(schedule=-1, blocks_per_cu=0, threads_per_block=0, sparse_stride=0, exclusive=-1, outlier_x10=0,
                probe_spp=0, head_pct=(0, 0, 0), scratch=None, plan=-1, wave_priority=-1, lane_stride=0, promote_after=-1,
                cost_probe=-1, first_pass=-1, fast_path=0):
    """``scratch``: a torch uint8/int32 CUDA tensor of at least ``scratch_bytes(frame)`` bytes that holds ALL
    per-call state of the render (keep it alive until the render has finished)."""
    o = RenderOpts(C.sizeof(RenderOpts), schedule, blocks_per_cu, threads_per_block, sparse_stride, exclusive,
                   outlier_x10, probe_spp, (C.c_int32 * 3)(*head_pct), plan, wave_priority, lane_stride, promote_after,
                   cost_probe, first_pass, fast_path, None, 0)
    if scratch is not None:
        o.d_scratch = scratch.data_ptr()
        o.scratch_bytes = scratch.numel() * scratch.element_size()
    return o


class AdaptiveOpts(C.Structure):
    """rtmi_adaptive_opts of include/rtmi.h (the stopping rule of rtmi_budget_plan)."""
    _fields_ = [("size", C.c_int32), ("min_samples", C.c_int32), ("max_samples", C.c_int32), ("step", C.c_int32),
                ("tolerance", C.c_float), ("floor", C.c_float)]


def adaptive_opts(min_spp, max_spp, step, tolerance, floor=0.01):
    return AdaptiveOpts(C.sizeof(AdaptiveOpts), int(min_spp), int(max_spp), int(step), float(tolerance), float(floor))


class Features(C.Structure):
    """rtmi_features of include/rtmi.h (first-hit feature buffers, each nullable)."""
    _fields_ = [("size", C.c_int32), ("reserved", C.c_int32), ("d_albedo", C.c_void_p), ("d_normal", C.c_void_p),
                ("d_depth", C.c_void_p), ("d_coverage", C.c_void_p)]


def feature_bufs(albedo=None, normal=None, depth=None, coverage=None):
    """An rtmi_features over torch tensors (None: that buffer is left out); keep the tensors alive while it is used."""
    ptr = lambda t: None if t is None else t.data_ptr()
    return Features(C.sizeof(Features), 0, ptr(albedo), ptr(normal), ptr(depth), ptr(coverage))


class Projection(C.Structure):
    """rtmi_projection of include/rtmi.h (how rtmi_camera_rays turns a pixel's jitter into a ray)."""
    _fields_ = [("size", C.c_int32), ("kind", C.c_int32), ("fov", C.c_float), ("reserved", C.c_int32)]


PROJECTIONS = {"camera": 0, "orthographic": 1, "equirect": 2, "fisheye": 3}  # RTMI_PROJ_*


def projection(kind="camera", fov=0.0):
    """An rtmi_projection: ``kind`` "camera" (the scene's own, the render's), "orthographic", "equirect" or "fisheye";
    ``fov``: a fisheye's full angle of the image circle in radians, in (0, 2 pi]."""
    if kind not in PROJECTIONS:
        raise RtmiError("projection kind must be one of %s" % ", ".join(sorted(PROJECTIONS)))
    return Projection(C.sizeof(Projection), PROJECTIONS[kind], float(fov), 0)


class PathAdvanceArgs(C.Structure):
    """rtmi_path_advance_args of include/rtmi.h (the arrays of one rtmi_path_advance call)."""
    _fields_ = [("size", C.c_int32), ("reserved", C.c_int32), ("proj", C.POINTER(Projection)), ("d_budget", C.c_void_p),
                ("d_list", C.c_void_p), ("n_list", C.c_int64), ("d_count", C.c_void_p), ("d_origins", C.c_void_p),
                ("d_dirs", C.c_void_p), ("d_states", C.c_void_p), ("d_steps", C.c_void_p), ("d_emitted", C.c_void_p),
                ("d_attenuation", C.c_void_p), ("d_emitted_stack", C.c_void_p), ("d_attenuation_stack", C.c_void_p),
                ("d_cursor", C.c_void_p), ("d_sum", C.c_void_p), ("d_sq", C.c_void_p), ("d_samples", C.c_void_p),
                ("d_ray_counts", C.c_void_p), ("d_counts", C.c_void_p)]


class DirectSampleMisArgs(C.Structure):
    """rtmi_direct_sample_mis_args of include/rtmi.h (the arrays of one rtmi_direct_sample_mis call)."""
    _fields_ = [("size", C.c_int32), ("reserved", C.c_int32), ("n", C.c_int64), ("d_list", C.c_void_p), ("n_list", C.c_int64),
                ("d_count", C.c_void_p), ("step", C.c_uint32), ("sample", C.c_int32), ("d_origins", C.c_void_p),
                ("d_dirs", C.c_void_p), ("d_hits", C.c_void_p), ("d_steps", C.c_void_p), ("d_emitted", C.c_void_p),
                ("d_attenuation", C.c_void_p), ("d_light_states", C.c_void_p), ("d_flags", C.c_void_p),
                ("d_shadow_origins", C.c_void_p), ("d_shadow_dirs", C.c_void_p), ("d_shadow_t_max", C.c_void_p),
                ("d_direct", C.c_void_p), ("d_carry", C.c_void_p), ("d_counts", C.c_void_p)]


class DenoiseOpts(C.Structure):
    """rtmi_denoise_opts of include/rtmi.h."""
    _fields_ = [("size", C.c_int32), ("iterations", C.c_int32), ("normal_squarings", C.c_int32), ("demodulate", C.c_int32),
                ("sigma_color", C.c_float), ("sigma_depth", C.c_float)]


class DenoiseGuides(C.Structure):
    """rtmi_denoise_guides of include/rtmi.h (row-major, whole-frame guide buffers)."""
    _fields_ = [("size", C.c_int32), ("reserved", C.c_int32), ("d_variance", C.c_void_p), ("d_albedo", C.c_void_p),
                ("d_normal", C.c_void_p), ("d_depth", C.c_void_p), ("d_alpha", C.c_void_p)]


# rtmi.denoise's defaults (include/rtmi.h names the same figures)
DENOISE_DEFAULTS = dict(iterations=5, sigma_color=1.0, sigma_depth=0.05, normal_squarings=0)


class AccumulateOpts(C.Structure):
    """rtmi_accumulate_opts of include/rtmi.h."""
    _fields_ = [("size", C.c_int32), ("reserved", C.c_int32), ("normal_min", C.c_float), ("depth_tolerance", C.c_float),
                ("min_blend", C.c_float)]


# rtmi.accumulate's defaults (include/rtmi.h names the same figures)
ACCUMULATE_DEFAULTS = dict(normal_min=0.8, depth_tolerance=0.05, min_blend=0.1)


TRANSFORM_FN = C.CFUNCTYPE(None, C.POINTER(C.c_float), C.POINTER(C.c_float), C.c_void_p)

_lib = None

# every symbol include/rtmi.h declares: (name, restype, argtypes)
_fp = C.POINTER(C.c_float)
_u32p = C.POINTER(C.c_uint32)
_frp = C.POINTER(Frame)
SYMBOLS = [
    ("rtmi_last_error", C.c_char_p, []),
    ("rtmi_version", C.c_int, []),
    ("rtmi_device_count", C.c_int, []),
    ("rtmi_scene_create", C.c_void_p, []),
    ("rtmi_scene_destroy", None, [C.c_void_p]),
    ("rtmi_constant_texture", C.c_int, [C.c_void_p, _fp]),
    ("rtmi_image_texture", C.c_int, [C.c_void_p, C.POINTER(C.c_uint8), C.c_int, C.c_int, C.c_size_t]),
    ("rtmi_lambertian", C.c_int, [C.c_void_p, _fp]),
    ("rtmi_lambertian_tex", C.c_int, [C.c_void_p, C.c_int]),
    ("rtmi_metal", C.c_int, [C.c_void_p, _fp, C.c_float]),
    ("rtmi_dielectric", C.c_int, [C.c_void_p, _fp, C.c_double]),
    ("rtmi_diffuse_light", C.c_int, [C.c_void_p, C.c_int]),
    ("rtmi_add_sphere", C.c_int, [C.c_void_p, _fp, C.c_double, C.c_int]),
    ("rtmi_add_triangle", C.c_int, [C.c_void_p, _fp, C.c_int]),
    ("rtmi_add_parallelogram", C.c_int, [C.c_void_p, _fp, C.c_int]),
    ("rtmi_add_parallelepiped", C.c_int, [C.c_void_p, _fp, C.c_int]),
    ("rtmi_add_parallelepiped_lengths", C.c_int, [C.c_void_p, _fp, C.c_int, TRANSFORM_FN, C.c_void_p]),
    ("rtmi_add_parallelepiped_faces", C.c_int, [C.c_void_p, _fp, C.c_int]),
    ("rtmi_add_sky", C.c_int, [C.c_void_p]),
    ("rtmi_list_begin", C.c_int, [C.c_void_p]),
    ("rtmi_list_end", C.c_int, [C.c_void_p]),
    ("rtmi_add_bvh", C.c_int, [C.c_void_p, _fp, _fp, C.c_int, C.c_int, C.c_int]),
    ("rtmi_camera_pinhole", C.c_int, [C.c_void_p, _fp, _fp, _fp, C.c_double, C.c_double]),
    ("rtmi_camera_defocus", C.c_int, [C.c_void_p, _fp, _fp, _fp, C.c_double, C.c_double, C.c_double, C.c_double]),
    ("rtmi_camera_raw", C.c_int, [C.c_void_p, _fp, _fp, _fp, _fp]),
    ("rtmi_camera_get", C.c_int, [C.c_void_p, _fp]),
    ("rtmi_camera_set", C.c_int, [C.c_void_p, _fp, C.c_int, C.c_double]),
    ("rtmi_scene_commit", C.c_int, [C.c_void_p]),
    ("rtmi_scene_stats", C.c_int, [C.c_void_p, C.POINTER(C.c_int64)]),
    ("rtmi_scene_bytes_per_ray", C.c_int64, [C.c_void_p]),
    ("rtmi_scene_sliver_faces", C.c_int64, [C.c_void_p]),
    ("rtmi_frame_work_items", C.c_int64, [_frp]),
    ("rtmi_frame_pixel_of", C.c_int64, [_frp, C.c_int64]),
    ("rtmi_frame_pixel_map", C.c_int, [_frp, C.POINTER(C.c_int64)]),
    ("rtmi_states_bytes", C.c_size_t, [_frp]),
    ("rtmi_tiles_bytes", C.c_size_t, [_frp]),
    ("rtmi_rng_init", C.c_int, [C.c_uint64, _frp, C.c_void_p, C.c_void_p]),
    ("rtmi_rng_host_state", C.c_int, [C.c_uint64, C.c_uint64, _u32p]),
    ("rtmi_rng_host_random_float", C.c_float, [C.c_float, C.c_float, _u32p]),
    ("rtmi_rng_set_state", C.c_int, [_frp, C.c_void_p, C.c_int64, _u32p, C.c_void_p]),
    ("rtmi_rng_get_state", C.c_int, [_frp, C.c_void_p, C.c_int64, _u32p, C.c_void_p]),
    ("rtmi_render", C.c_int, [C.c_void_p, _frp, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    ("rtmi_render_ex", C.c_int, [C.c_void_p, _frp, C.POINTER(RenderOpts), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    ("rtmi_render_scratch_bytes", C.c_size_t, [_frp]),
    ("rtmi_render_launch_shape", C.c_int, [C.c_void_p, _frp, C.POINTER(RenderOpts), C.POINTER(C.c_int32)]),
    ("rtmi_render_mode", C.c_int, [C.c_void_p, _frp, C.POINTER(RenderOpts), C.POINTER(C.c_int32)]),
    ("rtmi_render_mode_ex", C.c_int, [C.c_void_p, _frp, C.POINTER(RenderOpts), C.POINTER(C.c_int32), C.c_int]),
    ("rtmi_fast_path_kernel", C.c_int, [C.POINTER(C.c_int32)]),
    ("rtmi_render_status", C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(C.c_uint64), C.c_void_p]),
    ("rtmi_last_ray_total", C.c_int, [C.c_void_p, C.POINTER(C.c_uint64), C.c_void_p]),
    ("rtmi_debug_counters", C.c_int, [C.c_void_p, C.POINTER(C.c_ulonglong), C.c_void_p]),
    ("rtmi_debug_counters_ex", C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(C.c_ulonglong), C.c_void_p]),
    ("rtmi_debug_scratch_regions", C.c_int, [_frp, C.POINTER(C.c_int64), C.c_int]),
    ("rtmi_debug_schedule", C.c_int, [_frp, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_int, C.c_uint32, C.c_int, C.c_int,
                                      C.POINTER(C.c_int32), C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p]),
    ("rtmi_gather", C.c_int, [C.c_void_p, _frp, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]),
    ("rtmi_reduce_sum", C.c_int, [C.c_void_p, _frp, C.c_void_p, C.c_int, C.c_void_p]),
    ("rtmi_untile", C.c_int, [_frp, C.c_void_p, C.c_void_p, C.c_void_p]),
    ("rtmi_untile_u32", C.c_int, [_frp, C.c_void_p, C.c_void_p, C.c_void_p]),
    ("rtmi_post_process", C.c_int, [C.c_void_p, C.c_int64, C.c_int, C.c_void_p]),
    ("rtmi_get_workload", C.c_int, [C.c_int, C.c_int, C.c_int]),
    ("rtmi_selftest_arithmetic", C.c_int, [C.POINTER(C.c_ulonglong)]),
    ("rtmi_set_launch", C.c_int, [C.c_int, C.c_int]),
    ("rtmi_set_schedule", C.c_int, [C.c_int]),
    ("rtmi_intersect", C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                 C.c_void_p]),
    ("rtmi_occluded", C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                C.c_void_p]),
    ("rtmi_trace", C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                             C.c_void_p, C.c_void_p]),
    ("rtmi_rng_init_n", C.c_int, [C.c_uint64, C.c_uint64, C.c_int64, C.c_void_p, C.c_void_p]),
    ("rtmi_render_budget", C.c_int, [C.c_void_p, _frp, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                     C.c_void_p, C.c_void_p, C.c_void_p]),
    ("rtmi_budget_plan", C.c_int, [_frp, C.POINTER(AdaptiveOpts), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                   C.c_void_p, C.c_void_p]),
    ("rtmi_resolve", C.c_int, [_frp, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]),
    ("rtmi_render_features", C.c_int, [C.c_void_p, _frp, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                       C.c_void_p, C.POINTER(Features), C.c_void_p, C.c_void_p]),
    ("rtmi_resolve_features", C.c_int, [_frp, C.POINTER(Features), C.c_void_p, C.POINTER(Features), C.c_void_p]),
    ("rtmi_resolve_variance", C.c_int, [_frp, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    ("rtmi_denoise_scratch_bytes", C.c_size_t, [C.c_int, C.c_int]),
    ("rtmi_denoise", C.c_int, [C.c_int, C.c_int, C.POINTER(DenoiseOpts), C.c_void_p, C.POINTER(DenoiseGuides), C.c_void_p,
                               C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    ("rtmi_camera_update", C.c_int, [C.c_void_p, _fp, C.c_int, C.c_double]),
    ("rtmi_history_bytes", C.c_size_t, [C.c_int, C.c_int]),
    ("rtmi_accumulate", C.c_int, [C.c_int, C.c_int, C.POINTER(AccumulateOpts), C.c_void_p, C.POINTER(DenoiseGuides), _fp,
                                  C.c_void_p, _fp, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    ("rtmi_camera_rays", C.c_int, [C.c_void_p, _frp, C.POINTER(Projection), C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p,
                                   C.c_void_p, C.c_void_p]),
    ("rtmi_sample_add", C.c_int, [_frp, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                  C.c_void_p, C.c_void_p]),
    ("rtmi_bounce", C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                              C.c_void_p, C.c_void_p, C.c_void_p]),
    ("rtmi_path_fold", C.c_int, [C.c_int64, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    ("rtmi_path_compact_scratch_bytes", C.c_size_t, [C.c_int64]),
    ("rtmi_path_compact", C.c_int, [C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p,
                                    C.c_void_p, C.c_void_p, C.c_void_p]),
    ("rtmi_bounce_list", C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p,
                                   C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    ("rtmi_scene_light_count", C.c_int64, [C.c_void_p]),
    ("rtmi_scene_lights", C.c_int, [C.c_void_p, C.c_void_p, C.c_int64]),
    ("rtmi_direct_sample", C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_uint32, C.c_int] +
                                    [C.c_void_p] * 14),
    ("rtmi_path_fold_direct", C.c_int, [C.c_int64, C.c_int] + [C.c_void_p] * 8),
    ("rtmi_direct_sample_mis", C.c_int, [C.c_void_p, C.POINTER(DirectSampleMisArgs), C.c_void_p]),
    ("rtmi_occluded_list", C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_int64] + [C.c_void_p] * 7),
    ("rtmi_path_advance", C.c_int, [C.c_void_p, _frp, C.POINTER(PathAdvanceArgs), C.c_void_p]),
]

# rtmi_light of include/rtmi.h, as a numpy record (88 bytes)
LIGHT_DTYPE = np.dtype([("p0", np.float32, 3), ("e1", np.float32, 3), ("e2", np.float32, 3), ("n", np.float32, 3),
                        ("emission", np.float32, 3), ("area", np.float32), ("cdf", np.float32), ("scale", np.float32),
                        ("kind", np.int32), ("entry", np.int32), ("element", np.int32), ("material", np.int32)])


def lib():
    """Load librtmi.so; raises RtmiError when it has not been built (no fallback)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RtmiError("%s is missing: build it with __graft_entry__.build() "
                            "(make -C ray-tracing-cuda_amd/csrc); there is no CPU fallback" % LIB_PATH)
        # PyTorch bundles its own HIP runtime (torch/lib/libamdhip64.so).  Import torch first so
        # librtmi.so binds to that already-loaded runtime; loading /opt/rocm's copy first would
        # put two HIP runtimes in one process and torch would then see no device.
        import torch  # noqa: F401
        L = C.CDLL(LIB_PATH)
        for name, res, args in SYMBOLS:
            fn = getattr(L, name)
            fn.restype = res
            fn.argtypes = args
        _lib = L
    return _lib


def _check(rc, what):
    if rc < 0:
        raise RtmiError("%s failed (%d): %s" % (what, rc, lib().rtmi_last_error().decode()))
    return rc


def _f(a):
    a = np.ascontiguousarray(np.asarray(a, dtype=np.float32).reshape(-1))
    return a, a.ctypes.data_as(_fp)


def make_frame(height, width, spp, max_depth=10, post=True, rank=0, world_size=1):
    return Frame(height, width, spp, max_depth, 1 if post else 0, rank, world_size)


def work_items(frame):
    return _check(lib().rtmi_frame_work_items(C.byref(frame)), "rtmi_frame_work_items")


def pixel_map(frame):
    """int64 array: global pixel index of each work item of this shard (-1 = padding)."""
    out = np.empty(work_items(frame), dtype=np.int64)
    _check(lib().rtmi_frame_pixel_map(C.byref(frame), out.ctypes.data_as(C.POINTER(C.c_int64))),
           "rtmi_frame_pixel_map")
    return out


SCRATCH_REGIONS = ("states", "rays", "cost", "order", "meta", "head", "work", "qcost", "qsorted", "qmap", "qmax", "fut", "next",
                   "claims", "first", "prio_tab", "params", "total")  # rtmi_debug_scratch_regions' order (RTMI_SCRATCH_REGIONS)


def scratch_regions(frame):
    """{region: byte offset} of a frame's render scratch, and its ``total`` size (rtmi_debug_scratch_regions; no GPU)."""
    out = (C.c_int64 * len(SCRATCH_REGIONS))()
    _check(lib().rtmi_debug_scratch_regions(C.byref(frame), out, len(SCRATCH_REGIONS)), "rtmi_debug_scratch_regions")
    return dict(zip(SCRATCH_REGIONS, (int(v) for v in out)))


def debug_schedule(frame, scratch, ray_counts, work_counts=None, pixel_head=False, sparse_cap=0, grid_waves=0, outlier_x10=20,
                   head_pct=(50, 25, 12), simds=0, rounds=0, spp=1, probe_spp=1):
    """The scheduler step of a scheduled render on the caller's own counts (rtmi_debug_schedule): ``scratch``, ``ray_counts``
    and ``work_counts`` are torch CUDA tensors; the plan is left in ``scratch`` (``scratch_regions``), the head's marks in
    ``ray_counts``.  On torch's current stream."""
    import torch
    with torch.cuda.device(scratch.device):
        _check(lib().rtmi_debug_schedule(C.byref(frame), C.c_void_p(scratch.data_ptr()), scratch.numel() * scratch.element_size(),
                                         C.c_void_p(ray_counts.data_ptr()),
                                         C.c_void_p(work_counts.data_ptr()) if work_counts is not None else None,
                                         1 if pixel_head else 0, int(sparse_cap), int(grid_waves), int(outlier_x10),
                                         (C.c_int32 * 3)(*head_pct), int(simds), int(rounds), int(spp), int(probe_spp),
                                         C.c_void_p(torch.cuda.current_stream().cuda_stream)), "rtmi_debug_schedule")


def get_workload(rank, world_size, spp):
    return lib().rtmi_get_workload(rank, world_size, spp)


class Hits(collections.namedtuple("Hits", "t uv normal material kind entry element")):
    """What ``SceneBuilder.intersect`` returns: views into one (N, 12) int32 buffer of rtmi_hit records (``raw``) --
    t (N,) float32 (+inf: no hit), uv (N, 2) float32, normal (N, 3) float32, material / kind / entry / element (N,)
    int32.  ``check()`` waits for the query and raises when it abandoned a mesh search (its answers are then not to
    be used)."""

    def check(self):
        n = int(self.abandoned.item())  # (a device-to-host copy: waits for the query)
        if n:
            raise RtmiError("rtmi_intersect abandoned %d mesh search(es): the answers are incomplete" % n)
        return self


class Occlusion:
    """What ``SceneBuilder.occluded`` returns: ``mask`` (N,) torch.bool, a view of the (N,) uint8 output ``raw`` (1:
    occluded).  ``check()`` waits for the query and raises when it abandoned a mesh search (the answers are then not
    to be used); ``fallback_rays()`` is how many rays the exact unbounded fallback answered (rtmi_occluded's
    d_counts[1])."""

    def __init__(self, raw, counts, rays):
        import torch
        self.raw, self.counts = raw, counts
        self.mask = raw.view(torch.bool)
        self._rays = rays  # (kept alive while the query may still read them)

    def check(self):
        n = int(self.counts[0].item())  # (a device-to-host copy: waits for the query)
        if n:
            raise RtmiError("rtmi_occluded abandoned %d mesh search(es): the answers are incomplete" % n)
        return self

    def fallback_rays(self):
        return int(self.counts[1].item())


class Trace:
    """What ``SceneBuilder.trace`` returns: ``rgb`` (N, 3) float32, each ray's raw radiance estimate (no
    post-processing); ``rays`` (N,) int32 closest-hit queries per ray, or None when they were not asked for; ``work``
    the call's (RTMI_TRACE_WORK_WORDS,) int64 device words.  ``check()`` waits for the call and raises when it abandoned
    a mesh search (the answers are then not to be used); ``total_rays()`` is the queries of all rays."""

    def __init__(self, rgb, rays, work, keep):
        self.rgb, self.rays, self.work = rgb, rays, work
        self._keep = keep  # (kept alive while the call may still read them)

    def check(self):
        n = int(self.work[0].item())  # (a device-to-host copy: waits for the call)
        if n:
            raise RtmiError("rtmi_trace abandoned %d mesh search(es): the answers are incomplete" % n)
        return self

    def total_rays(self):
        return int(self.work[1].item())


class Bounce:
    """What ``SceneBuilder.bounce`` returns: ``emitted`` and ``attenuation`` (N, 3) float32; ``hits`` the step's ``Hits``
    (views into an (N, 12) int32 buffer, ``hits.raw``) or None when they were not asked for; ``steps`` (N,) int32, each
    path's step count so far, or None; ``work`` the call's (RTMI_TRACE_WORK_WORDS,) int64 device words; ``origins``,
    ``directions`` and ``states``: the caller's tensors, which now hold the scattered rays.  ``check()`` waits for the call
    and raises when it abandoned a mesh search (the answers are then not to be used); ``stepped()`` is how many paths
    the call stepped.  ``paths``: the ``Paths`` a ``bounce_list`` stepped (None: every path was a candidate)."""

    def __init__(self, origins, directions, states, emitted, attenuation, hits, steps, work, paths=None):
        self.origins, self.directions, self.states = origins, directions, states
        self.emitted, self.attenuation, self.hits, self.steps, self.work = emitted, attenuation, hits, steps, work
        self.paths = paths

    def check(self):
        n = int(self.work[0].item())  # (a device-to-host copy: waits for the call)
        if n:
            raise RtmiError("rtmi_bounce abandoned %d mesh search(es): the answers are incomplete" % n)
        return self

    def stepped(self):
        return int(self.work[1].item())


class Steps(collections.namedtuple("Steps", "rgb steps alive origins directions emitted attenuation works direct occluded flags",
                                   defaults=(None, None, None))):
    """What ``SceneBuilder.trace_steps`` returns: ``rgb`` (N, 3) float32, the folded radiance; ``steps`` (N,) int32, the
    steps each path made; ``alive`` (N,) bool, the paths whose direction is still non-zero (``steps + alive`` is
    rtmi_trace's ray count); ``origins`` / ``directions``: the loop's own copies of the rays as the last step left them;
    ``emitted`` / ``attenuation``: the (max(max_depth, 1), N, 3) float32 layer stacks; ``works``: every step's work words.
    With ``direct=True`` also ``direct`` (layers, N, 3) float32, ``occluded`` (layers, N) uint8 -- the stacks
    ``path_fold_direct`` read -- and ``flags`` (N,) int32; else None.  With ``direct="mis"`` the attribute ``carry`` is the
    loop's one (N, 4) float32 carry tensor, else None: an attribute beside the tuple's fields, so that unpacking a ``Steps``
    gives what it gave.  ``check()`` waits for the loop and raises when a step abandoned a mesh search."""

    carry = None

    def check(self):
        for k, w in enumerate(self.works):
            n = int(w[0].item())
            if n:
                raise RtmiError("rtmi_bounce abandoned %d mesh search(es) in step %d: the answers are incomplete" % (n, k))
        return self


def path_fold(directions, steps, emitted_stack, attenuation_stack, out=None):
    """Trace's return expression over the layers the steps wrote (rtmi_path_fold), enqueued on torch's current stream.

    ``directions`` (N, 3) float32: the paths' directions after the last step (a zero vector: the path ended); ``steps``
    (N,) int32; ``emitted_stack`` / ``attenuation_stack``: contiguous (layers, N, 3) float32, layer k what step k wrote,
    1 <= layers <= 64.  All CUDA tensors on one device.  ``out``: an optional (N, 3) float32 tensor to write into.  Returns
    the radiance."""
    try:
        import torch
    except ImportError:
        raise RtmiError("directions: torch is needed for rtmi_path_fold")
    if not (isinstance(directions, torch.Tensor) and directions.is_cuda and directions.dtype == torch.float32 and
            directions.dim() == 2 and directions.shape[1] == 3 and directions.is_contiguous()):
        raise RtmiError("directions must be a contiguous CUDA float32 tensor of shape (N, 3): rtmi_path_fold has no CPU path")
    n, dev = int(directions.shape[0]), directions.device
    if not _is_buffer(steps, (n,), dev, torch.int32):
        raise RtmiError("steps must be a contiguous CUDA int32 tensor of shape (N,) on the directions' device")
    if not (isinstance(emitted_stack, torch.Tensor) and emitted_stack.dim() == 3 and 1 <= emitted_stack.shape[0] <= MAX_DEPTH):
        raise RtmiError("emitted_stack must have shape (layers, N, 3) with 1 <= layers <= %d" % MAX_DEPTH)
    layers = int(emitted_stack.shape[0])
    for name, t in (("emitted_stack", emitted_stack), ("attenuation_stack", attenuation_stack)):
        if not _is_buffer(t, (layers, n, 3), dev, torch.float32):
            raise RtmiError("%s must be a contiguous CUDA float32 tensor of shape (layers, N, 3) on the directions' device" % name)
    out = _out_buffer(out, "float32 tensor of shape (N, 3)", (n, 3), dev, torch.float32)
    with torch.cuda.device(dev):
        _check(lib().rtmi_path_fold(n, layers, C.c_void_p(directions.data_ptr()), C.c_void_p(steps.data_ptr()),
                                    C.c_void_p(emitted_stack.data_ptr()), C.c_void_p(attenuation_stack.data_ptr()),
                                    C.c_void_p(out.data_ptr()), C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)),
               "rtmi_path_fold")
    return out


def path_fold_direct(directions, steps, emitted_stack, attenuation_stack, direct_stack, occluded_stack, out=None):
    """``path_fold`` with the direct light of every layer added where its shadow ray was clear (rtmi_path_fold_direct):
    wherever that fold reads E[k] this one reads ``occluded[k] ? E[k] : E[k] + D[k]``.  ``direct_stack``: contiguous
    (layers, N, 3) float32, layer k what ``SceneBuilder.direct_sample`` wrote after step k; ``occluded_stack``: contiguous
    (layers, N) uint8 or bool, what ``SceneBuilder.occluded`` answered for layer k's shadow rays.  The rest as ``path_fold``."""
    try:
        import torch
    except ImportError:
        raise RtmiError("directions: torch is needed for rtmi_path_fold_direct")
    if not (isinstance(directions, torch.Tensor) and directions.is_cuda and directions.dtype == torch.float32 and
            directions.dim() == 2 and directions.shape[1] == 3 and directions.is_contiguous()):
        raise RtmiError("directions must be a contiguous CUDA float32 tensor of shape (N, 3): rtmi_path_fold_direct has no CPU path")
    n, dev = int(directions.shape[0]), directions.device
    if not _is_buffer(steps, (n,), dev, torch.int32):
        raise RtmiError("steps must be a contiguous CUDA int32 tensor of shape (N,) on the directions' device")
    if not (isinstance(emitted_stack, torch.Tensor) and emitted_stack.dim() == 3 and 1 <= emitted_stack.shape[0] <= MAX_DEPTH):
        raise RtmiError("emitted_stack must have shape (layers, N, 3) with 1 <= layers <= %d" % MAX_DEPTH)
    layers = int(emitted_stack.shape[0])
    for name, t in (("emitted_stack", emitted_stack), ("attenuation_stack", attenuation_stack), ("direct_stack", direct_stack)):
        if not _is_buffer(t, (layers, n, 3), dev, torch.float32):
            raise RtmiError("%s must be a contiguous CUDA float32 tensor of shape (layers, N, 3) on the directions' device" % name)
    if not _is_buffer(occluded_stack, (layers, n), dev, torch.uint8, torch.bool):
        raise RtmiError("occluded_stack must be a contiguous CUDA uint8 or bool tensor of shape (layers, N) on the directions' device")
    out = _out_buffer(out, "float32 tensor of shape (N, 3)", (n, 3), dev, torch.float32)
    with torch.cuda.device(dev):
        _check(lib().rtmi_path_fold_direct(n, layers, _ptr(directions), _ptr(steps), _ptr(emitted_stack), _ptr(attenuation_stack),
                                           _ptr(direct_stack), _ptr(occluded_stack), _ptr(out),
                                           C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)), "rtmi_path_fold_direct")
    return out


DirectSample = collections.namedtuple("DirectSample", "origins directions t_max direct flags counts carry", defaults=(None,))
"""What ``SceneBuilder.direct_sample`` returns: the shadow rays ``origins`` / ``directions`` (N, 3) float32 and ``t_max``
(N,) float32 -- a zero direction where a path has none, which ``occluded`` answers "clear" --, ``direct`` (N, 3) float32,
the unoccluded contribution, ``flags`` (N,) int32 and ``counts`` (2,) int64: paths sampled, emissions dropped (with
``mis=True``: weighed); ``carry`` (N, 4) float32 with ``mis=True``, else None."""


class Paths:
    """A list of path indices on the device, as ``path_compact`` makes it and ``SceneBuilder.bounce_list`` steps it:
    ``index``, a contiguous int32 CUDA tensor whose length is the list's CAPACITY; ``count``, a 1-element int32 CUDA tensor
    holding how many of its leading entries are the list (None: all of them).  The count stays on the device; ``n()``
    reads it back, which waits for the call that writes it."""

    def __init__(self, index, count=None):
        self.index, self.count = index, count
        self._keep = None  # (what the call that fills the list may still read)

    def n(self):
        cap = int(self.index.shape[0])
        return cap if self.count is None else min(cap, int(self.count.item()))


def _list_args(paths, n, dev, what="paths"):
    """(index tensor or None, n_list, count tensor or None) of a ``Paths`` (None: the identity over all n paths)."""
    import torch
    if paths is None:
        return None, n, None
    if not isinstance(paths, Paths):
        raise RtmiError("%s must be an rtmi.Paths or None" % what)
    idx, cnt = paths.index, paths.count
    if not (isinstance(idx, torch.Tensor) and idx.is_cuda and idx.dtype == torch.int32 and idx.dim() == 1 and
            idx.is_contiguous() and idx.device == dev):
        raise RtmiError("%s.index must be a contiguous CUDA int32 tensor of shape (capacity,) on the rays' device" % what)
    if cnt is not None and not _is_buffer(cnt, (1,), dev, torch.int32):
        raise RtmiError("%s.count must be a CUDA int32 tensor of shape (1,) on the rays' device, or None" % what)
    if int(idx.shape[0]) > 0x7fffffff:
        raise RtmiError("%s.index holds more than 2^31 - 1 entries" % what)
    return idx, int(idx.shape[0]), cnt


def _ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _path_compact(n, origins, directions, idx, n_list, cnt, out, dev):
    """rtmi_path_compact on checked arguments, with a scratch of its own, on torch's current stream."""
    import torch
    words = lib().rtmi_path_compact_scratch_bytes(n_list) // 4
    scratch = torch.empty((max(words, 1),), dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        _check(lib().rtmi_path_compact(n, _ptr(origins), _ptr(directions), _ptr(idx), n_list, _ptr(cnt), _ptr(out.index),
                                       _ptr(out.count), _ptr(scratch),
                                       C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)), "rtmi_path_compact")
    out._keep = (origins, directions, idx, cnt, scratch)
    return out


def path_compact(origins, directions, paths=None, out=None):
    """The live paths among ``paths`` as a list, in the list's own order (rtmi_path_compact), enqueued on torch's
    current stream; nothing is read back.

    ``origins`` / ``directions``: CUDA float32 (N, 3) tensors, only read.  A path is live exactly when the next step
    would step it (``SceneBuilder.bounce``'s bad rays, ended paths among them, are not).  ``paths``: the candidates, a
    ``Paths`` (entries >= N are dropped), or None for all N paths.  ``out``: an optional ``Paths`` to write into, with a
    count tensor and room for every candidate, and not ``paths`` itself (two lists are ping-ponged).  Returns the
    ``Paths``: ascending indices for ascending (or no) ``paths``."""
    import torch
    n, dev, _ = _check_batch("rtmi_path_compact", origins, directions)
    idx, n_list, cnt = _list_args(paths, n, dev)
    if out is None:
        out = Paths(torch.empty((n_list,), dtype=torch.int32, device=dev), torch.empty((1,), dtype=torch.int32, device=dev))
    else:
        o_idx, o_cap, o_cnt = _list_args(out, n, dev, "out")
        if o_idx is None or o_cnt is None or o_cap < n_list:
            raise RtmiError("out must be an rtmi.Paths with a count tensor and room for every candidate (%d)" % n_list)
        if (idx is not None and o_idx.data_ptr() == idx.data_ptr() and n_list > 0) or \
                (cnt is not None and o_cnt.data_ptr() == cnt.data_ptr()):
            raise RtmiError("out must not be paths: rtmi_path_compact reads one list while it writes the other")
    return _path_compact(n, origins.contiguous(), directions.contiguous(), idx, n_list, cnt, out, dev)


class Adaptive(collections.namedtuple("Adaptive", "tiles samples passes total_samples features", defaults=(None,))):
    """What ``Renderer.render_adaptive`` returns: ``tiles`` (items, 3) float32, the resolved tile buffer; ``samples``
    (items,) int32, the samples each work item got; ``passes`` rendered; ``total_samples`` over the shard;
    ``features``: with ``features=True`` the resolved ``ResolvedFeatures``, else None."""


ResolvedFeatures = collections.namedtuple("ResolvedFeatures", "albedo normal depth alpha")
"""What ``Renderer.resolve_features`` returns, tile-major: ``albedo`` and ``normal`` (items, 3) float32 (the mean normal
is not renormalised), ``depth`` (items,) float32 (the mean over the samples that hit a surface, 0 where none did),
``alpha`` (items,) float32 (the share of the samples that hit a surface)."""


def rng_states(seed, n, first=0, device=None):
    """(6, n) int32 CUDA tensor of RNG states: curand_init(seed, first + i, 0) for ray i (rtmi_rng_init_n), in the
    layout ``SceneBuilder.trace`` reads.  ``device``: a CUDA device (default: torch's current one)."""
    import torch
    n, first = int(n), int(first)
    if n < 0 or first < 0 or first + n > 1 << 40:
        raise RtmiError("rng_states: n and first must be >= 0 with first + n <= 2^40")
    dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
    if dev.type != "cuda":
        raise RtmiError("rng_states: the states live on a GPU (device %s)" % dev)
    out = torch.empty((STATE_WORDS, n), dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
        _check(lib().rtmi_rng_init_n(C.c_uint64(int(seed) & (2**64 - 1)), C.c_uint64(first), n,
                                     C.c_void_p(out.data_ptr()), stream), "rtmi_rng_init_n")
    return out


def denoise(color, variance, normal, depth, alpha, albedo=None, iterations=DENOISE_DEFAULTS["iterations"],
            sigma_color=DENOISE_DEFAULTS["sigma_color"], sigma_depth=DENOISE_DEFAULTS["sigma_depth"],
            normal_squarings=DENOISE_DEFAULTS["normal_squarings"], demodulate=None, out=None, return_variance=False):
    """The variance- and feature-guided a-trous filter (rtmi_denoise; the rule is in include/rtmi.h), enqueued on torch's
    current stream.  Row-major contiguous CUDA float32 tensors on one device: ``color``, ``variance`` (of the pixel MEAN:
    ``Renderer.resolve_variance``), ``normal`` (the mean normal, not renormalised) and ``albedo`` (H, W, 3); ``depth`` and
    ``alpha`` (H, W).  Defaults: 5 iterations (steps 1, 2, 4, 8, 16 pixels), ``sigma_color`` 1 (standard errors of the two
    pixels), ``sigma_depth`` 0.05 (of the pixel's depth), 0 ``normal_squarings`` (the plain cosine of the mean normals, whose
    lengths are the pixels' coverage: a power of it lets covered neighbours outweigh a silhouette pixel itself).
    ``demodulate``: filter colour / albedo and multiply back; None means "when albedo is given".  ``out``: an optional
    (H, W, 3) tensor to write into, which may be ``color`` itself.  The call allocates its own scratch.  Returns the
    filtered image, or with ``return_variance`` (image, what is left of the variance)."""
    try:
        import torch
    except ImportError:
        raise RtmiError("color: torch is needed for rtmi_denoise")
    if not (isinstance(color, torch.Tensor) and color.is_cuda and color.dim() == 3 and color.shape[2] == 3):
        raise RtmiError("color must be a CUDA float32 tensor of shape (H, W, 3): rtmi_denoise has no CPU path")
    h, w, dev = int(color.shape[0]), int(color.shape[1]), color.device
    demodulate = (albedo is not None) if demodulate is None else bool(demodulate)
    if demodulate and albedo is None:
        raise RtmiError("demodulate needs an albedo")
    for name, t, shape in (("color", color, (h, w, 3)), ("variance", variance, (h, w, 3)), ("normal", normal, (h, w, 3)),
                           ("depth", depth, (h, w)), ("alpha", alpha, (h, w)), ("albedo", albedo, (h, w, 3))):
        if t is not None and not _is_buffer(t, shape, dev, torch.float32):
            raise RtmiError("%s must be a contiguous CUDA float32 tensor of shape %s on color's device" % (name, shape))
    if out is None:
        out = torch.empty((h, w, 3), dtype=torch.float32, device=dev)
    elif not _is_buffer(out, (h, w, 3), dev, torch.float32):
        raise RtmiError("out must be a contiguous CUDA float32 tensor of shape (H, W, 3) on color's device")
    out_var = torch.empty((h, w, 3), dtype=torch.float32, device=dev) if return_variance else None
    o = DenoiseOpts(C.sizeof(DenoiseOpts), int(iterations), int(normal_squarings), 1 if demodulate else 0,
                    float(sigma_color), float(sigma_depth))
    g = DenoiseGuides(C.sizeof(DenoiseGuides), 0, variance.data_ptr(), albedo.data_ptr() if albedo is not None else None,
                      normal.data_ptr(), depth.data_ptr(), alpha.data_ptr())
    L = lib()
    nbytes = int(L.rtmi_denoise_scratch_bytes(h, w))  # (0 for an extent the call refuses: it says why)
    # (freed on return, while the call is still queued: the caching allocator hands the block out again in this stream's order)
    scratch = torch.empty((max(nbytes, 16),), dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        _check(L.rtmi_denoise(h, w, C.byref(o), C.c_void_p(color.data_ptr()), C.byref(g), C.c_void_p(out.data_ptr()),
                              C.c_void_p(out_var.data_ptr()) if out_var is not None else None,
                              C.c_void_p(scratch.data_ptr()), nbytes,
                              C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)), "rtmi_denoise")
    return (out, out_var) if return_variance else out


def _camera21(camera, name):
    a = np.ascontiguousarray(np.asarray(camera, dtype=np.float32).reshape(-1))
    if a.size != 21:
        raise RtmiError("%s must hold the 21 floats of rtmi_camera_get" % name)
    return a


def accumulate(color, variance, normal, depth, alpha, camera, history=None, prev_camera=None, out_history=None, **opts):
    """Temporal accumulation (rtmi_accumulate; the rule is in include/rtmi.h), enqueued on torch's current stream.  Row-major
    contiguous CUDA float32 tensors on one device, as for ``denoise``: ``color``, ``variance`` and ``normal`` (H, W, 3),
    ``depth`` and ``alpha`` (H, W).  ``camera``: this frame's, the 21 floats of ``SceneBuilder.camera_get`` (any shape).
    ``history`` and ``prev_camera``: what the previous call returned as its history, and the camera of that frame; both None
    for the first frame.  ``out_history``: an optional uint8 tensor of ``rtmi_history_bytes(H, W)`` bytes to write the new
    history into (never ``history`` itself).  ``opts``: normal_min, depth_tolerance, min_blend (ACCUMULATE_DEFAULTS).
    Returns (color, variance, length, history): the accumulated image and its variance (H, W, 3), the number of frames
    each pixel holds (H, W), and the new history, a uint8 tensor that only the next call can read."""
    try:
        import torch
    except ImportError:
        raise RtmiError("color: torch is needed for rtmi_accumulate")
    if not (isinstance(color, torch.Tensor) and color.is_cuda and color.dim() == 3 and color.shape[2] == 3):
        raise RtmiError("color must be a CUDA float32 tensor of shape (H, W, 3): rtmi_accumulate has no CPU path")
    unknown = set(opts) - set(ACCUMULATE_DEFAULTS)
    if unknown:
        raise RtmiError("rtmi.accumulate has no option %s" % ", ".join(sorted(unknown)))
    opts = dict(ACCUMULATE_DEFAULTS, **opts)
    h, w, dev = int(color.shape[0]), int(color.shape[1]), color.device
    for name, t, shape in (("color", color, (h, w, 3)), ("variance", variance, (h, w, 3)), ("normal", normal, (h, w, 3)),
                           ("depth", depth, (h, w)), ("alpha", alpha, (h, w))):
        if not _is_buffer(t, shape, dev, torch.float32):
            raise RtmiError("%s must be a contiguous CUDA float32 tensor of shape %s on color's device" % (name, shape))
    if (history is None) != (prev_camera is None):
        raise RtmiError("history and prev_camera go together: both None (the first frame) or neither")
    L = lib()
    nbytes = int(L.rtmi_history_bytes(h, w))  # (0 for an extent the call refuses: it says why)
    for name, t in (("history", history), ("out_history", out_history)):
        if t is not None and not _is_buffer(t, (nbytes,), dev, torch.uint8):
            raise RtmiError("%s must be a contiguous CUDA uint8 tensor of rtmi_history_bytes(H, W) = %d bytes on color's device"
                            % (name, nbytes))
    if out_history is None:
        out_history = torch.empty((max(nbytes, 16),), dtype=torch.uint8, device=dev)[:nbytes]
    elif history is not None and out_history.data_ptr() == history.data_ptr():
        raise RtmiError("out_history must not be history: the call reads one while it writes the other")
    cur = _camera21(camera, "camera")
    prev = _camera21(prev_camera, "prev_camera") if prev_camera is not None else None
    out = torch.empty((h, w, 3), dtype=torch.float32, device=dev)
    out_var = torch.empty((h, w, 3), dtype=torch.float32, device=dev)
    length = torch.empty((h, w), dtype=torch.float32, device=dev)
    o = AccumulateOpts(C.sizeof(AccumulateOpts), 0, float(opts["normal_min"]), float(opts["depth_tolerance"]),
                       float(opts["min_blend"]))
    g = DenoiseGuides(C.sizeof(DenoiseGuides), 0, variance.data_ptr(), None, normal.data_ptr(), depth.data_ptr(), alpha.data_ptr())
    with torch.cuda.device(dev):
        _check(L.rtmi_accumulate(h, w, C.byref(o), C.c_void_p(color.data_ptr()), C.byref(g), cur.ctypes.data_as(_fp),
                                 C.c_void_p(history.data_ptr()) if history is not None else None,
                                 prev.ctypes.data_as(_fp) if prev is not None else None, C.c_void_p(out_history.data_ptr()),
                                 C.c_void_p(out.data_ptr()), C.c_void_p(out_var.data_ptr()), C.c_void_p(length.data_ptr()),
                                 C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)), "rtmi_accumulate")
    return out, out_var, length, out_history


class Accumulator:
    """A sequence's accumulation state: the two histories ``rtmi.accumulate`` swaps between, and the previous frame's camera.
    ``height``, ``width``: the frames' extent; ``device``: a CUDA device (default: torch's current one); ``opts``:
    rtmi.accumulate's options, for every step."""

    def __init__(self, height, width, device=None, **opts):
        import torch
        unknown = set(opts) - set(ACCUMULATE_DEFAULTS)
        if unknown:
            raise RtmiError("rtmi.accumulate has no option %s" % ", ".join(sorted(unknown)))
        self.height, self.width, self.opts = int(height), int(width), opts
        self.device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        nbytes = int(lib().rtmi_history_bytes(self.height, self.width))
        if nbytes == 0:
            raise RtmiError("height and width must be within 1..65535 (RTMI_MAX_EXTENT)")
        self._histories = [torch.empty((nbytes,), dtype=torch.uint8, device=self.device) for _ in range(2)]
        self.reset()

    def reset(self):
        """Forget the history: the next step is a first frame."""
        self.frames = 0
        self._prev_camera = None
        return self

    def step(self, color, variance, normal, depth, alpha, camera):
        """Accumulate one frame seen from ``camera`` (rtmi.accumulate's arguments) and swap the histories.  Returns
        (color, variance, length)."""
        cur = _camera21(camera, "camera").copy()
        first = self._prev_camera is None
        out, var, length, _ = accumulate(color, variance, normal, depth, alpha, cur,
                                         history=None if first else self._histories[0], prev_camera=self._prev_camera,
                                         out_history=self._histories[1], **self.opts)
        self._histories.reverse()
        self._prev_camera = cur
        self.frames += 1
        return out, var, length

    @property
    def history(self):
        """The history the last step wrote (what the next one reads)."""
        return self._histories[0]


class SceneBuilder:
    """Builder protocol of rtmi/scenes.py over the C ABI's scene recorder.

    ``seed`` seeds the host copy of pixel 0's RNG stream that scene programs may draw
    from (scenes/spheres.cu:105); ``Renderer`` stores the advanced state back into the
    device state of pixel 0 so rendering continues that stream (quirk g5)."""

    def __init__(self, seed=0):
        self.L = lib()
        self.h = C.c_void_p(self.L.rtmi_scene_create())
        self.seed = seed
        self._keep = []
        self.state0 = np.zeros(STATE_WORDS, dtype=np.uint32)
        _check(self.L.rtmi_rng_host_state(C.c_uint64(seed), C.c_uint64(0), self.state0.ctypes.data_as(_u32p)),
               "rtmi_rng_host_state")
        self.state0_fresh = self.state0.copy()

    def __del__(self):
        try:
            self.L.rtmi_scene_destroy(self.h)
        except Exception:
            pass

    def constant_texture(self, rgb):
        return _check(self.L.rtmi_constant_texture(self.h, _f(rgb)[1]), "rtmi_constant_texture")

    def image_texture(self, rgba):
        rgba = np.ascontiguousarray(rgba, dtype=np.uint8)
        return _check(self.L.rtmi_image_texture(self.h, rgba.ctypes.data_as(C.POINTER(C.c_uint8)), rgba.shape[0],
                                                rgba.shape[1], rgba.shape[1] * 4), "rtmi_image_texture")

    def lambertian(self, rgb):
        return _check(self.L.rtmi_lambertian(self.h, _f(rgb)[1]), "rtmi_lambertian")

    def lambertian_tex(self, tex):
        return _check(self.L.rtmi_lambertian_tex(self.h, tex), "rtmi_lambertian_tex")

    def metal(self, rgb, fuzz):
        return _check(self.L.rtmi_metal(self.h, _f(rgb)[1], C.c_float(float(fuzz))), "rtmi_metal")

    def dielectric(self, rgb, index):
        return _check(self.L.rtmi_dielectric(self.h, _f(rgb)[1], float(index)), "rtmi_dielectric")

    def diffuse_light(self, tex):
        return _check(self.L.rtmi_diffuse_light(self.h, tex), "rtmi_diffuse_light")

    def sphere(self, c, r, mat):
        _check(self.L.rtmi_add_sphere(self.h, _f(c)[1], float(r), mat), "rtmi_add_sphere")

    def triangle(self, p, mat):
        _check(self.L.rtmi_add_triangle(self.h, _f(p)[1], mat), "rtmi_add_triangle")

    def parallelogram(self, p, mat):
        _check(self.L.rtmi_add_parallelogram(self.h, _f(p)[1], mat), "rtmi_add_parallelogram")

    def parallelepiped(self, p, mat):
        _check(self.L.rtmi_add_parallelepiped(self.h, _f(p)[1], mat), "rtmi_add_parallelepiped")

    def parallelepiped_lengths(self, lengths, mat, transform):
        def cb(pin, pout, _user):
            o = transform(np.array([pin[0], pin[1], pin[2]], dtype=np.float32))
            pout[0], pout[1], pout[2] = float(o[0]), float(o[1]), float(o[2])

        cfn = TRANSFORM_FN(cb)
        self._keep.append(cfn)
        _check(self.L.rtmi_add_parallelepiped_lengths(self.h, _f(lengths)[1], mat, cfn, None),
               "rtmi_add_parallelepiped_lengths")

    def sky(self):
        _check(self.L.rtmi_add_sky(self.h), "rtmi_add_sky")

    def list_begin(self):
        """``l = new HitableList()`` appended to the list under construction; closed by list_end()."""
        _check(self.L.rtmi_list_begin(self.h), "rtmi_list_begin")

    def list_end(self):
        _check(self.L.rtmi_list_end(self.h), "rtmi_list_end")

    def bvh(self, faces, mat, uvs=None, k_min=2048):
        faces = np.ascontiguousarray(faces, dtype=np.float32).reshape(-1, 9)
        uvp = None
        if uvs is not None:
            uvs = np.ascontiguousarray(uvs, dtype=np.float32).reshape(-1, 6)
            uvp = uvs.ctypes.data_as(_fp)
        _check(self.L.rtmi_add_bvh(self.h, faces.ctypes.data_as(_fp), uvp, faces.shape[0],
                                   -1 if mat is None else mat, k_min), "rtmi_add_bvh")

    def camera_pinhole(self, pos, look_at, up, fov, aspect):
        _check(self.L.rtmi_camera_pinhole(self.h, _f(pos)[1], _f(look_at)[1], _f(up)[1], float(fov), float(aspect)),
               "rtmi_camera_pinhole")

    def camera_defocus(self, pos, look_at, up, fov, aspect, aperture, focus):
        _check(self.L.rtmi_camera_defocus(self.h, _f(pos)[1], _f(look_at)[1], _f(up)[1], float(fov), float(aspect),
                                          float(aperture), float(focus)), "rtmi_camera_defocus")

    def camera_raw(self, pos, llc, horiz, vert):
        _check(self.L.rtmi_camera_raw(self.h, _f(pos)[1], _f(llc)[1], _f(horiz)[1], _f(vert)[1]), "rtmi_camera_raw")

    def camera_get(self):
        out = np.zeros(21, dtype=np.float32)
        _check(self.L.rtmi_camera_get(self.h, out.ctypes.data_as(_fp)), "rtmi_camera_get")
        return out.reshape(7, 3)

    def camera_update(self, frame21, defocus=False, lens_radius=-1.0):
        """Move the camera (rtmi_camera_update): ``frame21`` is the 21 floats of ``camera_get``, any shape.  A committed
        scene stays committed, and nothing is uploaded; renders already enqueued keep the camera they were enqueued with."""
        f = _camera21(frame21, "frame21")
        _check(self.L.rtmi_camera_update(self.h, f.ctypes.data_as(_fp), 1 if defocus else 0, float(lens_radius)),
               "rtmi_camera_update")
        return self

    def camera_look(self, pos, look_at, up, fov, aspect):
        """``camera_update`` to a pinhole look-at camera (``camera_pinhole``'s arguments), whose 21 floats a throw-away
        scene makes: no device work."""
        tmp = C.c_void_p(self.L.rtmi_scene_create())
        try:
            _check(self.L.rtmi_camera_pinhole(tmp, _f(pos)[1], _f(look_at)[1], _f(up)[1], float(fov), float(aspect)),
                   "rtmi_camera_pinhole")
            f = np.zeros(21, dtype=np.float32)
            _check(self.L.rtmi_camera_get(tmp, f.ctypes.data_as(_fp)), "rtmi_camera_get")
        finally:
            self.L.rtmi_scene_destroy(tmp)
        return self.camera_update(f)

    def random_float(self, mn, mx):
        return np.float32(self.L.rtmi_rng_host_random_float(C.c_float(float(np.float32(mn))),
                                                            C.c_float(float(np.float32(mx))),
                                                            self.state0.ctypes.data_as(_u32p)))

    def stats(self):
        out = (C.c_int64 * 8)()
        _check(self.L.rtmi_scene_stats(self.h, out), "rtmi_scene_stats")
        keys = ["world", "spheres", "parallelograms", "triangles", "bvh_faces", "bvh_nodes", "materials", "textures"]
        return dict(zip(keys, list(out)))

    def list_records(self):
        """The culled list scan's records (rtmi_debug_list_records): (tri_pts uint32 (P, 2, 12), hot_tris uint32
        (P, 2, 16), corners float32 (P, 4, 3)) for the P pairs of the world list.  Host only."""
        fn = self.L.rtmi_debug_list_records  # (a diagnostic: bound here, so that lib() asks no A/B build for it)
        fn.restype, fn.argtypes = C.c_int64, [C.c_void_p, C.c_int64, _u32p, _u32p, _fp]
        n = _check(fn(self.h, 0, None, None, None), "rtmi_debug_list_records")
        tp, ht, co = np.zeros((n, 2, 12), np.uint32), np.zeros((n, 2, 16), np.uint32), np.zeros((n, 4, 3), np.float32)
        _check(fn(self.h, n, tp.ctypes.data_as(_u32p), ht.ctypes.data_as(_u32p), co.ctypes.data_as(_fp)), "rtmi_debug_list_records")
        return tp, ht, co

    def pair_slabs(self):
        """The pairs' bounds in both forms (rtmi_debug_pair_slabs): (slabs float32 (P + 1, 8): c[3], h[3], two spare
        words; boxes float32 (P + 1, 8): mn[3], mx[3], two spare words; list_mag) for the P pairs of the world list and
        the padding record behind them.  Host only."""
        fn = self.L.rtmi_debug_pair_slabs
        fn.restype, fn.argtypes = C.c_int64, [C.c_void_p, C.c_int64, _u32p, _u32p, _fp]
        n = _check(fn(self.h, 0, None, None, None), "rtmi_debug_pair_slabs")
        sl, bx, mag = np.zeros((n, 8), np.uint32), np.zeros((n, 8), np.uint32), np.zeros(1, np.float32)
        _check(fn(self.h, n, sl.ctypes.data_as(_u32p), bx.ctypes.data_as(_u32p), mag.ctypes.data_as(_fp)), "rtmi_debug_pair_slabs")
        return sl.view(np.float32), bx.view(np.float32), float(mag[0])

    def slab_reach(self):
        """Whether the slab table's reach covers a render from this scene's camera (rtmi_debug_slab_reach).  Host only."""
        fn = self.L.rtmi_debug_slab_reach
        fn.restype, fn.argtypes = C.c_int, [C.c_void_p]
        return bool(_check(fn(self.h), "rtmi_debug_slab_reach"))

    def render_lds_bytes(self, max_depth, threads=256):
        """Dynamic LDS per workgroup of a render of this scene (rtmi_debug_render_lds_bytes).  Host only."""
        fn = self.L.rtmi_debug_render_lds_bytes
        fn.restype, fn.argtypes = C.c_int64, [C.c_void_p, C.c_int, C.c_int]
        return _check(fn(self.h, max_depth, threads), "rtmi_debug_render_lds_bytes")

    def sliver_faces(self):
        return _check(self.L.rtmi_scene_sliver_faces(self.h), "rtmi_scene_sliver_faces")

    def bytes_per_ray(self):
        return _check(self.L.rtmi_scene_bytes_per_ray(self.h), "rtmi_scene_bytes_per_ray")

    def commit(self):
        _check(self.L.rtmi_scene_commit(self.h), "rtmi_scene_commit")
        self.device = None
        try:
            import torch
            if torch.cuda.is_available():
                self.device = torch.device("cuda", torch.cuda.current_device())
        except ImportError:
            pass
        return self

    def lights(self):
        """The committed scene's light table (rtmi_scene_lights): a numpy record array of dtype ``LIGHT_DTYPE`` with the
        fields p0, e1, e2, n, emission (each (L, 3) float32), area, cdf, scale (float32), kind, entry, element, material
        (int32) -- ``lights()["cdf"]`` and so on; length 0 when no world-list triangle or parallelogram emits."""
        n = _check(self.L.rtmi_scene_light_count(self.h), "rtmi_scene_light_count")
        out = np.zeros((n,), dtype=LIGHT_DTYPE)
        _check(self.L.rtmi_scene_lights(self.h, out.ctypes.data_as(C.c_void_p), n), "rtmi_scene_lights")
        return out

    def direct_sample(self, step, result, light_states, flags, sample=True, out=None, counts=None, mis=False, carry=None):
        """Next-event estimation after step number ``step`` of a loop (rtmi_direct_sample), on torch's current stream.

        ``result``: the ``Bounce`` of that step, made with ``hits=True``, ``steps`` and the layer tensors ``emitted`` /
        ``attenuation`` of the fold's stacks; its candidates are the step's (``result.paths``, or all N).  ``light_states``:
        a contiguous (6, N) int32 tensor of RNG states of their own (``rng_states`` with another seed, or ``first=N``),
        advanced by three draws per sampled path; ``flags``: an (N,) int32 tensor, zeroed once before the loop.
        ``sample=False`` (a loop's last step) only drops.  A path that hits a table light after its previous vertex
        sampled the lights has ``result.emitted`` zeroed.  ``out``: an optional ``(origins, directions, t_max, direct)`` of
        (N, 3), (N, 3), (N,), (N, 3) float32 tensors to write into (tensors made here start as zeros); ``counts``: an
        optional (2,) int64 tensor to add into.  Returns ``DirectSample``.

        ``mis=True`` is rtmi_direct_sample_mis: the light a vertex samples and the light its scattered ray then finds are
        both kept, weighted by the balance heuristic (``result.emitted`` of such a hit is scaled, not zeroed, and
        ``counts[1]`` counts the emissions weighed).  ``carry``: the loop's (N, 4) float32 tensor, the same one in every call
        of a loop; made here when None and returned in the result."""
        import torch
        if not isinstance(result, Bounce) or result.hits is None or result.steps is None:
            raise RtmiError("result must be the Bounce of a step made with hits=True and steps")
        o, d = result.origins, result.directions
        n, dev, _ = _check_batch("rtmi_direct_sample", o, d)
        step = int(step)
        if not 0 <= step < MAX_DEPTH:
            raise RtmiError("step %d outside [0, %d)" % (step, MAX_DEPTH))
        idx, n_list, cnt = _list_args(result.paths, n, dev)
        if not _is_buffer(light_states, (STATE_WORDS, n), dev, torch.int32):
            raise RtmiError("light_states must be a contiguous CUDA int32 tensor of shape (6, N) on the rays' device")
        if not _is_buffer(flags, (n,), dev, torch.int32):
            raise RtmiError("flags must be a contiguous CUDA int32 tensor of shape (N,) on the rays' device")
        if counts is None:
            counts = torch.zeros((2,), dtype=torch.int64, device=dev)
        elif not _is_buffer(counts, (2,), dev, torch.int64):
            raise RtmiError("counts must be a CUDA int64 tensor of shape (2,) on the rays' device")
        if out is None:
            out = (torch.zeros((n, 3), dtype=torch.float32, device=dev), torch.zeros((n, 3), dtype=torch.float32, device=dev),
                   torch.zeros((n,), dtype=torch.float32, device=dev), torch.zeros((n, 3), dtype=torch.float32, device=dev))
        so, sd, st, dd = out
        for name, t, shape in (("origins", so, (n, 3)), ("directions", sd, (n, 3)), ("t_max", st, (n,)), ("direct", dd, (n, 3))):
            if not _is_buffer(t, shape, dev, torch.float32):
                raise RtmiError("out's %s must be a contiguous CUDA float32 tensor of shape %s on the rays' device" % (name, shape))
        stream = self._stream(dev)
        if mis:
            if carry is None:
                carry = torch.zeros((n, 4), dtype=torch.float32, device=dev)
            elif not _is_buffer(carry, (n, 4), dev, torch.float32):
                raise RtmiError("carry must be a contiguous CUDA float32 tensor of shape (N, 4) on the rays' device")
            a = DirectSampleMisArgs()
            a.size, a.reserved, a.n, a.n_list, a.step, a.sample = C.sizeof(DirectSampleMisArgs), 0, n, n_list, step, 1 if sample else 0
            val = lambda t: t.data_ptr() if t is not None else None
            a.d_list, a.d_count, a.d_origins, a.d_dirs = val(idx), val(cnt), val(o), val(d)
            a.d_hits, a.d_steps, a.d_emitted, a.d_attenuation = val(result.hits.raw), val(result.steps), val(result.emitted), val(result.attenuation)
            a.d_light_states, a.d_flags = val(light_states), val(flags)
            a.d_shadow_origins, a.d_shadow_dirs, a.d_shadow_t_max, a.d_direct = val(so), val(sd), val(st), val(dd)
            a.d_carry, a.d_counts = val(carry), val(counts)
            with torch.cuda.device(dev):
                _check(self.L.rtmi_direct_sample_mis(self.h, C.byref(a), stream), "rtmi_direct_sample_mis")
            return DirectSample(so, sd, st, dd, flags, counts, carry)
        if carry is not None:
            raise RtmiError("carry is rtmi_direct_sample_mis's: pass mis=True")
        with torch.cuda.device(dev):
            _check(self.L.rtmi_direct_sample(self.h, n, _ptr(idx), n_list, _ptr(cnt), step, 1 if sample else 0, _ptr(o), _ptr(d),
                                             _ptr(result.hits.raw), _ptr(result.steps), _ptr(result.emitted),
                                             _ptr(result.attenuation), _ptr(light_states), _ptr(flags), _ptr(so), _ptr(sd),
                                             _ptr(st), _ptr(dd), _ptr(counts), stream), "rtmi_direct_sample")
        return DirectSample(so, sd, st, dd, flags, counts)

    def intersect(self, origins, directions, t_max=None, out=None):
        """Closest hit of each ray on the committed scene (rtmi_intersect), enqueued on torch's current stream.

        ``origins`` / ``directions``: CUDA float32 (N, 3) tensors on the scene's device (directions need not be unit
        length: Ray normalises them, and t is along the unit direction); ``t_max`` (N,) float32 or None: a hit is
        reported only where t <= t_max.  ``out``: an optional (N, 12) int32 CUDA tensor to write into.  Returns
        ``Hits`` (views into that buffer); call ``.check()`` on it before trusting the answers of a mesh scene."""
        import torch
        n, dev, t_max = _check_batch("rtmi_intersect", origins, directions, t_max)
        out = _out_buffer(out, "int32 tensor of shape (N, 12)", (n, HIT_WORDS), dev, torch.int32)
        stream = self._stream(dev)
        origins, directions = origins.contiguous(), directions.contiguous()
        abandoned = torch.zeros((1,), dtype=torch.int64, device=dev)
        with torch.cuda.device(dev):
            _check(self.L.rtmi_intersect(self.h, n, C.c_void_p(origins.data_ptr()), C.c_void_p(directions.data_ptr()),
                                         _ptr(t_max), C.c_void_p(out.data_ptr()), C.c_void_p(abandoned.data_ptr()), stream),
                   "rtmi_intersect")
        f = out.view(torch.float32)
        hits = Hits(f[:, 0], f[:, 1:3], f[:, 3:6], out[:, 6], out[:, 7], out[:, 8], out[:, 9])
        hits.raw, hits.abandoned = out, abandoned
        hits._rays = (origins, directions, t_max)  # (kept alive while the query may still read them)
        return hits

    def occluded(self, origins, directions, t_max=None, out=None):
        """Is anything in the way of each ray within t_max (rtmi_occluded), enqueued on torch's current stream.

        The answer for ray i is exactly ``intersect(...).kind[i] != RTMI_HIT_NONE`` with the same t_max (Sky counts,
        at t = 1e9; a NaN t_max is clear), found with t_max as a traversal bound and an early stop.  ``origins`` /
        ``directions`` / ``t_max`` as for ``intersect``; ``out``: an optional (N,) uint8 or bool CUDA tensor to
        write into.  Returns ``Occlusion``; call ``.check()`` on it before trusting the answers of a mesh scene."""
        import torch
        n, dev, t_max = _check_batch("rtmi_occluded", origins, directions, t_max)
        out = _out_buffer(out, "uint8 or bool tensor of shape (N,)", (n,), dev, torch.uint8, torch.bool)
        stream = self._stream(dev)
        origins, directions = origins.contiguous(), directions.contiguous()
        raw = out.view(torch.uint8)
        counts = torch.zeros((2,), dtype=torch.int64, device=dev)
        with torch.cuda.device(dev):
            _check(self.L.rtmi_occluded(self.h, n, C.c_void_p(origins.data_ptr()), C.c_void_p(directions.data_ptr()),
                                        _ptr(t_max), C.c_void_p(raw.data_ptr()), C.c_void_p(counts.data_ptr()), stream),
                   "rtmi_occluded")
        return Occlusion(raw, counts, (origins, directions, t_max))

    def occluded_list(self, paths, origins, directions, t_max=None, out=None):
        """``occluded`` for the paths of a list only (rtmi_occluded_list), enqueued on torch's current stream.

        ``paths``: a ``Paths`` (``path_compact`` makes them; a step's ``Bounce.paths``), or None for the identity list over
        all N.  Every tensor is indexed by path and has ``occluded``'s shape with N paths.  A listed path gets exactly the
        byte ``occluded`` gives its ray; an entry >= N is skipped; the entries need not be distinct (the query changes no
        state).  The list's count is read on the device and the launch is sized by the list's capacity, not by N.
        ``out``: an optional (N,) uint8 or bool CUDA tensor that is UPDATED -- a path that is not listed keeps its byte;
        when it is None the answers start as zeros, so unlisted paths read "clear".  Returns ``Occlusion`` and refuses what
        ``occluded`` refuses."""
        import torch
        n, dev, t_max = _check_batch("rtmi_occluded_list", origins, directions, t_max)
        idx, n_list, cnt = _list_args(paths, n, dev)
        if out is None:
            out = torch.zeros((n,), dtype=torch.uint8, device=dev)
        elif not _is_buffer(out, (n,), dev, torch.uint8, torch.bool):
            raise RtmiError("out must be a contiguous CUDA uint8 or bool tensor of shape (N,) on the rays' device")
        stream = self._stream(dev)
        origins, directions = origins.contiguous(), directions.contiguous()
        raw = out.view(torch.uint8)
        counts = torch.zeros((2,), dtype=torch.int64, device=dev)
        with torch.cuda.device(dev):
            _check(self.L.rtmi_occluded_list(self.h, n, _ptr(idx), n_list, _ptr(cnt), _ptr(origins), _ptr(directions),
                                             _ptr(t_max), _ptr(raw), _ptr(counts), stream), "rtmi_occluded_list")
        return Occlusion(raw, counts, (origins, directions, t_max, idx, cnt))

    def trace(self, origins, directions, states, max_depth, count_rays=False, out=None):
        """Path-traced radiance of each ray (rtmi_trace): Trace(world, Ray(o, d), &state, max_depth) as a render runs
        it for one sample, enqueued on torch's current stream.

        ``origins`` / ``directions`` as for ``intersect``; ``states``: a contiguous (6, N) int32 CUDA tensor of RNG
        states (``rng_states``), advanced in place by the draws each path makes; ``max_depth`` in [0, 64];
        ``count_rays``: also return each ray's closest-hit queries; ``out``: an optional (N, 3) float32 CUDA tensor to
        write the radiance into.  Returns ``Trace``; call ``.check()`` on it before trusting the answers of a mesh
        scene."""
        import torch
        n, dev, _ = _check_batch("rtmi_trace", origins, directions)
        if not _is_buffer(states, (STATE_WORDS, n), dev, torch.int32):
            raise RtmiError("states must be a contiguous CUDA int32 tensor of shape (6, N) on the rays' device")
        max_depth = int(max_depth)
        if not 0 <= max_depth <= MAX_DEPTH:
            raise RtmiError("max_depth %d outside [0, %d]" % (max_depth, MAX_DEPTH))
        out = _out_buffer(out, "float32 tensor of shape (N, 3)", (n, 3), dev, torch.float32)
        stream = self._stream(dev)
        origins, directions = origins.contiguous(), directions.contiguous()
        rays = torch.empty((n,), dtype=torch.int32, device=dev) if count_rays else None
        work = torch.zeros((TRACE_WORK_WORDS,), dtype=torch.int64, device=dev)  # (n == 0 leaves it untouched)
        with torch.cuda.device(dev):
            _check(self.L.rtmi_trace(self.h, n, C.c_void_p(origins.data_ptr()), C.c_void_p(directions.data_ptr()),
                                     max_depth, C.c_void_p(states.data_ptr()), C.c_void_p(out.data_ptr()),
                                     _ptr(rays), C.c_void_p(work.data_ptr()), stream), "rtmi_trace")
        return Trace(out, rays, work, (origins, directions, states))

    def bounce(self, origins, directions, states, emitted=None, attenuation=None, hits=False, steps=None):
        """One iteration of Trace's loop for each path (rtmi_bounce), enqueued on torch's current stream.

        ``origins`` / ``directions``: contiguous CUDA float32 (N, 3) tensors on the scene's device, REPLACED in place by
        the scattered rays (a zero direction: the path has ended, and further steps leave it alone); ``states``: a
        contiguous (6, N) int32 CUDA tensor of RNG states, advanced in place by Scatter's draws.  ``emitted`` /
        ``attenuation``: optional (N, 3) float32 tensors to write into (a layer of the stacks ``path_fold`` reads);
        ``hits``: True for the step's hit records, or an (N, 12) int32 tensor to write them into; ``steps``: an optional
        (N,) int32 tensor whose entry is incremented for every path this call steps.  Returns ``Bounce``; call
        ``.check()`` on it before trusting the answers of a mesh scene."""
        return self._step(False, None, origins, directions, states, emitted, attenuation, hits, steps)

    def bounce_list(self, paths, origins, directions, states, emitted=None, attenuation=None, hits=False, steps=None):
        """``bounce`` for the paths of a list only (rtmi_bounce_list), enqueued on torch's current stream.

        ``paths``: a ``Paths`` (``path_compact`` makes them), or None for the identity list over all N.  Every tensor is
        indexed by path and has ``bounce``'s shape with N paths; a listed path gets exactly what ``bounce`` gives it, a
        path that is not listed keeps every word, an entry >= N is skipped.  The entries must be distinct: a path listed
        twice gets an unspecified result.  The list's count is read on the device.  Returns ``Bounce``, its ``paths`` the
        list."""
        return self._step(True, paths, origins, directions, states, emitted, attenuation, hits, steps)

    def _step(self, listed, paths, origins, directions, states, emitted, attenuation, hits, steps):
        import torch
        n, dev, _ = _check_batch("rtmi_bounce_list" if listed else "rtmi_bounce", origins, directions)
        idx, n_list, cnt = _list_args(paths, n, dev)
        if not (origins.is_contiguous() and directions.is_contiguous()):
            raise RtmiError("origins and directions must be contiguous: rtmi_bounce writes the scattered rays into them")
        if not _is_buffer(states, (STATE_WORDS, n), dev, torch.int32):
            raise RtmiError("states must be a contiguous CUDA int32 tensor of shape (6, N) on the rays' device")
        for name, t in (("emitted", emitted), ("attenuation", attenuation)):
            if t is not None and not _is_buffer(t, (n, 3), dev, torch.float32):
                raise RtmiError("%s must be a contiguous CUDA float32 tensor of shape (N, 3) on the rays' device" % name)
        if steps is not None and not _is_buffer(steps, (n,), dev, torch.int32):
            raise RtmiError("steps must be a contiguous CUDA int32 tensor of shape (N,) on the rays' device")
        raw = None
        if isinstance(hits, torch.Tensor):
            raw = _out_buffer(hits, "int32 tensor of shape (N, 12)", (n, HIT_WORDS), dev, torch.int32)
        elif hits:
            raw = torch.empty((n, HIT_WORDS), dtype=torch.int32, device=dev)
        stream = self._stream(dev)
        if emitted is None:
            emitted = torch.empty((n, 3), dtype=torch.float32, device=dev)
        if attenuation is None:
            attenuation = torch.empty((n, 3), dtype=torch.float32, device=dev)
        work = torch.zeros((TRACE_WORK_WORDS,), dtype=torch.int64, device=dev)  # (n == 0 leaves it untouched)
        with torch.cuda.device(dev):
            if listed:
                _check(self.L.rtmi_bounce_list(self.h, n, _ptr(idx), n_list, _ptr(cnt), C.c_void_p(origins.data_ptr()),
                                               C.c_void_p(directions.data_ptr()), C.c_void_p(states.data_ptr()),
                                               C.c_void_p(emitted.data_ptr()), C.c_void_p(attenuation.data_ptr()),
                                               _ptr(raw), _ptr(steps), C.c_void_p(work.data_ptr()), stream),
                       "rtmi_bounce_list")
            else:
                _check(self.L.rtmi_bounce(self.h, n, C.c_void_p(origins.data_ptr()), C.c_void_p(directions.data_ptr()),
                                          C.c_void_p(states.data_ptr()), C.c_void_p(emitted.data_ptr()),
                                          C.c_void_p(attenuation.data_ptr()), _ptr(raw), _ptr(steps),
                                          C.c_void_p(work.data_ptr()), stream), "rtmi_bounce")
        rec = None
        if raw is not None:
            f = raw.view(torch.float32)
            rec = Hits(f[:, 0], f[:, 1:3], f[:, 3:6], raw[:, 6], raw[:, 7], raw[:, 8], raw[:, 9])
            rec.raw = raw
        return Bounce(origins, directions, states, emitted, attenuation, rec, steps, work, paths if listed else None)

    def trace_steps(self, origins, directions, states, max_depth, each=None, hits=None, compact=False, direct=False,
                    light_states=None, shadow=None):
        """rtmi_trace as a loop of ``max_depth`` steps and one fold, on copies of the rays: bit for bit ``trace``'s
        radiance while ``each`` changes nothing.  ``states`` advance in place, as in ``trace``.  ``each(step, result)``
        is called after every step is enqueued, with the step's ``Bounce`` (``result.origins`` / ``.directions`` are the
        loop's own ray tensors): the place for shadow rays from ``result.hits``, or a termination rule -- zeroing a path's
        direction ends it, and the fold then takes its last layer's emitted as the path's end.  ``hits``: whether the
        steps record hits (default: when ``each`` is given).  Returns ``Steps``.

        ``compact``: False (the default) steps all N paths every time (``bounce``).  True steps the live paths only: every
        step is a ``bounce_list`` on a list that ``path_compact`` made from the list of the step before (the first from
        all N), two lists ping-ponged, their counts never read back; ``result.paths`` is the list the step used.  The
        radiance is the same bit for bit.  A path that ``each`` revives or redirects while it is NOT in the current list
        is not seen by the next compaction, which starts from that list: for such hooks ``compact="full"`` compacts from
        all N paths before every step.

        ``direct=True`` (needs ``light_states``, a (6, N) int32 tensor of RNG states of their own; implies hits) is the
        same loop with next-event estimation: after step k ``direct_sample(step=k, sample=k + 1 < max_depth)`` on that
        step's list (or on all paths), ``occluded`` on its shadow rays into layer k of an occlusion stack, and
        ``path_fold_direct`` at the end.  The paths themselves -- states, attenuation, hits, steps, final rays -- are the
        plain loop's bit for bit, and the radiance has ``trace``'s expectation.  ``each`` runs after the step's direct
        sampling.

        ``direct="mis"`` is the ``direct=True`` loop with ``direct_sample(mis=True)``: one carry tensor for the loop
        (``Steps.carry``), ``shadow`` and the fold as with ``direct=True``.  The light a vertex samples and the light its
        scattered ray finds are weighted by the balance heuristic, so a light close to a diffuse surface no longer gives
        unbounded samples; the paths are still the plain loop's and the expectation ``trace``'s.

        ``shadow`` chooses the visibility query of ``direct=True``: ``"all"`` is ``occluded`` over all N shadow rays,
        ``"list"`` is ``occluded_list`` on the list the step used (``result.paths``), valid only with ``compact`` and
        ``direct=True``; None (the default) is ``SHADOW_DEFAULT`` where ``"list"`` is valid, else ``"all"``.  Every output
        is the same bit for bit either way.  The occlusion stack starts as zeros, so a byte the list form does not write
        reads "clear"; ``"all"`` writes 0 there too, because the path's shadow direction is the zero vector (a bad ray):
        ``direct_sample`` gives every candidate that does not sample a zero shadow direction, the shadow tensors start as
        zeros, and a path that leaves the list was a candidate in its last step, where -- ended, its direction zero -- it
        did not sample.  (The one path outside this argument is ``bounce``'s documented bad scattered ray, a non-zero
        direction that does not normalise: it may sample, leaves the list alive, and ``"all"`` answers its stale shadow
        ray again in the layers after its last, which no fold reads.)"""
        import torch
        if not (direct is False or direct is True or direct == "mis"):
            raise RtmiError("direct must be False, True or \"mis\"")
        if direct and light_states is None:
            raise RtmiError("direct=True needs light_states: RNG states of their own, e.g. rng_states(seed, N, first=N)")
        if not (compact is False or compact is True or compact == "full"):
            raise RtmiError("compact must be False, True or \"full\"")
        if shadow not in (None, "all", "list"):
            raise RtmiError("shadow must be None, \"all\" or \"list\"")
        if shadow == "list" and not (compact and direct):
            raise RtmiError("shadow=\"list\" needs compact and direct=True: it queries the list a compacted step used")
        if shadow is None:
            shadow = SHADOW_DEFAULT if (compact and direct) else "all"
        n, dev, _ = _check_batch("rtmi_bounce", origins, directions)
        max_depth = int(max_depth)
        if not 0 <= max_depth <= MAX_DEPTH:
            raise RtmiError("max_depth %d outside [0, %d]" % (max_depth, MAX_DEPTH))
        if not _is_buffer(states, (STATE_WORDS, n), dev, torch.int32):
            raise RtmiError("states must be a contiguous CUDA int32 tensor of shape (6, N) on the rays' device")
        self._stream(dev)
        o, d = origins.clone().contiguous(), directions.clone().contiguous()
        layers = max(max_depth, 1)
        E = torch.empty((layers, n, 3), dtype=torch.float32, device=dev)
        A = torch.empty((layers, n, 3), dtype=torch.float32, device=dev)
        steps = torch.zeros((n,), dtype=torch.int32, device=dev)
        want_hits = (each is not None) if hits is None else bool(hits)
        mis = direct == "mis"
        Dk = occ = flags = rays = carry = None
        if direct:
            want_hits = True
            if not _is_buffer(light_states, (STATE_WORDS, n), dev, torch.int32):
                raise RtmiError("light_states must be a contiguous CUDA int32 tensor of shape (6, N) on the rays' device")
            Dk = torch.zeros((layers, n, 3), dtype=torch.float32, device=dev)
            occ = torch.zeros((layers, n), dtype=torch.uint8, device=dev)
            flags = torch.zeros((n,), dtype=torch.int32, device=dev)
            rays = (torch.zeros((n, 3), dtype=torch.float32, device=dev), torch.zeros((n, 3), dtype=torch.float32, device=dev),
                    torch.zeros((n,), dtype=torch.float32, device=dev))  # (the shadow rays: one set, rewritten every step)
            counts = torch.zeros((2,), dtype=torch.int64, device=dev)
            if mis:
                carry = torch.zeros((n, 4), dtype=torch.float32, device=dev)  # (one for the loop)
        works = []
        lists, cur = None, None
        if compact and max_depth > 0:
            lists = [Paths(torch.empty((n,), dtype=torch.int32, device=dev), torch.empty((1,), dtype=torch.int32, device=dev))
                     for _ in range(2)]
            cur = _path_compact(n, o, d, None, n, None, lists[0], dev)
        for k in range(max_depth):
            if compact:
                r = self.bounce_list(cur, o, d, states, emitted=E[k], attenuation=A[k], hits=want_hits, steps=steps)
            else:
                r = self.bounce(o, d, states, emitted=E[k], attenuation=A[k], hits=want_hits, steps=steps)
            works.append(r.work)
            if direct:
                self.direct_sample(k, r, light_states, flags, sample=k + 1 < max_depth, out=rays + (Dk[k],), counts=counts,
                                   mis=mis, carry=carry)
                if shadow == "list":
                    q = self.occluded_list(r.paths, rays[0], rays[1], rays[2], out=occ[k])
                else:
                    q = self.occluded(rays[0], rays[1], rays[2], out=occ[k])
                r.work[0] += q.counts[0]  # (abandoned searches: check())
            if each is not None:
                each(k, r)
            if compact and k + 1 < max_depth:  # the next step's list: the live ones of this step's (or of all N)
                nxt = lists[(k + 1) & 1]
                if compact == "full":
                    cur = _path_compact(n, o, d, None, n, None, nxt, dev)
                else:
                    cur = _path_compact(n, o, d, cur.index, n, cur.count, nxt, dev)
        if direct:
            rgb = path_fold_direct(d, steps, E, A, Dk, occ)
            st = Steps(rgb, steps, (d != 0).any(dim=1), o, d, E, A, works, Dk, occ, flags)
            st.carry = carry
            return st
        rgb = path_fold(d, steps, E, A)
        return Steps(rgb, steps, (d != 0).any(dim=1), o, d, E, A, works)

    def _stream(self, dev):
        """torch's current stream on dev, the rays' device; raises unless the scene was committed there."""
        if self.h.value is None or getattr(self, "device", None) is None:
            raise RtmiError("scene not committed")
        if dev != self.device:
            raise RtmiError("the rays are on %s, the scene was committed on %s" % (dev, self.device))
        import torch
        return C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)


def _check_batch(entry, origins, directions, t_max=None):
    """(N, the rays' device, t_max made contiguous) of a batch for ``entry``; raises before any GPU work unless
    origins and directions are (N, 3) CUDA float32 tensors on one device and t_max is None or (N,) float32 there."""
    try:
        import torch
    except ImportError:
        raise RtmiError("origins: torch is needed for %s" % entry)
    for what, a in (("origins", origins), ("directions", directions)):
        if not isinstance(a, torch.Tensor):
            raise RtmiError("%s must be a torch tensor" % what)
        if not a.is_cuda:
            raise RtmiError("%s is on the CPU: %s has no CPU path (move it to the scene's GPU)" % (what, entry))
        if a.dtype != torch.float32:
            raise RtmiError("%s must be float32, not %s" % (what, a.dtype))
        if a.dim() != 2 or a.shape[1] != 3:
            raise RtmiError("%s must have shape (N, 3), not %s" % (what, tuple(a.shape)))
    n = int(origins.shape[0])
    if directions.shape[0] != n:
        raise RtmiError("origins and directions differ in length")
    if origins.device != directions.device:
        raise RtmiError("origins and directions are on different devices")
    dev = origins.device
    if t_max is not None:
        if not (isinstance(t_max, torch.Tensor) and t_max.is_cuda and t_max.dtype == torch.float32 and
                t_max.shape == (n,) and t_max.device == dev):
            raise RtmiError("t_max must be a CUDA float32 tensor of shape (N,) on the rays' device")
        t_max = t_max.contiguous()
    return n, dev, t_max


def _is_buffer(t, shape, dev, *dtypes):
    import torch
    return (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype in dtypes and t.shape == shape and t.is_contiguous()
            and t.device == dev)


def _out_buffer(out, desc, shape, dev, *dtypes):
    """A new tensor of the first of dtypes for out=None, else out itself, which must match (desc: its words in the error)."""
    import torch
    if out is None:
        return torch.empty(shape, dtype=dtypes[0], device=dev)
    if not _is_buffer(out, shape, dev, *dtypes):
        raise RtmiError("out must be a contiguous CUDA %s on the rays' device" % desc)
    return out


class Renderer:
    """One rank's share of a frame: device buffers (torch), RNG init, render, untile.

    Mirrors what the reference's ``Main``/``DistributedMain`` do around the kernel
    (utils.cu:132-242) — allocation, CudaRandomInit, PathTracing launch — but keeps
    results on the device; the caller decides when to copy or gather."""

    def __init__(self, scene, height, width, spp, max_depth=10, post=True, rank=0, world_size=1, device=None):
        import torch
        if not torch.cuda.is_available():
            raise RtmiError("no GPU visible to torch: the render path has no CPU fallback")
        self.torch = torch
        self.L = lib()
        self.scene = scene
        self.device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        self.frame = make_frame(height, width, spp, max_depth, post, rank, world_size)
        self.items = work_items(self.frame)
        with torch.cuda.device(self.device):
            self.states = torch.empty((STATE_WORDS, self.items), dtype=torch.int32, device=self.device)
            self.tiles = torch.empty((self.items, 3), dtype=torch.float32, device=self.device)
            self.ray_counts = torch.empty((self.items,), dtype=torch.int32, device=self.device)

    def _stream(self):
        return C.c_void_p(self.torch.cuda.current_stream(self.device).cuda_stream)

    def init_rng(self, seed=None):
        seed = self.scene.seed if seed is None else seed
        with self.torch.cuda.device(self.device):
            _check(self.L.rtmi_rng_init(C.c_uint64(seed), C.byref(self.frame), C.c_void_p(self.states.data_ptr()),
                                        self._stream()), "rtmi_rng_init")
            # pixel 0 (work item 0 of rank 0) continues the stream the scene program drew from
            if self.frame.rank == 0 and seed == self.scene.seed and \
                    not np.array_equal(self.scene.state0, self.scene.state0_fresh):
                _check(self.L.rtmi_rng_set_state(C.byref(self.frame), C.c_void_p(self.states.data_ptr()), 0,
                                                 self.scene.state0.ctypes.data_as(_u32p), self._stream()),
                       "rtmi_rng_set_state")
        return self

    def render(self, count_rays=True, opts=None):
        """Enqueue the trace kernel on torch's current stream (asynchronous).  ``opts``: a
        ``render_opts(...)`` structure with per-call scheduling options (None = the defaults)."""
        self._last_scratch = opts.d_scratch if opts is not None else None
        with self.torch.cuda.device(self.device):
            rc = self.L.rtmi_render_ex(self.scene.h, C.byref(self.frame), C.byref(opts) if opts is not None else None,
                                       C.c_void_p(self.states.data_ptr()), C.c_void_p(self.tiles.data_ptr()),
                                       C.c_void_p(self.ray_counts.data_ptr()) if count_rays else None, self._stream())
        _check(rc, "rtmi_render_ex")
        return self

    def check(self):
        """Wait for the last render and raise if it reported an incomplete frame (rtmi_render_status); with budget
        renders behind it (``render_budget``), also if any of them abandoned a mesh search."""
        if getattr(self, "budget_abandoned", None) is not None:
            n = int(self.budget_abandoned.item())  # (a device-to-host copy: waits for the calls)
            if n:
                raise RtmiError("rtmi_render_budget abandoned %d mesh search(es): the sums are incomplete" % n)
        with self.torch.cuda.device(self.device):
            _check(self.L.rtmi_render_status(self.scene.h, C.c_void_p(getattr(self, "_last_scratch", None)), None,
                                             self._stream()), "rtmi_render_status")
        return self

    # -------------------------------------------------------------- per-pixel sample budgets
    def _budget_buffers(self):
        if getattr(self, "sum", None) is None:
            torch, n, dev = self.torch, self.items, self.device
            self.sum = torch.zeros((n, 3), dtype=torch.float32, device=dev)
            self.sq = torch.zeros((n, 3), dtype=torch.float32, device=dev)
            self.samples = torch.zeros((n,), dtype=torch.int32, device=dev)
            self.budget_rays = torch.zeros((n,), dtype=torch.int32, device=dev)
            self.d_work = torch.zeros((BUDGET_WORK_WORDS,), dtype=torch.int64, device=dev)
            self.budget_abandoned = torch.zeros((), dtype=torch.int64, device=dev)  # d_work[0] over all calls
            self.budget = torch.zeros((n,), dtype=torch.int32, device=dev)
            self.totals = torch.zeros((2,), dtype=torch.int64, device=dev)

    def _feature_buffers(self):
        if getattr(self, "albedo", None) is None:
            torch, n, dev = self.torch, self.items, self.device
            self.albedo = torch.zeros((n, 3), dtype=torch.float32, device=dev)
            self.normal = torch.zeros((n, 3), dtype=torch.float32, device=dev)
            self.depth = torch.zeros((n,), dtype=torch.float32, device=dev)
            self.coverage = torch.zeros((n,), dtype=torch.int32, device=dev)

    def render_budget(self, budget, count_rays=True, features=False):
        """``budget[q]`` more samples (at most the frame's spp per call) of every pixel q of this shard
        (rtmi_render_budget), enqueued on torch's current stream: continues each pixel's RNG stream in ``states`` and
        adds to ``sum`` (radiance), ``sq`` (squares), ``samples`` and, with ``count_rays``, ``budget_rays`` -- zeroed
        on first use and kept as attributes.  ``budget``: a contiguous (items,) int32 CUDA tensor.  The frame must
        have been made with ``post=False``.  ``features``: also add the primary hit of every sample to ``albedo``,
        ``normal``, ``depth`` and ``coverage`` (rtmi_render_features; zeroed on first use; max_depth >= 1)."""
        torch = self.torch
        if not _is_buffer(budget, (self.items,), self.device, torch.int32):
            raise RtmiError("budget must be a contiguous CUDA int32 tensor of shape (items,) on the renderer's device")
        self._budget_buffers()
        args = (self.scene.h, C.byref(self.frame), C.c_void_p(budget.data_ptr()), C.c_void_p(self.states.data_ptr()),
                C.c_void_p(self.sum.data_ptr()), C.c_void_p(self.sq.data_ptr()), C.c_void_p(self.samples.data_ptr()),
                C.c_void_p(self.budget_rays.data_ptr()) if count_rays else None)
        with torch.cuda.device(self.device):
            if features:
                self._feature_buffers()
                feat = feature_bufs(self.albedo, self.normal, self.depth, self.coverage)
                _check(self.L.rtmi_render_features(*args, C.byref(feat), C.c_void_p(self.d_work.data_ptr()), self._stream()),
                       "rtmi_render_features")
            else:
                _check(self.L.rtmi_render_budget(*args, C.c_void_p(self.d_work.data_ptr()), self._stream()),
                       "rtmi_render_budget")
            self.budget_abandoned += self.d_work[0]  # (stream-ordered: the next call resets d_work)
        return self

    # -------------------------------------------------------------- camera rays
    def _budget_arg(self, budget):
        if budget is not None and not _is_buffer(budget, (self.items,), self.device, self.torch.int32):
            raise RtmiError("budget must be a contiguous CUDA int32 tensor of shape (items,) on the renderer's device")
        return C.c_void_p(budget.data_ptr()) if budget is not None else None

    def camera_rays(self, sample, budget=None, projection=None, out=None):
        """The primary rays of sample index ``sample`` of every pixel of this shard (rtmi_camera_rays), enqueued on torch's
        current stream: what the render makes from ``states`` for each pixel's next sample, the states advanced in place
        by the jitter and lens draws.  ``budget``: None (every pixel has the frame's spp) or a contiguous (items,) int32
        CUDA tensor; an item with no sample ``sample`` left, and padding, gets a zero ray and keeps its state.
        ``projection``: an ``rtmi.projection(...)`` (None: the scene's camera).  ``out``: an optional pair of (items, 3)
        float32 CUDA tensors to write into.  Returns (origins, directions), tile-major; the directions are normalised once
        (``SceneBuilder.trace`` and ``intersect`` normalise once more, as Ray's constructor does)."""
        torch = self.torch
        if projection is not None and not isinstance(projection, Projection):
            raise RtmiError("projection must be an rtmi.projection(...)")
        d_budget = self._budget_arg(budget)
        shape = (self.items, 3)
        if out is None:
            out = (None, None)
        elif not (isinstance(out, (tuple, list)) and len(out) == 2):
            raise RtmiError("out must be a pair of (items, 3) float32 CUDA tensors: (origins, directions)")
        origins = _out_buffer(out[0], "float32 tensor of shape (items, 3)", shape, self.device, torch.float32)
        dirs = _out_buffer(out[1], "float32 tensor of shape (items, 3)", shape, self.device, torch.float32)
        with torch.cuda.device(self.device):
            _check(self.L.rtmi_camera_rays(self.scene.h, C.byref(self.frame), C.byref(projection) if projection is not None else None,
                                           d_budget, int(sample), C.c_void_p(self.states.data_ptr()),
                                           C.c_void_p(origins.data_ptr()), C.c_void_p(dirs.data_ptr()), self._stream()),
                   "rtmi_camera_rays")
        return origins, dirs

    def sample_add(self, sample, radiance, trace_counts=None, budget=None):
        """Fold the traced sample ``sample`` into ``sum``, ``sq``, ``samples`` and -- with ``trace_counts`` --
        ``budget_rays`` (rtmi_sample_add; the buffers of ``render_budget``, zeroed on first use), on torch's current stream.
        ``radiance``: (items, 3) float32, ``trace_counts``: (items,) int32 or None, as ``SceneBuilder.trace`` returns them;
        ``budget`` as for ``camera_rays``: only the items active in this sample are touched."""
        torch = self.torch
        if not _is_buffer(radiance, (self.items, 3), self.device, torch.float32):
            raise RtmiError("radiance must be a contiguous CUDA float32 tensor of shape (items, 3) on the renderer's device")
        if trace_counts is not None and not _is_buffer(trace_counts, (self.items,), self.device, torch.int32):
            raise RtmiError("trace_counts must be a contiguous CUDA int32 tensor of shape (items,) on the renderer's device")
        d_budget = self._budget_arg(budget)
        self._budget_buffers()
        with torch.cuda.device(self.device):
            _check(self.L.rtmi_sample_add(C.byref(self.frame), d_budget, int(sample), C.c_void_p(radiance.data_ptr()),
                                          C.c_void_p(trace_counts.data_ptr()) if trace_counts is not None else None,
                                          C.c_void_p(self.sum.data_ptr()), C.c_void_p(self.sq.data_ptr()),
                                          C.c_void_p(self.samples.data_ptr()),
                                          C.c_void_p(self.budget_rays.data_ptr()) if trace_counts is not None else None,
                                          self._stream()), "rtmi_sample_add")
        return self

    def render_rays(self, budget=None, projection=None, count_rays=True, each=None, direct=False):
        """``render_budget(budget)`` as the composed loop -- for every sample index: ``camera_rays``, ``SceneBuilder.trace``,
        ``sample_add`` -- on torch's current stream, bit for bit the same sums, moments, counts and states with the scene's
        camera.  ``budget``: None for the frame's spp everywhere; the largest active budget is read back once (a
        synchronisation).  ``projection``: an ``rtmi.projection(...)``.  ``each(sample, origins, directions)``: called
        between the generation of a sample's rays and their tracing -- the place to run ``intersect`` or ``occluded`` on
        the very rays of the frame (or to change them in place).  Adds each trace's closest-hit queries to ``rays_total``
        and its abandoned mesh searches to ``budget_abandoned`` (``check()`` raises on them).  The frame must have been
        made with ``post=False``.

        ``direct=True`` traces every sample with ``SceneBuilder.trace_steps(compact=True, direct=True)`` instead (its
        shadow query is that loop's default, ``SHADOW_DEFAULT``; the sums are the same with either): the same
        paths with next-event estimation, the same expectation and less variance where small lights light the scene; the
        sums are then not ``render_budget``'s.  Its light states are seeded from the renderer's seed with first = items on
        the first such call and carried on.  ``direct="mis"`` is passed through to ``trace_steps`` in the same way
        (multiple importance sampling); ``self.carry`` is then the last sample's carry tensor, else None."""
        torch = self.torch
        if self.frame.post_process:
            raise RtmiError("render_rays needs a frame made with post=False: per-pixel sample counts have no uniform division (resolve)")
        self._budget_arg(budget)
        self._budget_buffers()
        if getattr(self, "rays_total", None) is None:
            self.rays_total = torch.zeros((), dtype=torch.int64, device=self.device)
        spp = int(self.frame.spp)
        n_samples = spp
        if budget is not None:  # (the budget words are uint32: a negative int32 is a large one)
            n_samples = min(spp, int((budget.to(torch.int64) & 0xffffffff).max().item())) if self.items else 0
        with torch.cuda.device(self.device):
            origins = torch.empty((self.items, 3), dtype=torch.float32, device=self.device)
            dirs = torch.empty((self.items, 3), dtype=torch.float32, device=self.device)
            radiance = torch.empty((self.items, 3), dtype=torch.float32, device=self.device)
            counts = torch.empty((self.items,), dtype=torch.int32, device=self.device) if count_rays else None
            work = torch.zeros((TRACE_WORK_WORDS,), dtype=torch.int64, device=self.device)  # one d_work, reused in stream order
            stream = self._stream()
            for sample in range(n_samples):
                self.camera_rays(sample, budget, projection, out=(origins, dirs))
                if each is not None:
                    each(sample, origins, dirs)
                if direct:
                    if getattr(self, "light_states", None) is None:
                        self.light_states = rng_states(self.scene.seed, self.items, first=self.items, device=self.device)
                    st = self.scene.trace_steps(origins, dirs, self.states, int(self.frame.max_depth), compact=True, direct=direct,
                                                light_states=self.light_states)
                    self.carry = st.carry
                    for w in st.works:
                        self.budget_abandoned += w[0]
                    queries = st.steps + st.alive.to(torch.int32)
                    self.rays_total += queries.sum()
                    self.sample_add(sample, st.rgb, queries if count_rays else None, budget)
                    continue
                _check(self.L.rtmi_trace(self.scene.h, self.items, C.c_void_p(origins.data_ptr()), C.c_void_p(dirs.data_ptr()),
                                         int(self.frame.max_depth), C.c_void_p(self.states.data_ptr()),
                                         C.c_void_p(radiance.data_ptr()), C.c_void_p(counts.data_ptr()) if count_rays else None,
                                         C.c_void_p(work.data_ptr()), stream), "rtmi_trace")
                self.budget_abandoned += work[0]  # (stream-ordered: the next trace resets d_work)
                self.rays_total += work[1]
                self.sample_add(sample, radiance, counts, budget)
            n = int(self.budget_abandoned.item())  # (waits for the loop, as Trace.check does)
        if n:
            raise RtmiError("rtmi_trace abandoned %d mesh search(es): the sums are incomplete" % n)
        return self

    # -------------------------------------------------------------- a wavefront that stays full
    def path_advance(self, paths, origins, directions, steps, emitted, attenuation, stacks, cursor, budget=None,
                     projection=None, counts=None, count_rays=True):
        """Finish the ended paths among ``paths`` and refill them in place with their pixel's next camera ray
        (rtmi_path_advance; include/rtmi.h states the rule), enqueued on torch's current stream.

        ``paths``: the ``Paths`` the last ``SceneBuilder.bounce_list`` stepped, or None for all items (the call that
        starts a render).  ``origins`` / ``directions`` (items, 3) float32 and ``steps`` (items,) int32: the arrays the
        steps step, with the renderer's ``states``.  ``emitted`` / ``attenuation`` (items, 3) float32: the ONE layer every
        step writes.  ``stacks``: a pair of (max_depth, items, 3) float32 tensors, each path's own layers (None when the
        frame's max_depth is 0).  ``cursor``: (items, 2) int32, zeroed before a render.  ``budget`` / ``projection``: as
        ``camera_rays``.  ``counts``: an optional (3,) int64 tensor: += samples finished, their closest-hit queries, camera
        rays made.  Finished samples are added to ``sum``, ``sq``, ``samples`` and -- with ``count_rays`` --
        ``budget_rays`` (the buffers of ``render_budget``, zeroed on first use).  All tensors contiguous, on the
        renderer's device.  Returns ``self``."""
        a, keep = self._advance_args(paths, origins, directions, steps, emitted, attenuation, stacks, cursor, budget, projection,
                                     counts, count_rays)
        with self.torch.cuda.device(self.device):
            _check(self.L.rtmi_path_advance(self.scene.h, C.byref(self.frame), C.byref(a), self._stream()), "rtmi_path_advance")
        return self

    def _advance_args(self, paths, origins, directions, steps, emitted, attenuation, stacks, cursor, budget, projection, counts,
                      count_rays):
        """The checked rtmi_path_advance_args of ``path_advance``'s arguments, and what it points into (to be kept alive)."""
        torch = self.torch
        n, dev, depth = self.items, self.device, int(self.frame.max_depth)
        idx, n_list, cnt = _list_args(paths, n, dev)
        if projection is not None and not isinstance(projection, Projection):
            raise RtmiError("projection must be an rtmi.projection(...)")
        for name, t in (("origins", origins), ("directions", directions), ("emitted", emitted), ("attenuation", attenuation)):
            if not _is_buffer(t, (n, 3), dev, torch.float32):
                raise RtmiError("%s must be a contiguous CUDA float32 tensor of shape (items, 3) on the renderer's device" % name)
        if not _is_buffer(steps, (n,), dev, torch.int32):
            raise RtmiError("steps must be a contiguous CUDA int32 tensor of shape (items,) on the renderer's device")
        if not _is_buffer(cursor, (n, 2), dev, torch.int32):
            raise RtmiError("cursor must be a contiguous CUDA int32 tensor of shape (items, 2) on the renderer's device")
        if stacks is None:
            stacks = (None, None)
        if not (isinstance(stacks, (tuple, list)) and len(stacks) == 2):
            raise RtmiError("stacks must be a pair of (max_depth, items, 3) float32 CUDA tensors, or None at max_depth 0")
        for t in stacks:
            if not (t is None and depth == 0) and not _is_buffer(t, (depth, n, 3), dev, torch.float32):
                raise RtmiError("stacks must be a pair of contiguous CUDA float32 tensors of shape (max_depth, items, 3)")
        if counts is not None and not _is_buffer(counts, (3,), dev, torch.int64):
            raise RtmiError("counts must be a CUDA int64 tensor of shape (3,) on the renderer's device")
        d_budget = self._budget_arg(budget)
        self._budget_buffers()
        val = lambda t: t.data_ptr() if t is not None else None
        a = PathAdvanceArgs()
        a.size, a.reserved = C.sizeof(PathAdvanceArgs), 0
        a.proj = C.pointer(projection) if projection is not None else None
        a.d_budget = d_budget
        a.d_list, a.n_list, a.d_count = val(idx), n_list, val(cnt)
        a.d_origins, a.d_dirs, a.d_states, a.d_steps = val(origins), val(directions), val(self.states), val(steps)
        a.d_emitted, a.d_attenuation = val(emitted), val(attenuation)
        a.d_emitted_stack, a.d_attenuation_stack = val(stacks[0]), val(stacks[1])
        a.d_cursor = val(cursor)
        a.d_sum, a.d_sq, a.d_samples = val(self.sum), val(self.sq), val(self.samples)
        a.d_ray_counts = val(self.budget_rays) if count_rays else None
        a.d_counts = val(counts)
        return a, (paths, origins, directions, steps, emitted, attenuation, stacks, cursor, budget, projection, counts)

    def render_wavefront(self, budget=None, projection=None, count_rays=True, each=None, poll=8):
        """``render_budget(budget)`` as a wavefront that stays full, on torch's current stream: ``path_advance`` on all
        items starts every pixel's first path, then every iteration is one ``SceneBuilder.bounce_list`` on the live paths,
        one ``path_advance`` on the same list -- which finishes the paths that ended and gives their pixels the next
        sample's camera ray in place -- and one ``path_compact`` from that list, two ``Paths`` ping-ponged.  Bit for bit
        ``render_budget``'s sums, moments, sample and ray counts and states (a pixel's samples stay one serial chain on its
        RNG state).  Its steps run on fuller lists than the per-sample loop's, but on an MI355X the whole loop is not faster
        than ``render_rays`` or the ``trace_steps`` loop (DESIGN.md 2.16 has the figures): use it for what it holds between
        two steps -- every path's vertex, at whatever depth -- not for speed.

        ``budget``: None for the frame's spp everywhere; the largest active budget is read back once before the loop (it
        bounds the loop).  ``projection``: an ``rtmi.projection(...)``.  ``each(iteration, result)`` gets each step's
        ``Bounce`` (with hits, and ``result.paths`` the list it stepped) after its advance is enqueued: between two steps
        the caller holds every path's vertex, whatever its depth.  ``poll``: the live count is read back once every
        ``poll`` iterations, the loop's only synchronisation; the iterations enqueued after the last path has ended run on
        an empty list and change nothing.  The loop makes at most (largest active budget) x max(max_depth, 1) + 1
        iterations and raises ``RtmiError`` if paths are still live then.  Adds the finished samples' closest-hit queries
        to ``rays_total``, every step's abandoned mesh searches to ``budget_abandoned`` (``check()`` raises on them) and
        the call's counters to ``wavefront_counts`` ((3,) int64: samples finished, their queries, camera rays made);
        ``wavefront_iterations`` is how many iterations this call enqueued.  The frame must have been made with
        ``post=False``.  Returns ``self``: ``resolve``, ``plan``, ``resolve_variance`` and ``denoise`` follow unchanged."""
        torch = self.torch
        if self.frame.post_process:
            raise RtmiError("render_wavefront needs a frame made with post=False: per-pixel sample counts have no uniform division (resolve)")
        poll = int(poll)
        if poll < 1:
            raise RtmiError("poll must be at least 1")
        self._budget_arg(budget)
        self._budget_buffers()
        n, dev, depth, spp = self.items, self.device, int(self.frame.max_depth), int(self.frame.spp)
        if not 0 <= depth <= MAX_DEPTH:
            raise RtmiError("max_depth %d outside [0, %d]" % (depth, MAX_DEPTH))
        if getattr(self, "rays_total", None) is None:
            self.rays_total = torch.zeros((), dtype=torch.int64, device=dev)
        if getattr(self, "wavefront_counts", None) is None:
            self.wavefront_counts = torch.zeros((3,), dtype=torch.int64, device=dev)
        most = spp
        if budget is not None:  # (the budget words are uint32: a negative int32 is a large one)
            most = min(spp, int((budget.to(torch.int64) & 0xffffffff).max().item())) if n else 0
        bound = most * max(depth, 1) + 1
        self.wavefront_iterations = 0
        with torch.cuda.device(dev):
            zeros = lambda *shape: torch.zeros(shape, dtype=torch.float32, device=dev)
            origins, dirs = zeros(n, 3), zeros(n, 3)
            steps = torch.zeros((n,), dtype=torch.int32, device=dev)
            cursor = torch.zeros((n, 2), dtype=torch.int32, device=dev)
            emitted, attenuation = zeros(n, 3), zeros(n, 3)
            stacks = None
            if depth > 0:
                stacks = (torch.empty((depth, n, 3), dtype=torch.float32, device=dev),
                          torch.empty((depth, n, 3), dtype=torch.float32, device=dev))
            queries_before = self.wavefront_counts[1].clone()
            lists = [Paths(torch.empty((n,), dtype=torch.int32, device=dev), torch.empty((1,), dtype=torch.int32, device=dev))
                     for _ in range(2)]
            # Everything an iteration passes is checked and turned into ctypes values ONCE: with them an iteration is three
            # foreign calls, and the loop is bound by the device, not by the interpreter (DESIGN.md 2.16 has the figures).
            L, h, fr, stream = self.L, self.scene.h, C.byref(self.frame), self.scene._stream(dev)
            rest = (origins, dirs, steps, emitted, attenuation, stacks, cursor, budget, projection, self.wavefront_counts, count_rays)
            start, keep = self._advance_args(None, *rest)
            adv = [self._advance_args(p, *rest)[0] for p in lists]
            p_o, p_d, p_st, p_steps = _ptr(origins), _ptr(dirs), _ptr(self.states), _ptr(steps)
            p_em, p_at = _ptr(emitted), _ptr(attenuation)
            p_idx, p_cnt = [_ptr(p.index) for p in lists], [_ptr(p.count) for p in lists]
            scratch = torch.empty((max(L.rtmi_path_compact_scratch_bytes(n) // 4, 1),), dtype=torch.int32, device=dev)
            p_scratch = _ptr(scratch)  # (one scratch: the compactions follow each other on one stream)
            # the steps' work blocks: a ring, its abandoned searches summed and the ring cleared whenever it has gone round
            ring = torch.zeros((64, TRACE_WORK_WORDS), dtype=torch.int64, device=dev)
            p_work = [C.c_void_p(ring.data_ptr() + j * TRACE_WORK_WORDS * 8) for j in range(ring.shape[0])]
            _check(L.rtmi_path_advance(h, fr, C.byref(start), stream), "rtmi_path_advance")
            _check(L.rtmi_path_compact(n, p_o, p_d, None, n, None, p_idx[0], p_cnt[0], p_scratch, stream), "rtmi_path_compact")
            def flush():  # (stream-ordered; a block no step used holds zeros)
                self.budget_abandoned += ring[:, 0].sum()
                ring.zero_()

            it, c, cur = 0, 0, lists[0]
            while True:
                if each is None and it and it % len(p_work) == 0:
                    flush()  # the ring is about to be used again from its first block
                if it % poll == 0 or it >= bound:
                    live = int(cur.count.item())  # (a device-to-host copy: the loop's one synchronisation)
                    if live == 0:
                        flush()
                        break
                    if it >= bound:
                        flush()
                        raise RtmiError("render_wavefront: %d path(s) still live after %d iterations (the bound for a "
                                        "largest budget of %d at max_depth %d)" % (live, it, most, depth))
                if each is None:
                    _check(L.rtmi_bounce_list(h, n, p_idx[c], n, p_cnt[c], p_o, p_d, p_st, p_em, p_at, None, p_steps,
                                              p_work[it % len(p_work)], stream), "rtmi_bounce_list")
                    _check(L.rtmi_path_advance(h, fr, C.byref(adv[c]), stream), "rtmi_path_advance")
                else:  # the step through the binding: its Bounce, hit records and a work block of its own for the hook
                    r = self.scene.bounce_list(cur, origins, dirs, self.states, emitted=emitted, attenuation=attenuation,
                                               hits=True, steps=steps)
                    self.budget_abandoned += r.work[0]  # (stream-ordered)
                    _check(L.rtmi_path_advance(h, fr, C.byref(adv[c]), stream), "rtmi_path_advance")
                    each(it, r)
                it += 1
                _check(L.rtmi_path_compact(n, p_o, p_d, p_idx[c], n, p_cnt[c], p_idx[c ^ 1], p_cnt[c ^ 1], p_scratch, stream),
                       "rtmi_path_compact")
                c ^= 1
                cur = lists[c]
            cur._keep = (origins, dirs, scratch, keep)
            self.wavefront_iterations = it
            self.rays_total += self.wavefront_counts[1] - queries_before
            self.wavefront_cursor, self.wavefront_paths = cursor, cur  # (what the loop left: every k == b, an empty list)
        return self

    def resolve_features(self):
        """``ResolvedFeatures`` (albedo, normal, depth, alpha) of the feature sums so far, tile-major
        (rtmi_resolve_features; the rule is in include/rtmi.h): 0 where a pixel has no samples and for padding."""
        self._budget_buffers()
        self._feature_buffers()
        torch, n, dev = self.torch, self.items, self.device
        out = ResolvedFeatures(torch.empty((n, 3), dtype=torch.float32, device=dev), torch.empty((n, 3), dtype=torch.float32, device=dev),
                               torch.empty((n,), dtype=torch.float32, device=dev), torch.empty((n,), dtype=torch.float32, device=dev))
        sums = feature_bufs(self.albedo, self.normal, self.depth, self.coverage)
        to = feature_bufs(*out)
        with torch.cuda.device(dev):
            _check(self.L.rtmi_resolve_features(C.byref(self.frame), C.byref(sums), C.c_void_p(self.samples.data_ptr()),
                                                C.byref(to), self._stream()), "rtmi_resolve_features")
        return out

    def plan(self, min_spp, max_spp, step, tolerance, floor=0.01):
        """The next pass's budget from the sums so far (rtmi_budget_plan; the rule is in include/rtmi.h).  Returns
        (budget tensor, pixels with a budget, sum of the budgets); reading the two totals waits for the stream."""
        self._budget_buffers()
        o = adaptive_opts(min_spp, max_spp, step, tolerance, floor)
        with self.torch.cuda.device(self.device):
            _check(self.L.rtmi_budget_plan(C.byref(self.frame), C.byref(o), C.c_void_p(self.sum.data_ptr()),
                                           C.c_void_p(self.sq.data_ptr()), C.c_void_p(self.samples.data_ptr()),
                                           C.c_void_p(self.budget.data_ptr()), C.c_void_p(self.totals.data_ptr()),
                                           self._stream()), "rtmi_budget_plan")
            active, total = self.totals.tolist()
        return self.budget, active, total

    def resolve(self, post=True):
        """(items, 3) tile buffer: sum / samples per pixel, post-processed like a render's (rtmi_resolve)."""
        self._budget_buffers()
        out = self.torch.empty((self.items, 3), dtype=self.torch.float32, device=self.device)
        with self.torch.cuda.device(self.device):
            _check(self.L.rtmi_resolve(C.byref(self.frame), C.c_void_p(self.sum.data_ptr()),
                                       C.c_void_p(self.samples.data_ptr()), 1 if post else 0, C.c_void_p(out.data_ptr()),
                                       self._stream()), "rtmi_resolve")
        return out

    def resolve_variance(self):
        """(items, 3) tile buffer: the variance of each pixel's MEAN from the sums so far (rtmi_resolve_variance; the
        rule is in include/rtmi.h): 0 where a pixel has no samples and for padding."""
        self._budget_buffers()
        out = self.torch.empty((self.items, 3), dtype=self.torch.float32, device=self.device)
        with self.torch.cuda.device(self.device):
            _check(self.L.rtmi_resolve_variance(C.byref(self.frame), C.c_void_p(self.sum.data_ptr()),
                                                C.c_void_p(self.sq.data_ptr()), C.c_void_p(self.samples.data_ptr()),
                                                C.c_void_p(out.data_ptr()), self._stream()), "rtmi_resolve_variance")
        return out

    def denoise_inputs(self):
        """The row-major buffers ``denoise`` filters, as a dict of rtmi.denoise's arguments: color (resolved without
        post-processing), variance, normal, depth, alpha, albedo."""
        if self.frame.world_size != 1:
            raise RtmiError("Renderer.denoise works on a whole frame (world_size 1): gather the resolved colour, variance "
                            "and feature buffers of all ranks, untile them and call rtmi.denoise")
        if getattr(self, "sum", None) is None or getattr(self, "albedo", None) is None:
            raise RtmiError("nothing to denoise: render_budget(features=True) or render_adaptive(features=True) comes first")
        self.check()
        feat = self.resolve_features()
        color, depth = self.untile(self.resolve(post=False), feat.depth)
        variance, alpha = self.untile(self.resolve_variance(), feat.alpha)
        three = lambda t: self.untile(t, feat.depth)[0]  # (untile moves a 32-bit buffer too: its own ray counts if given none)
        return dict(color=color, variance=variance, normal=three(feat.normal), depth=depth, alpha=alpha,
                    albedo=three(feat.albedo))

    def denoise(self, post=True, **opts):
        """The denoised row-major (H, W, 3) image of the samples so far, after ``render_budget(features=True)`` or
        ``render_adaptive(features=True)`` on a whole frame (world_size 1): resolves colour (without post-processing),
        variance and features, untiles each and calls ``rtmi.denoise`` with ``opts`` (its keyword arguments; the
        defaults are its own).  ``post``: finish with the render's post-processing, sqrt(clamp(., 0, 1))."""
        if opts.get("return_variance"):
            raise RtmiError("Renderer.denoise returns the image alone: call rtmi.denoise on denoise_inputs() for the variance")
        img = denoise(**self.denoise_inputs(), **opts)
        if post:
            with self.torch.cuda.device(self.device):
                _check(self.L.rtmi_post_process(C.c_void_p(img.data_ptr()), self.frame.height * self.frame.width, 1,
                                                self._stream()), "rtmi_post_process")
        return img

    def new_frame(self):
        """Start the next frame of a sequence: zero ``sum``, ``sq``, ``samples``, ``budget_rays``, ``budget_abandoned``, the
        four feature sums and ``render_rays``' ``rays_total`` on torch's current stream.  The RNG states go on, so every frame draws new samples."""
        self._budget_buffers()
        self._feature_buffers()
        with self.torch.cuda.device(self.device):
            for t in (self.sum, self.sq, self.samples, self.budget_rays, self.budget_abandoned, self.albedo, self.normal,
                      self.depth, self.coverage):
                t.zero_()
            if getattr(self, "rays_total", None) is not None:
                self.rays_total.zero_()
        return self

    def accumulate(self, acc):
        """``denoise_inputs()`` of the frame so far, accumulated into ``acc`` (an ``Accumulator`` of this frame's extent) as
        seen from the scene's present camera: the same dict with ``color`` and ``variance`` replaced by the accumulated
        ones, so a sequence is ``scene.camera_look(...)``, ``new_frame()``, ``render_budget(..., features=True)``,
        ``rtmi.denoise(**R.accumulate(acc))`` per frame."""
        if self.frame.world_size != 1:
            raise RtmiError("Renderer.denoise works on a whole frame (world_size 1): gather the resolved colour, variance "
                            "and feature buffers of all ranks, untile them and call rtmi.denoise")
        buf = self.denoise_inputs()
        color, variance, _ = acc.step(buf["color"], buf["variance"], buf["normal"], buf["depth"], buf["alpha"],
                                      camera=self.scene.camera_get())
        return dict(buf, color=color, variance=variance)

    def render_adaptive(self, min_spp, max_spp, step, tolerance, floor=0.01, post=True, features=False):
        """Plan / render passes until no pixel has a budget left: every pixel gets ``min_spp`` samples, then ``step``
        more per pass until it meets the stopping rule or has ``max_spp``.  One host read of the plan's totals per
        pass is the only synchronisation.  The frame's spp must be at least max(min_spp, step).  ``features``: every
        pass also adds to the first-hit feature buffers, and the result's ``features`` holds them resolved."""
        if self.frame.spp < max(int(min_spp), int(step)):
            raise RtmiError("the frame's spp (%d) caps one pass: it must be at least max(min_spp, step)" % self.frame.spp)
        passes = total = 0
        while True:
            budget, active, pass_total = self.plan(min_spp, max_spp, step, tolerance, floor)
            if active == 0:
                break
            self.render_budget(budget, features=features)
            passes, total = passes + 1, total + pass_total
        self.check()
        return Adaptive(self.resolve(post), self.samples, passes, total, self.resolve_features() if features else None)

    def scratch_bytes(self):
        return int(self.L.rtmi_render_scratch_bytes(C.byref(self.frame)))

    def new_scratch(self):
        """Device memory for the per-call state of one render (``render_opts(scratch=...)``)."""
        return self.torch.zeros((self.scratch_bytes() + 7) // 8, dtype=self.torch.int64, device=self.device)

    def launch_shape(self, opts=None):
        """{workgroups, lanes per workgroup, workgroups per CU, CUs} of a render of this frame."""
        out = (C.c_int32 * 4)()
        with self.torch.cuda.device(self.device):
            _check(self.L.rtmi_render_launch_shape(self.scene.h, C.byref(self.frame),
                                                   C.byref(opts) if opts is not None else None, out),
                   "rtmi_render_launch_shape")
        return dict(zip(("blocks", "threads", "blocks_per_cu", "compute_units"), list(out)))

    def mode(self, opts=None):
        """How a render of this frame would be scheduled, and whether its last launch is a fast kernel (rtmi_render_mode_ex)."""
        out = (C.c_int32 * MODE_FIELDS)()
        with self.torch.cuda.device(self.device):
            _check(self.L.rtmi_render_mode_ex(self.scene.h, C.byref(self.frame), C.byref(opts) if opts is not None else None, out,
                                              MODE_FIELDS), "rtmi_render_mode_ex")
        return dict(zip(("scheduled", "first_pass_samples", "first_pass_resumed", "planned_chains", "wave_priority_every",
                         "lane_stride", "waves", "tiles", "fast_path"), list(out)))

    def total_rays(self, scratch=None):
        """Closest-hit queries of the last render (of the one that used ``scratch``, if given); raises when that
        render reported an incomplete frame."""
        out = C.c_uint64(0)
        with self.torch.cuda.device(self.device):
            _check(self.L.rtmi_render_status(self.scene.h, C.c_void_p(scratch.data_ptr()) if scratch is not None else None,
                                             C.byref(out), self._stream()), "rtmi_render_status")
        return out.value

    def untile(self, all_tiles=None, all_counts=None):
        """Row-major (H,W,3) image [and (H,W) ray counts] from tile-major buffers of all ranks.  ``all_tiles`` may be
        any 3-channel float32 buffer (resolved albedo or normal), ``all_counts`` any 32-bit one: a float32 buffer
        (resolved depth or alpha) is moved by its bits and comes back as float32."""
        torch = self.torch
        f = self.frame
        with torch.cuda.device(self.device):
            if all_tiles is None:  # this rank's own render: an incomplete frame must not be handed on
                self.check()
            tiles = self.tiles if all_tiles is None else all_tiles
            assert tiles.numel() == self.items * 3 * f.world_size, "expected the buffers of all ranks back to back"
            img = torch.zeros((f.height, f.width, 3), dtype=torch.float32, device=self.device)
            _check(self.L.rtmi_untile(C.byref(f), C.c_void_p(tiles.data_ptr()), C.c_void_p(img.data_ptr()),
                                      self._stream()), "rtmi_untile")
            cnt = None
            counts = self.ray_counts if (all_counts is None and f.world_size == 1) else all_counts
            if counts is not None:
                cnt = torch.zeros((f.height, f.width), device=self.device,
                                  dtype=torch.float32 if counts.dtype == torch.float32 else torch.int32)
                _check(self.L.rtmi_untile_u32(C.byref(f), C.c_void_p(counts.data_ptr()), C.c_void_p(cnt.data_ptr()),
                                              self._stream()), "rtmi_untile_u32")
        return img, cnt
