"""The C ABI of librtmi.so as ctypes: the constants and structures of include/rtmi.h, every symbol's signature, the loader,
and the calls that need no device memory.  Host only: nothing here imports torch before ``lib()`` does."""
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


def _addr(t):
    """A tensor's address as the value of a structure's pointer field (None: a null pointer)."""
    return t.data_ptr() if t is not None else None


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
    return Features(C.sizeof(Features), 0, _addr(albedo), _addr(normal), _addr(depth), _addr(coverage))


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


class TraceDirectArgs(C.Structure):
    """rtmi_trace_direct_args of include/rtmi.h (the arrays of one rtmi_trace_direct call)."""
    _fields_ = [("size", C.c_int32), ("reserved", C.c_int32), ("n", C.c_int64), ("d_origins", C.c_void_p), ("d_dirs", C.c_void_p),
                ("max_depth", C.c_int32), ("d_states", C.c_void_p), ("d_light_states", C.c_void_p), ("d_radiance", C.c_void_p),
                ("d_ray_counts", C.c_void_p), ("d_counts", C.c_void_p), ("d_work", C.c_void_p)]


class PathRouletteArgs(C.Structure):
    """rtmi_path_roulette_args of include/rtmi.h (the arrays of one rtmi_path_roulette call)."""
    _fields_ = [("size", C.c_int32), ("reserved", C.c_int32), ("n", C.c_int64), ("d_list", C.c_void_p), ("n_list", C.c_int64),
                ("d_count", C.c_void_p), ("step", C.c_uint32), ("first_step", C.c_uint32), ("p_min", C.c_float),
                ("reserved2", C.c_int32), ("d_steps", C.c_void_p), ("d_dirs", C.c_void_p), ("d_attenuation", C.c_void_p),
                ("d_states", C.c_void_p), ("d_throughput", C.c_void_p), ("d_counts", C.c_void_p)]


class TraceRouletteArgs(C.Structure):
    """rtmi_trace_roulette_args of include/rtmi.h (the arrays of one rtmi_trace_roulette call)."""
    _fields_ = [("size", C.c_int32), ("reserved", C.c_int32), ("n", C.c_int64), ("d_origins", C.c_void_p), ("d_dirs", C.c_void_p),
                ("max_depth", C.c_int32), ("first_step", C.c_uint32), ("p_min", C.c_float), ("d_states", C.c_void_p),
                ("d_radiance", C.c_void_p), ("d_ray_counts", C.c_void_p), ("d_counts", C.c_void_p), ("d_work", C.c_void_p)]


class RenderDirectArgs(C.Structure):
    """rtmi_render_direct_args of include/rtmi.h (the arrays of one rtmi_render_direct call)."""
    _fields_ = [("size", C.c_int32), ("reserved", C.c_int32), ("d_budget", C.c_void_p), ("d_states", C.c_void_p),
                ("d_light_states", C.c_void_p), ("d_sum", C.c_void_p), ("d_sq", C.c_void_p), ("d_samples", C.c_void_p),
                ("d_ray_counts", C.c_void_p), ("features", C.POINTER(Features)), ("d_counts", C.c_void_p), ("d_work", C.c_void_p)]


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
    ("rtmi_render_pins", C.c_int, [C.c_void_p, _frp, C.POINTER(RenderOpts), _u32p]),
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
    ("rtmi_scene_light_kinds", C.c_int, [C.c_void_p, C.c_uint32]),
    ("rtmi_occluded_list", C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_int64] + [C.c_void_p] * 7),
    ("rtmi_path_advance", C.c_int, [C.c_void_p, _frp, C.POINTER(PathAdvanceArgs), C.c_void_p]),
    ("rtmi_trace_direct", C.c_int, [C.c_void_p, C.POINTER(TraceDirectArgs), C.c_void_p]),
    ("rtmi_render_direct", C.c_int, [C.c_void_p, _frp, C.POINTER(RenderDirectArgs), C.c_void_p]),
    ("rtmi_path_roulette", C.c_int, [C.POINTER(PathRouletteArgs), C.c_void_p]),
    ("rtmi_trace_roulette", C.c_int, [C.c_void_p, C.POINTER(TraceRouletteArgs), C.c_void_p]),
]

# RTMI_LIGHTS_* of include/rtmi.h (rtmi_scene_light_kinds)
LIGHTS_FLAT, LIGHTS_SPHERES = 1, 2

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


def _camera21(camera, name):
    a = np.ascontiguousarray(np.asarray(camera, dtype=np.float32).reshape(-1))
    if a.size != 21:
        raise RtmiError("%s must hold the 21 floats of rtmi_camera_get" % name)
    return a


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


def get_workload(rank, world_size, spp):
    return lib().rtmi_get_workload(rank, world_size, spp)
