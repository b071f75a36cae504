"""rtmi — Python binding of librtmi.so (the MI355X path-tracing hot path).

This package is plumbing over the C ABI declared in include/rtmi.h: ctypes calls
for the scene recorder / RNG / render entry points and PyTorch tensors for device
memory, streams and ``torch.distributed``.  There is no CPU rendering path: every
compute call raises ``RtmiError`` when librtmi.so or a GPU is missing.

The modules, by layer: ``_abi`` (the ABI as ctypes, the loader), ``_tensors`` (the tensor checks, pointers, streams),
``wavefront`` (the queries' and paths' value types, folds, compaction, RNG states), ``filters`` (denoise, accumulate),
``builder`` (``SceneBuilder``), ``renderer`` (``Renderer`` and the scheduler diagnostic ``debug_schedule``); this file only gathers their public names.
"""
import ctypes as C  # (rtmi.C: callers size their ctypes arrays with it)

from ._abi import (ACCUMULATE_DEFAULTS, BUDGET_WORK_WORDS, DENOISE_DEFAULTS, FAST_PATH_FACTS, HIT_WORDS, LIB_PATH, LIGHT_DTYPE,
                   MAX_DEPTH, MAX_MATERIALS, MODE_FIELDS, PATH_COMPACT_ITEMS, PROJECTIONS, RTMI_HIT_MESH, RTMI_HIT_NONE,
                   RTMI_HIT_PARALLELEPIPED, RTMI_HIT_PARALLELOGRAM, RTMI_HIT_SKY, RTMI_HIT_SPHERE, RTMI_HIT_TRIANGLE,
                   SCRATCH_REGIONS, SHADOW_DEFAULT, STATE_WORDS, SYMBOLS, TILE, TRACE_WORK_WORDS, TRANSFORM_FN, AccumulateOpts,
                   AdaptiveOpts, DenoiseGuides, DenoiseOpts, DirectSampleMisArgs, Features, Frame, PathAdvanceArgs, Projection,
                   RenderOpts, RtmiError, adaptive_opts, feature_bufs, get_workload, lib, make_frame, pixel_map, projection,
                   render_opts, scratch_regions, work_items)
from .builder import SceneBuilder
from .filters import Accumulator, accumulate, denoise
from .renderer import Adaptive, Renderer, ResolvedFeatures, debug_schedule
from .wavefront import (Bounce, DirectSample, Hits, Occlusion, Paths, Steps, Trace, path_compact, path_fold, path_fold_direct,
                        rng_states)
