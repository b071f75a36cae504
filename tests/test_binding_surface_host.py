"""The public surface of the rtmi package, pinned: every public class, function and constant with its signature, as recorded
before the package was split into modules by layer (TABLE), and that ``import rtmi`` alone loads neither torch nor
librtmi.so.  No GPU, no library."""
import ctypes
import inspect
import os
import subprocess
import sys
import types

import numpy as np

import rtmi

# the classes whose public methods are pinned one by one
METHODS_OF = ("SceneBuilder", "Renderer", "Accumulator", "Paths", "Hits", "Steps")


def describe(v):
    """A signature where there is one; a structure's field names; else the type's name."""
    if inspect.isclass(v) and issubclass(v, ctypes.Structure):
        return "struct " + " ".join(name for name, _ in v._fields_)
    if isinstance(v, property):
        return "property"
    if isinstance(v, np.dtype):
        return "dtype " + " ".join(v.names)
    if callable(v):
        try:
            return str(inspect.signature(v))
        except (ValueError, TypeError):
            pass
    return type(v).__name__


def surface(pkg):
    """{name: description} of what the package defines itself (imported modules are not its own)."""
    out = {}
    for name, v in vars(pkg).items():
        if name.startswith("_") or isinstance(v, types.ModuleType):
            continue
        out[name] = describe(v)
        if inspect.isclass(v) and hasattr(v, "_fields") and issubclass(v, tuple):
            out[name + "._fields"] = " ".join(v._fields)
        if name in METHODS_OF:
            for attr, m in vars(v).items():
                if not attr.startswith("_"):
                    out["%s.%s" % (name, attr)] = describe(m)
    return out


TABLE = {'ACCUMULATE_DEFAULTS': 'dict',
 'AccumulateOpts': 'struct size reserved normal_min depth_tolerance min_blend',
 'Accumulator': '(height, width, device=None, **opts)',
 'Accumulator.history': 'property',
 'Accumulator.reset': '(self)',
 'Accumulator.step': '(self, color, variance, normal, depth, alpha, camera)',
 'Adaptive': '(tiles, samples, passes, total_samples, features=None)',
 'Adaptive._fields': 'tiles samples passes total_samples features',
 'AdaptiveOpts': 'struct size min_samples max_samples step tolerance floor',
 'BUDGET_WORK_WORDS': 'int',
 'Bounce': '(origins, directions, states, emitted, attenuation, hits, steps, work, paths=None)',
 'DENOISE_DEFAULTS': 'dict',
 'DenoiseGuides': 'struct size reserved d_variance d_albedo d_normal d_depth d_alpha',
 'DenoiseOpts': 'struct size iterations normal_squarings demodulate sigma_color sigma_depth',
 'DirectSample': '(origins, directions, t_max, direct, flags, counts, carry=None)',
 'DirectSample._fields': 'origins directions t_max direct flags counts carry',
 'DirectSampleMisArgs': 'struct size reserved n d_list n_list d_count step sample d_origins d_dirs d_hits d_steps d_emitted '
                        'd_attenuation d_light_states d_flags d_shadow_origins d_shadow_dirs d_shadow_t_max d_direct d_carry d_counts',
 'FAST_PATH_FACTS': 'int',
 'Features': 'struct size reserved d_albedo d_normal d_depth d_coverage',
 'Frame': 'struct height width spp max_depth post_process rank world_size',
 'HIT_WORDS': 'int',
 'Hits': '(t, uv, normal, material, kind, entry, element)',
 'Hits._fields': 't uv normal material kind entry element',
 'Hits.check': '(self)',
 'LIB_PATH': 'str',
 'LIGHT_DTYPE': 'dtype p0 e1 e2 n emission area cdf scale kind entry element material',
 'MAX_DEPTH': 'int',
 'MAX_MATERIALS': 'int',
 'MODE_FIELDS': 'int',
 'Occlusion': '(raw, counts, rays)',
 'PATH_COMPACT_ITEMS': 'int',
 'PROJECTIONS': 'dict',
 'PathAdvanceArgs': 'struct size reserved proj d_budget d_list n_list d_count d_origins d_dirs d_states d_steps d_emitted '
                    'd_attenuation d_emitted_stack d_attenuation_stack d_cursor d_sum d_sq d_samples d_ray_counts d_counts',
 'Paths': '(index, count=None)',
 'Paths.n': '(self)',
 'Projection': 'struct size kind fov reserved',
 'RTMI_HIT_MESH': 'int',
 'RTMI_HIT_NONE': 'int',
 'RTMI_HIT_PARALLELEPIPED': 'int',
 'RTMI_HIT_PARALLELOGRAM': 'int',
 'RTMI_HIT_SKY': 'int',
 'RTMI_HIT_SPHERE': 'int',
 'RTMI_HIT_TRIANGLE': 'int',
 'RenderOpts': 'struct size schedule blocks_per_cu threads_per_block sparse_stride exclusive outlier_x10 probe_spp head_pct plan '
               'wave_priority lane_stride promote_after cost_probe first_pass fast_path d_scratch scratch_bytes',
 'Renderer': '(scene, height, width, spp, max_depth=10, post=True, rank=0, world_size=1, device=None)',
 'Renderer.accumulate': '(self, acc)',
 'Renderer.camera_rays': '(self, sample, budget=None, projection=None, out=None)',
 'Renderer.check': '(self)',
 'Renderer.denoise': '(self, post=True, **opts)',
 'Renderer.denoise_inputs': '(self)',
 'Renderer.init_rng': '(self, seed=None)',
 'Renderer.launch_shape': '(self, opts=None)',
 'Renderer.mode': '(self, opts=None)',
 'Renderer.new_frame': '(self)',
 'Renderer.new_scratch': '(self)',
 'Renderer.path_advance': '(self, paths, origins, directions, steps, emitted, attenuation, stacks, cursor, budget=None, '
                          'projection=None, counts=None, count_rays=True)',
 'Renderer.plan': '(self, min_spp, max_spp, step, tolerance, floor=0.01)',
 'Renderer.render': '(self, count_rays=True, opts=None)',
 'Renderer.render_adaptive': '(self, min_spp, max_spp, step, tolerance, floor=0.01, post=True, features=False)',
 'Renderer.render_budget': '(self, budget, count_rays=True, features=False)',
 'Renderer.render_rays': '(self, budget=None, projection=None, count_rays=True, each=None, direct=False)',
 'Renderer.render_wavefront': '(self, budget=None, projection=None, count_rays=True, each=None, poll=8)',
 'Renderer.resolve': '(self, post=True)',
 'Renderer.resolve_features': '(self)',
 'Renderer.resolve_variance': '(self)',
 'Renderer.sample_add': '(self, sample, radiance, trace_counts=None, budget=None)',
 'Renderer.scratch_bytes': '(self)',
 'Renderer.total_rays': '(self, scratch=None)',
 'Renderer.untile': '(self, all_tiles=None, all_counts=None)',
 'ResolvedFeatures': '(albedo, normal, depth, alpha)',
 'ResolvedFeatures._fields': 'albedo normal depth alpha',
 'RtmiError': 'type',
 'SCRATCH_REGIONS': 'tuple',
 'SHADOW_DEFAULT': 'str',
 'STATE_WORDS': 'int',
 'SYMBOLS': 'list',
 'SceneBuilder': '(seed=0)',
 'SceneBuilder.bounce': '(self, origins, directions, states, emitted=None, attenuation=None, hits=False, steps=None)',
 'SceneBuilder.bounce_list': '(self, paths, origins, directions, states, emitted=None, attenuation=None, hits=False, steps=None)',
 'SceneBuilder.bvh': '(self, faces, mat, uvs=None, k_min=2048)',
 'SceneBuilder.bytes_per_ray': '(self)',
 'SceneBuilder.camera_defocus': '(self, pos, look_at, up, fov, aspect, aperture, focus)',
 'SceneBuilder.camera_get': '(self)',
 'SceneBuilder.camera_look': '(self, pos, look_at, up, fov, aspect)',
 'SceneBuilder.camera_pinhole': '(self, pos, look_at, up, fov, aspect)',
 'SceneBuilder.camera_raw': '(self, pos, llc, horiz, vert)',
 'SceneBuilder.camera_update': '(self, frame21, defocus=False, lens_radius=-1.0)',
 'SceneBuilder.commit': '(self)',
 'SceneBuilder.constant_texture': '(self, rgb)',
 'SceneBuilder.dielectric': '(self, rgb, index)',
 'SceneBuilder.diffuse_light': '(self, tex)',
 'SceneBuilder.direct_sample': '(self, step, result, light_states, flags, sample=True, out=None, counts=None, mis=False, carry=None)',
 'SceneBuilder.image_texture': '(self, rgba)',
 'SceneBuilder.intersect': '(self, origins, directions, t_max=None, out=None)',
 'SceneBuilder.lambertian': '(self, rgb)',
 'SceneBuilder.lambertian_tex': '(self, tex)',
 'SceneBuilder.lights': '(self)',
 'SceneBuilder.list_begin': '(self)',
 'SceneBuilder.list_end': '(self)',
 'SceneBuilder.list_records': '(self)',
 'SceneBuilder.metal': '(self, rgb, fuzz)',
 'SceneBuilder.occluded': '(self, origins, directions, t_max=None, out=None)',
 'SceneBuilder.occluded_list': '(self, paths, origins, directions, t_max=None, out=None)',
 'SceneBuilder.pair_slabs': '(self)',
 'SceneBuilder.parallelepiped': '(self, p, mat)',
 'SceneBuilder.parallelepiped_lengths': '(self, lengths, mat, transform)',
 'SceneBuilder.parallelogram': '(self, p, mat)',
 'SceneBuilder.random_float': '(self, mn, mx)',
 'SceneBuilder.render_lds_bytes': '(self, max_depth, threads=256)',
 'SceneBuilder.sky': '(self)',
 'SceneBuilder.slab_reach': '(self)',
 'SceneBuilder.sliver_faces': '(self)',
 'SceneBuilder.sphere': '(self, c, r, mat)',
 'SceneBuilder.stats': '(self)',
 'SceneBuilder.trace': '(self, origins, directions, states, max_depth, count_rays=False, out=None)',
 'SceneBuilder.trace_steps': '(self, origins, directions, states, max_depth, each=None, hits=None, compact=False, direct=False, '
                             'light_states=None, shadow=None)',
 'SceneBuilder.triangle': '(self, p, mat)',
 'Steps': '(rgb, steps, alive, origins, directions, emitted, attenuation, works, direct=None, occluded=None, flags=None)',
 'Steps._fields': 'rgb steps alive origins directions emitted attenuation works direct occluded flags',
 'Steps.carry': 'NoneType',
 'Steps.check': '(self)',
 'TILE': 'int',
 'TRACE_WORK_WORDS': 'int',
 'TRANSFORM_FN': 'PyCFuncPtrType',
 'Trace': '(rgb, rays, work, keep)',
 'accumulate': '(color, variance, normal, depth, alpha, camera, history=None, prev_camera=None, out_history=None, **opts)',
 'adaptive_opts': '(min_spp, max_spp, step, tolerance, floor=0.01)',
 'debug_schedule': '(frame, scratch, ray_counts, work_counts=None, pixel_head=False, sparse_cap=0, grid_waves=0, outlier_x10=20, '
                   'head_pct=(50, 25, 12), simds=0, rounds=0, spp=1, probe_spp=1)',
 'denoise': '(color, variance, normal, depth, alpha, albedo=None, iterations=5, sigma_color=1.0, sigma_depth=0.05, '
            'normal_squarings=0, demodulate=None, out=None, return_variance=False)',
 'feature_bufs': '(albedo=None, normal=None, depth=None, coverage=None)',
 'get_workload': '(rank, world_size, spp)',
 'lib': '()',
 'make_frame': '(height, width, spp, max_depth=10, post=True, rank=0, world_size=1)',
 'path_compact': '(origins, directions, paths=None, out=None)',
 'path_fold': '(directions, steps, emitted_stack, attenuation_stack, out=None)',
 'path_fold_direct': '(directions, steps, emitted_stack, attenuation_stack, direct_stack, occluded_stack, out=None)',
 'pixel_map': '(frame)',
 'projection': "(kind='camera', fov=0.0)",
 'render_opts': '(schedule=-1, blocks_per_cu=0, threads_per_block=0, sparse_stride=0, exclusive=-1, outlier_x10=0, probe_spp=0, '
                'head_pct=(0, 0, 0), scratch=None, plan=-1, wave_priority=-1, lane_stride=0, promote_after=-1, cost_probe=-1, '
                'first_pass=-1, fast_path=0)',
 'rng_states': '(seed, n, first=0, device=None)',
 'scratch_regions': '(frame)',
 'work_items': '(frame)'}


def test_the_package_gives_the_recorded_surface():
    got = surface(rtmi)
    missing = sorted(set(TABLE) - set(got))
    assert not missing, "public names that are gone: %s" % missing
    changed = {k: (TABLE[k], got[k]) for k in TABLE if got[k] != TABLE[k]}
    assert not changed, "signatures that changed (recorded, now): %s" % changed
    added = sorted(set(got) - set(TABLE))
    assert not added, "public names that were not there: %s" % added


def test_import_loads_neither_torch_nor_the_library():
    code = ("import sys, rtmi, rtmi._abi\n"
            "assert 'torch' not in sys.modules, 'import rtmi imported torch'\n"
            "assert rtmi._abi._lib is None, 'import rtmi loaded librtmi.so'\n"
            "assert not any('librtmi' in line for line in open('/proc/self/maps')), 'librtmi.so is mapped'\n")
    pkg_dir = os.path.dirname(os.path.dirname(os.path.abspath(rtmi.__file__)))
    r = subprocess.run([sys.executable, "-c", code], cwd=pkg_dir, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout
