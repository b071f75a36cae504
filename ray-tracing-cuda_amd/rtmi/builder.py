"""``SceneBuilder``: the C ABI's scene recorder, and the ray queries and path steps that run on a committed scene."""
import ctypes as C

import numpy as np

from . import _abi
from ._abi import (HIT_WORDS, LIGHT_DTYPE, MAX_DEPTH, STATE_WORDS, TRACE_WORK_WORDS, TRANSFORM_FN, DirectSampleMisArgs, RtmiError,
                   TraceDirectArgs, TraceRouletteArgs, _addr, _camera21, _check, _f, _fp, _u32p, lib)
from ._tensors import _check_batch, _need, _new, _out_buffer, _ptr, _ptrs, _stream, _torch
from .wavefront import (Bounce, DirectSample, Hits, Occlusion, Roulette, Steps, Trace, TraceDirect, TraceRoulette, _list_args,
                        _new_paths, _path_compact, path_fold, path_fold_direct, path_roulette)


class _CommitOptions:
    """What a scene opts into before ``commit``.  A base of ``SceneBuilder``: the options are the builder's methods."""

    def light_kinds(self, spheres=False):
        """Which hitables the light table may hold (rtmi_scene_light_kinds), to be called before ``commit``: triangles,
        parallelograms and box faces always; with ``spheres=True`` also emissive spheres of positive radius, sampled in
        the cone they subtend.  ``lights()``, ``direct_sample``, ``trace_steps(direct=...)`` and
        ``Renderer.render_rays(direct=...)`` work unchanged on such a scene.  Returns the builder."""
        _check(self.L.rtmi_scene_light_kinds(self.h, _abi.LIGHTS_FLAT | (_abi.LIGHTS_SPHERES if spheres else 0)),
               "rtmi_scene_light_kinds")
        return self


class _FusedTraces:
    """The entries that run a whole loop of steps in one kernel, and the loop that a fused rule is held to where
    ``trace_steps`` itself cannot take it (its parameter list is recorded).  A base of ``SceneBuilder``: they are the
    builder's methods."""

    def trace_direct(self, origins, directions, states, light_states, max_depth, count_rays=False, out=None):
        """``trace`` with next-event estimation inside the kernel (rtmi_trace_direct), enqueued on torch's current stream:
        per path the samples, weights and shadow answers of ``trace_steps(compact=True, direct="mis")`` in one launch, the
        visible light summed forward along the path (include/rtmi.h states the sum; it differs from that loop's fold by the
        rounding order only).

        ``origins`` / ``directions`` / ``states`` / ``max_depth`` / ``count_rays`` / ``out`` as for ``trace``;
        ``light_states``: a contiguous (6, N) int32 CUDA tensor of RNG states of their own (``rng_states`` with
        ``first=N``), advanced in place by exactly the loop's draws, and not ``states`` itself.  Returns ``TraceDirect``;
        call ``.check()`` on it before trusting the answers of a mesh scene."""
        torch = _torch()
        n, dev, _ = _check_batch("rtmi_trace_direct", origins, directions)
        _need(states, "states", (STATE_WORDS, n), dev, torch.int32, words="(6, N)")
        _need(light_states, "light_states", (STATE_WORDS, n), dev, torch.int32, words="(6, N)")
        max_depth = int(max_depth)
        if not 0 <= max_depth <= MAX_DEPTH:
            raise RtmiError("max_depth %d outside [0, %d]" % (max_depth, MAX_DEPTH))
        out = _out_buffer(out, "(N, 3)", (n, 3), dev, torch.float32)
        stream = self._stream(dev)
        origins, directions = origins.contiguous(), directions.contiguous()
        rays = _new(dev, (n,), torch.int32) if count_rays else None
        work = _new(dev, (TRACE_WORK_WORDS,), torch.int64, zero=True)  # (n == 0 leaves it untouched)
        counts = _new(dev, (3,), torch.int64, zero=True)
        a = TraceDirectArgs()
        a.size, a.reserved, a.n, a.max_depth = C.sizeof(TraceDirectArgs), 0, n, max_depth
        a.d_origins, a.d_dirs, a.d_states, a.d_light_states = _addr(origins), _addr(directions), _addr(states), _addr(light_states)
        a.d_radiance, a.d_ray_counts, a.d_counts, a.d_work = _addr(out), _addr(rays), _addr(counts), _addr(work)
        with torch.cuda.device(dev):
            _check(self.L.rtmi_trace_direct(self.h, C.byref(a), stream), "rtmi_trace_direct")
        return TraceDirect(out, rays, work, counts, (origins, directions, states, light_states))

    def trace_roulette(self, origins, directions, states, max_depth, first_step=3, p_min=0.05, count_rays=False, out=None):
        """``trace`` with Russian roulette played inside the kernel (rtmi_trace_roulette), enqueued on torch's current stream:
        per path the steps, draws and kills of ``trace_steps_roulette(compact=True)`` in one launch, the radiance summed
        forward along the path (include/rtmi.h states the product; it differs from that loop's fold by the rounding order
        only).  The expectation is ``trace``'s.

        ``origins`` / ``directions`` / ``states`` / ``max_depth`` / ``count_rays`` / ``out`` as for ``trace``; ``first_step``,
        ``p_min`` as ``Roulette``'s.  Returns ``TraceRoulette``; call ``.check()`` on it before trusting the answers of a mesh
        scene."""
        torch = _torch()
        n, dev, _ = _check_batch("rtmi_trace_roulette", origins, directions)
        _need(states, "states", (STATE_WORDS, n), dev, torch.int32, words="(6, N)")
        max_depth = int(max_depth)
        if not 0 <= max_depth <= MAX_DEPTH:
            raise RtmiError("max_depth %d outside [0, %d]" % (max_depth, MAX_DEPTH))
        rule = Roulette(first_step, p_min)  # (its checks)
        out = _out_buffer(out, "(N, 3)", (n, 3), dev, torch.float32)
        stream = self._stream(dev)
        origins, directions = origins.contiguous(), directions.contiguous()
        rays = _new(dev, (n,), torch.int32) if count_rays else None
        work = _new(dev, (TRACE_WORK_WORDS,), torch.int64, zero=True)  # (n == 0 leaves it untouched)
        counts = _new(dev, (2,), torch.int64, zero=True)
        a = TraceRouletteArgs()
        a.size, a.reserved, a.n, a.max_depth = C.sizeof(TraceRouletteArgs), 0, n, max_depth
        a.first_step, a.p_min = rule.first_step, rule.p_min
        a.d_origins, a.d_dirs, a.d_states = _addr(origins), _addr(directions), _addr(states)
        a.d_radiance, a.d_ray_counts, a.d_counts, a.d_work = _addr(out), _addr(rays), _addr(counts), _addr(work)
        with torch.cuda.device(dev):
            _check(self.L.rtmi_trace_roulette(self.h, C.byref(a), stream), "rtmi_trace_roulette")
        return TraceRoulette(out, rays, work, counts, (origins, directions, states))

    def trace_steps_roulette(self, origins, directions, states, max_depth, roulette, each=None, hits=None, compact=False,
                             direct=False, light_states=None, shadow=None):
        """``trace_steps`` with Russian roulette: the same loop, every argument with ``trace_steps``' meaning, and after every
        step but the last ``path_roulette(k, result, states, roulette)`` on the step's candidates -- with ``direct`` behind
        that step's ``direct_sample`` and shadow query, and before ``each``.  With ``compact`` the compaction that follows
        drops the killed paths.  ``roulette``: a ``Roulette``, reset here; afterwards its ``throughput`` and ``counts`` are the
        loop's.  ``states`` advance by one more draw per roulette played; the radiance has ``trace``'s expectation.  Returns
        ``Steps``, exactly its fields."""
        if not isinstance(roulette, Roulette):
            raise RtmiError("roulette must be an rtmi.wavefront.Roulette")
        roulette.reset()
        return self._steps_loop(origins, directions, states, max_depth, each, hits, compact, direct, light_states, shadow, roulette)


class SceneBuilder(_CommitOptions, _FusedTraces):
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
        (int32) -- ``lights()["cdf"]`` and so on; length 0 when no world-list triangle or parallelogram emits (and, after
        ``light_kinds(spheres=True)``, no sphere: such a light has kind 2, p0 its centre, e1 = (R, R * R, 0))."""
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
        torch = _torch()
        if not isinstance(result, Bounce) or result.hits is None or result.steps is None:
            raise RtmiError("result must be the Bounce of a step made with hits=True and steps")
        o, d = result.origins, result.directions
        n, dev, _ = _check_batch("rtmi_direct_sample", o, d)
        step = int(step)
        if not 0 <= step < MAX_DEPTH:
            raise RtmiError("step %d outside [0, %d)" % (step, MAX_DEPTH))
        idx, n_list, cnt = _list_args(result.paths, n, dev)
        _need(light_states, "light_states", (STATE_WORDS, n), dev, torch.int32, words="(6, N)")
        _need(flags, "flags", (n,), dev, torch.int32, words="(N,)")
        counts = _out_buffer(counts, "(2,)", (2,), dev, torch.int64, zero=True, name="counts")
        if out is None:
            out = tuple(_new(dev, shape, torch.float32, zero=True) for shape in ((n, 3), (n, 3), (n,), (n, 3)))
        so, sd, st, dd = out
        for name, t, shape in (("origins", so, (n, 3)), ("directions", sd, (n, 3)), ("t_max", st, (n,)), ("direct", dd, (n, 3))):
            _need(t, "out's %s" % name, shape, dev, torch.float32)
        stream = self._stream(dev)
        if mis:
            carry = _out_buffer(carry, "(N, 4)", (n, 4), dev, torch.float32, zero=True, name="carry")
            a = DirectSampleMisArgs()
            a.size, a.reserved, a.n, a.n_list, a.step, a.sample = C.sizeof(DirectSampleMisArgs), 0, n, n_list, step, 1 if sample else 0
            a.d_list, a.d_count, a.d_origins, a.d_dirs = _addr(idx), _addr(cnt), _addr(o), _addr(d)
            a.d_hits, a.d_steps = _addr(result.hits.raw), _addr(result.steps)
            a.d_emitted, a.d_attenuation = _addr(result.emitted), _addr(result.attenuation)
            a.d_light_states, a.d_flags = _addr(light_states), _addr(flags)
            a.d_shadow_origins, a.d_shadow_dirs, a.d_shadow_t_max, a.d_direct = _addr(so), _addr(sd), _addr(st), _addr(dd)
            a.d_carry, a.d_counts = _addr(carry), _addr(counts)
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
        torch = _torch()
        n, dev, t_max = _check_batch("rtmi_intersect", origins, directions, t_max)
        out = _out_buffer(out, "(N, 12)", (n, HIT_WORDS), dev, torch.int32)
        stream = self._stream(dev)
        origins, directions = origins.contiguous(), directions.contiguous()
        abandoned = _new(dev, (1,), torch.int64, zero=True)
        with torch.cuda.device(dev):
            _check(self.L.rtmi_intersect(self.h, n, _ptr(origins), _ptr(directions), _ptr(t_max), _ptr(out), _ptr(abandoned), stream),
                   "rtmi_intersect")
        hits = Hits._from_raw(out)
        hits.abandoned = abandoned
        hits._rays = (origins, directions, t_max)  # (kept alive while the query may still read them)
        return hits

    def occluded(self, origins, directions, t_max=None, out=None):
        """Is anything in the way of each ray within t_max (rtmi_occluded), enqueued on torch's current stream.

        The answer for ray i is exactly ``intersect(...).kind[i] != RTMI_HIT_NONE`` with the same t_max (Sky counts,
        at t = 1e9; a NaN t_max is clear), found with t_max as a traversal bound and an early stop.  ``origins`` /
        ``directions`` / ``t_max`` as for ``intersect``; ``out``: an optional (N,) uint8 or bool CUDA tensor to
        write into.  Returns ``Occlusion``; call ``.check()`` on it before trusting the answers of a mesh scene."""
        return self._occlusion(False, None, origins, directions, t_max, out)

    def occluded_list(self, paths, origins, directions, t_max=None, out=None):
        """``occluded`` for the paths of a list only (rtmi_occluded_list), enqueued on torch's current stream.

        ``paths``: a ``Paths`` (``path_compact`` makes them; a step's ``Bounce.paths``), or None for the identity list over
        all N.  Every tensor is indexed by path and has ``occluded``'s shape with N paths.  A listed path gets exactly the
        byte ``occluded`` gives its ray; an entry >= N is skipped; the entries need not be distinct (the query changes no
        state).  The list's count is read on the device and the launch is sized by the list's capacity, not by N.
        ``out``: an optional (N,) uint8 or bool CUDA tensor that is UPDATED -- a path that is not listed keeps its byte;
        when it is None the answers start as zeros, so unlisted paths read "clear".  Returns ``Occlusion`` and refuses what
        ``occluded`` refuses."""
        return self._occlusion(True, paths, origins, directions, t_max, out)

    def _occlusion(self, listed, paths, origins, directions, t_max, out):
        torch = _torch()
        n, dev, t_max = _check_batch("rtmi_occluded_list" if listed else "rtmi_occluded", origins, directions, t_max)
        idx, n_list, cnt = _list_args(paths, n, dev)
        out = _out_buffer(out, "(N,)", (n,), dev, torch.uint8, torch.bool, zero=listed)  # (a list leaves unlisted bytes alone)
        stream = self._stream(dev)
        origins, directions = origins.contiguous(), directions.contiguous()
        raw = out.view(torch.uint8)
        counts = _new(dev, (2,), torch.int64, zero=True)
        args = (*_ptrs(origins, directions, t_max, raw, counts), stream)
        with torch.cuda.device(dev):
            if listed:
                _check(self.L.rtmi_occluded_list(self.h, n, _ptr(idx), n_list, _ptr(cnt), *args), "rtmi_occluded_list")
            else:
                _check(self.L.rtmi_occluded(self.h, n, *args), "rtmi_occluded")
        return Occlusion(raw, counts, (origins, directions, t_max, idx, cnt) if listed else (origins, directions, t_max))

    def trace(self, origins, directions, states, max_depth, count_rays=False, out=None):
        """Path-traced radiance of each ray (rtmi_trace): Trace(world, Ray(o, d), &state, max_depth) as a render runs
        it for one sample, enqueued on torch's current stream.

        ``origins`` / ``directions`` as for ``intersect``; ``states``: a contiguous (6, N) int32 CUDA tensor of RNG
        states (``rng_states``), advanced in place by the draws each path makes; ``max_depth`` in [0, 64];
        ``count_rays``: also return each ray's closest-hit queries; ``out``: an optional (N, 3) float32 CUDA tensor to
        write the radiance into.  Returns ``Trace``; call ``.check()`` on it before trusting the answers of a mesh
        scene."""
        torch = _torch()
        n, dev, _ = _check_batch("rtmi_trace", origins, directions)
        _need(states, "states", (STATE_WORDS, n), dev, torch.int32, words="(6, N)")
        max_depth = int(max_depth)
        if not 0 <= max_depth <= MAX_DEPTH:
            raise RtmiError("max_depth %d outside [0, %d]" % (max_depth, MAX_DEPTH))
        out = _out_buffer(out, "(N, 3)", (n, 3), dev, torch.float32)
        stream = self._stream(dev)
        origins, directions = origins.contiguous(), directions.contiguous()
        rays = _new(dev, (n,), torch.int32) if count_rays else None
        work = _new(dev, (TRACE_WORK_WORDS,), torch.int64, zero=True)  # (n == 0 leaves it untouched)
        with torch.cuda.device(dev):
            _check(self.L.rtmi_trace(self.h, n, _ptr(origins), _ptr(directions), max_depth, _ptr(states), _ptr(out), _ptr(rays),
                                     _ptr(work), stream), "rtmi_trace")
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
        torch = _torch()
        n, dev, _ = _check_batch("rtmi_bounce_list" if listed else "rtmi_bounce", origins, directions)
        idx, n_list, cnt = _list_args(paths, n, dev)
        if not (origins.is_contiguous() and directions.is_contiguous()):
            raise RtmiError("origins and directions must be contiguous: rtmi_bounce writes the scattered rays into them")
        # (a loop calls this once per step: what is None is not handed to a check, and torch allocates without a helper between)
        _need(states, "states", (STATE_WORDS, n), dev, torch.int32, words="(6, N)")
        for name, t in (("emitted", emitted), ("attenuation", attenuation)):
            if t is not None:
                _need(t, name, (n, 3), dev, torch.float32, words="(N, 3)")
        if steps is not None:
            _need(steps, "steps", (n,), dev, torch.int32, words="(N,)")
        raw = None
        if isinstance(hits, torch.Tensor):
            raw = _out_buffer(hits, "(N, 12)", (n, HIT_WORDS), dev, torch.int32)
        elif hits:
            raw = torch.empty((n, HIT_WORDS), dtype=torch.int32, device=dev)
        stream = self._stream(dev)
        if emitted is None:
            emitted = torch.empty((n, 3), dtype=torch.float32, device=dev)
        if attenuation is None:
            attenuation = torch.empty((n, 3), dtype=torch.float32, device=dev)
        work = torch.zeros((TRACE_WORK_WORDS,), dtype=torch.int64, device=dev)  # (n == 0 leaves it untouched)
        args = _ptrs(origins, directions, states, emitted, attenuation, raw, steps, work)
        with torch.cuda.device(dev):
            if listed:
                _check(self.L.rtmi_bounce_list(self.h, n, _ptr(idx), n_list, _ptr(cnt), *args, stream), "rtmi_bounce_list")
            else:
                _check(self.L.rtmi_bounce(self.h, n, *args, stream), "rtmi_bounce")
        rec = Hits._from_raw(raw) if raw is not None else None
        return Bounce(origins, directions, states, emitted, attenuation, rec, steps, work, paths if listed else None)

    def trace_steps(self, origins, directions, states, max_depth, each=None, hits=None, compact=False, direct=False,
                    light_states=None, shadow=None):
        """rtmi_trace as a loop of ``max_depth`` steps and one fold, on copies of the rays: bit for bit ``trace``'s
        radiance while ``each`` changes nothing.  ``states`` advance in place, as in ``trace``.  ``each(step, result)``
        is called after every step is enqueued, with the step's ``Bounce`` (``result.origins`` / ``.directions`` are the
        loop's own ray tensors): the place for shadow rays from ``result.hits``, or a termination rule -- zeroing a path's
        direction ends it, and the fold then takes its last layer's emitted as the path's end (Russian roulette is built:
        ``trace_steps_roulette``).  ``hits``: whether the
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
        return self._steps_loop(origins, directions, states, max_depth, each, hits, compact, direct, light_states, shadow, None)

    def _steps_loop(self, origins, directions, states, max_depth, each, hits, compact, direct, light_states, shadow, roulette):
        """The loop of ``trace_steps`` and, with a ``Roulette``, of ``trace_steps_roulette``."""
        torch = _torch()
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
            shadow = _abi.SHADOW_DEFAULT if (compact and direct) else "all"
        n, dev, _ = _check_batch("rtmi_bounce", origins, directions)
        max_depth = int(max_depth)
        if not 0 <= max_depth <= MAX_DEPTH:
            raise RtmiError("max_depth %d outside [0, %d]" % (max_depth, MAX_DEPTH))
        _need(states, "states", (STATE_WORDS, n), dev, torch.int32, words="(6, N)")
        self._stream(dev)
        o, d = origins.clone().contiguous(), directions.clone().contiguous()
        layers = max(max_depth, 1)
        # (a per-sample loop calls this once per sample: torch allocates without a helper between)
        zeros = lambda shape, dtype=torch.float32: torch.zeros(shape, dtype=dtype, device=dev)
        E, A = (torch.empty((layers, n, 3), dtype=torch.float32, device=dev) for _ in range(2))
        steps = zeros((n,), torch.int32)
        want_hits = (each is not None) if hits is None else bool(hits)
        mis = direct == "mis"
        Dk = occ = flags = rays = carry = None
        if direct:
            want_hits = True
            _need(light_states, "light_states", (STATE_WORDS, n), dev, torch.int32, words="(6, N)")
            Dk, occ, flags = zeros((layers, n, 3)), zeros((layers, n), torch.uint8), zeros((n,), torch.int32)
            rays = (zeros((n, 3)), zeros((n, 3)), zeros((n,)))  # (the shadow rays: one set, rewritten every step)
            counts = zeros((2,), torch.int64)
            if mis:
                carry = zeros((n, 4))  # (one for the loop)
        works = []
        lists, cur = None, None
        if compact and max_depth > 0:
            lists = [_new_paths(dev, n), _new_paths(dev, n)]
            cur = _path_compact(n, o, d, None, n, None, lists[0], dev)
        for k in range(max_depth):
            r = self._step(bool(compact), cur, o, d, states, E[k], A[k], want_hits, steps)  # (bounce_list on cur, or bounce)
            works.append(r.work)
            if direct:
                self.direct_sample(k, r, light_states, flags, sample=k + 1 < max_depth, out=rays + (Dk[k],), counts=counts,
                                   mis=mis, carry=carry)
                if shadow == "list":
                    q = self.occluded_list(r.paths, rays[0], rays[1], rays[2], out=occ[k])
                else:
                    q = self.occluded(rays[0], rays[1], rays[2], out=occ[k])
                r.work[0] += q.counts[0]  # (abandoned searches: check())
            if roulette is not None and k + 1 < max_depth:  # (behind the step's direct light: D[k] is formed from the unscaled A[k])
                path_roulette(k, r, states, roulette)
            if each is not None:
                each(k, r)
            if compact and k + 1 < max_depth:  # the next step's list: the live ones of this step's (or of all N)
                nxt = lists[(k + 1) & 1]
                idx, cnt = (None, None) if compact == "full" else (cur.index, cur.count)
                cur = _path_compact(n, o, d, idx, n, cnt, nxt, dev)
        rgb = path_fold_direct(d, steps, E, A, Dk, occ) if direct else path_fold(d, steps, E, A)
        st = Steps(rgb, steps, (d != 0).any(dim=1), o, d, E, A, works, Dk, occ, flags)  # (None where the loop was not direct)
        st.carry = carry
        return st

    def _stream(self, dev):
        """torch's current stream on dev, the rays' device; raises unless the scene was committed there."""
        if self.h.value is None or getattr(self, "device", None) is None:
            raise RtmiError("scene not committed")
        if dev != self.device:
            raise RtmiError("the rays are on %s, the scene was committed on %s" % (dev, self.device))
        return _stream(dev)
