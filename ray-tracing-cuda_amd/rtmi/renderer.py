"""``Renderer``: one rank's share of a frame -- its device buffers, the render entries, the per-pixel sample budgets, the
composed loops over camera rays and wavefronts, and the way back to a row-major image."""
import collections
import ctypes as C

import numpy as np

from ._abi import (BUDGET_WORK_WORDS, MAX_DEPTH, MODE_FIELDS, STATE_WORDS, TRACE_WORK_WORDS, Projection, PathAdvanceArgs,
                   RenderDirectArgs, RtmiError, _addr, _check, _u32p, adaptive_opts, feature_bufs, lib, make_frame, work_items)
from ._tensors import _need, _new, _out_buffer, _ptr, _stream
from .filters import denoise
from .wavefront import _list_args, _new_paths, rng_states


class Adaptive(collections.namedtuple("Adaptive", "tiles samples passes total_samples features", defaults=(None,))):
    """What ``Renderer.render_adaptive`` returns: ``tiles`` (items, 3) float32, the resolved tile buffer; ``samples``
    (items,) int32, the samples each work item got; ``passes`` rendered; ``total_samples`` over the shard;
    ``features``: with ``features=True`` the resolved ``ResolvedFeatures``, else None."""


ResolvedFeatures = collections.namedtuple("ResolvedFeatures", "albedo normal depth alpha")
"""What ``Renderer.resolve_features`` returns, tile-major: ``albedo`` and ``normal`` (items, 3) float32 (the mean normal
is not renormalised), ``depth`` (items,) float32 (the mean over the samples that hit a surface, 0 where none did),
``alpha`` (items,) float32 (the share of the samples that hit a surface)."""


class _DirectRenders:
    """The budget renders with next-event estimation inside the kernel.  A base of ``Renderer``: they are the renderer's
    methods."""

    def render_direct(self, budget, count_rays=True, features=False):
        """``render_budget(budget, count_rays, features)`` with every sample traced with next-event estimation inside the
        kernel (rtmi_render_direct), enqueued on torch's current stream: one launch for what
        ``render_rays(budget, direct="fused")`` composes of three per sample index, bit for bit its sums, moments, counts
        and states, in the buffers of ``render_budget`` -- so ``plan``, ``resolve``, ``resolve_variance``, ``denoise`` and
        ``accumulate`` follow unchanged.  The light states are ``render_rays``' own -- seeded from the scene's seed with
        first = items on first use, kept in ``light_states`` -- so the two interleave; the three counters (vertices
        sampled, emissions weighed, shadow rays answered occluded) add up in ``direct_counts``, a (3,) int64 tensor zeroed
        on first use."""
        self._need(budget, "budget", (), self.torch.int32)
        self._budget_buffers()
        with self.torch.cuda.device(self.device):
            if self.direct_counts is None:
                self.direct_counts = self._new((3,), self.torch.int64, zero=True)
            a = RenderDirectArgs()
            a.size, a.reserved = C.sizeof(RenderDirectArgs), 0
            a.d_budget, a.d_states, a.d_light_states = _addr(budget), _addr(self.states), _addr(self._light_states())
            a.d_sum, a.d_sq, a.d_samples = _addr(self.sum), _addr(self.sq), _addr(self.samples)
            a.d_ray_counts = _addr(self.budget_rays) if count_rays else None
            a.d_counts, a.d_work = _addr(self.direct_counts), _addr(self.d_work)
            feat = None
            if features:
                self._feature_buffers()
                feat = feature_bufs(self.albedo, self.normal, self.depth, self.coverage)
                a.features = C.pointer(feat)
            _check(self.L.rtmi_render_direct(self.scene.h, C.byref(self.frame), C.byref(a), self._stream()), "rtmi_render_direct")
            self.budget_abandoned += self.d_work[0]  # (stream-ordered: the next call resets d_work)
        return self

    def render_adaptive_direct(self, min_spp, max_spp, step, tolerance, floor=0.01, post=True, features=False):
        """``render_adaptive`` whose every pass is ``render_direct``: the same plan, stopping rule and result."""
        return self._adaptive(self.render_direct, min_spp, max_spp, step, tolerance, floor, post, features)


class Renderer(_DirectRenders):
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
            self.states = self._new((STATE_WORDS, self.items), torch.int32)
            self.tiles = self._new((self.items, 3))
            self.ray_counts = self._new((self.items,), torch.int32)
        # made and zeroed on first use: the budget buffers (_budget_buffers), the feature sums (_feature_buffers), ...
        self.sum = self.sq = self.samples = self.budget_rays = self.d_work = self.budget_abandoned = None
        self.budget = self.totals = None
        self.albedo = self.normal = self.depth = self.coverage = None
        # ... and what render_rays and render_wavefront keep between calls; the scratch of the last render(opts)
        self.rays_total = self.wavefront_counts = self.light_states = self.carry = self._last_scratch = None
        self.direct_counts = None  # render_direct: (3,) int64, vertices sampled, emissions weighed, shadow rays occluded

    def _stream(self):
        return _stream(self.device)

    def _call(self, entry, *args):
        """``entry(*args, stream)`` on the renderer's device and torch's current stream, checked."""
        with self.torch.cuda.device(self.device):
            return _check(getattr(self.L, entry)(*args, self._stream()), entry)

    def _new(self, shape, dtype=None, zero=False):
        """A tensor on the renderer's device (float32 unless ``dtype`` says otherwise; ``zero``: of zeros)."""
        return _new(self.device, shape, dtype or self.torch.float32, zero)

    def _need(self, t, name, tail, dtype, optional=False):
        """``_need`` for a tensor of shape (items, *tail) on the renderer's device."""
        words = "(items%s)" % ("".join(", %d" % k for k in tail) or ",")
        return _need(t, name, (self.items,) + tail, self.device, dtype, words=words, where="the renderer's", optional=optional)

    def init_rng(self, seed=None):
        seed = self.scene.seed if seed is None else seed
        self._call("rtmi_rng_init", C.c_uint64(seed), C.byref(self.frame), _ptr(self.states))
        # pixel 0 (work item 0 of rank 0) continues the stream the scene program drew from
        if self.frame.rank == 0 and seed == self.scene.seed and not np.array_equal(self.scene.state0, self.scene.state0_fresh):
            self._call("rtmi_rng_set_state", C.byref(self.frame), _ptr(self.states), 0, self.scene.state0.ctypes.data_as(_u32p))
        return self

    def render(self, count_rays=True, opts=None):
        """Enqueue the trace kernel on torch's current stream (asynchronous).  ``opts``: a
        ``render_opts(...)`` structure with per-call scheduling options (None = the defaults)."""
        self._last_scratch = opts.d_scratch if opts is not None else None
        self._call("rtmi_render_ex", self.scene.h, C.byref(self.frame), C.byref(opts) if opts is not None else None,
                   _ptr(self.states), _ptr(self.tiles), _ptr(self.ray_counts) if count_rays else None)
        return self

    def check(self):
        """Wait for the last render and raise if it reported an incomplete frame (rtmi_render_status); with budget
        renders behind it (``render_budget``), also if any of them abandoned a mesh search."""
        if self.budget_abandoned is not None:
            n = int(self.budget_abandoned.item())  # (a device-to-host copy: waits for the calls)
            if n:
                raise RtmiError("rtmi_render_budget abandoned %d mesh search(es): the sums are incomplete" % n)
        self._call("rtmi_render_status", self.scene.h, C.c_void_p(self._last_scratch), None)
        return self

    # -------------------------------------------------------------- per-pixel sample budgets
    def _budget_buffers(self):
        if self.sum is None:
            torch, n, zeros = self.torch, self.items, lambda shape, dtype=None: self._new(shape, dtype, zero=True)
            self.sum, self.sq = zeros((n, 3)), zeros((n, 3))
            self.samples, self.budget_rays, self.budget = zeros((n,), torch.int32), zeros((n,), torch.int32), zeros((n,), torch.int32)
            self.d_work = zeros((BUDGET_WORK_WORDS,), torch.int64)
            self.budget_abandoned = zeros((), torch.int64)  # d_work[0] over all calls
            self.totals = zeros((2,), torch.int64)

    def _feature_buffers(self):
        if self.albedo is None:
            n = self.items
            self.albedo, self.normal, self.depth = (self._new(shape, zero=True) for shape in ((n, 3), (n, 3), (n,)))
            self.coverage = self._new((n,), self.torch.int32, zero=True)

    def _count_rays_total(self):
        if self.rays_total is None:
            self.rays_total = self._new((), self.torch.int64, zero=True)

    def _unposted(self, method):
        if self.frame.post_process:
            raise RtmiError("%s needs a frame made with post=False: per-pixel sample counts have no uniform division (resolve)" % method)

    def _most(self, budget):
        """The largest active budget, capped by the frame's spp (None: that spp); one read-back, a synchronisation."""
        spp = int(self.frame.spp)
        if budget is None:
            return spp
        if not self.items:
            return 0
        return min(spp, int((budget.to(self.torch.int64) & 0xffffffff).max().item()))  # (uint32 words: a negative int32 is a large one)

    def _light_states(self):
        """The light states of the direct renders (``render_rays(direct=...)``, ``render_direct``): seeded from
        the scene's seed with first = items on first use and carried on, so the ways to direct light interleave."""
        if self.light_states is None:
            self.light_states = rng_states(self.scene.seed, self.items, first=self.items, device=self.device)
        return self.light_states

    def render_budget(self, budget, count_rays=True, features=False):
        """``budget[q]`` more samples (at most the frame's spp per call) of every pixel q of this shard
        (rtmi_render_budget), enqueued on torch's current stream: continues each pixel's RNG stream in ``states`` and
        adds to ``sum`` (radiance), ``sq`` (squares), ``samples`` and, with ``count_rays``, ``budget_rays`` -- zeroed
        on first use and kept as attributes.  ``budget``: a contiguous (items,) int32 CUDA tensor.  The frame must
        have been made with ``post=False``.  ``features``: also add the primary hit of every sample to ``albedo``,
        ``normal``, ``depth`` and ``coverage`` (rtmi_render_features; zeroed on first use; max_depth >= 1)."""
        self._need(budget, "budget", (), self.torch.int32)
        self._budget_buffers()
        args = (self.scene.h, C.byref(self.frame), _ptr(budget), _ptr(self.states), _ptr(self.sum), _ptr(self.sq), _ptr(self.samples),
                _ptr(self.budget_rays) if count_rays else None)
        with self.torch.cuda.device(self.device):
            if features:
                self._feature_buffers()
                feat = feature_bufs(self.albedo, self.normal, self.depth, self.coverage)
                _check(self.L.rtmi_render_features(*args, C.byref(feat), _ptr(self.d_work), self._stream()), "rtmi_render_features")
            else:
                _check(self.L.rtmi_render_budget(*args, _ptr(self.d_work), self._stream()), "rtmi_render_budget")
            self.budget_abandoned += self.d_work[0]  # (stream-ordered: the next call resets d_work)
        return self

    # -------------------------------------------------------------- camera rays
    def _budget_arg(self, budget):
        return _ptr(self._need(budget, "budget", (), self.torch.int32, optional=True))

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
        if out is None:
            out = (None, None)
        elif not (isinstance(out, (tuple, list)) and len(out) == 2):
            raise RtmiError("out must be a pair of (items, 3) float32 CUDA tensors: (origins, directions)")
        origins, dirs = (_out_buffer(t, "(items, 3)", (self.items, 3), self.device, torch.float32) for t in out)
        self._call("rtmi_camera_rays", self.scene.h, C.byref(self.frame), C.byref(projection) if projection is not None else None,
                   d_budget, int(sample), _ptr(self.states), _ptr(origins), _ptr(dirs))
        return origins, dirs

    def sample_add(self, sample, radiance, trace_counts=None, budget=None):
        """Fold the traced sample ``sample`` into ``sum``, ``sq``, ``samples`` and -- with ``trace_counts`` --
        ``budget_rays`` (rtmi_sample_add; the buffers of ``render_budget``, zeroed on first use), on torch's current stream.
        ``radiance``: (items, 3) float32, ``trace_counts``: (items,) int32 or None, as ``SceneBuilder.trace`` returns them;
        ``budget`` as for ``camera_rays``: only the items active in this sample are touched."""
        self._need(radiance, "radiance", (3,), self.torch.float32)
        self._need(trace_counts, "trace_counts", (), self.torch.int32, optional=True)
        d_budget = self._budget_arg(budget)
        self._budget_buffers()
        self._call("rtmi_sample_add", C.byref(self.frame), d_budget, int(sample), _ptr(radiance), _ptr(trace_counts), _ptr(self.sum),
                   _ptr(self.sq), _ptr(self.samples), _ptr(self.budget_rays) if trace_counts is not None else None)
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
        (multiple importance sampling); ``self.carry`` is then the last sample's carry tensor, else None.
        ``direct="fused"`` traces every sample with one ``SceneBuilder.trace_direct`` on the same light states: the
        ``"mis"`` loop's samples in one kernel per sample, its sums up to the rounding order of the direct light's sum."""
        torch = self.torch
        self._unposted("render_rays")
        self._budget_arg(budget)
        self._budget_buffers()
        self._count_rays_total()
        n_samples = self._most(budget)
        with torch.cuda.device(self.device):
            origins, dirs, radiance = (self._new((self.items, 3)) for _ in range(3))
            counts = self._new((self.items,), torch.int32) if count_rays else None
            work = self._new((TRACE_WORK_WORDS,), torch.int64, zero=True)  # one d_work, reused in stream order
            stream = self._stream()
            for sample in range(n_samples):
                self.camera_rays(sample, budget, projection, out=(origins, dirs))
                if each is not None:
                    each(sample, origins, dirs)
                if isinstance(direct, str) and direct == "fused":
                    t = self.scene.trace_direct(origins, dirs, self.states, self._light_states(), int(self.frame.max_depth),
                                                count_rays=count_rays, out=radiance)
                    self.budget_abandoned += t.work[0]
                    self.rays_total += t.work[1]
                    self.sample_add(sample, radiance, t.rays, budget)
                    continue
                if direct:
                    st = self.scene.trace_steps(origins, dirs, self.states, int(self.frame.max_depth), compact=True, direct=direct,
                                                light_states=self._light_states())
                    self.carry = st.carry
                    for w in st.works:
                        self.budget_abandoned += w[0]
                    queries = st.steps + st.alive.to(torch.int32)
                    self.rays_total += queries.sum()
                    self.sample_add(sample, st.rgb, queries if count_rays else None, budget)
                    continue
                _check(self.L.rtmi_trace(self.scene.h, self.items, _ptr(origins), _ptr(dirs), int(self.frame.max_depth),
                                         _ptr(self.states), _ptr(radiance), _ptr(counts), _ptr(work), stream), "rtmi_trace")
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
        self._call("rtmi_path_advance", self.scene.h, C.byref(self.frame), C.byref(a))
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
            self._need(t, name, (3,), torch.float32)
        self._need(steps, "steps", (), torch.int32)
        self._need(cursor, "cursor", (2,), torch.int32)
        if stacks is None:
            stacks = (None, None)
        if not (isinstance(stacks, (tuple, list)) and len(stacks) == 2):
            raise RtmiError("stacks must be a pair of (max_depth, items, 3) float32 CUDA tensors, or None at max_depth 0")
        for k, t in enumerate(stacks):
            _need(t, "stacks[%d]" % k, (depth, n, 3), dev, torch.float32, words="(max_depth, items, 3)", where="the renderer's",
                  optional=depth == 0)
        _need(counts, "counts", (3,), dev, torch.int64, words="(3,)", where="the renderer's", optional=True)
        d_budget = self._budget_arg(budget)
        self._budget_buffers()
        a = PathAdvanceArgs()
        a.size, a.reserved, a.d_budget = C.sizeof(PathAdvanceArgs), 0, d_budget
        a.proj = C.pointer(projection) if projection is not None else None
        a.d_list, a.n_list, a.d_count = _addr(idx), n_list, _addr(cnt)
        a.d_origins, a.d_dirs, a.d_states, a.d_steps = _addr(origins), _addr(directions), _addr(self.states), _addr(steps)
        a.d_emitted, a.d_attenuation, a.d_cursor = _addr(emitted), _addr(attenuation), _addr(cursor)
        a.d_emitted_stack, a.d_attenuation_stack = _addr(stacks[0]), _addr(stacks[1])
        a.d_sum, a.d_sq, a.d_samples = _addr(self.sum), _addr(self.sq), _addr(self.samples)
        a.d_ray_counts, a.d_counts = _addr(self.budget_rays) if count_rays else None, _addr(counts)
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
        self._unposted("render_wavefront")
        poll = int(poll)
        if poll < 1:
            raise RtmiError("poll must be at least 1")
        self._budget_arg(budget)
        self._budget_buffers()
        n, dev, depth = self.items, self.device, int(self.frame.max_depth)
        if not 0 <= depth <= MAX_DEPTH:
            raise RtmiError("max_depth %d outside [0, %d]" % (depth, MAX_DEPTH))
        self._count_rays_total()
        if self.wavefront_counts is None:
            self.wavefront_counts = self._new((3,), torch.int64, zero=True)
        most = self._most(budget)
        bound = most * max(depth, 1) + 1
        self.wavefront_iterations = 0
        with torch.cuda.device(dev):
            origins, dirs, emitted, attenuation = (self._new((n, 3), zero=True) for _ in range(4))
            steps = self._new((n,), torch.int32, zero=True)
            cursor = self._new((n, 2), torch.int32, zero=True)
            stacks = (self._new((depth, n, 3)), self._new((depth, n, 3))) if depth > 0 else None
            queries_before = self.wavefront_counts[1].clone()
            lists = [_new_paths(dev, n), _new_paths(dev, n)]
            # Everything an iteration passes is checked and turned into ctypes values ONCE: with them an iteration is three
            # foreign calls, and the loop is bound by the device, not by the interpreter (DESIGN.md 2.16 has the figures).
            L, h, fr, stream = self.L, self.scene.h, C.byref(self.frame), self.scene._stream(dev)
            rest = (origins, dirs, steps, emitted, attenuation, stacks, cursor, budget, projection, self.wavefront_counts, count_rays)
            start, keep = self._advance_args(None, *rest)
            adv = [self._advance_args(p, *rest)[0] for p in lists]
            p_o, p_d, p_st, p_steps = _ptr(origins), _ptr(dirs), _ptr(self.states), _ptr(steps)
            p_em, p_at = _ptr(emitted), _ptr(attenuation)
            p_idx, p_cnt = [_ptr(p.index) for p in lists], [_ptr(p.count) for p in lists]
            scratch = self._new((max(L.rtmi_path_compact_scratch_bytes(n) // 4, 1),), torch.int32)
            p_scratch = _ptr(scratch)  # (one scratch: the compactions follow each other on one stream)
            # the steps' work blocks: a ring, its abandoned searches summed and the ring cleared whenever it has gone round
            ring = self._new((64, TRACE_WORK_WORDS), torch.int64, zero=True)
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
        n = self.items
        out = ResolvedFeatures(*(self._new(shape) for shape in ((n, 3), (n, 3), (n,), (n,))))
        sums = feature_bufs(self.albedo, self.normal, self.depth, self.coverage)
        to = feature_bufs(*out)
        self._call("rtmi_resolve_features", C.byref(self.frame), C.byref(sums), _ptr(self.samples), C.byref(to))
        return out

    def plan(self, min_spp, max_spp, step, tolerance, floor=0.01):
        """The next pass's budget from the sums so far (rtmi_budget_plan; the rule is in include/rtmi.h).  Returns
        (budget tensor, pixels with a budget, sum of the budgets); reading the two totals waits for the stream."""
        self._budget_buffers()
        o = adaptive_opts(min_spp, max_spp, step, tolerance, floor)
        self._call("rtmi_budget_plan", C.byref(self.frame), C.byref(o), _ptr(self.sum), _ptr(self.sq), _ptr(self.samples),
                   _ptr(self.budget), _ptr(self.totals))
        active, total = self.totals.tolist()
        return self.budget, active, total

    def resolve(self, post=True):
        """(items, 3) tile buffer: sum / samples per pixel, post-processed like a render's (rtmi_resolve)."""
        self._budget_buffers()
        out = self._new((self.items, 3))
        self._call("rtmi_resolve", C.byref(self.frame), _ptr(self.sum), _ptr(self.samples), 1 if post else 0, _ptr(out))
        return out

    def resolve_variance(self):
        """(items, 3) tile buffer: the variance of each pixel's MEAN from the sums so far (rtmi_resolve_variance; the
        rule is in include/rtmi.h): 0 where a pixel has no samples and for padding."""
        self._budget_buffers()
        out = self._new((self.items, 3))
        self._call("rtmi_resolve_variance", C.byref(self.frame), _ptr(self.sum), _ptr(self.sq), _ptr(self.samples), _ptr(out))
        return out

    def denoise_inputs(self):
        """The row-major buffers ``denoise`` filters, as a dict of rtmi.denoise's arguments: color (resolved without
        post-processing), variance, normal, depth, alpha, albedo."""
        if self.frame.world_size != 1:
            raise RtmiError("Renderer.denoise works on a whole frame (world_size 1): gather the resolved colour, variance "
                            "and feature buffers of all ranks, untile them and call rtmi.denoise")
        if self.sum is None or self.albedo is None:
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
            self._call("rtmi_post_process", _ptr(img), self.frame.height * self.frame.width, 1)
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
            if self.rays_total is not None:
                self.rays_total.zero_()
        return self

    def accumulate(self, acc):
        """``denoise_inputs()`` of the frame so far, accumulated into ``acc`` (an ``Accumulator`` of this frame's extent) as
        seen from the scene's present camera: the same dict with ``color`` and ``variance`` replaced by the accumulated
        ones, so a sequence is ``scene.camera_look(...)``, ``new_frame()``, ``render_budget(..., features=True)``,
        ``rtmi.denoise(**R.accumulate(acc))`` per frame."""
        buf = self.denoise_inputs()  # (refuses a shard first, as for denoise)
        color, variance, _ = acc.step(buf["color"], buf["variance"], buf["normal"], buf["depth"], buf["alpha"],
                                      camera=self.scene.camera_get())
        return dict(buf, color=color, variance=variance)

    def render_adaptive(self, min_spp, max_spp, step, tolerance, floor=0.01, post=True, features=False):
        """Plan / render passes until no pixel has a budget left: every pixel gets ``min_spp`` samples, then ``step``
        more per pass until it meets the stopping rule or has ``max_spp``.  One host read of the plan's totals per
        pass is the only synchronisation.  The frame's spp must be at least max(min_spp, step).  ``features``: every
        pass also adds to the first-hit feature buffers, and the result's ``features`` holds them resolved."""
        return self._adaptive(self.render_budget, min_spp, max_spp, step, tolerance, floor, post, features)

    def _adaptive(self, render, min_spp, max_spp, step, tolerance, floor, post, features):
        """The loop of ``render_adaptive``, its passes rendered by ``render`` (``render_budget`` or ``render_direct``)."""
        if self.frame.spp < max(int(min_spp), int(step)):
            raise RtmiError("the frame's spp (%d) caps one pass: it must be at least max(min_spp, step)" % self.frame.spp)
        passes = total = 0
        while True:
            budget, active, pass_total = self.plan(min_spp, max_spp, step, tolerance, floor)
            if active == 0:
                break
            render(budget, features=features)
            passes, total = passes + 1, total + pass_total
        self.check()
        return Adaptive(self.resolve(post), self.samples, passes, total, self.resolve_features() if features else None)

    def scratch_bytes(self):
        return int(self.L.rtmi_render_scratch_bytes(C.byref(self.frame)))

    def new_scratch(self):
        """Device memory for the per-call state of one render (``render_opts(scratch=...)``)."""
        return self._new((self.scratch_bytes() + 7) // 8, self.torch.int64, zero=True)

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
        self._call("rtmi_render_status", self.scene.h, _ptr(scratch), C.byref(out))
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
            img = self._new((f.height, f.width, 3), zero=True)
            _check(self.L.rtmi_untile(C.byref(f), _ptr(tiles), _ptr(img), self._stream()), "rtmi_untile")
            cnt = None
            counts = self.ray_counts if (all_counts is None and f.world_size == 1) else all_counts
            if counts is not None:
                cnt = self._new((f.height, f.width), torch.float32 if counts.dtype == torch.float32 else torch.int32, zero=True)
                _check(self.L.rtmi_untile_u32(C.byref(f), _ptr(counts), _ptr(cnt), self._stream()), "rtmi_untile_u32")
        return img, cnt


def debug_schedule(frame, scratch, ray_counts, work_counts=None, pixel_head=False, sparse_cap=0, grid_waves=0, outlier_x10=20,
                   head_pct=(50, 25, 12), simds=0, rounds=0, spp=1, probe_spp=1):
    """The scheduler step of a scheduled render on the caller's own counts (rtmi_debug_schedule): ``scratch``, ``ray_counts``
    and ``work_counts`` are torch CUDA tensors; the plan is left in ``scratch`` (``scratch_regions``), the head's marks in
    ``ray_counts``.  On torch's current stream."""
    import torch
    with torch.cuda.device(scratch.device):
        _check(lib().rtmi_debug_schedule(C.byref(frame), _ptr(scratch), scratch.numel() * scratch.element_size(), _ptr(ray_counts),
                                         _ptr(work_counts), 1 if pixel_head else 0, int(sparse_cap), int(grid_waves),
                                         int(outlier_x10), (C.c_int32 * 3)(*head_pct), int(simds), int(rounds), int(spp),
                                         int(probe_spp), _stream(scratch.device)), "rtmi_debug_schedule")
