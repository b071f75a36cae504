"""The value types of the ray queries and of a wavefront of paths, and the free functions over path arrays: the folds,
the compaction, Russian roulette and the RNG states (rtmi_path_fold, rtmi_path_fold_direct, rtmi_path_compact,
rtmi_path_roulette, rtmi_rng_init_n)."""
import collections
import ctypes as C

from ._abi import MAX_DEPTH, STATE_WORDS, PathRouletteArgs, RtmiError, _addr, _check, lib
from ._tensors import _check_batch, _lead, _need, _new, _out_buffer, _ptr, _ptrs, _stream, _torch


def _complete(abandoned, entry, where=""):
    """Wait for the call that counts its abandoned mesh searches in ``abandoned`` (a device-to-host copy); raise if there are any."""
    n = int(abandoned.item())
    if n:
        raise RtmiError("%s abandoned %d mesh search(es)%s: the answers are incomplete" % (entry, n, where))


class Hits(collections.namedtuple("Hits", "t uv normal material kind entry element")):
    """What ``SceneBuilder.intersect`` returns: views into one (N, 12) int32 buffer of rtmi_hit records (``raw``) --
    t (N,) float32 (+inf: no hit), uv (N, 2) float32, normal (N, 3) float32, material / kind / entry / element (N,)
    int32.  ``check()`` waits for the query and raises when it abandoned a mesh search (its answers are then not to
    be used)."""

    @classmethod
    def _from_raw(cls, raw):
        """The views over an (N, 12) int32 buffer of records, which ``raw`` then names."""
        f = raw.view(_torch().float32)
        hits = cls(f[:, 0], f[:, 1:3], f[:, 3:6], raw[:, 6], raw[:, 7], raw[:, 8], raw[:, 9])
        hits.raw = raw
        return hits

    def check(self):
        _complete(self.abandoned, "rtmi_intersect")
        return self


class Occlusion:
    """What ``SceneBuilder.occluded`` returns: ``mask`` (N,) torch.bool, a view of the (N,) uint8 output ``raw`` (1:
    occluded).  ``check()`` waits for the query and raises when it abandoned a mesh search (the answers are then not
    to be used); ``fallback_rays()`` is how many rays the exact unbounded fallback answered (rtmi_occluded's
    d_counts[1])."""

    def __init__(self, raw, counts, rays):
        torch = _torch()
        self.raw, self.counts = raw, counts
        self.mask = raw.view(torch.bool)
        self._rays = rays  # (kept alive while the query may still read them)

    def check(self):
        _complete(self.counts[0], "rtmi_occluded")
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
        _complete(self.work[0], "rtmi_trace")
        return self

    def total_rays(self):
        return int(self.work[1].item())


class TraceDirect(Trace):
    """What ``SceneBuilder.trace_direct`` returns: a ``Trace`` (``rgb``, ``rays``, ``work``, ``check()``, ``total_rays()`` --
    the paths' closest-hit queries, shadow queries not among them) and ``counts`` (3,) int64: vertices sampled, emissions
    weighed, shadow rays answered occluded."""

    def __init__(self, rgb, rays, work, counts, keep):
        Trace.__init__(self, rgb, rays, work, keep)
        self.counts = counts

    def check(self):
        _complete(self.work[0], "rtmi_trace_direct")
        return self


class TraceRoulette(Trace):
    """What ``SceneBuilder.trace_roulette`` returns: a ``Trace`` (``rgb``, ``rays``, ``work``, ``check()``, ``total_rays()``) and
    ``counts`` (2,) int64: roulettes played, paths killed."""

    def __init__(self, rgb, rays, work, counts, keep):
        Trace.__init__(self, rgb, rays, work, keep)
        self.counts = counts

    def check(self):
        _complete(self.work[0], "rtmi_trace_roulette")
        return self


class Roulette:
    """Russian roulette for a loop of steps (rtmi_path_roulette): no roulette at steps below ``first_step``, and ``p_min`` in
    (0, 1], the floor of the survival probability.  A small holder: after a call it carries ``throughput`` (N, 3) float32,
    each path's forward product of the attenuation layers as the rule left them, and ``counts`` (2,) int64 on the device:
    roulettes played, paths killed.  ``reset()`` forgets both, for the next loop."""

    def __init__(self, first_step=3, p_min=0.05):
        first_step, p_min = int(first_step), float(p_min)
        if not 0 <= first_step < 1 << 32:
            raise RtmiError("first_step must be in [0, 2^32)")
        if not 0.0 < p_min <= 1.0:
            raise RtmiError("p_min must be in (0, 1]")
        self.first_step, self.p_min = first_step, p_min
        self.throughput = self.counts = None

    def reset(self):
        self.throughput = self.counts = None
        return self


def path_roulette(step, result, states, roulette, paths=None):
    """Russian roulette after step number ``step`` of a loop (rtmi_path_roulette), enqueued on torch's current stream.

    ``result``: the ``Bounce`` of that step, made with ``steps`` and the layer tensor ``attenuation`` of the fold's stack;
    ``states``: the paths' own (6, N) int32 RNG states, advanced by one draw per roulette played; ``roulette``: the loop's
    ``Roulette``, whose ``throughput`` (ones at a loop's start) and ``counts`` are made here when None and updated;
    ``paths``: the candidates, a ``Paths`` with distinct entries (None: the step's own, ``result.paths``, or all N).  A
    survivor's ``result.attenuation`` is divided by its survival probability; a killed path gets a zero attenuation and a
    zero direction, and is an ended path for the compaction, the later steps and both folds.  In a loop with direct
    sampling call it after that step's ``direct_sample``.  Returns ``roulette``."""
    torch = _torch()
    if not isinstance(result, Bounce) or result.steps is None:
        raise RtmiError("result must be the Bounce of a step made with steps")
    if not isinstance(roulette, Roulette):
        raise RtmiError("roulette must be an rtmi.wavefront.Roulette")
    d = result.directions
    _lead(d, "result.directions", "rtmi_path_roulette", 2, "(N, 3)", True)
    n, dev = int(d.shape[0]), d.device
    step = int(step)
    if not 0 <= step < MAX_DEPTH:
        raise RtmiError("step %d outside [0, %d)" % (step, MAX_DEPTH))
    idx, n_list, cnt = _list_args(result.paths if paths is None else paths, n, dev)
    _need(states, "states", (STATE_WORDS, n), dev, torch.int32, words="(6, N)")
    _need(result.attenuation, "result.attenuation", (n, 3), dev, torch.float32, words="(N, 3)")
    _need(result.steps, "result.steps", (n,), dev, torch.int32, words="(N,)")
    if roulette.throughput is None:
        roulette.throughput = torch.ones((n, 3), dtype=torch.float32, device=dev)
    if roulette.counts is None:
        roulette.counts = torch.zeros((2,), dtype=torch.int64, device=dev)
    _need(roulette.throughput, "roulette.throughput", (n, 3), dev, torch.float32, words="(N, 3)")
    _need(roulette.counts, "roulette.counts", (2,), dev, torch.int64, words="(2,)")
    a = PathRouletteArgs()
    a.size, a.reserved, a.reserved2, a.n, a.n_list = C.sizeof(PathRouletteArgs), 0, 0, n, n_list
    a.step, a.first_step, a.p_min = step, roulette.first_step, roulette.p_min
    a.d_list, a.d_count, a.d_steps, a.d_dirs = _addr(idx), _addr(cnt), _addr(result.steps), _addr(d)
    a.d_attenuation, a.d_states = _addr(result.attenuation), _addr(states)
    a.d_throughput, a.d_counts = _addr(roulette.throughput), _addr(roulette.counts)
    with torch.cuda.device(dev):
        _check(lib().rtmi_path_roulette(C.byref(a), _stream(dev)), "rtmi_path_roulette")
    return roulette


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
        _complete(self.work[0], "rtmi_bounce")
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
            _complete(w[0], "rtmi_bounce", " in step %d" % k)
        return self


def path_fold(directions, steps, emitted_stack, attenuation_stack, out=None):
    """Trace's return expression over the layers the steps wrote (rtmi_path_fold), enqueued on torch's current stream.

    ``directions`` (N, 3) float32: the paths' directions after the last step (a zero vector: the path ended); ``steps``
    (N,) int32; ``emitted_stack`` / ``attenuation_stack``: contiguous (layers, N, 3) float32, layer k what step k wrote,
    1 <= layers <= 64.  All CUDA tensors on one device.  ``out``: an optional (N, 3) float32 tensor to write into.  Returns
    the radiance."""
    return _fold("rtmi_path_fold", directions, steps, out, emitted_stack=emitted_stack, attenuation_stack=attenuation_stack)


def path_fold_direct(directions, steps, emitted_stack, attenuation_stack, direct_stack, occluded_stack, out=None):
    """``path_fold`` with the direct light of every layer added where its shadow ray was clear (rtmi_path_fold_direct):
    wherever that fold reads E[k] this one reads ``occluded[k] ? E[k] : E[k] + D[k]``.  ``direct_stack``: contiguous
    (layers, N, 3) float32, layer k what ``SceneBuilder.direct_sample`` wrote after step k; ``occluded_stack``: contiguous
    (layers, N) uint8 or bool, what ``SceneBuilder.occluded`` answered for layer k's shadow rays.  The rest as ``path_fold``."""
    return _fold("rtmi_path_fold_direct", directions, steps, out, (occluded_stack,), emitted_stack=emitted_stack,
                 attenuation_stack=attenuation_stack, direct_stack=direct_stack)


def _fold(entry, directions, steps, out, occluded=(), **stacks):
    """The body of both folds: ``stacks``, the (layers, N, 3) stacks by name in the entry's order, ``emitted_stack`` first;
    ``occluded``: the (layers, N) stack behind them, if the entry takes one."""
    torch = _lead(directions, "directions", entry, 2, "(N, 3)", True)
    n, dev, where = int(directions.shape[0]), directions.device, "the directions'"
    _need(steps, "steps", (n,), dev, torch.int32, words="(N,)", where=where)
    first = stacks["emitted_stack"]
    if not (isinstance(first, torch.Tensor) and first.dim() == 3 and 1 <= first.shape[0] <= MAX_DEPTH):
        raise RtmiError("emitted_stack must have shape (layers, N, 3) with 1 <= layers <= %d" % MAX_DEPTH)
    layers = int(first.shape[0])
    for name, t in stacks.items():
        _need(t, name, (layers, n, 3), dev, torch.float32, words="(layers, N, 3)", where=where)
    for t in occluded:
        _need(t, "occluded_stack", (layers, n), dev, torch.uint8, torch.bool, words="(layers, N)", where=where)
    out = _out_buffer(out, "(N, 3)", (n, 3), dev, torch.float32)
    with torch.cuda.device(dev):
        _check(getattr(lib(), entry)(n, layers, *_ptrs(directions, steps, *stacks.values(), *occluded, out), _stream(dev)), entry)
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
    if paths is None:
        return None, n, None
    torch = _torch()
    if not isinstance(paths, Paths):
        raise RtmiError("%s must be an rtmi.Paths or None" % what)
    idx, cnt = paths.index, paths.count
    if not (isinstance(idx, torch.Tensor) and idx.is_cuda and idx.dtype == torch.int32 and idx.dim() == 1 and
            idx.is_contiguous() and idx.device == dev):
        raise RtmiError("%s.index must be a contiguous CUDA int32 tensor of shape (capacity,) on the rays' device" % what)
    _need(cnt, "%s.count" % what, (1,), dev, torch.int32, optional=True)
    if int(idx.shape[0]) > 0x7fffffff:
        raise RtmiError("%s.index holds more than 2^31 - 1 entries" % what)
    return idx, int(idx.shape[0]), cnt


def _new_paths(dev, n):
    """An unfilled ``Paths`` with room for n entries and a count tensor."""
    torch = _torch()
    return Paths(torch.empty((n,), dtype=torch.int32, device=dev), torch.empty((1,), dtype=torch.int32, device=dev))


def _path_compact(n, origins, directions, idx, n_list, cnt, out, dev):
    """rtmi_path_compact on checked arguments, with a scratch of its own, on torch's current stream."""
    torch = _torch()
    words = lib().rtmi_path_compact_scratch_bytes(n_list) // 4
    scratch = torch.empty((max(words, 1),), dtype=torch.int32, device=dev)  # (once per step of a loop: no helper between)
    with torch.cuda.device(dev):
        p_o, p_d, p_idx, p_cnt, *p_out = _ptrs(origins, directions, idx, cnt, out.index, out.count, scratch)
        _check(lib().rtmi_path_compact(n, p_o, p_d, p_idx, n_list, p_cnt, *p_out, _stream(dev)), "rtmi_path_compact")
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
    n, dev, _ = _check_batch("rtmi_path_compact", origins, directions)
    idx, n_list, cnt = _list_args(paths, n, dev)
    if out is None:
        out = _new_paths(dev, n_list)
    else:
        o_idx, o_cap, o_cnt = _list_args(out, n, dev, "out")
        if o_idx is None or o_cnt is None or o_cap < n_list:
            raise RtmiError("out must be an rtmi.Paths with a count tensor and room for every candidate (%d)" % n_list)
        if (idx is not None and o_idx.data_ptr() == idx.data_ptr() and n_list > 0) or \
                (cnt is not None and o_cnt.data_ptr() == cnt.data_ptr()):
            raise RtmiError("out must not be paths: rtmi_path_compact reads one list while it writes the other")
    return _path_compact(n, origins.contiguous(), directions.contiguous(), idx, n_list, cnt, out, dev)


def rng_states(seed, n, first=0, device=None):
    """(6, n) int32 CUDA tensor of RNG states: curand_init(seed, first + i, 0) for ray i (rtmi_rng_init_n), in the
    layout ``SceneBuilder.trace`` reads.  ``device``: a CUDA device (default: torch's current one)."""
    torch = _torch()
    n, first = int(n), int(first)
    if n < 0 or first < 0 or first + n > 1 << 40:
        raise RtmiError("rng_states: n and first must be >= 0 with first + n <= 2^40")
    dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
    if dev.type != "cuda":
        raise RtmiError("rng_states: the states live on a GPU (device %s)" % dev)
    out = _new(dev, (STATE_WORDS, n), torch.int32)
    with torch.cuda.device(dev):
        _check(lib().rtmi_rng_init_n(C.c_uint64(int(seed) & (2**64 - 1)), C.c_uint64(first), n, _ptr(out), _stream(dev)),
               "rtmi_rng_init_n")
    return out
