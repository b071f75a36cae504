"""Russian roulette on the host side: the rule by hand, the bias bound of the draw grid, the forward product held to the
fold it replaces, the nine kernels and both entries in both builds, the refusals that come before any HIP call, and the
binding's surface.  No GPU involved."""
import ctypes as C
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

import bouncelib
import roulettelib as rl
import rtmi
import steerlib
import tracedirectlib
from abi_host import DUMMY, LIBS, QUERY_VARIANTS, ROOT, _count, _refused
from common import code_object_notes, kernel_notes
from parity import bits
from rtmi import _abi, wavefront

f32 = np.float32
NAN = f32("nan")


# ------------------------------------------------------------------ the rule by hand
def _state_with_draw(u):
    """A state whose next CudaRandomFloat(0, 1) is exactly the binary32 u."""
    return steerlib.state_for([steerlib.draw_for_01(f32(u))])


def _one(A, T, u=0.5, steps=3, D=(0, 0, 1), **kw):
    ps = rl.RouletteState([steps], [D], [A], [_state_with_draw(u)], [T], counts=(0, 0))
    before = ps.copy()
    rl.step(ps, kw.pop("step_no", 2), kw.pop("first_step", 0), kw.pop("p_min", 0.05), **kw)
    return before, ps


def test_below_first_step_only_the_throughput_moves():
    before, ps = _one((0.5, 0.25, 0.125), (0.5, 1, 1), first_step=3)
    assert ps.T.tolist() == [[0.25, 0.25, 0.125]]
    assert rl.diff(before, ps) == ["T"]  # no draw, no count, the layer as it was


def test_q_of_one_or_more_is_not_played():
    before, ps = _one((0.5, 1.0, 0.125), (1, 1, 1))  # q == 1: not below 1
    assert ps.T.tolist() == [[0.5, 1.0, 0.125]] and rl.diff(before, ps) == ["T"]
    before, ps = _one((0.5, 0.5, 0.5), (1, 4, 1))
    assert ps.T.tolist() == [[0.5, 2.0, 0.5]] and rl.diff(before, ps) == ["T"]


def test_survive():
    before, ps = _one((0.5, 0.25, 0.125), (0.5, 1, 1), u=0.25)  # t = (0.25, 0.25, 0.125), q = p = 0.25, u == p survives
    assert ps.A.tolist() == [[2.0, 1.0, 0.5]]                    # a * (1 / 0.25)
    assert ps.T.tolist() == [[1.0, 1.0, 0.5]]                    # P * a'
    assert ps.counts.tolist() == [1, 0] and ps.D.tolist() == [[0, 0, 1]]
    want = before.S.copy()
    steerlib.rng_next(want)
    assert np.array_equal(ps.S, want)  # exactly one draw


def test_throughput_is_the_product_with_the_scaled_layer_not_t_times_inv():
    """P * (a * inv) and (P * a) * inv differ in the last place for some operands; the rule is the first."""
    rng = np.random.default_rng(3)
    a, P = rng.uniform(0.1, 0.9, (4000, 3)).astype(f32), rng.uniform(0.1, 0.9, (4000, 3)).astype(f32)
    n = len(a)
    ps = rl.RouletteState(np.full(n, 1), np.tile(f32([0, 1, 0]), (n, 1)), a, steerlib.state_for(np.zeros((n, 1), np.uint64)), P)
    t = (P * a).astype(f32)
    inv = (f32(1) / np.maximum(t.max(1), f32(0.05))).astype(f32)
    rl.step(ps, 0, 0, 0.05)  # the draw is the smallest there is: everyone survives
    a2 = (a * inv[:, None]).astype(f32)
    assert np.array_equal(bits(ps.A), bits(a2)) and np.array_equal(bits(ps.T), bits((P * a2).astype(f32)))
    assert (bits(ps.T) != bits((t * inv[:, None]).astype(f32))).any()


def test_kill():
    u_above = np.nextafter(f32(0.25), f32(1))
    before, ps = _one((0.5, 0.25, 0.125), (0.5, 1, 1), u=u_above)
    for k in ("A", "D", "T"):
        assert not getattr(ps, k).any() and not np.signbit(getattr(ps, k)).any(), k
    assert ps.counts.tolist() == [1, 1]
    want = before.S.copy()
    steerlib.rng_next(want)
    assert np.array_equal(ps.S, want)


def test_q_at_or_below_the_floor_plays_at_the_floor():
    before, ps = _one((0.125, 0.125, 0.125), (0.125, 0.25, 0.125), u=0.0625, p_min=0.0625)  # q = 2^-5 < p_min = 2^-4
    assert ps.A.tolist() == [[2.0, 2.0, 2.0]] and ps.T.tolist() == [[0.25, 0.5, 0.25]] and ps.counts.tolist() == [1, 0]
    before, ps = _one((0.5, 0.5, 0.5), (0.125, 0.125, 0.125), u=0.0625, p_min=0.0625)  # q == p_min: the floor itself
    assert ps.A.tolist() == [[8.0, 8.0, 8.0]] and ps.counts.tolist() == [1, 0]
    before, ps = _one((0, 0, 0), (1, 1, 1), u=np.nextafter(f32(0.0625), f32(1)), p_min=0.0625)  # q = 0, and a draw above the floor
    assert ps.counts.tolist() == [1, 1] and not ps.D.any()


def test_a_nan_channel():
    # q starts as t.x: a NaN there stays (no comparison with it holds) and `q < 1` fails: not played, t is stored
    before, ps = _one((NAN, 0.25, 0.25), (1, 1, 1))
    assert rl.diff(before, ps) == ["T"] and np.isnan(ps.T[0, 0]) and ps.T[0, 1:].tolist() == [0.25, 0.25]
    # a NaN in y or z is never "greater": q is the largest of the others
    before, ps = _one((0.5, NAN, 0.25), (1, 1, 1), u=0.5)
    assert ps.counts.tolist() == [1, 0] and ps.A[0, 0] == 1.0 and np.isnan(ps.A[0, 1]) and ps.A[0, 2] == 0.5
    # a NaN direction is not the zero vector: the path is a candidate like any other
    before, ps = _one((0.5, 0.5, 0.5), (1, 1, 1), u=0.75, D=(NAN, 0, 0))
    assert ps.counts.tolist() == [1, 1] and not ps.D.any()


def test_not_stepped_ended_and_unlisted_paths_keep_every_word():
    S = steerlib.state_for(np.zeros((5, 1), np.uint64))
    ps = rl.RouletteState([2, 3, 3, 3, 3], [[0, 0, 1], [0, 0, 0], [-0.0, 0, -0.0], [0, 1, 0], [0, 1, 0]], np.full((5, 3), 0.5, f32), S,
                          np.full((5, 3), 0.5, f32), counts=(0, 0))
    before = ps.copy()
    rl.step(ps, 2, 0, 0.05, cand=[0, 1, 2, 3, 7, 0xffffffff])  # 0 not stepped; 1, 2 ended; 4 not listed; 7, 2^32 - 1 no paths
    assert ps.counts.tolist() == [1, 0]
    for k in ("steps", "D", "A", "S", "T"):
        got, was = getattr(ps, k), getattr(before, k)
        keep = [0, 1, 2, 4]
        assert np.array_equal(bits(got[keep]) if got.dtype == f32 else got[keep], bits(was[keep]) if was.dtype == f32 else was[keep]), k
    assert ps.A[3].tolist() == [2.0, 2.0, 2.0] and ps.T[3].tolist() == [1.0, 1.0, 1.0]


# ------------------------------------------------------------------ the draw grid
def _count_at_most(p):
    """How many of the 2^32 draw words x have CudaRandomFloat(0, 1)(x) <= p: the draw is monotone in x, so by bisection."""
    p = f32(p)
    u = lambda x: steerlib.rng_01_of(np.array([x], dtype=np.uint64).astype(np.uint32))[0]
    if not u(0) <= p:
        return 0
    lo, hi = 0, 0xffffffff  # u(lo) <= p
    if u(hi) <= p:
        return 1 << 32
    while hi - lo > 1:
        mid = (lo + hi) // 2
        if u(mid) <= p:
            lo = mid
        else:
            hi = mid
    return lo + 1


@pytest.mark.parametrize("p", [2.0 ** -10, 0.05, 0.3, 0.73, 1 - 2.0 ** -24])
def test_the_survival_probability_is_p_to_2_pow_minus_24(p):
    """The bias bound DESIGN.md 2.22 quotes: P(u <= p) is within 2^-24 of the binary32 p, absolutely."""
    p = f32(p)
    count = _count_at_most(p)
    x = np.arange(0, 1 << 32, 65537, dtype=np.uint64).astype(np.uint32)
    assert (np.diff(steerlib.rng_01_of(x)) >= 0).all()  # (monotone on a sample of the grid: the bisection's premise)
    err = abs(count / 2.0 ** 32 - float(p))
    print("p %r: %d words survive, |count / 2^32 - p| = %.3g (2^-24 = %.3g)" % (float(p), count, err, 2.0 ** -24))
    assert err <= 2.0 ** -24


# ------------------------------------------------------------------ the forward product
def _stacks(rng, c, n):
    """n paths of c steps that ended by their own hit: E = 0 and a (compensated, so up to 1 / p_min) attenuation on every
    layer that scattered, an emission and A = 0 on the last."""
    L = max(c, 1)
    E, A = np.zeros((L, n, 3), f32), np.zeros((L, n, 3), f32)
    for k in range(c):
        if k == c - 1:
            E[k] = rng.uniform(0, 8, (n, 3)).astype(f32)
        else:
            A[k] = (rng.uniform(0.05, 1, (n, 3)) * rng.choice([1.0, 1.0, 2.5, 20.0], (n, 1))).astype(f32)
    return np.zeros((n, 3), f32), np.full(n, c, np.int32), E, A


@pytest.mark.parametrize("c", [0, 1, 2, 7, 64])
def test_forward_product_is_the_fold(c):
    """With E = 0 on the scattering layers rtmi_path_fold's value is E[c-1] * A[c-2] * ... * A[0]: the forward product
    multiplies the same factors in the other order.  In binary64 the two agree to 1e-12; each binary32 form makes at most
    c roundings (the fold's additions of a zero are exact), each within 2^-24 relative, so 2 (c + 1) 2^-24 of the value
    bounds either with room."""
    rng = np.random.default_rng(900 + c)
    n = 257
    dirs, steps, E, A = _stacks(rng, c, n)
    ended = np.ones(n, bool)
    fwd64 = rl.forward(ended, steps, E, A, dtype=np.float64)
    bwd64 = tracedirectlib.path_fold64(ended, steps, E, A)  # (rtmi_path_fold's rule in binary64)
    assert (np.abs(fwd64 - bwd64) <= 1e-12 * np.abs(bwd64)).all()
    fwd32, bwd32 = rl.forward(ended, steps, E, A), bouncelib.fold(dirs, steps, E, A)
    tol = 2 * (c + 1) * 2.0 ** -24 * np.abs(bwd64)
    assert (np.abs(fwd32 - fwd64) <= tol).all() and (np.abs(bwd32 - bwd64) <= tol).all()
    if c == 0:
        assert not fwd32.any() and not bwd32.any()
    else:
        assert (fwd64 > 0).all()
    # a killed or cut path is zero whatever its stacks hold
    assert not rl.forward(np.zeros(n, bool), steps, E, A).any()


def test_forward_by_hand():
    E = np.array([[[0, 0, 0]], [[0, 0, 0]], [[2, 4, 8]]], f32)
    A = np.array([[[0.5, 0.25, 1]], [[4, 0.5, 0.5]], [[0, 0, 0]]], f32)
    assert rl.forward([True], [3], E, A).tolist() == [[4.0, 0.5, 4.0]]
    assert rl.forward([True], [1], E, A).tolist() == [[0, 0, 0]]   # E[0] is zero
    assert rl.forward([False], [3], E, A).tolist() == [[0, 0, 0]]
    assert rl.forward([True], [0], E, A).tolist() == [[0, 0, 0]]


# ------------------------------------------------------------------ the symbols
@pytest.mark.parametrize("lib", LIBS)
def test_nine_kernels_and_both_entries_in_both_builds(lib):
    notes = kernel_notes(lib)
    mine = sorted(k for k in notes if "trace_roulette_kernel" in k)
    assert len(mine) == QUERY_VARIANTS, mine
    variants = lambda ks: sorted(int(re.search(r"ILj(\d+)E", k).group(1)) for k in ks)
    trace = [k for k in notes if re.search(r"\d+trace_kernelILj", k)]
    assert variants(mine) == variants(trace)  # kQueryVariants, as rtmi_trace's
    assert len([k for k in notes if "path_roulette_kernel" in k]) == 1
    per_object = code_object_notes(lib)
    names = [k for notes_k in per_object for k in notes_k]
    assert len(names) == len(set(names)), "a kernel name in two code objects"
    syms = subprocess.run(["nm", "-D", "--defined-only", lib], stdout=subprocess.PIPE, text=True, check=True).stdout
    assert re.search(r"\bT rtmi_trace_roulette$", syms, re.M) and re.search(r"\bT rtmi_path_roulette$", syms, re.M)


@pytest.mark.parametrize("lib", LIBS)
def test_kernel_metadata(lib):
    notes = kernel_notes(lib)
    step = [v for k, v in notes.items() if "path_roulette_kernel" in k][0]
    for key in ("group_segment_fixed_size", "private_segment_fixed_size", "vgpr_spill_count", "sgpr_spill_count"):
        assert _count(step, key) == 0, key
    twins = {int(re.search(r"ILj(\d+)E", k).group(1)): v for k, v in notes.items() if re.search(r"\d+trace_kernelILj", k)}
    for k, v in notes.items():
        if "trace_roulette_kernel" in k:
            f = int(re.search(r"ILj(\d+)E", k).group(1))
            assert _count(v, "private_segment_fixed_size") <= _count(twins[f], "private_segment_fixed_size"), (f, k)
            assert _count(v, "group_segment_fixed_size") == 0  # dynamic LDS only, as every trace-loop kernel


def test_entries_are_declared_and_bound_without_a_version_change():
    assert rtmi.lib().rtmi_version() == 3
    header = open(os.path.join(ROOT, "include", "rtmi.h")).read()
    names = [s[0] for s in rtmi.SYMBOLS]
    for entry, struct in (("rtmi_path_roulette", "rtmi_path_roulette_args"), ("rtmi_trace_roulette", "rtmi_trace_roulette_args")):
        assert re.search(r"\b%s\(" % entry, header) and re.search(r"typedef struct %s \{" % struct, header) and entry in names
    assert C.sizeof(_abi.PathRouletteArgs) == 104 and C.sizeof(_abi.TraceRouletteArgs) == 88
    assert [f[0] for f in _abi.PathRouletteArgs._fields_] == ["size", "reserved", "n", "d_list", "n_list", "d_count", "step",
                                                              "first_step", "p_min", "reserved2", "d_steps", "d_dirs",
                                                              "d_attenuation", "d_states", "d_throughput", "d_counts"]
    assert [f[0] for f in _abi.TraceRouletteArgs._fields_] == ["size", "reserved", "n", "d_origins", "d_dirs", "max_depth",
                                                               "first_step", "p_min", "d_states", "d_radiance", "d_ray_counts",
                                                               "d_counts", "d_work"]
    # the header's structures, field by field, in the binding's order
    for struct, cls in (("rtmi_path_roulette_args", _abi.PathRouletteArgs), ("rtmi_trace_roulette_args", _abi.TraceRouletteArgs)):
        body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (struct, struct), header, re.S).group(1)
        body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
        fields = []
        for decl in (d.strip() for d in body.split(";")):
            if decl:  # "type name" or "type *a, *b": the last word of the first part, then the other parts
                parts = decl.split(",")
                fields += [parts[0].split()[-1].lstrip("*")] + [w.strip().lstrip("*") for w in parts[1:]]
        assert fields == [f[0] for f in cls._fields_], (struct, fields)


# ------------------------------------------------------------------ the refusals
STEP_ARRAYS = ("d_steps", "d_dirs", "d_attenuation", "d_states", "d_throughput")
TRACE_ARRAYS = ("d_origins", "d_dirs", "d_states", "d_radiance", "d_work")


def _step_args(n, **kw):
    a = _abi.PathRouletteArgs()
    a.size, a.n, a.n_list, a.step, a.first_step, a.p_min = C.sizeof(_abi.PathRouletteArgs), n, n, 2, 3, 0.05
    for k in STEP_ARRAYS:
        setattr(a, k, DUMMY.value)
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def _step_call(a):
    return rtmi.lib().rtmi_path_roulette(C.byref(a) if a is not None else None, None)


def test_path_roulette_refusals_before_any_hip_call():
    assert _refused(_step_call(None), b"null rtmi_path_roulette_args")
    for size in (0, 8, 96, 112):
        assert _refused(_step_call(_step_args(8, size=size)), b"size")
    assert _refused(_step_call(_step_args(8, reserved=1)), b"reserved")
    assert _refused(_step_call(_step_args(8, reserved2=1)), b"reserved")
    assert _refused(_step_call(_step_args(-1)), b"negative path count")
    assert _refused(_step_call(_step_args(1 << 31)), b"2^31 - 1")
    assert _refused(_step_call(_step_args(8, n_list=-1)), b"negative list length")
    assert _refused(_step_call(_step_args(8, n_list=1 << 31, d_list=DUMMY.value)), b"2^31 - 1")
    assert _refused(_step_call(_step_args(8, n_list=9)), b"n_list must not exceed n")
    for k in STEP_ARRAYS:
        assert _refused(_step_call(_step_args(8, **{k: None})), b"null step, direction"), k
    assert _refused(_step_call(_step_args(8, step=rtmi.MAX_DEPTH)), b"step outside")
    for p_min in (0.0, -0.5, 1.0000001, float("nan"), float("inf")):
        assert _refused(_step_call(_step_args(8, p_min=p_min)), b"p_min"), p_min
    # nothing to do launches nothing and needs no array: no HIP call is made for these either
    assert _step_call(_step_args(0, **{k: None for k in STEP_ARRAYS})) == 0
    assert _step_call(_step_args(8, n_list=0, **{k: None for k in STEP_ARRAYS})) == 0
    assert _step_call(_step_args(8, n_list=0, p_min=1.0)) == 0


def _trace_args(n, **kw):
    a = _abi.TraceRouletteArgs()
    a.size, a.n, a.max_depth, a.first_step, a.p_min = C.sizeof(_abi.TraceRouletteArgs), n, 6, 3, 0.05
    for k in TRACE_ARRAYS:
        setattr(a, k, DUMMY.value)
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def _trace_call(s, a):
    return rtmi.lib().rtmi_trace_roulette(s, C.byref(a) if a is not None else None, None)


def test_trace_roulette_refusals_before_any_hip_call():
    b = rtmi.SceneBuilder(1)  # never committed: the last refusal of all
    assert _refused(_trace_call(None, _trace_args(8)), b"null scene")
    assert _refused(_trace_call(b.h, None), b"null rtmi_trace_roulette_args")
    for size in (0, 8, 80, 96):
        assert _refused(_trace_call(b.h, _trace_args(8, size=size)), b"size")
    assert _refused(_trace_call(b.h, _trace_args(8, reserved=1)), b"reserved")
    for p_min in (0.0, -1.0, 1.5, float("nan")):
        assert _refused(_trace_call(b.h, _trace_args(8, p_min=p_min)), b"p_min"), p_min
    # every case of rtmi_trace
    assert _refused(_trace_call(b.h, _trace_args(-1)), b"negative ray count")
    assert _refused(_trace_call(b.h, _trace_args(1 << 31)), b"2^31 - 1")
    for k in TRACE_ARRAYS:
        assert _refused(_trace_call(b.h, _trace_args(8, **{k: None})), b"null ray, state"), k
    # nothing wrong but the scene: the checks above all came first (the depth is checked behind this one, as rtmi_trace's:
    # tests/test_gpu_roulette.py)
    assert _refused(_trace_call(b.h, _trace_args(8)), b"committed")
    assert _refused(_trace_call(b.h, _trace_args(0, d_origins=None)), b"committed")  # no arrays needed for no rays


# ------------------------------------------------------------------ the binding
def test_binding_surface():
    p = inspect.signature(rtmi.SceneBuilder.trace_steps).parameters
    assert list(p)[:8] == ["self", "origins", "directions", "states", "max_depth", "each", "hits", "compact"]
    assert [p[k].default for k in ("each", "hits", "compact", "direct", "light_states", "shadow")] == [None, None, False, False, None, None]
    # the loop with a roulette: trace_steps' parameters with `roulette` behind max_depth (the package's recorded surface
    # keeps trace_steps' own list as it is: tests/test_binding_surface_host.py)
    q = inspect.signature(rtmi.SceneBuilder.trace_steps_roulette).parameters
    assert list(q) == list(p)[:5] + ["roulette"] + list(p)[5:]
    assert all(q[k].default == p[k].default for k in list(p)[5:])
    sig = inspect.signature(rtmi.SceneBuilder.trace_roulette)
    assert list(sig.parameters) == ["self", "origins", "directions", "states", "max_depth", "first_step", "p_min", "count_rays", "out"]
    assert [sig.parameters[k].default for k in ("first_step", "p_min", "count_rays", "out")] == [3, 0.05, False, None]
    assert "trace_roulette" not in vars(rtmi.SceneBuilder) and "trace_steps_roulette" not in vars(rtmi.SceneBuilder)
    assert issubclass(wavefront.TraceRoulette, rtmi.Trace)
    assert list(inspect.signature(wavefront.path_roulette).parameters) == ["step", "result", "states", "roulette", "paths"]
    assert inspect.signature(wavefront.path_roulette).parameters["paths"].default is None
    assert list(inspect.signature(rtmi.Renderer.render_rays).parameters) == ["self", "budget", "projection", "count_rays", "each",
                                                                             "direct"]
    assert rtmi.Steps._fields == ("rgb", "steps", "alive", "origins", "directions", "emitted", "attenuation", "works", "direct",
                                  "occluded", "flags")


def test_roulette_holder():
    r = wavefront.Roulette()
    assert (r.first_step, r.p_min, r.throughput, r.counts) == (3, 0.05, None, None)
    assert wavefront.Roulette(0, 1.0).p_min == 1.0
    for bad in (dict(p_min=0.0), dict(p_min=1.5), dict(p_min=float("nan")), dict(first_step=-1)):
        with pytest.raises(rtmi.RtmiError):
            wavefront.Roulette(**bad)
    b = rtmi.SceneBuilder(1)
    with pytest.raises(rtmi.RtmiError):
        b.trace_roulette(None, None, None, 4)
    with pytest.raises(rtmi.RtmiError):
        b.trace_steps_roulette(None, None, None, 4, roulette=None)
    with pytest.raises(rtmi.RtmiError):
        wavefront.path_roulette(0, None, None, r)
