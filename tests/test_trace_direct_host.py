"""rtmi_trace_direct on the host side: the forward sum restated and held to the backward fold it replaces, the sixteen
kernels and the entry in both builds, the refusals that come before any HIP call, and the binding's surface.  No GPU
involved."""
import ctypes as C
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

import directlib as dl
import rtmi
import tracedirectlib as tdl
from abi_host import DUMMY, LIBS, QUERY_VARIANTS, ROOT, _refused
from common import kernel_notes
from parity import bits
from rtmi import _abi, wavefront

f32 = np.float32
ARRAYS = ("d_origins", "d_dirs", "d_states", "d_radiance", "d_work")
LAYERS = [0, 1, 2, 7, 64]


# ------------------------------------------------------------------ the forward sum
@pytest.mark.parametrize("alive", [False, True])
@pytest.mark.parametrize("c", LAYERS)
def test_forward_and_backward_folds_are_one_estimator(c, alive):
    """In binary64 r_path + acc and rtmi_path_fold_direct's rule agree to 1e-12 of the sum of the absolute terms: the same
    terms, summed in another order.  The binary32 forms (tracedirectlib.forward_direct on bouncelib.fold, and
    directlib.fold_direct) each stay within their own rounding of that value: at most 2 c + 2 operations on a term, every
    partial result non-negative and below the sum of the terms, so 4 (c + 1) 2^-24 of it bounds either."""
    rng = np.random.default_rng(1000 * c + alive)
    dirs, steps, E, A, D, occ = tdl.random_stacks(rng, c, 257, alive)
    ended = ~dirs.any(axis=1)
    fwd, mag = tdl.forward64(ended, steps, E, A, D, occ)
    bwd = tdl.backward64(ended, steps, E, A, D, occ)
    assert (np.abs(fwd - bwd) <= 1e-12 * mag).all(), np.abs(fwd - bwd).max()
    if c == 0:
        assert not fwd.any() and not bwd.any()
    import bouncelib
    fwd32 = (bouncelib.fold(dirs, steps, E, A) + tdl.forward_direct(A, D, occ, steps)).astype(f32)
    bwd32 = dl.fold_direct(dirs, steps, E, A, D, occ)
    tol = 4 * (c + 1) * 2.0 ** -24 * mag
    assert (np.abs(fwd32 - fwd) <= tol).all() and (np.abs(bwd32 - bwd) <= tol).all()
    assert c == 0 or (mag > 0).any(axis=1).sum() > 64  # (the bounds above are not vacuous)


@pytest.mark.parametrize("c", LAYERS)
def test_skipping_zero_layers_changes_no_bit(c):
    rng = np.random.default_rng(77 + c)
    dirs, steps, E, A, D, occ = tdl.random_stacks(rng, c, 257, True)
    if c:
        D[rng.integers(0, c, 40), rng.integers(0, 257, 40)] = f32(-0.0)  # both zeros among the layers
        D[rng.integers(0, c, 40), rng.integers(0, 257, 40)] = f32(0.0)
    assert np.array_equal(bits(tdl.forward_direct(A, D, occ, steps)), bits(tdl.forward_direct_skipping(A, D, occ, steps)))
    assert not np.signbit(tdl.forward_direct(A, D, occ, steps)).any()  # acc began at +0.0f and never becomes -0.0f


def test_forward_sum_by_hand():
    A = np.array([[[0.5, 0.25, 1]], [[0.5, 0.5, 0.5]], [[0, 0, 0]]], f32)
    D = np.array([[[2, 4, 8]], [[1, 1, 1]], [[9, 9, 9]]], f32)
    occ = np.array([[0], [0], [0]], np.uint8)
    assert tdl.forward_direct(A, D, occ, [3]).tolist() == [[2 + 0.5 + 0.25 * 9, 4 + 0.25 + 0.125 * 9, 8 + 1 + 0.5 * 9]]
    assert tdl.forward_direct(A, D, occ, [2]).tolist() == [[2.5, 4.25, 9]]
    assert tdl.forward_direct(A, D, np.array([[0], [1], [0]]), [3]).tolist() == [[2 + 2.25, 4 + 1.125, 8 + 4.5]]
    assert tdl.forward_direct(A, D, occ, [0]).tolist() == [[0, 0, 0]]


# ------------------------------------------------------------------ the symbols
@pytest.mark.parametrize("lib", LIBS)
def test_sixteen_kernels_and_the_entry_in_both_builds(lib):
    notes = kernel_notes(lib)
    mine = sorted(k for k in notes if "trace_direct_kernel" in k)
    assert len(mine) == 2 * QUERY_VARIANTS, mine
    flat = [k for k in mine if re.search(r"trace_direct_kernelILj\d+ELb0EE", k)]
    sph = [k for k in mine if re.search(r"trace_direct_kernelILj\d+ELb1EE", k)]
    assert len(flat) == QUERY_VARIANTS and len(sph) == QUERY_VARIANTS
    variants = lambda ks: sorted(int(re.search(r"ILj(\d+)E", k).group(1)) for k in ks)
    trace = [k for k in notes if re.search(r"\d+trace_kernelILj", k)]
    assert variants(flat) == variants(sph) == variants(trace)  # kQueryVariants, as rtmi_trace's
    syms = subprocess.run(["nm", "-D", "--defined-only", lib], stdout=subprocess.PIPE, text=True, check=True).stdout
    assert re.search(r"\bT rtmi_trace_direct$", syms, re.M) and re.search(r"\bT rtmi_trace$", syms, re.M)


def test_entry_is_declared_and_bound_without_a_version_change():
    assert rtmi.lib().rtmi_version() == 3
    header = open(os.path.join(ROOT, "include", "rtmi.h")).read()
    assert re.search(r"\brtmi_trace_direct\(", header) and re.search(r"typedef struct rtmi_trace_direct_args \{", header)
    assert "rtmi_trace_direct" in [s[0] for s in rtmi.SYMBOLS]
    assert C.sizeof(_abi.TraceDirectArgs) == 88
    assert [f[0] for f in _abi.TraceDirectArgs._fields_] == ["size", "reserved", "n", "d_origins", "d_dirs", "max_depth", "d_states",
                                                             "d_light_states", "d_radiance", "d_ray_counts", "d_counts", "d_work"]


# ------------------------------------------------------------------ the refusals
def _args(n, **kw):
    a = _abi.TraceDirectArgs()
    a.size, a.reserved, a.n, a.max_depth = C.sizeof(_abi.TraceDirectArgs), 0, n, 6
    for k in ARRAYS:
        setattr(a, k, DUMMY.value)
    a.d_light_states = DUMMY.value + 4096
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def _call(s, a):
    return rtmi.lib().rtmi_trace_direct(s, C.byref(a) if a is not None else None, None)


def test_argument_checks_before_any_hip_call():
    b = rtmi.SceneBuilder(1)  # never committed: the last refusal of all
    assert _refused(_call(None, _args(8)), b"null scene")
    assert _refused(_call(b.h, None), b"null rtmi_trace_direct_args")
    for size in (0, 8, 80, 96):
        assert _refused(_call(b.h, _args(8, size=size)), b"size")
    assert _refused(_call(b.h, _args(8, reserved=1)), b"reserved")
    # its own cases: the light states
    assert _refused(_call(b.h, _args(8, d_light_states=None)), b"light state")
    assert _refused(_call(b.h, _args(8, d_light_states=DUMMY.value)), b"must not be d_states")
    # every case of rtmi_trace
    assert _refused(_call(b.h, _args(-1)), b"negative ray count")
    assert _refused(_call(b.h, _args(1 << 31)), b"2^31 - 1")
    for k in ARRAYS:
        assert _refused(_call(b.h, _args(8, **{k: None})), b"null ray, state"), k
    # nothing wrong but the scene: the checks above all came first (the depth is checked behind this one, as rtmi_trace's:
    # tests/test_gpu_trace_direct.py)
    assert _refused(_call(b.h, _args(8)), b"committed")
    assert _refused(_call(b.h, _args(0, d_light_states=None, d_origins=None)), b"committed")  # no arrays needed for no rays


# ------------------------------------------------------------------ the binding
def test_binding_surface():
    sig = inspect.signature(rtmi.SceneBuilder.trace_direct)
    assert list(sig.parameters) == ["self", "origins", "directions", "states", "light_states", "max_depth", "count_rays", "out"]
    assert sig.parameters["count_rays"].default is False and sig.parameters["out"].default is None
    assert "trace_direct" not in vars(rtmi.SceneBuilder)  # from a private base, as light_kinds
    assert issubclass(wavefront.TraceDirect, rtmi.Trace) and not hasattr(rtmi, "TraceDirect") and not hasattr(rtmi, "TraceDirectArgs")
    assert inspect.signature(rtmi.Renderer.render_rays).parameters["direct"].default is False
    assert list(inspect.signature(rtmi.Renderer.render_rays).parameters) == ["self", "budget", "projection", "count_rays", "each",
                                                                             "direct"]
    src = inspect.getsource(rtmi.Renderer.render_rays)
    assert '"fused"' in src


def test_trace_direct_checks_its_tensors_before_the_library():
    b = rtmi.SceneBuilder(1)
    with pytest.raises(rtmi.RtmiError):
        b.trace_direct(None, None, None, None, 4)
