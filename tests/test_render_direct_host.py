"""rtmi_render_direct on the host side: the binding's surface held to the header, the thirty-two kernels and the entry in
both builds, the refusals that come before any HIP call, the binding's check of its budget, and the header's sample
rule restated in binary32 and held to rtmi_trace_direct's radiance followed by rtmi_sample_add's fold.  No GPU involved."""
import ctypes as C
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

import bouncelib
import budgetlib
import renderdirectlib as rdl
import rtmi
import tracedirectlib as tdl
from abi_host import DUMMY, ERR_DEPTH, LIBS, QUERY_VARIANTS, F_DEFOCUS, ROOT, _frame, _refused
from common import kernel_notes
from parity import bits
from rtmi import _abi

f32 = np.float32
FIELDS = ["size", "reserved", "d_budget", "d_states", "d_light_states", "d_sum", "d_sq", "d_samples", "d_ray_counts", "features",
          "d_counts", "d_work"]
ARRAYS = ("d_budget", "d_states", "d_sum", "d_samples", "d_work")


# ------------------------------------------------------------------ the surface
def test_entry_is_declared_and_bound_without_a_version_change():
    assert rtmi.lib().rtmi_version() == 3
    header = open(os.path.join(ROOT, "include", "rtmi.h")).read()
    assert re.search(r"^int rtmi_render_direct\(const rtmi_scene \*s, const rtmi_frame \*f, const rtmi_render_direct_args \*args, "
                     r"void \*stream\);", header, re.M)
    body = re.search(r"typedef struct rtmi_render_direct_args \{(.*?)\} rtmi_render_direct_args;", header, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    assert [re.search(r"(\w+)\s*$", d).group(1) for d in body.split(";") if d.strip()] == FIELDS  # the header's order
    assert [f[0] for f in _abi.RenderDirectArgs._fields_] == FIELDS
    assert C.sizeof(_abi.RenderDirectArgs) == 88
    assert _abi.RenderDirectArgs.features.offset == 64 and _abi.RenderDirectArgs.d_work.offset == 80
    sym = [s for s in rtmi.SYMBOLS if s[0] == "rtmi_render_direct"]
    assert len(sym) == 1 and sym[0][1] is C.c_int and len(sym[0][2]) == 4
    assert hasattr(rtmi.lib(), "rtmi_render_direct")
    assert re.search(r"#define RTMI_BUDGET_WORK_WORDS RTMI_TRACE_WORK_WORDS", header) and rtmi.BUDGET_WORK_WORDS == 256


@pytest.mark.parametrize("lib", LIBS)
def test_thirty_two_kernels_and_the_entry_in_both_builds(lib):
    notes = kernel_notes(lib)
    variants = lambda ks: sorted(int(re.search(r"ILj(\d+)E", k).group(1)) for k in ks)
    plain = variants(k for k in notes if re.search(r"\d+budget_kernelILj", k))
    assert len(plain) == QUERY_VARIANTS and all(v & F_DEFOCUS for v in plain)
    for kernel in ("budget_direct_kernel", "feature_direct_kernel"):
        for twin in (0, 1):
            mine = [k for k in notes if re.search(r"\d+%sILj\d+ELb%dEE" % (kernel, twin), k)]
            assert variants(mine) == plain, (kernel, twin, mine)  # the budget mode's variants, a flat and a sphere twin each
            for k in mine:  # the bodies address LDS by offsets of the dynamic array: no static LDS
                assert int(re.search(r"\.group_segment_fixed_size:\s+(\d+)", notes[k]).group(1)) == 0, k
    assert sum("params_write_kernel" in k and "RenderDirectParams" in k for k in notes) == 1  # a block type, and a writer, of its own
    syms = subprocess.run(["nm", "-D", "--defined-only", lib], stdout=subprocess.PIPE, text=True, check=True).stdout
    assert re.search(r"\bT rtmi_render_direct$", syms, re.M) and re.search(r"\bT rtmi_render_budget$", syms, re.M)


def test_binding_surface():
    """The two methods come from a private base, as SceneBuilder.trace_direct does: the pinned signatures of
    render_budget and render_adaptive (tests/test_binding_surface_host.py) stay what they were."""
    assert "render_direct" not in vars(rtmi.Renderer) and "render_adaptive_direct" not in vars(rtmi.Renderer)
    sig = inspect.signature(rtmi.Renderer.render_direct)
    assert list(sig.parameters) == ["self", "budget", "count_rays", "features"]
    assert sig.parameters["count_rays"].default is True and sig.parameters["features"].default is False
    assert str(sig) == str(inspect.signature(rtmi.Renderer.render_budget))  # render_budget's arguments, one for one
    assert str(inspect.signature(rtmi.Renderer.render_adaptive_direct)) == str(inspect.signature(rtmi.Renderer.render_adaptive))
    assert not hasattr(rtmi, "RenderDirectArgs")  # the structure stays in rtmi._abi, as TraceDirectArgs does
    src = inspect.getsource(rtmi.Renderer._light_states)
    assert "first=self.items" in src and "self.scene.seed" in src  # render_rays' own seeding: the two ways interleave
    assert "_light_states()" in inspect.getsource(rtmi.Renderer.render_rays)


def test_python_checks_its_budget_before_the_library():
    class Stub(rtmi.Renderer):  # no device: only what render_direct looks at before the library
        def __init__(self):
            import torch
            self.torch, self.items, self.device = torch, 4, torch.device("cpu")
    with pytest.raises(rtmi.RtmiError):
        Stub().render_direct(None)


# ------------------------------------------------------------------ the refusals before any HIP call
def _args(**kw):
    a = _abi.RenderDirectArgs()
    a.size, a.reserved = C.sizeof(_abi.RenderDirectArgs), 0
    for k in ARRAYS:
        setattr(a, k, DUMMY.value)
    a.d_light_states = DUMMY.value + 4096
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def _call(s, f, a):
    return rtmi.lib().rtmi_render_direct(s, C.byref(f) if f is not None else None, C.byref(a) if a is not None else None, None)


def test_argument_checks_before_any_hip_call():
    b = rtmi.SceneBuilder(1)  # never committed: the last refusal of these
    f = _frame()
    assert _refused(_call(None, f, _args()), b"null scene")
    assert _refused(_call(b.h, f, None), b"null rtmi_render_direct_args")
    for size in (0, 8, 80, 96):
        assert _refused(_call(b.h, f, _args(size=size)), b"size")
    assert _refused(_call(b.h, f, _args(reserved=1)), b"reserved")
    # its own cases: the light states
    assert _refused(_call(b.h, f, _args(d_light_states=None)), b"light state")
    assert _refused(_call(b.h, f, _args(d_light_states=DUMMY.value)), b"must not be d_states")
    # every case of rtmi_render_budget and rtmi_render_features that needs no committed scene
    assert _refused(_call(b.h, None, _args()), b"frame")
    assert _refused(_call(b.h, _frame(width=0), _args()), b"frame")
    assert _refused(_call(b.h, _frame(rank=1, world=1), _args()), b"frame")
    for k in ARRAYS:
        assert _refused(_call(b.h, f, _args(**{k: None})), b"null budget, state"), k
    feat = _abi.feature_bufs()
    feat.d_albedo = DUMMY.value
    feat.size = 8
    assert _refused(_call(b.h, f, _args(features=C.pointer(feat))), b"rtmi_features.size")
    feat.size, feat.reserved = C.sizeof(_abi.Features), 1
    assert _refused(_call(b.h, f, _args(features=C.pointer(feat))), b"rtmi_features.size")
    feat.reserved = 0
    assert _refused(_call(b.h, _frame(max_depth=0), _args(features=C.pointer(feat))), b"at least 1", ERR_DEPTH)
    # nothing wrong but the scene: the checks above all came first (depth, post_process and the device are checked behind
    # this one, as rtmi_render_budget's: tests/test_gpu_render_direct.py)
    assert _refused(_call(b.h, f, _args()), b"committed")
    assert _refused(_call(b.h, f, _args(d_sq=None, d_ray_counts=None, d_counts=None, features=None)), b"committed")


# ------------------------------------------------------------------ the sample rule
class _Host:
    """A host array where tracedirectlib.expected_radiance expects a device tensor."""

    def __init__(self, a):
        self.a = np.asarray(a)

    def cpu(self):
        return self

    def numpy(self):
        return self.a


class _Stacks:
    def __init__(self, dirs, steps, E, A, D, occ):
        self.directions, self.steps, self.emitted, self.attenuation = _Host(dirs), _Host(steps), _Host(E), _Host(A)
        self.direct, self.occluded = _Host(D), _Host(occ)


@pytest.mark.parametrize("alive", [False, True])
@pytest.mark.parametrize("c", [0, 1, 2, 7, 64])
def test_sample_rule_is_trace_direct_then_sample_add(c, alive, monkeypatch):
    """K samples of n items, each sample a recorded set of stacks.  The header's rule -- x = r_path + acc, then sum += x,
    sq += x * x -- against tracedirectlib.expected_radiance (what rtmi_trace_direct writes for the sample) folded by
    budgetlib.moments (rtmi_sample_add's rule): the order of roundings the kernel must follow, pinned in one place."""
    monkeypatch.setattr(rtmi, "path_fold", lambda d, s, E, A: _Host(bouncelib.fold(d.numpy(), s.numpy(), E.numpy(), A.numpy())),
                        raising=False)
    rng = np.random.default_rng(31 * c + alive)
    K, n = 5, 33
    samples = [tdl.random_stacks(rng, c, n, alive) for _ in range(K)]
    want_x = np.stack([tdl.expected_radiance(_Stacks(*s)) for s in samples])  # (K, n, 3)
    r_path = np.stack([bouncelib.fold(s[0], s[1], s[2], s[3]) for s in samples])
    acc = np.stack([tdl.forward_direct(s[3], s[4], s[5], s[1]) for s in samples])
    assert want_x.dtype == f32 and r_path.dtype == f32 and acc.dtype == f32
    for i in range(n):
        s, q, xs = rdl.fold_samples(r_path[:, i], acc[:, i])
        assert np.array_equal(bits(xs), bits(want_x[:, i]))
        for ch in range(3):
            k, S, Q = budgetlib.moments(want_x[:, i, ch])
            assert k == K and bits(S[0]) == bits(s[ch]) and bits(Q[0]) == bits(q[ch]), (i, ch)
    if c > 1:
        assert (acc != 0).any() and (alive or (r_path != 0).any())  # (the stacks are not all dark)


def test_sample_rule_by_hand():
    # one item, two samples: x0 = 1 + 2^-24 rounds to 1 (one addition), x1 = 0.5 + 0.25
    r_path = np.array([[1, 1, 1], [0.5, 0.5, 0.5]], f32)
    acc = np.array([[2.0 ** -24] * 3, [0.25] * 3], f32)
    s, q, xs = rdl.fold_samples(r_path, acc)
    assert xs.tolist() == [[1, 1, 1], [0.75, 0.75, 0.75]]
    assert s.tolist() == [1.75] * 3 and q.tolist() == [1 + 0.5625] * 3
    # carried on from what the buffers hold
    s2, q2, _ = rdl.fold_samples(r_path[:1], acc[:1], s0=s, q0=q)
    assert s2.tolist() == [2.75] * 3 and q2.tolist() == [2.5625] * 3
    # a sample's -0.0f joins the sum as +0.0f: r_path + acc with acc = +0.0f
    s3, _, xs3 = rdl.fold_samples(np.array([[-0.0] * 3], f32), np.zeros((1, 3), f32))
    assert not np.signbit(xs3).any() and not np.signbit(s3).any()
