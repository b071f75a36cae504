"""rtmi_render_budget / rtmi_budget_plan / rtmi_resolve on the host side: the exported symbols, the argument checks that
come before any HIP call, the budget kernels in both builds of the library, and the stopping rule restated in numpy
(tests/budgetlib.py: ``plan_rule``, which tests/test_gpu_budget.py holds the device against).  No GPU involved.

The refusals that need a COMMITTED scene (max_depth, post_process, spp x depth) cannot be reached without a device,
because committing a scene uploads it: tests/test_gpu_budget.py::test_budget_argument_checks_on_a_committed_scene."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import common
import rtmi
from abi_host import DUMMY, F_DEFOCUS, LIBS, QUERY_VARIANTS, _frame, _refused
from budgetlib import moments, plan_rule

ENTRIES = ("rtmi_render_budget", "rtmi_budget_plan", "rtmi_resolve")
F32 = np.float32


def test_stopping_rule_on_hand_worked_cases():
    """min 4, max 64, step 4 unless said otherwise.  Every figure below is exact in binary32, worked by hand:
    constant 0.5 x 4: S = 2, Q = 1, nf Q - S S = 0, lhs = 0 <= rhs: converged at min_samples;
    {0, 0, 0, 8}: S = 8, Q = 64, (256 - 64) / 3 = 64 > 0.0625 x (64 + 16 x 0.0001): not converged;
    {1, 1, 1, 2}: S = 5, Q = 7, (28 - 25) / 3 = 1; T = 0.25, F = 0: rhs = 1.5625, converged; T = 0.125: rhs = 0.390625, not;
    black with F = 0: 0 <= 0, converged; a NaN sum: not converged."""
    rule = lambda case, tol=0.25, floor=0.01, mn=4, mx=64, step=4: int(
        plan_rule([case[0]], [case[1]], [case[2]], mn, mx, step, tol, floor)[0])
    assert moments([0.5] * 4) == (4, [F32(2)] * 3, [F32(1)] * 3)
    assert rule(moments([0.5] * 4)) == 0
    assert moments([0, 0, 0, 8])[1:] == ([F32(8)] * 3, [F32(64)] * 3)
    assert rule(moments([0, 0, 0, 8])) == 4
    assert rule(moments([1, 1, 1, 2]), tol=0.25, floor=0.0) == 0
    assert rule(moments([1, 1, 1, 2]), tol=0.125, floor=0.0) == 4
    assert rule(moments([0] * 4), floor=0.0) == 0
    assert rule((4, [np.nan, 2, 2], [1, 1, 1])) == 4
    assert rule((4, [2, 2, 2], [1, np.nan, 1])) == 4
    # one channel out of three that has not converged keeps the pixel going
    assert rule((4, [2, 8, 2], [1, 64, 1])) == 4
    # below min_samples: up to it, whatever the moments; at max_samples: stop, whatever the moments
    assert rule((0, [0] * 3, [0] * 3)) == 4
    assert rule((3, [np.nan] * 3, [0] * 3)) == 1
    assert rule((64,) + moments([0, 0, 0, 8])[1:]) == 0
    assert rule((70,) + moments([0, 0, 0, 8])[1:]) == 0
    # the last step is cut at max_samples
    assert rule((62,) + moments([0, 0, 0, 8])[1:]) == 2
    assert rule(moments([0, 0, 0, 8]), step=100) == 60
    # padding gets nothing
    assert int(plan_rule([0], [[0] * 3], [[0] * 3], 4, 64, 4, 0.25, 0.01, pixel=np.array([False]))[0]) == 0


# ------------------------------------------------------------------ symbols
def test_budget_entries_are_exported_by_both_builds():
    L = rtmi.lib()
    assert L.rtmi_version() == 3  # additive: no version change
    names = [s[0] for s in rtmi.SYMBOLS]
    for e in ENTRIES:
        assert e in names
    assert os.path.exists(LIBS[1]), "librtmi_check1.so missing: __graft_entry__.build() builds it"
    for path in LIBS:
        lib = C.CDLL(path)
        for e in ENTRIES:
            assert hasattr(lib, e), (path, e)
    assert rtmi.BUDGET_WORK_WORDS >= 4
    assert C.sizeof(rtmi.AdaptiveOpts) == 24


def test_render_budget_argument_checks_before_any_hip_call():
    L = rtmi.lib()
    b = rtmi.SceneBuilder(1)
    names = ("budget", "states", "sum", "sq", "samples", "rays", "work")

    def call(s, frame, **null):
        a = {k: (None if k in null else DUMMY) for k in names}
        return L.rtmi_render_budget(s, C.byref(frame) if frame is not None else None, a["budget"], a["states"],
                                    a["sum"], a["sq"], a["samples"], a["rays"], a["work"], None)

    assert _refused(call(None, _frame()), b"scene")
    assert _refused(call(b.h, None), b"frame")
    assert _refused(call(b.h, _frame(height=0)), b"frame")
    assert _refused(call(b.h, _frame(rank=3, world=3)), b"frame")
    assert _refused(call(b.h, _frame(width=70000)), b"65535")
    for k in ("budget", "states", "sum", "samples", "work"):
        assert _refused(call(b.h, _frame(), **{k: True}), b"null"), k
    # the two optional arrays are not what is refused: with them null, the uncommitted scene is
    assert _refused(call(b.h, _frame(), sq=True, rays=True), b"committed")
    assert _refused(call(b.h, _frame()), b"committed")


def test_budget_plan_argument_checks_before_any_hip_call():
    L = rtmi.lib()
    names = ("sum", "sq", "samples", "budget", "totals")

    def call(frame, opts, **null):
        a = {k: (None if k in null else DUMMY) for k in names}
        return L.rtmi_budget_plan(C.byref(frame) if frame is not None else None, C.byref(opts) if opts is not None else None,
                                  a["sum"], a["sq"], a["samples"], a["budget"], a["totals"], None)

    good = lambda **kw: rtmi.adaptive_opts(**dict(dict(min_spp=4, max_spp=64, step=4, tolerance=0.25, floor=0.01), **kw))
    assert _refused(call(None, good()), b"frame")
    assert _refused(call(_frame(width=0), good()), b"frame")
    for k in names:
        assert _refused(call(_frame(), good(), **{k: True}), b"null"), k
    assert _refused(call(_frame(), None), b"null")
    wrong = good()
    wrong.size += 4
    assert _refused(call(_frame(), wrong), b"size")
    for kw in (dict(min_spp=1), dict(min_spp=0), dict(min_spp=8, max_spp=7), dict(step=0), dict(step=-3), dict(tolerance=0.0),
               dict(tolerance=-0.5), dict(tolerance=float("nan")), dict(tolerance=float("inf")), dict(floor=-1.0),
               dict(floor=float("nan"))):
        assert _refused(call(_frame(), good(**kw)), b"out of range"), kw


def test_resolve_argument_checks_before_any_hip_call():
    L = rtmi.lib()
    call = lambda frame, s=DUMMY, n=DUMMY, t=DUMMY: L.rtmi_resolve(C.byref(frame) if frame is not None else None, s, n, 1, t, None)
    assert _refused(call(None), b"frame")
    assert _refused(call(_frame(height=-1)), b"frame")
    assert _refused(call(_frame(), s=None), b"null")
    assert _refused(call(_frame(), n=None), b"null")
    assert _refused(call(_frame(), t=None), b"null")


# ------------------------------------------------------------------ the kernels
def test_budget_kernels_one_per_variant_without_static_lds():
    """The budget kernels address the layer stack at byte offsets of the DYNAMIC LDS array, as every mode of the trace
    loop does: right only while they declare no static LDS (group_segment_fixed_size == 0), in both builds.  Eight
    kernels -- the query variants, each with F_DEFOCUS set -- not sixteen."""
    for lib in LIBS:
        ks = {n: blk for n, blk in common.kernel_notes(lib).items() if "budget_kernel" in n}
        assert len(ks) == QUERY_VARIANTS, (lib, sorted(ks))
        for name, blk in ks.items():
            assert not any(k in name for k in ("render_kernel", "probe_kernel", "trace_kernel", "query_kernel")), name
            assert re.search(r"\.group_segment_fixed_size:\s+0\b", blk), (lib, name)
            feature_set = int(re.search(r"budget_kernelILj(\d+)E", name).group(1))
            assert feature_set & F_DEFOCUS, name
