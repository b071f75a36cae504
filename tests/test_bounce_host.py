"""rtmi_bounce / rtmi_path_fold on the host side: the exports of both builds, the argument checks that come before any
HIP call, the Python binding's refusals, the bounce kernels' metadata, and the numpy fold the GPU tests hold the device
to, itself held to hand-worked cases.  No GPU involved."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import common
import rtmi
from abi_host import DUMMY, ERR_INVALID, LIBS, OK, QUERY_VARIANTS, ROOT, _refused
from bouncelib import fold
from parity import bits


def test_bounce_entries_are_exported_by_both_builds_and_bound():
    L = rtmi.lib()
    assert L.rtmi_version() == 3  # additive: no version change
    names = [s[0] for s in rtmi.SYMBOLS]
    assert "rtmi_bounce" in names and "rtmi_path_fold" in names
    for lib in LIBS:
        syms = subprocess.run(["nm", "-D", "--defined-only", lib], stdout=subprocess.PIPE, text=True, check=True).stdout
        for name in ("rtmi_bounce", "rtmi_path_fold"):
            assert re.search(r"\bT %s$" % name, syms, re.M), (lib, name)
    header = open(os.path.join(ROOT, "include", "rtmi.h")).read()
    assert "int rtmi_bounce(" in header and "int rtmi_path_fold(" in header


def _bounce(s, n, o=DUMMY, d=DUMMY, st=DUMMY, em=DUMMY, at=DUMMY, hits=None, steps=None, work=DUMMY):
    return rtmi.lib().rtmi_bounce(s, n, o, d, st, em, at, hits, steps, work, None)


def test_bounce_argument_checks_before_any_hip_call():
    assert _refused(_bounce(None, 1), b"null scene")
    b = rtmi.SceneBuilder(1)
    assert _refused(_bounce(b.h, -1), b"negative")
    assert _refused(_bounce(b.h, 1 << 31), b"2^31")
    for k in ("o", "d", "st", "em", "at", "work"):
        assert _refused(_bounce(b.h, 1, **{k: None}), b"null"), k
    assert _refused(_bounce(b.h, 1), b"committed")
    assert _refused(_bounce(b.h, 0, None, None, None, None, None, None, None, None), b"committed")  # (whatever n)


def _fold(n, layers, d=DUMMY, steps=DUMMY, em=DUMMY, at=DUMMY, out=DUMMY):
    return rtmi.lib().rtmi_path_fold(n, layers, d, steps, em, at, out, None)


def test_path_fold_argument_checks_before_any_hip_call():
    assert _refused(_fold(-1, 1), b"negative")
    assert _refused(_fold(1 << 31, 1), b"2^31")
    for layers in (0, -1, 65):
        assert _refused(_fold(1, layers), b"layers")
    for k in ("d", "steps", "em", "at", "out"):
        assert _refused(_fold(1, 8, **{k: None}), b"null"), k
    assert _fold(0, 1, None, None, None, None, None) == OK  # nothing to do
    assert _refused(_fold(0, 0, None, None, None, None, None), b"layers")


def test_python_bounce_refusals():
    torch = pytest.importorskip("torch")
    b = rtmi.SceneBuilder(1)
    o = torch.zeros((4, 3), dtype=torch.float32)
    st = torch.zeros((6, 4), dtype=torch.int32)
    with pytest.raises(rtmi.RtmiError):
        b.bounce(o, o.clone(), st)  # CPU tensors: there is no CPU path
    with pytest.raises(rtmi.RtmiError):
        b.trace_steps(o, o.clone(), st, 4)
    with pytest.raises(rtmi.RtmiError):
        rtmi.path_fold(o, torch.zeros(4, dtype=torch.int32), torch.zeros((2, 4, 3)), torch.zeros((2, 4, 3)))
    with pytest.raises(rtmi.RtmiError):
        b.bounce(o.double(), o.clone(), st)
    with pytest.raises(rtmi.RtmiError):
        b.bounce(torch.zeros((4, 2)), o, st)


def test_bounce_kernels_declare_no_static_lds():
    """The step stages its tables at byte offsets of the DYNAMIC LDS array, as the trace loop it is a mode of: right only
    while the kernels declare no static LDS (group_segment_fixed_size == 0), in both builds, one kernel per query variant."""
    for lib in LIBS:
        notes = common.kernel_notes(lib)
        ks = {n: blk for n, blk in notes.items() if "bounce_kernel" in n}
        assert len(ks) == QUERY_VARIANTS, (lib, sorted(ks))
        for name, blk in ks.items():
            assert re.search(r"\.group_segment_fixed_size:\s+0\b", blk), (lib, name)
        assert any("path_fold_kernel" in n for n in notes), lib


# ------------------------------------------------------------------ the numpy fold, by hand
f32 = np.float32


def _stacks(layers, n=1):
    # canaries in every layer: a fold that reads past c shows
    return np.full((layers, n, 3), 1e30, dtype=f32), np.full((layers, n, 3), 1e30, dtype=f32)


def test_fold_of_a_path_ended_by_a_light():
    E, A = _stacks(4)
    A[0, 0], E[0, 0] = (0.5, 0.25, 1.0), 0
    A[1, 0], E[1, 0] = (0.5, 0.5, 0.5), 0
    E[2, 0], A[2, 0] = (8, 4, 2), 0  # the light: its layer's emitted is the path's end
    r = fold(np.zeros((1, 3), f32), [3], E, A)
    assert r.tolist() == [[2.0, 0.5, 1.0]]  # 0.5 * (0.5 * 8), 0.25 * (0.5 * 4), 1 * (0.5 * 2)


def test_fold_of_a_path_ended_by_a_miss():
    E, A = _stacks(3)
    A[0, 0], E[0, 0] = (0.5, 0.5, 0.5), (1, 2, 3)  # (a layer that both emits and attenuates: E + A * r)
    E[1, 0], A[1, 0] = 0, 0  # nothing hit: emitted 0, direction 0
    r = fold(np.zeros((1, 3), f32), [2], E, A)
    assert r.tolist() == [[1.0, 2.0, 3.0]]  # 1 + 0.5 * 0, ...


def test_fold_of_a_path_cut_while_alive():
    E, A = _stacks(3)
    A[0, 0], E[0, 0] = (0.5, 0.5, 0.5), (1, 0, 0)
    A[1, 0], E[1, 0] = (0.5, 0.5, 0.5), (4, 0, 0)
    d = np.array([[0, 0, 1]], dtype=f32)  # still going: Trace's depth limit returns 0 for what follows
    r = fold(d, [2], E, A)
    assert r.tolist() == [[3.0, 0.0, 0.0]]  # 1 + 0.5 * (4 + 0.5 * 0)
    # the clamp: three steps were made, two layers are kept -- the path is cut behind layer 1 (layer 2 is never read)
    assert bits(fold(d, [3], E, A, layers=2)).tolist() == bits(r).tolist()


def test_fold_of_no_steps_is_zero():
    E, A = _stacks(2)
    for d in ([0, 0, 0], [0, 1, 0]):
        r = fold(np.array([d], dtype=f32), [0], E, A)
        assert bits(r).tolist() == [[0, 0, 0]]  # +0.0f, and no layer read


def test_fold_keeps_an_emitted_negative_zero_on_the_last_layer():
    E, A = _stacks(2)
    E[0, 0] = (-0.0, 0.0, -0.0)
    r = fold(np.zeros((1, 3), f32), [1], E, A)
    assert bits(r).tolist() == [[0x80000000, 0, 0x80000000]]  # r = E[c-1] as it is: no 0 + ... in front of it
    # one layer further down it goes through E + A * r: (+0) + 1 * (-0) = +0
    E[1, 0], A[0, 0], E[0, 0] = (-0.0, 0.0, -0.0), (1, 1, 1), 0
    r = fold(np.zeros((1, 3), f32), [2], E, A)
    assert bits(r).tolist() == [[0, 0, 0]]
