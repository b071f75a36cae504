"""rtmi_trace / rtmi_rng_init_n on the host side: the argument checks that come before any HIP call, the Python
binding's refusals, and the trace kernels in both builds of the library.  No GPU involved."""
import ctypes as C
import re

import pytest

import common
import rtmi
from abi_host import ERR_INVALID, LIBS, OK, QUERY_VARIANTS

ERR_NO_DEVICE = -2  # include/rtmi.h


def test_trace_entries_are_exported_and_bound():
    L = rtmi.lib()
    assert L.rtmi_version() == 3  # additive: no version change
    names = [s[0] for s in rtmi.SYMBOLS]
    assert "rtmi_trace" in names and "rtmi_rng_init_n" in names
    assert rtmi.TRACE_WORK_WORDS >= 4


def test_trace_argument_checks_before_any_hip_call():
    L = rtmi.lib()
    dummy = C.c_void_p(16)  # never dereferenced: argument checks come first
    args = lambda s, n, o=dummy, d=dummy, depth=8, st=dummy, rgb=dummy, rays=None, work=dummy: \
        L.rtmi_trace(s, n, o, d, depth, st, rgb, rays, work, None)
    assert args(None, 1) == ERR_INVALID
    b = rtmi.SceneBuilder(1)
    assert args(b.h, -1) == ERR_INVALID
    assert args(b.h, 1 << 31) == ERR_INVALID  # above 2^31 - 1
    for k in ("o", "d", "st", "rgb", "work"):
        assert args(b.h, 1, **{k: None}) == ERR_INVALID, k
    assert args(b.h, 1) == ERR_INVALID  # not committed
    assert b"committed" in L.rtmi_last_error()
    assert args(b.h, 0, None, None, 8, None, None, None, None) == ERR_INVALID  # (uncommitted, whatever n)


def test_rng_init_n_argument_checks():
    L = rtmi.lib()
    dummy = C.c_void_p(16)
    assert L.rtmi_rng_init_n(1, 0, -1, dummy, None) == ERR_INVALID
    assert L.rtmi_rng_init_n(1, 0, 5, None, None) == ERR_INVALID
    assert L.rtmi_rng_init_n(1, (1 << 40) - 4, 5, dummy, None) == ERR_INVALID  # first + n > 2^40
    assert L.rtmi_rng_init_n(1, 1 << 41, 0, dummy, None) == ERR_INVALID
    assert L.rtmi_rng_init_n(1, 0, 1 << 31, dummy, None) == ERR_INVALID
    assert L.rtmi_rng_init_n(1, 0, 0, None, None) == OK  # nothing to do
    if L.rtmi_device_count() <= 0:
        assert L.rtmi_rng_init_n(1, (1 << 40) - 5, 5, dummy, None) == ERR_NO_DEVICE
    with pytest.raises(rtmi.RtmiError):
        rtmi.rng_states(1, 5, first=(1 << 40) - 4)
    with pytest.raises(rtmi.RtmiError):
        rtmi.rng_states(1, -1)


def test_python_trace_refusals():
    torch = pytest.importorskip("torch")
    b = rtmi.SceneBuilder(1)
    o = torch.zeros((4, 3), dtype=torch.float32)
    st = torch.zeros((6, 4), dtype=torch.int32)
    with pytest.raises(rtmi.RtmiError):
        b.trace(o, o, st, 8)  # CPU tensors: there is no CPU path


def test_trace_kernels_declare_no_static_lds():
    """The trace kernels fold the layer stack at LDS addresses formed from byte offsets of the DYNAMIC LDS array, as
    the render does: right only while they declare no static LDS (group_segment_fixed_size == 0), in both builds."""
    for lib in LIBS:
        ks = {n: blk for n, blk in common.kernel_notes(lib).items() if "trace_kernel" in n}
        assert len(ks) == QUERY_VARIANTS, (lib, sorted(ks))
        for name, blk in ks.items():
            assert re.search(r"\.group_segment_fixed_size:\s+0\b", blk), (lib, name)
