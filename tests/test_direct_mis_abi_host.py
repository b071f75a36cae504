"""rtmi_direct_sample_mis on the host side: the export of both builds and its declaration, the argument checks that come
before any HIP call, the Python binding's refusals and the kernel's metadata.  No GPU involved."""
import ctypes as C
import os
import re
import subprocess

import pytest

import rtmi
from abi_host import DUMMY, LIBS, ROOT, _count, _refused
from common import kernel_notes

ARRAYS = ("d_origins", "d_dirs", "d_hits", "d_steps", "d_emitted", "d_attenuation", "d_light_states", "d_flags",
          "d_shadow_origins", "d_shadow_dirs", "d_shadow_t_max", "d_direct")


def test_entry_is_exported_by_both_builds_declared_and_bound():
    L = rtmi.lib()
    assert L.rtmi_version() == 3  # additive: no version change
    header = open(os.path.join(ROOT, "include", "rtmi.h")).read()
    for lib in LIBS:
        syms = subprocess.run(["nm", "-D", "--defined-only", lib], stdout=subprocess.PIPE, text=True, check=True).stdout
        assert re.search(r"\bT rtmi_direct_sample_mis$", syms, re.M) and re.search(r"\bT rtmi_direct_sample$", syms, re.M), lib
    assert "rtmi_direct_sample_mis" in [s[0] for s in rtmi.SYMBOLS] and re.search(r"\brtmi_direct_sample_mis\(", header)
    assert re.search(r"typedef struct rtmi_direct_sample_mis_args \{", header)
    assert C.sizeof(rtmi.DirectSampleMisArgs) == 160
    assert "carry" not in rtmi.Steps._fields and rtmi.Steps(*range(8)).carry is None  # beside the fields: unpacking holds
    assert rtmi.DirectSample._fields[-1] == "carry" and rtmi.DirectSample(*range(6)).carry is None


def _args(n, n_list, **kw):
    a = rtmi.DirectSampleMisArgs()
    a.size, a.reserved, a.n, a.n_list = C.sizeof(rtmi.DirectSampleMisArgs), 0, n, n_list
    for k in ARRAYS:
        setattr(a, k, DUMMY.value)
    a.d_carry = DUMMY.value
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def _call(s, a):
    return rtmi.lib().rtmi_direct_sample_mis(s, C.byref(a) if a is not None else None, None)


def test_argument_checks_before_any_hip_call():
    b = rtmi.SceneBuilder(1)  # never committed: the last refusal of all
    assert _refused(_call(None, _args(8, 8)), b"null scene")
    assert _refused(_call(b.h, None), b"null rtmi_direct_sample_mis_args")
    for size in (0, 8, 152, 168):
        assert _refused(_call(b.h, _args(8, 8, size=size)), b"size")
    assert _refused(_call(b.h, _args(8, 8, reserved=1)), b"reserved")
    # the carry: required with n_list > 0, 16-byte aligned
    assert _refused(_call(b.h, _args(8, 8, d_carry=None)), b"carry")
    for off in (4, 8, 12, 1):
        assert _refused(_call(b.h, _args(8, 8, d_carry=DUMMY.value + off)), b"16-byte")
    # rtmi_direct_sample's own cases
    assert _refused(_call(b.h, _args(-1, 0)), b"negative path count")
    assert _refused(_call(b.h, _args(1 << 31, 8)), b"2^31 - 1")
    assert _refused(_call(b.h, _args(8, -1)), b"list")
    assert _refused(_call(b.h, _args(8, 9)), b"list")  # a null list longer than n
    assert _refused(_call(b.h, _args(8, 8, step=rtmi.MAX_DEPTH)), b"step")
    for k in ARRAYS:
        assert _refused(_call(b.h, _args(8, 8, **{k: None})), b"null ray, hit"), k
    # nothing wrong but the scene: the checks above all came first
    assert _refused(_call(b.h, _args(8, 8)), b"committed")
    assert _refused(_call(b.h, _args(8, 0, d_carry=None)), b"committed")  # no carry needed where nothing is listed


def test_binding_refuses_a_carry_without_mis_and_a_wrong_direct():
    import inspect
    sig = inspect.signature(rtmi.SceneBuilder.direct_sample)
    assert sig.parameters["mis"].default is False and sig.parameters["carry"].default is None
    assert inspect.signature(rtmi.SceneBuilder.trace_steps).parameters["direct"].default is False
    assert inspect.signature(rtmi.Renderer.render_rays).parameters["direct"].default is False


@pytest.mark.parametrize("lib", LIBS)
def test_kernel_metadata(lib):
    """direct_sample_mis_kernel is direct_sample_kernel's shape: 4 KiB of LDS for the cdf, no scratch, no spill, and no more
    vector registers than 64 (eight waves per SIMD), as its parent."""
    notes = kernel_notes(lib)
    mis = [v for k, v in notes.items() if "direct_sample_mis_kernel" in k]
    par = [v for k, v in notes.items() if "direct_sample_kernel" in k]
    assert len(mis) == 1 and len(par) == 1
    for blk in mis + par:
        assert _count(blk, "group_segment_fixed_size") == 4096 and _count(blk, "private_segment_fixed_size") == 0
        assert _count(blk, "vgpr_spill_count") == 0 and _count(blk, "sgpr_spill_count") == 0
        assert _count(blk, "vgpr_count") <= 64 and _count(blk, "max_flat_workgroup_size") == 256
