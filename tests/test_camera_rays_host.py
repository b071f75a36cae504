"""rtmi_camera_rays / rtmi_sample_add on the host side: the exported symbols, the struct, and every refusal that comes
before any HIP call, on recorded scenes that are never committed.  No GPU involved.

The library checks the projection and the camera's frame BEFORE it asks whether the scene is committed, so an
uncommitted scene that gets as far as "not committed" has passed every argument check: that is how the orthonormality
rule is seen to accept a look-at camera here."""
import ctypes as C
import math
import os
import re

import numpy as np

import common
import rtmi
from abi_host import DUMMY, LIBS, OK, _refused

ENTRIES = ("rtmi_camera_rays", "rtmi_sample_add")


def _frame(**kw):
    f = dict(height=20, width=28, spp=4, max_depth=8)
    f.update(kw)
    return rtmi.make_frame(f["height"], f["width"], f["spp"], f["max_depth"], False, f.get("rank", 0), f.get("world", 1))


def _scene(camera="pinhole"):
    b = rtmi.SceneBuilder(1)
    b.sky()
    if camera == "pinhole":
        b.camera_pinhole([0, 0, 1], [0.5, 0.25, -1], [0, 1, 0], 1.0, 1.4)
    elif camera == "defocus":
        b.camera_defocus([0, 0, 1], [0.5, 0.25, -1], [0, 1, 0], 1.0, 1.4, 0.2, 3.0)
    elif camera == "raw":
        b.camera_raw([0, 0, 1], [-1, -1, 0], [2, 0, 0], [0, 2, 0])
    return b


def _rays(b, frame, proj=None, **null):
    a = {k: (None if k in null else DUMMY) for k in ("budget", "states", "origins", "dirs")}
    return rtmi.lib().rtmi_camera_rays(b.h if b is not None else None, C.byref(frame) if frame is not None else None,
                                       C.byref(proj) if proj is not None else None, a["budget"], 0, a["states"], a["origins"],
                                       a["dirs"], None)


def test_entries_and_struct():
    L = rtmi.lib()
    assert L.rtmi_version() == 3  # additive: no version change
    names = [s[0] for s in rtmi.SYMBOLS]
    for path in LIBS:
        assert os.path.exists(path), path + " missing: __graft_entry__.build() builds it"
        lib = C.CDLL(path)
        for e in ENTRIES:
            assert e in names and hasattr(lib, e), (path, e)
    assert C.sizeof(rtmi.Projection) == 16
    p = rtmi.projection("fisheye", math.pi)
    assert (p.size, p.kind, p.reserved) == (16, 3, 0) and p.fov == np.float32(math.pi)
    assert [rtmi.projection(k).kind for k in ("camera", "orthographic", "equirect", "fisheye")] == [0, 1, 2, 3]
    header = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "rtmi.h")).read()
    assert re.search(r"RTMI_PROJ_CAMERA = 0, RTMI_PROJ_ORTHOGRAPHIC = 1, RTMI_PROJ_EQUIRECT = 2, RTMI_PROJ_FISHEYE = 3", header)


def test_both_kernels_are_in_both_builds():
    for lib in LIBS:
        ks = [n for n in common.kernel_notes(lib) if "camera_rays_kernel" in n or "sample_add_kernel" in n]
        assert len(ks) == 2, (lib, ks)


def test_camera_rays_argument_checks_before_any_hip_call():
    b = _scene()
    assert _refused(_rays(None, _frame()), b"scene")
    assert _refused(_rays(b, None), b"frame")
    assert _refused(_rays(b, _frame(height=0)), b"frame")
    assert _refused(_rays(b, _frame(rank=2, world=2)), b"frame")
    assert _refused(_rays(b, _frame(width=70000)), b"65535")
    for k in ("states", "origins", "dirs"):
        assert _refused(_rays(b, _frame(), **{k: True}), b"null"), k
    # the budget is optional: without it the call gets as far as the uncommitted scene
    assert _refused(_rays(b, _frame(), budget=True), b"committed")
    assert _refused(_rays(b, _frame()), b"committed")
    assert _refused(_rays(b, _frame(), rtmi.projection("camera")), b"committed")


def test_projection_struct_checks():
    b = _scene()
    wrong = rtmi.projection("equirect")
    wrong.size += 4
    assert _refused(_rays(b, _frame(), wrong), b"size")
    wrong = rtmi.projection("equirect")
    wrong.reserved = 1
    assert _refused(_rays(b, _frame(), wrong), b"reserved")
    for kind in (-1, 4, 99):
        wrong = rtmi.projection("camera")
        wrong.kind = kind
        assert _refused(_rays(b, _frame(), wrong), b"kind"), kind
    for fov in (0.0, -1.0, 6.2832, 7.0, float("nan"), float("inf"), -float("inf")):
        assert _refused(_rays(b, _frame(), rtmi.projection("fisheye", fov)), b"fov"), fov
    for fov in (1e-3, math.pi, 2 * math.pi):  # (2 pi as binary32) accepted: the next refusal is the scene's
        assert _refused(_rays(b, _frame(), rtmi.projection("fisheye", fov)), b"committed"), fov
    # the other kinds ignore fov
    assert _refused(_rays(b, _frame(), rtmi.projection("equirect", float("nan"))), b"committed")


def test_orthonormal_frame_rule():
    for kind in ("orthographic", "equirect", "fisheye"):
        p = rtmi.projection(kind, 1.0)
        for camera in ("pinhole", "defocus"):  # a look-at camera passes every argument check
            assert _refused(_rays(_scene(camera), _frame(), p), b"committed"), (kind, camera)
        assert _refused(_rays(_scene("raw"), _frame(), p), b"orthonormal"), kind
        assert _refused(_rays(_scene(None), _frame(), p), b"orthonormal"), kind  # no camera at all
    assert _refused(_rays(_scene("raw"), _frame(), None), b"committed")  # CAMERA needs no frame
    # rtmi_camera_set: a frame just inside and just outside the rule's 1e-3, and a non-finite one
    L = rtmi.lib()
    base = _scene("pinhole").camera_get().copy()

    def with_frame(u=None, v=None, w=None):
        b, f = _scene(None), base.copy()
        for k, x in ((4, u), (5, v), (6, w)):
            if x is not None:
                f[k] = np.asarray(x, dtype=np.float32)
        fp = np.ascontiguousarray(f.reshape(-1))
        assert L.rtmi_camera_set(b.h, fp.ctypes.data_as(C.POINTER(C.c_float)), 0, -1.0) == OK
        return b

    p = rtmi.projection("equirect")
    u, v = base[4].astype(np.float64), base[5].astype(np.float64)
    assert _refused(_rays(with_frame(), _frame(), p), b"committed")
    assert _refused(_rays(with_frame(u=u * math.sqrt(1.0009)), _frame(), p), b"committed")   # |u|^2 - 1 = 9e-4
    assert _refused(_rays(with_frame(u=u * math.sqrt(1.0011)), _frame(), p), b"orthonormal")  # 1.1e-3
    assert _refused(_rays(with_frame(w=base[6] * math.sqrt(0.9989)), _frame(), p), b"orthonormal")
    assert _refused(_rays(with_frame(u=u + 0.0009 * v), _frame(), p), b"committed")     # u.v = 9e-4
    assert _refused(_rays(with_frame(u=u + 0.0011 * v), _frame(), p), b"orthonormal")   # u.v = 1.1e-3
    assert _refused(_rays(with_frame(v=[float("nan"), 0, 0]), _frame(), p), b"orthonormal")
    assert _refused(_rays(with_frame(w=[float("inf"), 0, 0]), _frame(), p), b"orthonormal")


def test_sample_add_argument_checks_before_any_hip_call():
    L = rtmi.lib()
    names = ("budget", "radiance", "counts", "sum", "sq", "samples", "rays")

    def call(frame, **null):
        a = {k: (None if k in null else DUMMY) for k in names}
        return L.rtmi_sample_add(C.byref(frame) if frame is not None else None, a["budget"], 0, a["radiance"], a["counts"],
                                 a["sum"], a["sq"], a["samples"], a["rays"], None)

    assert _refused(call(None), b"frame")
    assert _refused(call(_frame(width=0)), b"frame")
    assert _refused(call(_frame(rank=1, world=1)), b"frame")
    assert _refused(call(_frame(height=70000)), b"65535")
    for k in ("radiance", "sum", "samples"):
        assert _refused(call(_frame(), **{k: True}), b"null"), k


def test_python_projection_refuses_unknown_kinds():
    import pytest
    with pytest.raises(rtmi.RtmiError, match="kind"):
        rtmi.projection("mercator")
