"""rtmi_accumulate / rtmi_camera_update on the host side: the accumulation rule restated in numpy
(tests/filter_rules.py: ``accumulate_rule``, which tests/test_gpu_accumulate.py holds the device against bit for bit), a synthetic room seen from two cameras
(``room``, ``MOVES``) whose frames reach every branch of the rule, hand-worked cases, the exported symbols, the struct
against the C compiler, the argument checks that come before any HIP call, and the code-object facts of the new kernel in
both builds of the library.  No GPU involved."""
import ctypes as C
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest

import common
import rtmi
from rtmi import AccumulateOpts, DenoiseGuides
from abi_host import DUMMY, LIBS, ROOT, _refused
from filter_rules import BRANCHES, FOV, MOVES, SHAPES, accumulate_rule, camera_of, camera_terms, room
from parity import same

ENTRIES = ("rtmi_camera_update", "rtmi_history_bytes", "rtmi_accumulate")
F32 = np.float32


def first_frame(h, w, seed=0):
    """(the home camera, its frame, the history the rule makes of it)"""
    cam = camera_of("static", h, w)
    d = room(h, w, cam, seed)
    return cam, d, accumulate_rule(**d, camera=cam)[3]


def moved(move, h, w, **opts):
    cam0, _, hist = first_frame(h, w)
    cam1 = camera_of(move, h, w)
    return accumulate_rule(**room(h, w, cam1, seed=1), camera=cam1, history=hist, prev_camera=cam0, **opts)


# ------------------------------------------------------------------ every branch is reached
@pytest.mark.parametrize("shape", [(16, 16), (33, 70)], ids=lambda s: "%dx%d" % s)
def test_the_four_moves_reach_every_branch(shape):
    """A condition, not a measurement: over the four moves together every one of the seven branches holds a pixel, and
    each move holds the branches it is there for.  Measured at 16 x 16 with the library's camera (shares of the pixels):
    static: snapped 0.81, background 0.19; slide: 1-3 taps, 4 taps and refused; pan: those and off-screen; about: off-screen
    and behind."""
    there_for = {"static": ("snapped", "background"), "slide": ("taps_1_3", "taps_4", "refused"),
                 "pan": ("taps_1_3", "taps_4", "refused", "off_screen"), "about": ("off_screen", "behind")}
    reached = set()
    for move, names in there_for.items():
        shares = moved(move, *shape)[4]
        print(shape, move, {k: round(s, 4) for k, s in shares.items() if s})
        assert abs(sum(shares.values()) - 1) < 1e-9
        for k in names:
            assert shares[k] > 0, (move, k, shares)
        reached |= {k for k, s in shares.items() if s > 0}
    assert reached == set(BRANCHES)


# ------------------------------------------------------------------ hand-worked cases
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d" % s)
def test_a_static_camera_is_the_exact_running_mean(shape):
    """min_blend 0, three frames from one camera: on surface pixels L is 1, 2, 3 exactly and
    C_k = (1 - 1/k) C_{k-1} + (1/k) c_k in binary32, V_k = (1 - 1/k)^2 V_{k-1} + (1/k)^2 v_k; the background stays fresh."""
    h, w = shape
    cam = camera_of("static", h, w)
    hist, Cm, Vm = None, None, None
    for k in (1, 2, 3):
        d = room(h, w, cam, seed=k)
        out, var, length, hist, shares = accumulate_rule(**d, camera=cam, history=hist, prev_camera=None if k == 1 else cam,
                                                         min_blend=0.0)
        surf = d["alpha"] > 0
        assert surf.any()
        if k == 1:
            Cm, Vm = d["color"], d["variance"]
        else:
            a = F32(1) / F32(k)
            o = F32(1) - a
            Cm = np.where(surf[..., None], o * Cm + a * d["color"], d["color"])
            Vm = np.where(surf[..., None], (o * o) * Vm + (a * a) * d["variance"], d["variance"])
            assert shares["snapped"] == surf.mean() and shares["background"] == (~surf).mean()
        assert same(length, np.where(surf, F32(k), F32(1)))
        assert same(out, Cm) and same(var, Vm)


def test_min_blend_one_returns_the_frame():
    counted = False
    for move in MOVES:
        out, var, length, hist, shares = moved(move, 16, 16, min_blend=1.0)
        counted |= bool((length > 1).any())
        cur = room(16, 16, camera_of(move, 16, 16), seed=1)
        assert same(out, cur["color"]) and same(var, cur["variance"])
        assert same(hist[1][..., :3], cur["color"]) and same(hist[0][..., 3], cur["depth"])
    assert counted  # (the lengths still count)


def test_without_a_history_everything_is_fresh():
    cam, d, hist = first_frame(33, 70)
    out, var, length, hist2, shares = accumulate_rule(**d, camera=cam)
    assert same(out, d["color"]) and same(var, d["variance"]) and same(length, np.ones((33, 70), F32))
    assert same(hist, hist2)
    assert same(hist[0][..., :3], d["normal"]) and same(hist[0][..., 3], d["depth"])
    assert same(hist[1][..., :3], d["color"]) and same(hist[1][..., 3], np.ones((33, 70), F32))
    assert same(hist[2][..., :3], d["variance"]) and same(hist[2][..., 3], (d["alpha"] > 0).astype(F32))


def test_a_background_pixel_is_fresh_whatever_the_history():
    """alpha 0 everywhere over a history that would be taken: every pixel comes back as it is, with length 1."""
    cam, d, hist = first_frame(16, 16)
    cur = room(16, 16, cam, seed=2)
    cur["alpha"][:] = 0
    out, var, length, hist2, shares = accumulate_rule(**cur, camera=cam, history=hist, prev_camera=cam, min_blend=0.0)
    assert shares["background"] == 1.0
    assert same(out, cur["color"]) and same(var, cur["variance"]) and same(length, np.ones((16, 16), F32))
    assert not hist2[2][..., 3].any()


def _raw_camera(p, llc, h, v):
    return np.array(list(p) + list(llc) + list(h) + list(v) + [0] * 9, F32)


def test_one_by_two_with_half_a_pixel_worked_by_hand():
    """1 x 2, both cameras at the origin looking down +z with h = (2, 0, 0), v = (0, 1/2, 0); the previous one has
    llc = (-1, -3/4, 1), the current one is shifted half a pixel to the right: llc = (-1/2, -3/4, 1).  Everything below is
    exact in binary32.  H = 1 makes yf = (1 + 0.5) / 1 = 3/2, so yf v = 3/4 and every centre ray has Dy = 0.  Pixel 0: xf = 1/4,
    D = (-1/2 + 1/2, 0, 1) = (0, 0, 1), l = 1; with z_p = 2: P = d = (0, 0, 2), ze = 2.  The inverse of [h' v' c'] has rows
    (1/2, 0, 1/2), (0, 2, 3/2), (0, 0, 1): alpha = 1, beta = 3, gamma = 2, so fx = (1/2) 2 - 1/2 = 1/2 and fy = 3/2 - (3/2) 1 = 0:
    no snap, j0 = 0, tx = 1/2, i0 = 0, ty = 0.  The taps of row 0 weigh 1/2 each; row 1 is outside.  History: lengths 1 and 3,
    colours 2 and 4, variances 1 and 3, depths 2 and 2.05 (within 0.05 * 2), normals equal; the frame: colour 8, variance 2,
    min_blend 0:
        sw = 1, Lh = (1/2 + 3/2) / 1 = 2, L' = 3, a = 1/3, Ch = 3, Vh = 2:  C' = (1 - a) 3 + a 8,  V' = (1 - a)^2 2 + a^2 2.
    With history pixel 1 not a surface only column 0 counts: sw = 1/2, Lh = 1, L' = 2, a = 1/2, Ch = 2, Vh = 1: C' = 1 + 4 = 5,
    V' = 1/4 + 2/4 = 3/4.  With history pixel 0 at depth 2.3 (0.3 > 0.1) and pixel 1 no surface: every tap refused.  Pixel 1 of
    the frame is background: fresh."""
    prev = _raw_camera((0, 0, 0), (-1, -0.75, 1), (2, 0, 0), (0, 0.5, 0))
    cur = _raw_camera((0, 0, 0), (-0.5, -0.75, 1), (2, 0, 0), (0, 0.5, 0))
    n = np.zeros((1, 2, 3), F32)
    n[..., 2] = -1
    hist = np.zeros((3, 1, 2, 4), F32)
    hist[0, ..., :3], hist[0, 0, :, 3] = n, [2, 2.05]
    hist[1, 0, :, :3], hist[1, 0, :, 3] = [[2] * 3, [4] * 3], [1, 3]
    hist[2, 0, :, :3], hist[2, 0, :, 3] = [[1] * 3, [3] * 3], 1
    frame = dict(color=np.full((1, 2, 3), 8, F32), variance=np.full((1, 2, 3), 2, F32), normal=n, depth=np.full((1, 2), 2, F32),
                 alpha=np.array([[1, 0]], F32), camera=cur, prev_camera=prev, min_blend=0.0)
    out, var, length, hist_out, shares = accumulate_rule(history=hist, **frame)
    assert shares["taps_1_3"] == 0.5 and shares["background"] == 0.5
    a = F32(1) / F32(3)
    o = F32(1) - a
    assert length.tolist() == [[3.0, 1.0]]
    assert out[0, 0].tolist() == [float(o * F32(3) + a * F32(8))] * 3
    assert var[0, 0].tolist() == [float((o * o) * F32(2) + (a * a) * F32(2))] * 3
    assert out[0, 1].tolist() == [8.0] * 3 and var[0, 1].tolist() == [2.0] * 3
    assert hist_out[1, 0, 0].tolist() == out[0, 0].tolist() + [3.0] and hist_out[2, 0, :, 3].tolist() == [1.0, 0.0]
    hist[2, 0, 1, 3] = 0
    out, var, length, _, shares = accumulate_rule(history=hist, **frame)
    assert shares["taps_1_3"] == 0.5 and length[0, 0] == 2 and out[0, 0].tolist() == [5.0] * 3 and var[0, 0].tolist() == [0.75] * 3
    hist[0, 0, 0, 3] = 2.3
    out, var, length, _, shares = accumulate_rule(history=hist, **frame)
    assert shares["refused"] == 0.5 and length[0, 0] == 1 and out[0, 0].tolist() == [8.0] * 3 and var[0, 0].tolist() == [2.0] * 3


def test_camera_terms_of_an_axis_camera():
    """h = (2, 0, 0), v = (0, 1/2, 0), c = (-1, -3/4, 1): det = 1, and the inverse of [h v c] has rows (1/2, 0, 1/2), (0, 2, 3/2),
    (0, 0, 1).  e is llc - p."""
    e, R, singular = camera_terms(_raw_camera((800, 0, 0), (800.25, -1, 3), (2, 0, 0), (0, 0.5, 0)),
                                  _raw_camera((0, 0, 0), (-1, -0.75, 1), (2, 0, 0), (0, 0.5, 0)))
    assert not singular and e.dtype == F32 and e.tolist() == [0.25, -1, 3]
    assert R.dtype == F32 and R.tolist() == [[0.5, 0, 0.5], [0, 2, 1.5], [0, 0, 1]]
    assert camera_terms(_raw_camera((0, 0, 0), (1, 0, 0), (2, 0, 0), (0, 1, 0)), _raw_camera((0, 0, 0), (1, 0, 0), (2, 0, 0), (0, 1, 0)))[2]  # (h, v and c in one plane)


# ------------------------------------------------------------------ symbols, the struct
def test_accumulate_entries_are_exported_by_both_builds():
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


def test_sizeof_accumulate_opts_agrees_with_the_header():
    """The C compiler's sizeof and field offsets, from include/rtmi.h itself, against the ctypes struct."""
    src = '#include <stdio.h>\n#include <stddef.h>\n#include "rtmi.h"\nint main(void) {\n'
    src += 'printf("%zu", sizeof(rtmi_accumulate_opts));\n'
    src += "".join('printf(" %%zu", offsetof(rtmi_accumulate_opts, %s));\n' % f[0] for f in AccumulateOpts._fields_)
    src += 'printf("\\n");\nreturn 0; }\n'
    with tempfile.TemporaryDirectory() as tmp:
        c, exe = os.path.join(tmp, "s.c"), os.path.join(tmp, "s")
        with open(c, "w") as fh:
            fh.write(src)
        subprocess.check_call(["cc", "-I", os.path.join(ROOT, "include"), c, "-o", exe])
        got = [int(x) for x in subprocess.check_output([exe], text=True).split()]
    assert got == [C.sizeof(AccumulateOpts)] + [getattr(AccumulateOpts, f[0]).offset for f in AccumulateOpts._fields_]
    assert C.sizeof(AccumulateOpts) == 20
    assert rtmi.ACCUMULATE_DEFAULTS == dict(normal_min=0.8, depth_tolerance=0.05, min_blend=0.1)


def _opts(**kw):
    f = dict(size=C.sizeof(AccumulateOpts), reserved=0, normal_min=0.8, depth_tolerance=0.05, min_blend=0.1)
    f.update(kw)
    return AccumulateOpts(f["size"], f["reserved"], f["normal_min"], f["depth_tolerance"], f["min_blend"])


def _guides(size=None, reserved=0, **null):
    g = DenoiseGuides(C.sizeof(DenoiseGuides) if size is None else size, reserved)
    for k in ("variance", "albedo", "normal", "depth", "alpha"):
        setattr(g, "d_" + k, None if k in null else DUMMY.value)
    return g


def test_accumulate_argument_checks_before_any_hip_call():
    L = rtmi.lib()
    H, W = 20, 28
    fp = C.POINTER(C.c_float)
    good = camera_of("static", H, W)
    nan, inf = good.copy(), good.copy()
    nan[7], inf[20] = np.nan, np.inf
    flat = _raw_camera((0, 0, 0), (1, 0, 0), (2, 0, 0), (0, 1, 0))  # (h, v and llc - p in one plane)
    cam = lambda a: None if a is None else a.ctypes.data_as(fp)

    def call(h=H, w=W, o=_opts(), g=_guides(), color=DUMMY, cur=good, hist_in=DUMMY, prev=good, hist_out=C.c_void_p(32),
             out=DUMMY, out_var=None, out_len=None):
        return L.rtmi_accumulate(h, w, C.byref(o) if o is not None else None, color, C.byref(g) if g is not None else None,
                                 cam(cur), hist_in, cam(prev), hist_out, out, out_var, out_len, None)

    assert L.rtmi_history_bytes(H, W) == 48 * H * W
    assert L.rtmi_history_bytes(1, 1) == 48 and L.rtmi_history_bytes(65535, 65535) == 48 * 65535 * 65535
    for kw in (dict(h=0), dict(w=0), dict(h=-4), dict(h=65536), dict(w=70000)):
        assert _refused(call(**kw), b"65535"), kw
        assert L.rtmi_history_bytes(kw.get("h", H), kw.get("w", W)) == 0
    for kw in (dict(o=None), dict(g=None), dict(color=None), dict(cur=None), dict(hist_out=None), dict(out=None)):
        assert _refused(call(**kw), b"null"), kw
    assert _refused(call(o=_opts(size=24)), b"size")
    assert _refused(call(o=_opts(size=0)), b"size")
    assert _refused(call(o=_opts(reserved=1)), b"reserved")
    assert _refused(call(g=_guides(size=C.sizeof(DenoiseGuides) + 8)), b"size")
    assert _refused(call(g=_guides(reserved=1)), b"reserved")
    for kw in (dict(normal_min=-1.5), dict(normal_min=1.5), dict(normal_min=float("nan")), dict(normal_min=float("-inf")),
               dict(depth_tolerance=0.0), dict(depth_tolerance=-0.05), dict(depth_tolerance=float("nan")),
               dict(depth_tolerance=float("inf")), dict(min_blend=-0.1), dict(min_blend=1.5), dict(min_blend=float("nan"))):
        assert _refused(call(o=_opts(**kw)), b"out of range"), kw
    for k in ("variance", "normal", "depth", "alpha"):
        assert _refused(call(g=_guides(**{k: True})), b"null guide"), k
    assert _refused(call(hist_in=None), b"go together")
    assert _refused(call(prev=None), b"go together")
    assert _refused(call(hist_in=C.c_void_p(24)), b"aligned")
    assert _refused(call(hist_out=C.c_void_p(40)), b"aligned")
    assert _refused(call(cur=nan), b"non-finite")
    assert _refused(call(prev=inf), b"non-finite")
    assert _refused(call(hist_in=None, prev=None, cur=inf), b"non-finite")
    assert _refused(call(prev=flat), b"singular")
    # the albedo is not looked at: with it null the next check is what refuses
    assert _refused(call(g=_guides(albedo=True), prev=flat), b"singular")


def test_camera_update_on_the_host():
    """On an uncommitted scene rtmi_camera_update is rtmi_camera_set: rtmi_camera_get returns what was set, and the scene
    stays uncommitted.  A null argument and a NaN are refused, and leave the camera as it was."""
    L = rtmi.lib()
    fp = C.POINTER(C.c_float)
    s = C.c_void_p(L.rtmi_scene_create())
    try:
        a = camera_of("slide", 16, 16)
        assert L.rtmi_camera_update(s, a.ctypes.data_as(fp), 0, -1.0) == 0
        got = np.zeros(21, F32)
        assert L.rtmi_camera_get(s, got.ctypes.data_as(fp)) == 0 and same(got, a)
        assert _refused(L.rtmi_camera_update(None, a.ctypes.data_as(fp), 0, -1.0), b"null")
        assert _refused(L.rtmi_camera_update(s, None, 0, -1.0), b"null")
        for k, bad in ((0, np.nan), (20, np.inf), (11, -np.inf)):
            b = camera_of("pan", 16, 16)
            b[k] = bad
            assert _refused(L.rtmi_camera_update(s, b.ctypes.data_as(fp), 0, -1.0), b"non-finite")
        assert L.rtmi_camera_get(s, got.ctypes.data_as(fp)) == 0 and same(got, a)
        out = (C.c_int32 * 4)()
        f = rtmi.make_frame(16, 16, 4)
        assert _refused(L.rtmi_render_launch_shape(s, C.byref(f), None, out), b"not committed")
    finally:
        L.rtmi_scene_destroy(s)
    b = rtmi.SceneBuilder()
    b.camera_look((318, 283, -780), (278, 273, 0), (0, 1, 0), FOV, 1.0)
    assert same(b.camera_get().reshape(-1), a)
    assert b.camera_update(camera_of("pan", 16, 16)) is b and same(b.camera_get().reshape(-1), camera_of("pan", 16, 16))


def test_python_accumulate_refuses_what_it_cannot_pass_on():
    """rtmi.accumulate has no CPU path, and Renderer.accumulate is for one rank's whole frame."""
    with pytest.raises(rtmi.RtmiError, match="CUDA"):
        rtmi.accumulate(np.zeros((4, 4, 3), F32), None, None, None, None, camera_of("static", 4, 4))
    R = rtmi.Renderer.__new__(rtmi.Renderer)  # (no GPU here: only the frame is looked at)
    R.frame = rtmi.make_frame(16, 16, 4, 10, False, 0, 2)
    with pytest.raises(rtmi.RtmiError, match="rtmi.denoise"):
        R.accumulate(None)


# ------------------------------------------------------------------ the kernel
def test_accumulate_kernels_have_no_scratch_and_no_spills():
    """Both builds: the two instantiations (with and without a history) keep everything in registers, use no LDS, and bear
    no name the other host tests select kernels by."""
    reserved = ("render_kernel", "probe_kernel", "trace_kernel", "query_kernel", "occlusion_kernel", "budget_kernel",
                "feature_kernel", "atrous_kernel", "denoise_prepare_kernel", "resolve_variance_kernel")
    for lib in LIBS:
        mine = {n: blk for n, blk in common.kernel_notes(lib).items() if "accumulate_kernel" in n}
        assert len(mine) == 2, (lib, sorted(mine))
        for name, blk in mine.items():
            assert not any(r in name for r in reserved), name
            for key in ("private_segment_fixed_size", "vgpr_spill_count", "sgpr_spill_count", "group_segment_fixed_size"):
                m = re.search(r"\.%s:\s+(\d+)" % key, blk)
                assert m and int(m.group(1)) == 0, (lib, name, key, m and m.group(1))
