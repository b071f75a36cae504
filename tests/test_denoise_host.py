"""rtmi_denoise / rtmi_resolve_variance on the host side: the filter and the variance rule restated in numpy
(tests/filter_rules.py: ``denoise_rule``, ``variance_rule``, which tests/test_gpu_denoise.py holds the device against bit
for bit), the exported symbols, the two structs against the C compiler, the argument checks that come before any HIP call, and the code-object
facts of the new kernels in both builds of the library.  No GPU involved."""
import ctypes as C
import os
import re
import subprocess
import tempfile

import numpy as np

import common
import rtmi
from rtmi import DenoiseGuides, DenoiseOpts
from abi_host import DUMMY, LIBS, ROOT, _frame, _refused
from filter_rules import denoise_rule, falloff, variance_rule

ENTRIES = ("rtmi_resolve_variance", "rtmi_denoise_scratch_bytes", "rtmi_denoise")
KERNELS = {"atrous_kernel": 4, "denoise_prepare_kernel": 1, "resolve_variance_kernel": 1}  # name part -> how many
F32 = np.float32


def test_falloff_on_hand_worked_values():
    """1 - x / 4 clamped at 0, to the fourth power: 1 at 0, (3/4)^4 = 81/256 at 1, 0 at 4 and beyond."""
    got = falloff(np.array([0, 1, 4, 5], F32))
    assert got.dtype == F32 and got.tolist() == [1.0, 0.31640625, 0.0, 0.0]


def test_denoise_rule_on_a_single_pixel():
    """1 x 1: every tap but the centre is outside, the centre's weight is h[2] h[2] = 9/64 times 1 (a unit normal against
    itself, the same depth, the same colour), and (9/64 x) / (9/64) = x for values of a few bits: the input comes back, and
    so does the variance through (w w V) / (w w).  A background pixel (alpha 0) likewise, whatever its normal."""
    c, v = np.array([[[1, 2, 0.5]]], F32), np.array([[[0.25, 0.5, 1]]], F32)
    for alpha, nrm in ((1.0, [0, 0, 1]), (0.0, [0, 0, 0])):
        for iterations in (1, 5):
            out, var = denoise_rule(c, v, np.array([[nrm]], F32), np.array([[3.0]], F32), np.array([[alpha]], F32),
                                    iterations=iterations)
            assert np.array_equal(out, c) and np.array_equal(var, v)
    # a surface pixel whose mean normal vanished has weight 0 all round: sw == 0 keeps the pixel as it is
    out, var = denoise_rule(c * F32(1.1), v, np.zeros((1, 1, 3), F32), np.array([[3.0]], F32), np.array([[1.0]], F32),
                            normal_squarings=5)
    assert np.array_equal(out, c * F32(1.1)) and np.array_equal(var, v)


def test_denoise_rule_averages_two_equal_neighbours():
    """1 x 2, background, colours 0 and 1 with a variance large enough that wc stays near 1: not demodulated, one pass.
    With sigma_color 4 and V = 4 per channel: vs = 24, d2 = 3, xc = 3 / (16 * 24 + 1e-10) = 1/128, m = 1 - 1/512, wc = m^4; pixel 0 gets
    (9/64 * 0 + 3/32 wc * 1) / (9/64 + 3/32 wc) -- checked against the same expression in Python's binary32."""
    c = np.array([[[0, 0, 0], [1, 1, 1]]], F32)
    v = np.full((1, 2, 3), 4, F32)
    z = np.zeros((1, 2), F32)
    out, var = denoise_rule(c, v, np.zeros((1, 2, 3), F32), z, z, iterations=1, sigma_color=4.0)
    m = F32(1) - F32(0.25) * (F32(3) / (F32(16) * F32(24) + F32(1e-10)))
    wc = (m * m) * (m * m)
    w0, w1 = F32(9 / 64), F32(3 / 32) * wc
    assert out[0, 0, 0] == (w0 * F32(0) + w1 * F32(1)) / (w0 + w1)
    assert var[0, 0, 0] == ((w0 * w0) * F32(4) + (w1 * w1) * F32(4)) / ((w0 + w1) * (w0 + w1))
    assert 0.39 < out[0, 0, 0] < 0.4  # (3/32 over 9/64 + 3/32, a little less for wc)


def test_variance_rule_on_hand_worked_cases():
    """n = 0 and padding: 0.  n = 1: the sample's square.  {0, 0, 0, 8}: S = 8, Q = 64, (4 * 64 - 64) / (16 * 3) = 4 (the
    sample variance 16 over n = 4).  Q too small for S by rounding (a - b < 0): clamped to 0."""
    n = np.array([0, 1, 4, 4, 4], np.uint32)
    S = np.array([[5] * 3, [3] * 3, [8] * 3, [2] * 3, [8] * 3], F32)
    Q = np.array([[9] * 3, [9] * 3, [64] * 3, [0.9] * 3, [64] * 3], F32)
    got = variance_rule(n, S, Q, pixel=np.array([True, True, True, True, False]))
    assert got.dtype == F32 and got.tolist() == [[0] * 3, [9] * 3, [4] * 3, [0] * 3, [0] * 3]


# ------------------------------------------------------------------ symbols, the structs
def test_denoise_entries_are_exported_by_both_builds():
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


def test_sizeof_denoise_structs_agrees_with_the_header():
    """The C compiler's sizeof and field offsets of both structs, from include/rtmi.h itself, against the ctypes structs."""
    src = '#include <stdio.h>\n#include <stddef.h>\n#include "rtmi.h"\nint main(void) {\n'
    pairs = (("rtmi_denoise_opts", DenoiseOpts), ("rtmi_denoise_guides", DenoiseGuides))
    for cname, cls in pairs:
        src += 'printf("%%zu", sizeof(%s));\n' % cname
        src += "".join('printf(" %%zu", offsetof(%s, %s));\n' % (cname, f[0]) for f in cls._fields_) + 'printf("\\n");\n'
    src += "return 0; }\n"
    with tempfile.TemporaryDirectory() as tmp:
        c, exe = os.path.join(tmp, "s.c"), os.path.join(tmp, "s")
        with open(c, "w") as fh:
            fh.write(src)
        subprocess.check_call(["cc", "-I", os.path.join(ROOT, "include"), c, "-o", exe])
        lines = subprocess.check_output([exe], text=True).splitlines()
    for line, (cname, cls) in zip(lines, pairs):
        got = [int(x) for x in line.split()]
        assert got == [C.sizeof(cls)] + [getattr(cls, f[0]).offset for f in cls._fields_], cname
    assert C.sizeof(DenoiseOpts) == 24 and C.sizeof(DenoiseGuides) == 48


def _opts(**kw):
    f = dict(size=C.sizeof(DenoiseOpts), iterations=5, normal_squarings=5, demodulate=1, sigma_color=4.0, sigma_depth=0.05)
    f.update(kw)
    return DenoiseOpts(f["size"], f["iterations"], f["normal_squarings"], f["demodulate"], f["sigma_color"], f["sigma_depth"])


def _guides(size=None, reserved=0, **null):
    g = DenoiseGuides(C.sizeof(DenoiseGuides) if size is None else size, reserved)
    for k in ("variance", "albedo", "normal", "depth", "alpha"):
        setattr(g, "d_" + k, None if k in null else DUMMY.value)
    return g


def test_denoise_argument_checks_before_any_hip_call():
    L = rtmi.lib()
    H, W = 20, 28
    enough = L.rtmi_denoise_scratch_bytes(H, W)
    assert enough >= H * W * 16 * 5  # (the guide records and two pairs of images)

    def call(h=H, w=W, o=_opts(), g=_guides(), color=DUMMY, out=DUMMY, out_var=None, scratch=DUMMY, nbytes=enough):
        return L.rtmi_denoise(h, w, C.byref(o) if o is not None else None, color, C.byref(g) if g is not None else None, out,
                              out_var, scratch, nbytes, None)

    for kw in (dict(h=0), dict(w=0), dict(h=-4), dict(h=65536), dict(w=70000)):
        assert _refused(call(**kw), b"65535"), kw
        assert L.rtmi_denoise_scratch_bytes(kw.get("h", H), kw.get("w", W)) == 0
    for kw in (dict(o=None), dict(g=None), dict(color=None), dict(out=None), dict(scratch=None)):
        assert _refused(call(**kw), b"null"), kw
    assert _refused(call(o=_opts(size=20)), b"size")
    assert _refused(call(o=_opts(size=0)), b"size")
    assert _refused(call(g=_guides(size=C.sizeof(DenoiseGuides) + 8)), b"size")
    assert _refused(call(g=_guides(reserved=1)), b"reserved")
    for kw in (dict(iterations=0), dict(iterations=9), dict(iterations=-1), dict(normal_squarings=-1), dict(normal_squarings=9),
               dict(demodulate=2), dict(demodulate=-1), dict(sigma_color=0.0), dict(sigma_color=-1.0),
               dict(sigma_color=float("nan")), dict(sigma_color=float("inf")), dict(sigma_depth=0.0), dict(sigma_depth=-0.05),
               dict(sigma_depth=float("nan")), dict(sigma_depth=float("inf"))):
        assert _refused(call(o=_opts(**kw)), b"out of range"), kw
    for k in ("variance", "normal", "depth", "alpha", "albedo"):
        assert _refused(call(g=_guides(**{k: True})), b"null guide"), k
    # without demodulate the albedo is not looked at: the next check is what refuses
    assert _refused(call(o=_opts(demodulate=0), g=_guides(albedo=True), nbytes=enough - 1), b"scratch_bytes")
    assert _refused(call(nbytes=0), b"scratch_bytes")
    assert _refused(call(nbytes=enough - 1), b"scratch_bytes")


def test_resolve_variance_argument_checks_before_any_hip_call():
    L = rtmi.lib()
    names = ("sum", "sq", "samples", "var")

    def call(frame, **null):
        a = {k: (None if k in null else DUMMY) for k in names}
        return L.rtmi_resolve_variance(C.byref(frame) if frame is not None else None, a["sum"], a["sq"], a["samples"], a["var"],
                                       None)

    assert _refused(call(None), b"frame")
    assert _refused(call(_frame(height=0)), b"frame")
    assert _refused(call(_frame(rank=2, world=2)), b"frame")
    assert _refused(call(_frame(width=70000)), b"65535")
    for k in names:
        assert _refused(call(_frame(), **{k: True}), b"null"), k


def test_python_denoise_refuses_what_it_cannot_pass_on():
    """rtmi.denoise has no CPU path, and Renderer.denoise is for one rank's whole frame."""
    import pytest
    with pytest.raises(rtmi.RtmiError, match="CUDA"):
        rtmi.denoise(np.zeros((4, 4, 3), F32), None, None, None, None)
    R = rtmi.Renderer.__new__(rtmi.Renderer)  # (no GPU here: only the frame is looked at)
    R.frame = rtmi.make_frame(16, 16, 4, 10, False, 0, 2)
    with pytest.raises(rtmi.RtmiError, match="rtmi.denoise"):
        R.denoise()


# ------------------------------------------------------------------ the kernels
def test_denoise_kernels_have_no_scratch_and_no_spills():
    """Both builds: the four a-trous instantiations (LDS-staged or global taps, an intermediate or the last pass), the
    prepare kernel and the variance kernel keep everything in registers, and none bears a name the other host tests select
    the trace kernels by."""
    reserved = ("render_kernel", "probe_kernel", "trace_kernel", "query_kernel", "occlusion_kernel", "budget_kernel",
                "feature_kernel")
    for lib in LIBS:
        ks = common.kernel_notes(lib)
        for part, count in KERNELS.items():
            mine = {n: blk for n, blk in ks.items() if part in n}
            assert len(mine) == count, (lib, part, sorted(mine))
            for name, blk in mine.items():
                assert not any(r in name for r in reserved), name
                for key in ("private_segment_fixed_size", "vgpr_spill_count", "sgpr_spill_count"):
                    m = re.search(r"\.%s:\s+(\d+)" % key, blk)
                    assert m and int(m.group(1)) == 0, (lib, name, key, m and m.group(1))
        # the staged passes hold tile + halo at step 2 (40 x 16 records of three kinds); the others nothing
        lds = {n: int(re.search(r"\.group_segment_fixed_size:\s+(\d+)", blk).group(1)) for n, blk in ks.items()
               if "atrous_kernel" in n}
        assert sorted(lds.values()) == [0, 0, 30720, 30720], lds
