"""rtmi_denoise / rtmi_resolve_variance on the host side: the filter and the variance rule restated in numpy
(``denoise_rule``, ``variance_rule``, which tests/test_gpu_denoise.py holds the device against bit for bit), the exported
symbols, the two structs against the C compiler, the argument checks that come before any HIP call, and the code-object
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
from test_budget_host import DUMMY, ERR_INVALID, LIBS, _frame

ENTRIES = ("rtmi_resolve_variance", "rtmi_denoise_scratch_bytes", "rtmi_denoise")
KERNELS = {"atrous_kernel": 4, "denoise_prepare_kernel": 1, "resolve_variance_kernel": 1}  # name part -> how many
F32 = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
H5 = [F32(1) / F32(16), F32(1) / F32(4), F32(3) / F32(8), F32(1) / F32(4), F32(1) / F32(16)]
MIN_WEIGHT_SUM = F32(2.0 ** -32)  # a pass filters a pixel only from this sum of weights on: below it sw * sw leaves the normals


# ------------------------------------------------------------------ the rules, restated
def falloff(x):
    m = np.fmax(F32(1) - F32(0.25) * x, F32(0))
    m2 = m * m
    return m2 * m2


def variance_rule(n, S, Q, pixel=None):
    """rtmi_resolve_variance in numpy, operation by operation as include/rtmi.h states it.  n (N,) uint32, S, Q (N, 3)
    float32, pixel (N,) bool (False: padding).  Returns (N, 3) float32."""
    n = np.asarray(n, dtype=np.uint32)
    S, Q = np.asarray(S, dtype=F32), np.asarray(Q, dtype=F32)
    if pixel is not None:
        n = np.where(np.asarray(pixel, dtype=bool), n, 0).astype(np.uint32)
    with np.errstate(all="ignore"):
        nf = n.astype(F32)[:, None]
        a = nf * Q
        b = S * S
        c = np.fmax(a - b, F32(0))
        d = nf * nf
        e = nf - F32(1)
        many = c / (d * e)
    for x in (a, b, c, d, e, many):
        assert x.dtype == F32
    n = n[:, None]
    return np.where(n == 0, F32(0), np.where(n == 1, b, many)).astype(F32)


def denoise_rule(color, variance, normal, depth, alpha, albedo=None, iterations=rtmi.DENOISE_DEFAULTS["iterations"],
                 sigma_color=rtmi.DENOISE_DEFAULTS["sigma_color"], sigma_depth=rtmi.DENOISE_DEFAULTS["sigma_depth"],
                 normal_squarings=rtmi.DENOISE_DEFAULTS["normal_squarings"], demodulate=None, decisions=None):
    """rtmi_denoise in numpy, operation by operation as include/rtmi.h states it: float32 throughout, vectorised over the
    image, the 25 taps in the stated order.  color, variance, normal, albedo (H, W, 3), depth, alpha (H, W).  Returns
    (out, out_variance), both (H, W, 3) float32.  decisions: a list that receives, per pass, the (H, W) bool array of the
    pixels the pass filtered (the others kept their value)."""
    C0, V0, N, Z, A = (np.asarray(x, dtype=F32) for x in (color, variance, normal, depth, alpha))
    demodulate = (albedo is not None) if demodulate is None else bool(demodulate)
    H, W = Z.shape
    sc2 = F32(sigma_color) * F32(sigma_color)
    sz = F32(sigma_depth)
    with np.errstate(all="ignore"):
        if demodulate:
            ad = np.fmax(np.asarray(albedo, dtype=F32), F32(0.01))
            Cc, V = C0 / ad, V0 / (ad * ad)
        else:
            Cc, V = C0.copy(), V0.copy()
        surf = A > 0
        I, J = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
        zden = sz * Z + F32(1e-6)
        for k in range(iterations):
            s = 1 << k
            vsum = (V[..., 0] + V[..., 1]) + V[..., 2]
            sw = np.zeros((H, W), F32)
            sc, sv = np.zeros((H, W, 3), F32), np.zeros((H, W, 3), F32)
            for dy in range(-2, 3):
                for dx in range(-2, 3):
                    qi, qj = I + dy * s, J + dx * s
                    inside = (qi >= 0) & (qi < H) & (qj >= 0) & (qj < W)
                    ci, cj = np.clip(qi, 0, H - 1), np.clip(qj, 0, W - 1)  # (gathered, then not taken)
                    Nq, Zq, Cq, Vq, surf_q = N[ci, cj], Z[ci, cj], Cc[ci, cj], V[ci, cj], surf[ci, cj]
                    take = inside & (surf == surf_q)
                    d = np.fmax((N[..., 0] * Nq[..., 0] + N[..., 1] * Nq[..., 1]) + N[..., 2] * Nq[..., 2], F32(0))
                    wn = d
                    for _ in range(normal_squarings):
                        wn = wn * wn
                    wz = falloff(np.abs(Z - Zq) / zden)
                    wn, wz = np.where(surf, wn, F32(1)), np.where(surf, wz, F32(1))
                    diff = Cc - Cq
                    d2 = (diff[..., 0] * diff[..., 0] + diff[..., 1] * diff[..., 1]) + diff[..., 2] * diff[..., 2]
                    vs = vsum + vsum[ci, cj]
                    wc = falloff(d2 / (sc2 * vs + F32(1e-10)))
                    w = (((H5[dy + 2] * H5[dx + 2]) * wn) * wz) * wc
                    for x in (d, wn, wz, d2, vs, wc, w):
                        assert x.dtype == F32
                    sw = np.where(take, sw + w, sw)
                    sc = np.where(take[..., None], sc + w[..., None] * Cq, sc)
                    sv = np.where(take[..., None], sv + (w * w)[..., None] * Vq, sv)
            ok = (sw >= MIN_WEIGHT_SUM)[..., None]
            if decisions is not None:
                decisions.append(ok[..., 0])
            Cc, V = np.where(ok, sc / sw[..., None], Cc), np.where(ok, sv / (sw * sw)[..., None], V)
            assert Cc.dtype == F32 and V.dtype == F32
        if demodulate:
            Cc, V = Cc * ad, V * (ad * ad)
    return Cc.astype(F32), V.astype(F32)


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


# ------------------------------------------------------------------ refusals before any HIP call
def _refused(rc, word):
    assert rc == ERR_INVALID, rc
    msg = rtmi.lib().rtmi_last_error()
    assert msg and word in msg, msg
    return True


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
