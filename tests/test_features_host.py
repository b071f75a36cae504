"""rtmi_render_features / rtmi_resolve_features on the host side: the exported symbols, sizeof(rtmi_features), the argument
checks that come before any HIP call, the feature kernels in both builds of the library, and the resolve rule restated in
numpy (tests/budgetlib.py: ``resolve_rule``, which tests/test_gpu_features.py holds the device against).  No GPU involved."""
import ctypes as C
import os
import re
import subprocess
import tempfile

import numpy as np

import common
import rtmi
from abi_host import DUMMY, ERR_DEPTH, F_DEFOCUS, LIBS, QUERY_VARIANTS, ROOT, _frame, _refused
from budgetlib import resolve_rule

ENTRIES = ("rtmi_render_features", "rtmi_resolve_features")
F32 = np.float32


def test_resolve_rule_on_hand_worked_cases():
    """n = 4, three of the samples on a surface: albedo 2 / 4, normal -3 / 4, depth 7.5 / 3, alpha 3 / 4 -- all exact in
    binary32; a pixel whose samples all went to the sky has depth 0 and alpha 0 but an albedo; n = 0 and padding: 0."""
    n = np.array([4, 4, 0, 4], np.uint32)
    alb = np.array([[2, 1, 0]] * 4, F32)
    nrm = np.array([[0, 0, -3]] * 4, F32)
    dep = np.array([7.5, 0, 9, 7.5], F32)
    cov = np.array([3, 0, 5, 3], np.uint32)
    a, m, d, alpha = resolve_rule(n, alb, nrm, dep, cov, pixel=np.array([True, True, True, False]))
    assert a.tolist() == [[0.5, 0.25, 0]] * 2 + [[0, 0, 0]] * 2
    assert m.tolist() == [[0, 0, -0.75]] * 2 + [[0, 0, 0]] * 2
    assert d.tolist() == [2.5, 0, 0, 0]
    assert alpha.tolist() == [0.75, 0, 0, 0]


# ------------------------------------------------------------------ symbols, the struct
def test_feature_entries_are_exported_by_both_builds():
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


def test_sizeof_rtmi_features_agrees_with_the_header():
    """The C compiler's sizeof and field offsets of rtmi_features, from include/rtmi.h itself, against the ctypes struct."""
    fields = [f[0] for f in rtmi.Features._fields_]
    src = '#include <stdio.h>\n#include <stddef.h>\n#include "rtmi.h"\nint main(void) { printf("%zu", sizeof(rtmi_features));\n'
    src += "".join('printf(" %%zu", offsetof(rtmi_features, %s));\n' % f for f in fields) + "return 0; }\n"
    with tempfile.TemporaryDirectory() as tmp:
        c, exe = os.path.join(tmp, "s.c"), os.path.join(tmp, "s")
        with open(c, "w") as fh:
            fh.write(src)
        subprocess.check_call(["cc", "-I", os.path.join(ROOT, "include"), c, "-o", exe])
        got = [int(x) for x in subprocess.check_output([exe], text=True).split()]
    assert got == [C.sizeof(rtmi.Features)] + [getattr(rtmi.Features, f).offset for f in fields]
    assert got[0] == 40


# ------------------------------------------------------------------ refusals before any HIP call
def _feat(size=None, reserved=0, **bufs):
    f = rtmi.Features(C.sizeof(rtmi.Features) if size is None else size, reserved)
    for k in bufs:
        setattr(f, "d_" + k, DUMMY.value)
    return f


def test_render_features_argument_checks_before_any_hip_call():
    L = rtmi.lib()
    b = rtmi.SceneBuilder(1)  # (never committed: every refusal below comes before the scene is used)

    def call(s, frame, feat, **null):
        a = {k: (None if k in null else DUMMY) for k in ("budget", "states", "sum", "sq", "samples", "rays", "work")}
        return L.rtmi_render_features(s, C.byref(frame), a["budget"], a["states"], a["sum"], a["sq"], a["samples"],
                                      a["rays"], C.byref(feat) if feat is not None else None, a["work"], None)

    assert _refused(call(None, _frame(), _feat(albedo=1)), b"scene")
    assert _refused(call(b.h, _frame(), _feat(size=C.sizeof(rtmi.Features) + 8, albedo=1)), b"size")
    assert _refused(call(b.h, _frame(), _feat(size=0)), b"size")
    assert _refused(call(b.h, _frame(), _feat(reserved=1, normal=1)), b"reserved")
    for k in ("albedo", "normal", "depth", "coverage"):  # any ONE feature buffer makes depth 0 an error
        assert _refused(call(b.h, _frame(max_depth=0), _feat(**{k: 1})), b"max_depth", ERR_DEPTH), k
    # without a feature buffer the call is rtmi_render_budget, which takes depth 0: the uncommitted scene is what is refused
    assert _refused(call(b.h, _frame(max_depth=0), _feat()), b"committed")
    assert _refused(call(b.h, _frame(max_depth=0), None), b"committed")
    assert _refused(call(b.h, _frame(), _feat(albedo=1, normal=1, depth=1, coverage=1)), b"committed")
    # rtmi_render_budget's own refusals hold
    assert _refused(call(b.h, _frame(height=0), _feat(albedo=1)), b"frame")
    for k in ("budget", "states", "sum", "samples", "work"):
        assert _refused(call(b.h, _frame(), _feat(albedo=1), **{k: True}), b"null"), k


def test_resolve_features_argument_checks_before_any_hip_call():
    L = rtmi.lib()

    def call(frame, sums, out, n=DUMMY):
        return L.rtmi_resolve_features(C.byref(frame) if frame is not None else None,
                                       C.byref(sums) if sums is not None else None, n,
                                       C.byref(out) if out is not None else None, None)

    full = dict(albedo=1, normal=1, depth=1, coverage=1)
    assert _refused(call(None, _feat(**full), _feat(**full)), b"frame")
    assert _refused(call(_frame(width=0), _feat(**full), _feat(**full)), b"frame")
    assert _refused(call(_frame(), None, _feat(**full)), b"null")
    assert _refused(call(_frame(), _feat(**full), None), b"null")
    assert _refused(call(_frame(), _feat(**full), _feat(**full), n=None), b"null")
    assert _refused(call(_frame(), _feat(size=4, **full), _feat(**full)), b"size")
    assert _refused(call(_frame(), _feat(**full), _feat(reserved=7, **full)), b"reserved")
    # an out buffer without its sums twin; depth and alpha need the coverage sums
    for k in ("albedo", "normal", "depth", "coverage"):
        sums = dict(full)
        del sums[k]
        assert _refused(call(_frame(), _feat(**sums), _feat(**{k: 1})), b"without its sums"), k
    assert _refused(call(_frame(), _feat(albedo=1, normal=1, depth=1), _feat(depth=1)), b"coverage")


# ------------------------------------------------------------------ the kernels
def test_feature_kernels_one_per_variant_without_static_lds():
    """The feature kernels are the budget kernels' twins: eight, each with F_DEFOCUS set, addressing the layer stack at
    byte offsets of the DYNAMIC LDS array (render_body.h: lds_byte) -- right only while they declare no static LDS, in
    both builds; and none runs at lower occupancy than its twin (the same VGPR step of the allocation table)."""
    waves = lambda v: next(w for lim, w in ((64, 8), (72, 7), (80, 6), (96, 5), (128, 4), (168, 3), (256, 2), (512, 1)) if v <= lim)
    for lib in LIBS:
        ks = common.kernel_notes(lib)
        fk = {n: blk for n, blk in ks.items() if "feature_kernel" in n}
        assert len(fk) == QUERY_VARIANTS, (lib, sorted(fk))
        for name, blk in fk.items():
            assert re.search(r"\.group_segment_fixed_size:\s+0\b", blk), (lib, name)
            feature_set = int(re.search(r"feature_kernelILj(\d+)E", name).group(1))
            assert feature_set & F_DEFOCUS, name
            twin = ks[name.replace("14feature_kernel", "13budget_kernel")]
            vgpr = lambda b: int(re.search(r"\.vgpr_count:\s+(\d+)", b).group(1))  # (the unified count: AGPRs included)
            assert waves(vgpr(blk)) >= waves(vgpr(twin)), (lib, name, vgpr(blk), vgpr(twin))
        rk = [n for n in ks if "resolve_features_kernel" in n]
        assert len(rk) == 1 and re.search(r"\.group_segment_fixed_size:\s+0\b", ks[rk[0]])
