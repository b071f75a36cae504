"""rtmi_path_compact / rtmi_bounce_list on the host side: the exports of both builds and their declarations, a C99 program
that links them, the argument checks that come before any HIP call, the Python binding's refusals, the new kernels'
metadata, and the numpy restatements of "live" and of the compaction (tests/bouncelistlib.py) held to hand-worked cases.
No GPU involved."""
import os
import re
import subprocess

import numpy as np
import pytest

import common
import rtmi
from abi_host import DUMMY, ERR_INVALID, LIBS, OK, QUERY_VARIANTS, ROOT, _count, _refused
from bouncelistlib import P, SCAN_THREADS, compact, live, make_bad

NEW = ("rtmi_path_compact_scratch_bytes", "rtmi_path_compact", "rtmi_bounce_list")
LIB_DIR = os.path.dirname(rtmi.LIB_PATH)
f32 = np.float32


def test_entries_are_exported_by_both_builds_declared_and_bound():
    L = rtmi.lib()
    assert L.rtmi_version() == 3  # additive: no version change
    names = [s[0] for s in rtmi.SYMBOLS]
    header = open(os.path.join(ROOT, "include", "rtmi.h")).read()
    for lib in LIBS:
        syms = subprocess.run(["nm", "-D", "--defined-only", lib], stdout=subprocess.PIPE, text=True, check=True).stdout
        for name in NEW:
            assert re.search(r"\bT %s$" % name, syms, re.M), (lib, name)
    for name in NEW:
        assert name in names and re.search(r"\b%s\(" % name, header), name
    assert int(re.search(r"#define RTMI_PATH_COMPACT_ITEMS (\d+)", header).group(1)) == rtmi.PATH_COMPACT_ITEMS == P
    src = open(os.path.join(ROOT, "ray-tracing-cuda_amd", "csrc", "paths.hip")).read()
    assert re.search(r"kCompactScanThreads = %d;" % SCAN_THREADS, src)  # what the GPU test's sizes are worked out from


def test_scratch_is_one_word_per_workgroup():
    sb = rtmi.lib().rtmi_path_compact_scratch_bytes
    assert sb(-1) == sb(0) == sb(1) == sb(P) == 4  # (never 0: a caller may allocate it as it is)
    assert sb(P + 1) == 8 and sb(3 * P) == 12 and sb((1 << 31) - 1) == 4 * (1 << 21)


C_PROG = r'''
#include <stdio.h>
#include <string.h>
#include "rtmi.h"
typedef size_t (*bytes_fn)(int64_t);
typedef int (*compact_fn)(int64_t, const float *, const float *, const uint32_t *, int64_t, const uint32_t *, uint32_t *,
                          uint32_t *, void *, void *);
typedef int (*list_fn)(const rtmi_scene *, int64_t, const uint32_t *, int64_t, const uint32_t *, float *, float *, void *,
                       float *, float *, rtmi_hit *, uint32_t *, unsigned long long *, void *);
int main(void) {
  bytes_fn bytes = &rtmi_path_compact_scratch_bytes;
  compact_fn compact = &rtmi_path_compact;
  list_fn step = &rtmi_bounce_list;
  float x[3] = {0, 0, 0};
  uint32_t a[4] = {0, 0, 0, 0}, b[4] = {0, 0, 0, 0};
  unsigned long long w[RTMI_TRACE_WORK_WORDS];
  rtmi_scene *s = rtmi_scene_create();
  if (bytes(RTMI_PATH_COMPACT_ITEMS) != 4 || bytes(RTMI_PATH_COMPACT_ITEMS + 1) != 8) return 1;
  if (compact(1, x, x, a, 1, NULL, a, b, b, NULL) != RTMI_ERR_INVALID || !strstr(rtmi_last_error(), "d_list_in")) return 2;
  if (compact(1, x, x, NULL, 2, NULL, a, b, b, NULL) != RTMI_ERR_INVALID || !strstr(rtmi_last_error(), "n_list")) return 3;
  if (compact(1, x, x, NULL, 0, NULL, NULL, NULL, NULL, NULL) != RTMI_OK) return 4;
  if (step(s, 1, NULL, 1, NULL, x, x, a, x, x, NULL, NULL, w, NULL) != RTMI_ERR_INVALID || !strstr(rtmi_last_error(), "committed")) return 5;
  if (step(NULL, 1, NULL, 1, NULL, x, x, a, x, x, NULL, NULL, w, NULL) != RTMI_ERR_INVALID) return 6;
  rtmi_scene_destroy(s);
  printf("bounce-list abi ok\n");
  return 0;
}
'''


def test_entries_link_from_c99(tmp_path):
    src = tmp_path / "list.c"
    src.write_text(C_PROG)
    exe = tmp_path / "list"
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), str(src),
                    "-L", LIB_DIR, "-lrtmi", "-Wl,-rpath," + LIB_DIR, "-Wl,-rpath,/opt/rocm/lib", "-o", str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, (r.returncode, r.stdout, r.stderr)
    assert "bounce-list abi ok" in r.stdout


# ------------------------------------------------------------------ refusals before any HIP call
A, B = DUMMY, __import__("ctypes").c_void_p(32)  # two distinct never-dereferenced pointers


def _compact(n, n_list, o=A, d=A, list_in=None, count_in=None, list_out=A, count_out=A, scratch=A):
    return rtmi.lib().rtmi_path_compact(n, o, d, list_in, n_list, count_in, list_out, count_out, scratch, None)


def test_path_compact_argument_checks_before_any_hip_call():
    assert _refused(_compact(-1, 0), b"negative")
    assert _refused(_compact(1 << 31, 1), b"2^31")
    assert _refused(_compact(4, -1), b"negative")
    assert _refused(_compact(4, 1 << 31, list_in=B), b"2^31")
    assert _refused(_compact(4, 5), b"n_list")  # a null list is the identity: no more entries than paths
    for k in ("o", "d", "list_out", "count_out", "scratch"):
        assert _refused(_compact(4, 4, **{k: None}), b"null"), k
    assert _refused(_compact(4, 4, list_in=A, list_out=A), b"d_list_in")
    assert _refused(_compact(4, 4, list_in=B, count_in=A, count_out=A), b"d_count_in")
    assert _compact(4, 0, None, None, None, None, None, None, None) == OK  # nothing to do, nowhere to write


def _list(s, n, n_list, lst=None, cnt=None, o=DUMMY, d=DUMMY, st=DUMMY, em=DUMMY, at=DUMMY, work=DUMMY):
    return rtmi.lib().rtmi_bounce_list(s, n, lst, n_list, cnt, o, d, st, em, at, None, None, work, None)


def test_bounce_list_argument_checks_before_any_hip_call():
    assert _refused(_list(None, 1, 1), b"null scene")
    b = rtmi.SceneBuilder(1)
    assert _refused(_list(b.h, -1, 0), b"negative")
    assert _refused(_list(b.h, 1 << 31, 1, lst=B), b"2^31")
    assert _refused(_list(b.h, 4, -1), b"negative")
    assert _refused(_list(b.h, 4, 1 << 31, lst=B), b"2^31")
    assert _refused(_list(b.h, 4, 5), b"n_list")
    for k in ("o", "d", "st", "em", "at", "work"):
        assert _refused(_list(b.h, 4, 4, **{k: None}), b"null"), k
    assert _refused(_list(b.h, 4, 4), b"committed")
    assert _refused(_list(b.h, 4, 9, lst=B, cnt=A), b"committed")  # (a list may be longer than n: entries >= n are skipped)


def test_python_refusals_come_before_any_gpu_work():
    torch = pytest.importorskip("torch")
    b = rtmi.SceneBuilder(1)
    o = torch.zeros((4, 3), dtype=torch.float32)
    st = torch.zeros((6, 4), dtype=torch.int32)
    with pytest.raises(rtmi.RtmiError):
        rtmi.path_compact(o, o.clone())  # CPU tensors: there is no CPU path
    with pytest.raises(rtmi.RtmiError):
        rtmi.path_compact(o.double(), o.clone())
    with pytest.raises(rtmi.RtmiError):
        rtmi.path_compact(torch.zeros((4, 2)), o)
    with pytest.raises(rtmi.RtmiError):
        b.bounce_list(None, o, o.clone(), st)
    with pytest.raises(rtmi.RtmiError):
        b.bounce_list(rtmi.Paths(torch.zeros(4, dtype=torch.int32)), o, o.clone(), st)
    with pytest.raises(rtmi.RtmiError):
        b.trace_steps(o, o.clone(), st, 4, compact=True)
    with pytest.raises(rtmi.RtmiError):
        b.trace_steps(o, o.clone(), st, 4, compact="sometimes")
    p = rtmi.Paths(torch.zeros(4, dtype=torch.int32), torch.zeros(1, dtype=torch.int32))
    assert p.n() == 0 and rtmi.Paths(torch.zeros(4, dtype=torch.int32)).n() == 4


# ------------------------------------------------------------------ the kernels' metadata
def test_list_kernels_spill_no_vgpr_and_use_no_more_than_the_plain_step():
    """One bounce_list_kernel per query variant in both builds; no static LDS (the step stages its tables at offsets of the
    dynamic array); no VGPR spilled; no more VGPRs than the variant's bounce_kernel.  The three compaction kernels exist,
    spill nothing and keep their few words of static LDS."""
    for lib in LIBS:
        notes = common.kernel_notes(lib)
        ls = {re.search(r"ILj(\d+)E", n).group(1): blk for n, blk in notes.items() if "bounce_list_kernel" in n}
        bs = {re.search(r"ILj(\d+)E", n).group(1): blk for n, blk in notes.items() if "13bounce_kernel" in n}
        assert len(ls) == len(bs) == QUERY_VARIANTS and sorted(ls) == sorted(bs), (lib, sorted(ls), sorted(bs))
        for f, blk in ls.items():
            assert _count(blk, "group_segment_fixed_size") == 0, (lib, f)
            assert _count(blk, "vgpr_spill_count") == 0, (lib, f)
            assert _count(blk, "vgpr_count") <= _count(bs[f], "vgpr_count"), (lib, f)
        for k in ("compact_count_kernel", "compact_scan_kernel", "compact_scatter_kernel"):
            blk = [b for n, b in notes.items() if k in n]
            assert len(blk) == 1, (lib, k)
            assert _count(blk[0], "vgpr_spill_count") == 0 and _count(blk[0], "sgpr_spill_count") == 0
            assert _count(blk[0], "private_segment_fixed_size") == 0, (lib, k)


# ------------------------------------------------------------------ "live" and the compaction, by hand
def _rays(n):
    O = np.zeros((n, 3), f32)
    D = np.tile(np.array([[0, 0, 1]], f32), (n, 1))
    return O, D


def test_live_by_hand():
    O, D = _rays(10)
    make_bad(O, D, 1, "neg_zero_dir")
    make_bad(O, D, 2, "nan_origin")
    make_bad(O, D, 3, "inf_dir")
    make_bad(O, D, 4, "tiny_dir")
    make_bad(O, D, 5, "zero_dir")
    make_bad(O, D, 6, "inf_origin")
    make_bad(O, D, 7, "huge_dir")
    D[8] = (3, 0, 4)        # not unit length: Ray's constructor normalises it, the path is live
    D[9] = (1e-30, 1, 0)    # one tiny component beside an ordinary one normalises
    assert (D[1] == 0).all() and np.signbit(D[1, 0])  # -0.0f is the zero direction
    assert live(O, D).tolist() == [True, False, False, False, False, False, False, False, True, True]
    assert live(np.zeros((0, 3), f32), np.zeros((0, 3), f32)).shape == (0,)


def test_compaction_by_hand():
    O, D = _rays(8)
    for i in (1, 4, 5):
        make_bad(O, D, i, "zero_dir")
    assert compact(O, D).tolist() == [0, 2, 3, 6, 7]                     # the identity: ascending
    assert compact(O, D, n_list=5).tolist() == [0, 2, 3]                 # a null list shorter than n
    assert compact(O, D, count_in=3).tolist() == [0, 2]                  # the device count cuts it short
    assert compact(O, D, count_in=100).tolist() == [0, 2, 3, 6, 7]       # ... and never lengthens it
    lst = [7, 1, 9, 3, 0, 4, 1 << 31, 2]
    assert compact(O, D, lst).tolist() == [7, 3, 0, 2]                   # the list's own order; 9 and 2^31 are no paths
    assert compact(O, D, lst, count_in=4).tolist() == [7, 3]             # live entries behind the count are ignored
    assert compact(O, D, lst, n_list=5, count_in=7).tolist() == [7, 3, 0]
    assert compact(O, D, []).tolist() == [] and compact(O, D, count_in=0).tolist() == []
    assert compact(O, D, lst).dtype == np.uint32
