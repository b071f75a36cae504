"""rtmi_occluded_list on the host side: the exports of both builds and the declaration, a C99 program that links the entry
and meets every refusal that comes before any HIP call, the Python binding's refusals, and the new kernels' metadata held
to their twins'.  No GPU involved."""
import os
import re
import subprocess

import pytest

import common
import rtmi
from abi_host import DUMMY, LIBS, QUERY_VARIANTS, ROOT, _count, _refused, _waves

NEW = "rtmi_occluded_list"
CHECK_ONLY = "rtmi_occluded_list_check_counts"
LIB_DIR = os.path.dirname(rtmi.LIB_PATH)


def test_entry_is_exported_by_both_builds_declared_and_bound():
    assert rtmi.lib().rtmi_version() == 3  # additive: no version change
    header = open(os.path.join(ROOT, "include", "rtmi.h")).read()
    for k, lib in enumerate(LIBS):
        syms = subprocess.run(["nm", "-D", "--defined-only", lib], stdout=subprocess.PIPE, text=True, check=True).stdout
        assert re.search(r"\bT %s$" % NEW, syms, re.M), lib
        assert bool(re.search(r"\bT %s$" % CHECK_ONLY, syms, re.M)) == (k == 1), lib  # only the check build has it
    assert re.search(r"^int %s\(" % NEW, header, re.M)
    assert CHECK_ONLY in header and not re.search(r"^int %s\(" % CHECK_ONLY, header, re.M)  # declared in words only
    assert "need NOT be distinct" in header  # the difference from rtmi_bounce_list is stated
    assert NEW in [s[0] for s in rtmi.SYMBOLS]
    assert hasattr(rtmi.SceneBuilder, "occluded_list")


C_PROG = r'''
#include <stdio.h>
#include <string.h>
#include "rtmi.h"
typedef int (*list_fn)(const rtmi_scene *, int64_t, const uint32_t *, int64_t, const uint32_t *, const float *, const float *,
                       const float *, uint8_t *, unsigned long long *, void *);
static int refused(int rc, const char *word) { return rc == RTMI_ERR_INVALID && strstr(rtmi_last_error(), word) != NULL; }
int main(void) {
  list_fn q = &rtmi_occluded_list;
  float x[3] = {0, 0, 0};
  uint32_t l[4] = {0, 0, 0, 0};
  uint8_t occ[4];
  const int64_t big = (int64_t)1 << 31;
  rtmi_scene *s = rtmi_scene_create();
  if (!refused(q(NULL, 1, NULL, 1, NULL, x, x, NULL, occ, NULL, NULL), "null scene")) return 1;
  if (!refused(q(s, -1, NULL, 0, NULL, x, x, NULL, occ, NULL, NULL), "n")) return 2;
  if (!refused(q(s, -1, NULL, 0, NULL, x, x, NULL, occ, NULL, NULL), "negative")) return 3;
  if (!refused(q(s, big, l, 1, NULL, x, x, NULL, occ, NULL, NULL), "2^31")) return 4;
  if (!refused(q(s, 4, l, -1, NULL, x, x, NULL, occ, NULL, NULL), "negative list")) return 5;
  if (!refused(q(s, 4, l, big, NULL, x, x, NULL, occ, NULL, NULL), "list entries")) return 6;
  if (!refused(q(s, 4, NULL, 5, NULL, x, x, NULL, occ, NULL, NULL), "n_list")) return 7;
  if (!refused(q(s, 4, l, 4, NULL, NULL, x, NULL, occ, NULL, NULL), "d_origins")) return 8;
  if (!refused(q(s, 4, l, 4, NULL, x, NULL, NULL, occ, NULL, NULL), "d_dirs")) return 9;
  if (!refused(q(s, 4, l, 4, NULL, x, x, NULL, NULL, NULL, NULL), "d_occluded")) return 10;
  if (!refused(q(s, 4, l, 4, NULL, x, x, NULL, occ, NULL, NULL), "committed")) return 11;
  /* nothing to do is still refused on an uncommitted scene, as rtmi_occluded refuses n == 0 there */
  if (!refused(q(s, 4, NULL, 0, NULL, NULL, NULL, NULL, NULL, NULL, NULL), "committed")) return 12;
  if (!refused(q(s, 0, NULL, 0, NULL, NULL, NULL, NULL, NULL, NULL, NULL), "committed")) return 13;
  /* a list may be longer than n (entries >= n are dropped): only the scene is wrong here */
  if (!refused(q(s, 4, l, 9, l, x, x, x, occ, NULL, NULL), "committed")) return 14;
  rtmi_scene_destroy(s);
  printf("occluded-list abi ok\n");
  return 0;
}
'''


def test_entry_links_from_c99_and_refuses_before_any_hip_call(tmp_path):
    src = tmp_path / "occlist.c"
    src.write_text(C_PROG)
    exe = tmp_path / "occlist"
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), str(src),
                    "-L", LIB_DIR, "-lrtmi", "-Wl,-rpath," + LIB_DIR, "-Wl,-rpath,/opt/rocm/lib", "-o", str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, (r.returncode, r.stdout, r.stderr)
    assert "occluded-list abi ok" in r.stdout


def _call(s, n, n_list, lst=None, cnt=None, o=DUMMY, d=DUMMY, tm=None, out=DUMMY, counts=None):
    return rtmi.lib().rtmi_occluded_list(s, n, lst, n_list, cnt, o, d, tm, out, counts, None)


def test_argument_checks_through_the_binding_s_library():
    assert _refused(_call(None, 1, 1), b"null scene")
    b = rtmi.SceneBuilder(1)
    assert _refused(_call(b.h, -1, 0), b"negative")
    assert _refused(_call(b.h, 1 << 31, 1, lst=DUMMY), b"2^31")
    assert _refused(_call(b.h, 4, -1), b"negative")
    assert _refused(_call(b.h, 4, 1 << 31, lst=DUMMY), b"2^31")
    assert _refused(_call(b.h, 4, 5), b"n_list")
    for k, word in (("o", b"d_origins"), ("d", b"d_dirs"), ("out", b"d_occluded")):
        assert _refused(_call(b.h, 4, 4, **{k: None}), word), k
    assert _refused(_call(b.h, 4, 4), b"committed")  # (t_max, the list, the count and the counts are optional)
    assert _refused(_call(b.h, 4, 0, o=None, d=None, out=None), b"committed")
    assert _refused(_call(b.h, 0, 0, o=None, d=None, out=None), b"committed")


def test_python_refusals_come_before_any_gpu_work():
    torch = pytest.importorskip("torch")
    b = rtmi.SceneBuilder(1)
    o = torch.zeros((4, 3), dtype=torch.float32)
    with pytest.raises(rtmi.RtmiError, match="CPU"):
        b.occluded_list(None, o, o)  # CPU tensors: there is no CPU path
    with pytest.raises(rtmi.RtmiError, match="torch tensor"):
        b.occluded_list(None, o.numpy(), o.numpy())
    with pytest.raises(rtmi.RtmiError, match="CPU"):
        b.occluded_list(None, o, o, t_max=torch.ones(4))
    st = torch.zeros((6, 4), dtype=torch.int32)
    for kw in (dict(shadow="list"), dict(shadow="list", compact=True), dict(shadow="list", direct=True, light_states=st),
               dict(shadow="some", compact=True, direct=True, light_states=st)):
        with pytest.raises(rtmi.RtmiError, match="shadow"):
            b.trace_steps(o, o.clone(), st, 4, **kw)
    assert rtmi.SHADOW_DEFAULT in ("all", "list")
    if torch.cuda.is_available():  # (on a GPU machine: what occluded refuses, the list, and an uncommitted scene)
        g = torch.zeros((4, 3), dtype=torch.float32, device="cuda")
        with pytest.raises(rtmi.RtmiError, match="float32"):
            b.occluded_list(None, g.double(), g)
        with pytest.raises(rtmi.RtmiError, match="differ in length"):
            b.occluded_list(None, g, g[:3])
        with pytest.raises(rtmi.RtmiError, match="t_max"):
            b.occluded_list(None, g, g, t_max=torch.ones(5, device="cuda"))
        with pytest.raises(rtmi.RtmiError, match="Paths"):
            b.occluded_list(torch.zeros(4, dtype=torch.int32, device="cuda"), g, g)
        with pytest.raises(rtmi.RtmiError, match="index"):
            b.occluded_list(rtmi.Paths(torch.zeros(4, dtype=torch.int32)), g, g)
        for bad in (torch.zeros(4, dtype=torch.uint8), torch.zeros(4, dtype=torch.int32, device="cuda"),
                    torch.zeros(5, dtype=torch.uint8, device="cuda"), torch.zeros(8, dtype=torch.uint8, device="cuda")[::2]):
            with pytest.raises(rtmi.RtmiError, match="out"):
                b.occluded_list(None, g, g, out=bad)
        with pytest.raises(rtmi.RtmiError, match="not committed"):
            b.occluded_list(None, g, g)


def test_list_kernels_one_per_variant_and_no_worse_than_their_twins():
    """One occlusion_list_kernel per query variant in both builds; no static LDS (the body stages its tables at offsets of
    the dynamic array); no lower occupancy step -- waves per SIMD that the VGPR allocation allows -- than the variant's
    occlusion_kernel; no private segment that the twin does not have."""
    for lib in LIBS:
        notes = common.kernel_notes(lib)
        ls = {re.search(r"ILj(\d+)E", n).group(1): blk for n, blk in notes.items() if "occlusion_list_kernel" in n}
        ts = {re.search(r"ILj(\d+)E", n).group(1): blk for n, blk in notes.items() if "occlusion_kernel" in n}
        assert len(ls) == len(ts) == QUERY_VARIANTS and sorted(ls) == sorted(ts), (lib, sorted(ls), sorted(ts))
        for f, blk in ls.items():
            assert _count(blk, "group_segment_fixed_size") == 0, (lib, f)
            assert _waves(_count(blk, "vgpr_count")) >= _waves(_count(ts[f], "vgpr_count")), (lib, f)
            if _count(ts[f], "private_segment_fixed_size") == 0:
                assert _count(blk, "private_segment_fixed_size") == 0, (lib, f)
