"""rtmi_occluded on the host side: the symbols of both builds, the argument checks that come before any HIP call, the
Python binding's refusals, and the occlusion kernels' presence in both builds of the library.  No GPU involved."""
import ctypes as C
import os
import re
import subprocess

import pytest

import common
import rtmi
from abi_host import CHECK_LIB, QUERY_VARIANTS, ROOT

LIB = os.path.dirname(CHECK_LIB)


def test_occluded_is_exported_by_both_builds():
    L = C.CDLL(rtmi.LIB_PATH)
    assert hasattr(L, "rtmi_occluded")
    assert not hasattr(L, "rtmi_occluded_check_counts")  # the diagnostic entry exists only in the check build
    assert rtmi.lib().rtmi_version() == 3  # additive: no version change
    assert os.path.exists(CHECK_LIB), "librtmi_check1.so missing: __graft_entry__.build() builds it"
    out = subprocess.check_output(["nm", "-D", "--defined-only", CHECK_LIB], text=True)
    names = {ln.split()[-1] for ln in out.splitlines() if ln.strip()}
    assert {"rtmi_occluded", "rtmi_occluded_check_counts", "rtmi_intersect_check_counts"} <= names


C_PROG = r'''
#include <stdint.h>
#include <stdio.h>
#include "rtmi.h"
int main(void) {
  /* argument checks before any HIP call */
  float dummy[3] = {0, 0, 0};
  uint8_t occ[1];
  unsigned long long counts[2];
  if (rtmi_occluded(NULL, 1, dummy, dummy, NULL, occ, counts, NULL) != RTMI_ERR_INVALID) return 1;
  rtmi_scene *s = rtmi_scene_create();
  if (rtmi_occluded(s, -1, dummy, dummy, NULL, occ, NULL, NULL) != RTMI_ERR_INVALID) return 2;
  if (rtmi_occluded(s, 1, NULL, dummy, NULL, occ, NULL, NULL) != RTMI_ERR_INVALID) return 3;
  if (rtmi_occluded(s, 1, dummy, NULL, dummy, occ, NULL, NULL) != RTMI_ERR_INVALID) return 4;
  if (rtmi_occluded(s, 1, dummy, dummy, NULL, NULL, counts, NULL) != RTMI_ERR_INVALID) return 5;
  if (rtmi_occluded(s, 1, dummy, dummy, NULL, occ, NULL, NULL) != RTMI_ERR_INVALID) return 6; /* uncommitted */
  if (rtmi_occluded(s, 0, NULL, NULL, NULL, NULL, NULL, NULL) != RTMI_ERR_INVALID) return 7; /* uncommitted */
  rtmi_scene_destroy(s);
  printf("rtmi_occluded ok\n");
  return 0;
}
'''


def test_argument_checks_from_c(tmp_path):
    src = tmp_path / "occ.c"
    src.write_text(C_PROG)
    exe = tmp_path / "occ"
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), str(src),
                    "-L", LIB, "-lrtmi", "-Wl,-rpath," + LIB, "-Wl,-rpath,/opt/rocm/lib", "-o", str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, (r.returncode, r.stdout, r.stderr)


def test_validation_errors_without_a_gpu():
    L = rtmi.lib()
    dummy = C.c_void_p(16)  # never dereferenced: the host does not read the arrays
    cases = [
        (None, 1, dummy, dummy, dummy, b"null scene"),
        ("scene", -1, dummy, dummy, dummy, b"negative"),
        ("scene", 4, None, dummy, dummy, b"null ray"),
        ("scene", 4, dummy, None, dummy, b"null ray"),
        ("scene", 4, dummy, dummy, None, b"null ray or output"),
        ("scene", 4, dummy, dummy, dummy, b"not committed"),
        ("scene", 0, None, None, None, b"not committed"),
    ]
    b = rtmi.SceneBuilder(1)
    m = b.lambertian([0.5, 0.5, 0.5])
    b.sphere([0, 0, -1], 0.5, m)
    b.camera_pinhole([0, 0, 1], [0, 0, -1], [0, 1, 0], 1.0, 1.0)  # recorded, never committed
    for scene, n, o, d, out, msg in cases:
        rc = L.rtmi_occluded(b.h if scene else None, n, o, d, None, out, None, None)
        assert rc == -1, (scene, n, msg)
        assert msg in L.rtmi_last_error(), (msg, L.rtmi_last_error())


def test_python_occluded_refuses_before_gpu_work():
    torch = pytest.importorskip("torch")
    b = rtmi.SceneBuilder(1)
    o = torch.zeros((4, 3), dtype=torch.float32)
    with pytest.raises(rtmi.RtmiError, match="CPU"):
        b.occluded(o, o)
    with pytest.raises(rtmi.RtmiError, match="torch tensor"):
        b.occluded(o.numpy(), o.numpy())
    with pytest.raises(rtmi.RtmiError, match="CPU"):
        b.occluded(o, o, t_max=torch.ones(4))
    if torch.cuda.is_available():  # (on a GPU machine: dtype, shape, t_max, out, and an uncommitted scene)
        g = torch.zeros((4, 3), dtype=torch.float32, device="cuda")
        with pytest.raises(rtmi.RtmiError, match="float32"):
            b.occluded(g.double(), g)
        with pytest.raises(rtmi.RtmiError, match="shape"):
            b.occluded(g.reshape(3, 4), g.reshape(3, 4))
        with pytest.raises(rtmi.RtmiError, match="differ in length"):
            b.occluded(g, g[:3])
        for bad in (torch.ones(4), torch.ones(4, device="cuda", dtype=torch.float64), torch.ones(5, device="cuda"),
                    torch.ones((4, 1), device="cuda"), [1.0] * 4):
            with pytest.raises(rtmi.RtmiError, match="t_max"):
                b.occluded(g, g, t_max=bad)
        for bad in (torch.zeros(4, dtype=torch.uint8), torch.zeros(4, dtype=torch.int32, device="cuda"),
                    torch.zeros(5, dtype=torch.uint8, device="cuda"), torch.zeros(8, dtype=torch.uint8, device="cuda")[::2]):
            with pytest.raises(rtmi.RtmiError, match="out"):
                b.occluded(g, g, out=bad)
        with pytest.raises(rtmi.RtmiError, match="not committed"):
            b.occluded(g, g)


def test_occlusion_kernels_one_per_variant_without_static_lds():
    """occlusion_body.h hands closest_hit LDS regions by byte offset of the dynamic array: every occlusion kernel of the
    product and of the margin-check build must declare no static LDS, and there is one per query variant."""
    for lib in (rtmi.LIB_PATH, CHECK_LIB):
        names = set()
        for name, blk in common.kernel_notes(lib).items():
            if "occlusion_kernel" in name:
                assert not any(k in name for k in ("query_kernel", "render_kernel", "probe_kernel")), name
                names.add(name)
                assert re.search(r"\.group_segment_fixed_size:\s+0\b", blk), (lib, name)
        assert len(names) == QUERY_VARIANTS, (lib, sorted(names))
