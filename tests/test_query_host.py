"""rtmi_intersect on the host side: the ABI of rtmi_hit, the argument checks that come before any HIP call, the Python
binding's refusals, and the query kernels' presence in both builds of the library.  No GPU involved."""
import ctypes as C
import os
import re
import subprocess

import pytest

import common
import rtmi
from abi_host import QUERY_VARIANTS, ROOT

LIB = os.path.join(ROOT, "ray-tracing-cuda_amd", "lib")


def test_intersect_is_exported():
    L = C.CDLL(rtmi.LIB_PATH)
    assert hasattr(L, "rtmi_intersect")
    assert rtmi.lib().rtmi_version() == 3  # additive: no version change
    assert not hasattr(L, "rtmi_intersect_check_counts")  # the diagnostic entry exists only in the check build


def test_hit_constants():
    assert (rtmi.RTMI_HIT_NONE, rtmi.RTMI_HIT_SPHERE, rtmi.RTMI_HIT_TRIANGLE, rtmi.RTMI_HIT_PARALLELOGRAM,
            rtmi.RTMI_HIT_PARALLELEPIPED, rtmi.RTMI_HIT_MESH, rtmi.RTMI_HIT_SKY) == (0, 1, 2, 3, 4, 5, 6)


C_PROG = r'''
#include <stddef.h>
#include <stdio.h>
#include "rtmi.h"
int main(void) {
  if (sizeof(rtmi_hit) != 48) return 1;
  if (offsetof(rtmi_hit, t) != 0 || offsetof(rtmi_hit, u) != 4 || offsetof(rtmi_hit, v) != 8) return 2;
  if (offsetof(rtmi_hit, normal) != 12 || offsetof(rtmi_hit, material) != 24 || offsetof(rtmi_hit, kind) != 28) return 3;
  if (offsetof(rtmi_hit, entry) != 32 || offsetof(rtmi_hit, element) != 36 || offsetof(rtmi_hit, reserved) != 40) return 4;
  if (RTMI_HIT_NONE != 0 || RTMI_HIT_SPHERE != 1 || RTMI_HIT_TRIANGLE != 2 || RTMI_HIT_PARALLELOGRAM != 3 ||
      RTMI_HIT_PARALLELEPIPED != 4 || RTMI_HIT_MESH != 5 || RTMI_HIT_SKY != 6) return 5;
  /* argument checks before any HIP call */
  float dummy[3] = {0, 0, 0};
  rtmi_hit hit;
  if (rtmi_intersect(NULL, 1, dummy, dummy, NULL, &hit, NULL, NULL) != RTMI_ERR_INVALID) return 6;
  rtmi_scene *s = rtmi_scene_create();
  if (rtmi_intersect(s, -1, dummy, dummy, NULL, &hit, NULL, NULL) != RTMI_ERR_INVALID) return 7;
  if (rtmi_intersect(s, 1, NULL, dummy, NULL, &hit, NULL, NULL) != RTMI_ERR_INVALID) return 8;
  if (rtmi_intersect(s, 1, dummy, NULL, NULL, &hit, NULL, NULL) != RTMI_ERR_INVALID) return 9;
  if (rtmi_intersect(s, 1, dummy, dummy, NULL, NULL, NULL, NULL) != RTMI_ERR_INVALID) return 10;
  if (rtmi_intersect(s, 0, NULL, NULL, NULL, NULL, NULL, NULL) != RTMI_ERR_INVALID) return 11; /* uncommitted */
  rtmi_scene_destroy(s);
  printf("rtmi_hit ok\n");
  return 0;
}
'''


def test_rtmi_hit_layout_from_c(tmp_path):
    src = tmp_path / "hit.c"
    src.write_text(C_PROG)
    exe = tmp_path / "hit"
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
        ("scene", 4, dummy, dummy, None, b"null ray"),
        ("scene", 4, dummy, dummy, dummy, b"not committed"),
        ("scene", 0, None, None, None, b"not committed"),
    ]
    b = rtmi.SceneBuilder(1)
    m = b.lambertian([0.5, 0.5, 0.5])
    b.sphere([0, 0, -1], 0.5, m)
    b.camera_pinhole([0, 0, 1], [0, 0, -1], [0, 1, 0], 1.0, 1.0)  # recorded, never committed
    for scene, n, o, d, out, msg in cases:
        rc = L.rtmi_intersect(b.h if scene else None, n, o, d, None, out, None, None)
        assert rc == -1, (scene, n, msg)
        assert msg in L.rtmi_last_error(), (msg, L.rtmi_last_error())


def test_python_intersect_refuses_before_gpu_work():
    torch = pytest.importorskip("torch")
    b = rtmi.SceneBuilder(1)
    o = torch.zeros((4, 3), dtype=torch.float32)
    with pytest.raises(rtmi.RtmiError, match="CPU"):
        b.intersect(o, o)
    with pytest.raises(rtmi.RtmiError, match="torch tensor"):
        b.intersect(o.numpy(), o.numpy())
    if torch.cuda.is_available():  # (on a GPU machine: dtype, shape, and an uncommitted scene)
        g = torch.zeros((4, 3), dtype=torch.float32, device="cuda")
        with pytest.raises(rtmi.RtmiError, match="float32"):
            b.intersect(g.double(), g)
        with pytest.raises(rtmi.RtmiError, match="shape"):
            b.intersect(g.reshape(3, 4), g.reshape(3, 4))
        with pytest.raises(rtmi.RtmiError, match="not committed"):
            b.intersect(g, g)


def test_query_kernels_declare_no_static_lds():
    """query_body.h hands closest_hit LDS regions by byte offset of the dynamic array, as render_body.h does: every
    query kernel of the product and of the margin-check build must declare no static LDS, and there is one per query
    variant."""
    for lib in (rtmi.LIB_PATH, os.path.join(os.path.dirname(rtmi.LIB_PATH), "librtmi_check1.so")):
        names = set()
        for name, blk in common.kernel_notes(lib).items():
            if "query_kernel" in name:
                names.add(name)
                assert re.search(r"\.group_segment_fixed_size:\s+0\b", blk), (lib, name)
        assert len(names) == QUERY_VARIANTS, (lib, sorted(names))
